// loop_kernels.hpp -- internal interface of the connection loop of a set
// (ugo_fec_loop_set_*, include/ugo_loop.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/ugo_loop.h"
#include "ack_kernels.hpp"
#include "sent_kernels.hpp"
#include "stream_set_kernels.hpp"
#include "stream_tx_kernels.hpp"

namespace ugo {
namespace kern {

// The device form of a member's record is the public struct; the records of a
// set are one dense array, 16-B aligned.
typedef ugo_loop_state LoopRecord;

constexpr uint32_t kLoopSetMaxConn = 1u << 20;
constexpr uint32_t kLoopScanBlock = 1024;  // members per block of the ranks of append and sent
constexpr uint32_t kKLoop = 16;            // UGO_FEC_KERNEL_LOOP
constexpr uint32_t kLoopIdle = 0xffffffffu;

// What receive's per-packet pass gathers for a member: the lowest batch index
// of a packet of each kind (device, owned by the set, all kLoopIdle between
// calls: the per-member pass resets it).  16 bytes.
struct LoopCall {
  uint32_t first;  // any packet of the member
  uint32_t end;    // a packet that ends the loop: E
  uint32_t pn;     // a packet with packet_number != 0
  uint32_t fin;    // a packet with flags & 0x10
};

// The neighbouring sets' device tables and the set's own arrays.
struct LoopTables {
  const StreamSetEntry* stream_rx;
  const AckEntry* ack_rx;
  const StreamTxEntry* stream_tx;
  const SentEntry* sent_tx;
  LoopRecord* recs;   // [nconn]
  LoopCall* call;     // [nconn]
  uint32_t* block_a;  // [kLoopScanBlock]: per scan block, pending members (append) / unreported exits (sent)
  uint32_t* block_b;  // [kLoopScanBlock]: per scan block, live members (sent)
  unsigned long long* words;  // [0] *total as append found it; [1] the deadline, UINT64_MAX between calls
  ugo_loop_params p;
  uint32_t nconn;
};

struct LoopReceiveArgs {
  LoopTables t;
  const ugo_pkt_info* info;
  uint32_t* conn_of;
  uint64_t npk;
  uint64_t now_us;
};
hipError_t launch_loop_receive(const LoopReceiveArgs& a, hipStream_t s);

struct LoopCloseArgs {
  LoopTables t;
  const uint8_t* how;
  const unsigned long long* linger_us;  // nullable
  uint64_t now_us;
};
hipError_t launch_loop_close(const LoopCloseArgs& a, hipStream_t s);

struct LoopCheckArgs {
  LoopTables t;
  uint32_t* budget;
  uint8_t* may_ack_only;
  uint64_t now_us;
};
hipError_t launch_loop_check(const LoopCheckArgs& a, hipStream_t s);

struct LoopAppendArgs {
  LoopTables t;
  const unsigned long long* total;
  ugo_pkt_info* info;
  ugo_pkt_segment* segs;
  uint32_t* conn_of;
  unsigned long long* total_out;
  uint8_t* appended;
  uint64_t max_packets;
  uint64_t max_segments;
};
hipError_t launch_loop_append(const LoopAppendArgs& a, hipStream_t s);

struct LoopSentArgs {
  LoopTables t;
  const uint32_t* n_packets;
  const uint8_t* attached;
  const unsigned long long* delay_us;  // nullable
  unsigned long long* deadline_us;
  uint32_t* exits;
  uint8_t* reasons;
  unsigned long long* n_exits;
  uint32_t* new_index;             // nullable
  unsigned long long* nconn_new;   // nullable
  uint64_t max_exits;
  uint64_t now_us;
};
hipError_t launch_loop_sent(const LoopSentArgs& a, hipStream_t s);

}  // namespace kern
}  // namespace ugo
