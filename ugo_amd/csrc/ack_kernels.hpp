// ack_kernels.hpp -- internal interface of the receive histories and their
// sets (ugo_fec_ack_*, include/ugo_ack.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/ugo_ack.h"

namespace ugo {
namespace kern {

// The device record of a receive history is the public struct itself.
typedef ugo_ack_state AckRecord;

// One member of a set, uploaded once by ugo_fec_ack_set_create (24 bytes).
struct AckEntry {
  uint64_t* bits;  // wp / 64 words; packet number n is bit n & 63 of word (n & (wp - 1)) >> 6
  AckRecord* rec;
  uint32_t wp;
  uint32_t reserved;
};

constexpr uint32_t kAckSetMaxConn = 1u << 20;
constexpr uint32_t kAckScanBlock = 1024;  // members per block of attach's scan
constexpr uint32_t kKAck = 12;            // UGO_FEC_KERNEL_ACK

// What the per-packet passes of one receive call gather for a member (device,
// owned by the set, all zero between calls: the advance pass clears it).
// fresh and lo are not gathered: the advance pass reads them off the bitmap.
struct AckCall {
  unsigned long long sw_max;  // the largest stop-waiting of the packets that take part
  uint32_t old, oow;
  uint32_t touched;           // a packet of the member takes part
  uint32_t reserved;
};

struct AckReceiveArgs {
  const AckEntry* table;
  AckCall* call;            // [nconn]
  const ugo_pkt_info* info; // [npk]
  const uint32_t* conn_of;  // [npk]
  const uint8_t* seg_status;  // [npk][max_segments] or null
  uint64_t npk;
  uint64_t now_us;
  uint32_t nconn;
  uint32_t max_segments;
};
hipError_t launch_ack_receive(const AckReceiveArgs& a, hipStream_t s);

hipError_t launch_ack_touch(const AckEntry* table, uint32_t nconn, const uint8_t* flags, hipStream_t s);

struct AckAttachArgs {
  const AckEntry* table;
  const unsigned long long* first_packet;  // [nconn]
  const uint32_t* n_packets;               // [nconn]
  const unsigned long long* total;
  const uint8_t* may_ack_only;             // [nconn] or null
  ugo_pkt_info* info;                      // [max_packets]
  uint64_t* ranges;                        // [max_packets][max_ranges][2]
  uint32_t* conn_of;                       // [max_packets]
  unsigned long long* total_out;
  uint8_t* attached;                       // [nconn]
  uint32_t* slot_local;   // [nconn]: a member's rank among its scan block's ACK-only candidates
  uint64_t* block_slots;  // [kAckScanBlock]: candidates per scan block, then their exclusive scan
  uint64_t* total_in;     // one word: *total as the call found it (total_out may alias total)
  uint64_t now_us;
  uint64_t max_packets;
  uint32_t nconn;
  uint32_t max_ranges;
};
hipError_t launch_ack_attach(const AckAttachArgs& a, hipStream_t s);

hipError_t launch_ack_gather(const AckEntry* table, uint32_t nconn, ugo_ack_state* out, hipStream_t s);

}  // namespace kern
}  // namespace ugo
