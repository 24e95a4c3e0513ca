// stream_tx_kernels.hpp -- internal interface of the send windows and
// send-window sets (ugo_fec_stream_tx_*, include/ugo_stream.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/ugo_stream.h"

namespace ugo {
namespace kern {

// The device record of a send window is the public struct itself.
typedef ugo_stream_tx_state StreamTxRecord;

// One member of a set, uploaded once by ugo_fec_stream_tx_set_create (40 bytes).
struct StreamTxEntry {
  uint8_t* win;                 // cap bytes; stream byte x at win[x & (cap - 1)]
  ugo_stream_tx_rq_entry* rq;   // rq_cap entries; the queue is rq[(rq_head + k) % rq_cap], k < rq_len
  StreamTxRecord* rec;
  uint64_t cap;
  uint32_t rq_cap;
  uint32_t reserved;
};

constexpr uint32_t kTxSetMaxConn = 1u << 20;
constexpr uint32_t kTxScanBlock = 1024;  // connections per block of the two scans
constexpr uint32_t kTxHeader = 4;        // frameHeaderLen of segment_sender.go

// Per-connection scratch of one plan call (device, owned by the set).
struct StreamTxPlanScratch {
  uint64_t budget_start;  // exclusive sum of budget[] within the scan block
  uint64_t first;         // exclusive sum of n_packets[] within the scan block
  uint64_t fresh_pos;     // write_pos where the arithmetic packets start
  uint64_t fresh_pending; // tail - fresh_pos
  uint64_t fresh_pn;      // packet number of the last packet before them
  uint32_t n_packets;
  uint32_t n_queue;       // packets that drew from the retransmission queue (written by the per-connection pass)
  uint32_t budget_eff;    // the clamped budget
  uint32_t reserved;
};

struct StreamTxWriteArgs {
  const StreamTxEntry* table;
  const uint8_t* src;
  const uint64_t* src_off;     // [nconn]
  const uint64_t* n;           // [nconn]
  unsigned long long* n_written;  // [nconn]
  uint32_t nconn;
  uint32_t wblocks;  // blocks per connection
};
hipError_t launch_stream_tx_write(const StreamTxWriteArgs& a, hipStream_t s);

hipError_t launch_stream_tx_release(const StreamTxEntry* table, uint32_t nconn, const uint64_t* upto, hipStream_t s);

struct StreamTxRetransmitArgs {
  const StreamTxEntry* table;
  const uint32_t* conn_of;  // [m]
  const uint64_t* offset;   // [m]
  const uint32_t* len;      // [m]
  uint8_t* status;          // [m]
  uint32_t* unsorted;       // device scratch, one word
  uint64_t m;
  uint32_t nconn;
};
hipError_t launch_stream_tx_retransmit(const StreamTxRetransmitArgs& a, hipStream_t s);

struct StreamTxPlanArgs {
  const StreamTxEntry* table;
  const uint32_t* budget;  // [nconn]
  ugo_pkt_info* info;      // [max_packets]
  ugo_pkt_segment* segs;   // [max_packets][max_segments]
  uint32_t* conn_of;       // [max_packets]
  unsigned long long* first_packet;  // [nconn]
  uint32_t* n_packets;               // [nconn]
  unsigned long long* total;
  StreamTxPlanScratch* scratch;  // [nconn]
  uint64_t* block_budget;        // [kTxScanBlock]: per scan block, exclusive
  uint64_t* block_first;         // [kTxScanBlock]
  uint64_t* first_dense;         // [nconn]: first_packet[], on the device for the per-packet pass
  uint64_t max_packets;
  uint32_t nconn;
  uint32_t max_payload;
  uint32_t max_segments;
};
hipError_t launch_stream_tx_plan(const StreamTxPlanArgs& a, hipStream_t s);

hipError_t launch_stream_tx_gather(const StreamTxEntry* table, uint32_t nconn, ugo_stream_tx_state* out,
                                   hipStream_t s);

uint32_t stream_tx_wblocks(uint64_t max_cap, uint32_t nconn);

}  // namespace kern
}  // namespace ugo
