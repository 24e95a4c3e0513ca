// sent_kernels.hpp -- internal interface of the sent histories and their sets
// (ugo_fec_sent_*, include/ugo_sent.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

#include "../../include/ugo_cc.h"
#include "../../include/ugo_sent.h"

namespace ugo {
namespace kern {

// The device forms of a slot and of the record are the public structs.
typedef ugo_sent_slot SentSlot;
typedef ugo_sent_state SentRecord;

constexpr uint32_t kSentSetMaxConn = 1u << 20;
constexpr uint32_t kSentChunk = 1024;      // numbers per block of the per-member scans (= UGO_SENT_MIN_WINDOW)
constexpr uint32_t kSentScanBlock = 1024;  // members per block of drain's scan over the members
constexpr uint32_t kKSent = 13;            // UGO_FEC_KERNEL_SENT
constexpr uint32_t kKCc = 14;              // UGO_FEC_KERNEL_CC

// One member of a set, uploaded once by ugo_fec_sent_set_create (56 bytes).
struct SentEntry {
  SentSlot* slots;               // [ws]
  ugo_stream_tx_rq_entry* segs;  // [ws][seg_cap]
  int32_t* diff;                 // [ws], zero between calls: the difference ring of set_ack
  uint32_t* claim;               // [ws], zero between calls: ~index of the lowest batch index that names a number
  SentRecord* rec;
  uint32_t ws;
  uint32_t seg_cap;
  uint32_t chunk_base;  // the member's first chunk: chunks [chunk_base, chunk_base + ws / kSentChunk)
  uint32_t reserved;
};

// What the passes of one call gather for a member (device, owned by the set,
// all zero between calls: the call's last pass clears it).  128 bytes.
struct SentCall {
  unsigned long long bytes;        // record: stored bytes
  unsigned long long max_n;        // record: the highest stored number; ack: the highest accepted la
  unsigned long long w_max;        // ack: the highest valid w
  unsigned long long acked_bytes;  // ack
  unsigned long long lost_bytes;   // ack
  unsigned long long first_inflight_inv;  // ack: ~ of the lowest in-flight number above lio, 0 = none
  unsigned long long lowest_occ_inv;      // ack, drain: ~ of the lowest number still occupied, 0 = none
  unsigned long long upto_inv;            // drain: ~ of the lowest min_offset still occupied, 0 = none
  unsigned long long rtt_us, delay_us;    // ack: the sample
  uint32_t stale, dup, stored;     // record
  uint32_t unsent, n_acc, n_pref;  // ack: accepted ACKs, and those of them that acknowledge from the bottom up
  uint32_t acked_pk, lost_pk, lost_segs;
  uint32_t qfreed, qfreed_segs;    // ack: queued slots an ACK freed; drain: slots drained
  uint32_t flags;                  // kCall* bits
};
constexpr uint32_t kCallErr = 1, kCallRtt = 2, kCallTouch = 4, kCallStop = 8;

// What ugo_fec_cc_sent_ack gathers beside SentCall (device, owned by the set,
// all zero between calls; the plain set_ack never touches it).  32 bytes.
struct SentCcCall {
  unsigned long long max_lost;   // the highest number the call declared lost
  unsigned long long max_acked;  // the highest number whose slot the call freed
  uint32_t acked_le;             // freed slots with n <= split[c]
  uint32_t reserved[3];
};

struct SentRecordArgs {
  const SentEntry* table;
  SentCall* call;  // [nconn]
  const ugo_pkt_info* info;
  const ugo_pkt_segment* segs;
  const uint32_t* conn_of;
  const uint16_t* wire_lens;
  const uint8_t* status;
  uint64_t npk;
  uint64_t now_us;
  uint32_t nconn;
  uint32_t max_segments;
};
hipError_t launch_sent_record(const SentRecordArgs& a, hipStream_t s);

struct SentAckArgs {
  const SentEntry* table;
  SentCall* call;                  // [nconn]
  const uint32_t* chunk_member;    // [nchunks]
  int2* chunk_sum;                 // [nchunks]
  const ugo_pkt_info* info;
  const uint64_t* ranges;
  const uint32_t* conn_of;
  ugo_sent_event* events;          // [nconn]
  // ugo_fec_cc_sent_ack only (include/ugo_cc.h); null in ugo_fec_sent_set_ack
  SentCcCall* cc_call;             // [nconn]
  const unsigned long long* split; // [nconn]
  ugo_cc_row* rows;                // [nconn]
  uint64_t npk;
  uint64_t now_us;
  uint32_t nconn;
  uint32_t max_ranges;
  uint32_t nchunks;
};
// rows != nullptr: the cc form, whose launches report as UGO_FEC_KERNEL_CC.
hipError_t launch_sent_ack(const SentAckArgs& a, hipStream_t s);

struct SentRtoArgs {
  const SentEntry* table;
  const unsigned long long* delay_us;
  uint8_t* fired;
  uint64_t now_us;
  uint32_t nconn;
};
hipError_t launch_sent_rto(const SentRtoArgs& a, hipStream_t s);

struct SentDrainArgs {
  const SentEntry* table;
  SentCall* call;
  const uint32_t* chunk_member;
  int2* chunk_sum;
  uint32_t* start_local;   // [nconn]: a member's start inside its scan block
  uint64_t* block_start;   // [kSentScanBlock]: entries per scan block, then their exclusive scan
  unsigned long long* n_written;  // one word: the end of the last member that drains
  uint32_t* conn_of;
  uint64_t* offset;
  uint32_t* len;
  unsigned long long* n_entries;
  uint8_t* touch;
  uint64_t* upto;
  uint64_t max_entries;
  uint32_t nconn;
  uint32_t nchunks;
};
hipError_t launch_sent_drain(const SentDrainArgs& a, hipStream_t s);

struct SentAttachArgs {
  const SentEntry* table;
  const unsigned long long* first_packet;
  const uint32_t* n_packets;
  ugo_pkt_info* info;
  uint8_t* attached;
  uint64_t max_packets;
  uint32_t nconn;
};
hipError_t launch_sent_attach(const SentAttachArgs& a, hipStream_t s);

hipError_t launch_sent_gather(const SentEntry* table, uint32_t nconn, ugo_sent_state* out, hipStream_t s);

}  // namespace kern
}  // namespace ugo
