// stream_kernels.hpp -- internal interface of stream delivery (include/ugo_stream.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/ugo_stream.h"

namespace ugo {
namespace kern {

// The connection's record on the device: the public mirror first, then what
// the kernels of one call hand to each other.  Between calls the scratch
// fields hold their idle values (stream_record_init).
struct StreamRecord {
  ugo_stream_rx_state pub;
  unsigned long long fatal_idx;  // arrival index (packet * max_segments + segment) of this call's fatal segment, or ~0
  unsigned long long scan_u;     // summary: lowest uncovered position found in [read_pos, hi), or ~0
  unsigned long long scan_head;  // read: 1 + highest start bit in the bytes read, or 0
  unsigned long long claim_end[64];  // highest end a segment of this call claimed up to (maximum over the words), or 0
  uint32_t scan_runs;            // summary: uncovered runs of [read_pos, hi)
  uint32_t n_contested;          // segments left to the ordered pass
  uint32_t accepted_data;        // this call accepted a non-empty segment
  uint32_t inert;                // err was set before this call: nothing is processed
  uint32_t ticket;               // read: blocks that have finished
  uint32_t touched;              // set calls only: a packet of this call belongs here (idle: 0)
};

void stream_record_init(StreamRecord* host);

struct StreamArgs {
  const uint8_t* pkts;  // packet i at pkts + i*slot (16-B aligned)
  const uint8_t* pad;   // nullable keystream, >= slot bytes
  const ugo_pkt_info* info;
  const ugo_pkt_segment* segs;  // [npk][max_segments]
  uint8_t* seg_status;          // [npk][max_segments]
  uint8_t* win;                 // cap bytes
  unsigned long long* C;        // cap / 64 words each
  unsigned long long* S;
  unsigned long long* claim;
  unsigned long long* cont;
  StreamRecord* rec;
  uint64_t npk;
  uint64_t slot;
  uint64_t cap;
  uint32_t max_segments;
};

hipError_t launch_stream_deliver(const StreamArgs& a, hipStream_t s);

struct StreamReadArgs {
  const uint8_t* win;
  unsigned long long* C;
  unsigned long long* S;
  StreamRecord* rec;
  uint8_t* dst;                // nullable: discard
  unsigned long long* n_read;
  uint8_t* eof;                // nullable
  uint64_t n;
  uint64_t cap;
};

hipError_t launch_stream_read(const StreamReadArgs& a, hipStream_t s);

}  // namespace kern
}  // namespace ugo
