// stream_set_kernels.hpp -- internal interface of stream delivery for a set of
// receive windows (ugo_fec_stream_set_*, include/ugo_stream.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "stream_kernels.hpp"

namespace ugo {
namespace kern {

// One member of a set, uploaded once by ugo_fec_stream_set_create (56 bytes).
struct StreamSetEntry {
  uint8_t* win;  // cap bytes
  unsigned long long* C;  // cap / 64 words each
  unsigned long long* S;
  unsigned long long* claim;
  unsigned long long* cont;
  StreamRecord* rec;
  uint64_t cap;
};

constexpr uint32_t kSetMaxConn = 1u << 20;

struct StreamSetArgs {
  const uint8_t* pkts;  // packet i at pkts + i*slot (16-B aligned)
  const uint8_t* pad;   // nullable keystream, >= slot bytes
  const ugo_pkt_info* info;
  const ugo_pkt_segment* segs;  // [npk][max_segments]
  uint8_t* seg_status;          // [npk][max_segments]
  const uint32_t* conn_of;      // [npk]: index into table, or anything >= nconn for "no connection"
  const StreamSetEntry* table;  // [nconn]
  uint64_t npk;
  uint64_t slot;
  uint32_t nconn;
  uint32_t max_segments;
  uint32_t wblocks;  // blocks per connection of the bitmap passes, from the largest member window
};

hipError_t launch_stream_set_deliver(const StreamSetArgs& a, hipStream_t s);

struct StreamSetReadArgs {
  const StreamSetEntry* table;  // [nconn]
  uint8_t* dst;                 // nullable: discard
  const uint64_t* dst_off;      // [nconn], unused without dst
  const uint64_t* n;            // [nconn]
  unsigned long long* n_read;   // [nconn]
  uint8_t* eof;                 // [nconn], nullable
  uint32_t nconn;
  uint32_t rblocks;  // blocks per connection, from the largest member window
};

hipError_t launch_stream_set_read(const StreamSetReadArgs& a, hipStream_t s);

// out[c] = the public record of member c
hipError_t launch_stream_set_gather(const StreamSetEntry* table, uint32_t nconn, ugo_stream_rx_state* out,
                                    hipStream_t s);

// the per-connection grid sizes for a largest member window of max_cap bytes
uint32_t stream_set_wblocks(uint64_t max_cap);
uint32_t stream_set_rblocks(uint64_t max_cap, uint32_t nconn);

}  // namespace kern
}  // namespace ugo
