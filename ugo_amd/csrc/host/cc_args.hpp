// cc_args.hpp -- the host half of congestion control (include/ugo_cc.h) that
// needs no device: the argument rules of every ugo_fec_cc_* entry point and the
// reference defaults.  Kept apart from ugo_cc.cpp as host/sent_args.hpp is.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../cc_kernels.hpp"
#include "sent_args.hpp"

namespace ugo {
namespace ccargs {

using sentargs::aligned;

// initialCongestionWindow and defaultMaxCongestionWindow of ugo/constants.go,
// defaultMinimumCongestionWindow, defaultNumConnections and defaultTCPMSS of ugo/congestion/.
inline ugo_cc_params defaults() { return ugo_cc_params{32, 200, 2, 2, 1460}; }

inline bool params_ok(const ugo_cc_params& p) {
  return p.min_cwnd >= 1 && p.min_cwnd <= p.initial_cwnd && p.initial_cwnd <= p.max_cwnd &&
         p.max_cwnd <= UGO_CC_MAX_CWND_LIMIT && p.num_connections >= 1 && p.mss >= 1;
}

// After create: cwnd = initial_cwnd, ssthresh = max_cwnd, everything else zero.
inline ugo_cc_state initial(const ugo_cc_params& p) {
  ugo_cc_state s{};
  s.cwnd = p.initial_cwnd;
  s.ssthresh = p.max_cwnd;
  return s;
}

inline bool sent_ack_ok(const void* info, const void* ranges, size_t max_ranges, const void* conn_of, size_t npackets,
                        const void* events, const void* split, const void* rows) {
  return sentargs::ack_ok(info, ranges, max_ranges, conn_of, npackets, events) && split && rows &&
         aligned(split, 8) && aligned(rows, 16);
}

inline bool ack_ok(const void* events, const void* rows, const void* delay_us) {
  return events && rows && delay_us && aligned(events, 16) && aligned(rows, 16) && aligned(delay_us, 8);
}

inline bool rto_ok(const void* fired, size_t packet_bytes, size_t max_budget, const void* budget) {
  return fired && budget && aligned(budget, 4) && packet_bytes >= 1 && max_budget <= (size_t(1) << 31);
}

}  // namespace ccargs
}  // namespace ugo
