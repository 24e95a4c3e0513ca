// loop_args.hpp -- the host half of the connection loop (include/ugo_loop.h)
// that needs no device: the argument rules of every ugo_fec_loop_* entry point
// and the reference defaults.  Kept apart from ugo_loop.cpp as host/cc_args.hpp is.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../loop_kernels.hpp"
#include "sent_args.hpp"

namespace ugo {
namespace loopargs {

using sentargs::aligned;

// ackSendDelay, initialIdleConnectionStateLifetime and maxRetriesAttempted of ugo/constants.go.
inline ugo_loop_params defaults() { return ugo_loop_params{5000, 300000000, 10, 0}; }

inline bool params_ok(const ugo_loop_params& p) { return p.idle_us >= 1; }

inline bool nconn_ok(size_t rx, size_t ack, size_t tx, size_t sent) {
  return rx >= 1 && rx <= kern::kLoopSetMaxConn && rx == ack && rx == tx && rx == sent;
}

// After create: last_activity_us = now_us, everything else zero.
inline ugo_loop_state initial(uint64_t now_us) {
  ugo_loop_state s{};
  s.last_activity_us = now_us;
  return s;
}

inline bool receive_ok(const void* info, const void* conn_of, size_t npackets) {
  return info && conn_of && aligned(info, 16) && aligned(conn_of, 4) && npackets <= (size_t(1) << 31);
}

inline bool close_ok(const void* how, const void* linger_us) { return how && aligned(linger_us, 8); }

inline bool check_ok(const void* budget, const void* may_ack_only) {
  return budget && may_ack_only && aligned(budget, 4);
}

inline bool append_ok(const void* total, size_t max_packets, const void* info, const void* segs, size_t max_segments,
                      const void* conn_of, const void* total_out, const void* appended) {
  return total && info && segs && conn_of && total_out && appended && aligned(total, 8) && aligned(info, 16) &&
         aligned(segs, 8) && aligned(conn_of, 4) && aligned(total_out, 8) && max_segments >= 1 &&
         max_segments <= 0xffff && max_packets <= (size_t(1) << 31);
}

inline bool sent_ok(const void* n_packets, const void* attached, const void* delay_us, const void* deadline_us,
                    const void* exits, const void* reasons, size_t max_exits, const void* n_exits,
                    const void* new_index, const void* nconn_new) {
  return n_packets && attached && deadline_us && n_exits && aligned(n_packets, 4) && aligned(delay_us, 8) &&
         aligned(deadline_us, 8) && aligned(n_exits, 8) && (max_exits == 0 || (exits && reasons)) &&
         aligned(exits, 4) && (new_index != nullptr) == (nconn_new != nullptr) && aligned(new_index, 4) &&
         aligned(nconn_new, 8);
}

}  // namespace loopargs
}  // namespace ugo
