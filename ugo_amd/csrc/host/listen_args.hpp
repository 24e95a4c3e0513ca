// listen_args.hpp -- the host half of the connection table (include/ugo_listen.h)
// that needs no device: the argument rules of every ugo_fec_listen_* entry point
// and the slot count.  Kept apart from ugo_listen.cpp as host/cc_args.hpp is.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../listen_kernels.hpp"
#include "sent_args.hpp"

namespace ugo {
namespace listenargs {

using sentargs::aligned;

constexpr size_t kMaxPackets = size_t(1) << 31;

inline bool max_conn_ok(size_t max_conn) { return max_conn >= 1 && max_conn <= UGO_LISTEN_MAX_CONN; }

// max(16, the power of two >= 2 * max_conn): at most half the slots hold
// members, the rest is room for the dead ones of deviation (b).
inline uint32_t slots_for(size_t max_conn) {
  uint32_t n = 16;
  while (n < 2 * max_conn) n *= 2;
  return n;
}

// The ring under the decoder's rules (ugo_fec_packet_decode).
inline bool ring_ok(const void* pkts, size_t slot, const void* lens) {
  return pkts && lens && slot != 0 && slot % 16 == 0 && slot <= 0xffff && aligned(pkts, 16) && aligned(lens, 2);
}

inline bool route_ok(const void* names, const void* pkts, size_t slot, const void* lens, size_t npackets,
                     const void* conn_of, const void* cls, const void* accepted, size_t max_accepted,
                     const void* n_accepted) {
  return names && aligned(names, 16) && ring_ok(pkts, slot, lens) && npackets <= kMaxPackets && conn_of &&
         aligned(conn_of, 4) && cls && n_accepted && aligned(n_accepted, 4) && (max_accepted == 0 || accepted) &&
         aligned(accepted, 16) && max_accepted <= kMaxPackets;
}

inline bool remap_ok(const void* new_index, size_t n_index, size_t nconn_new, const void* status) {
  (void)nconn_new;  // a count past max_conn is the device's to report, in *status
  return (n_index == 0 || new_index) && aligned(new_index, 4) && n_index <= UGO_LISTEN_MAX_CONN && status &&
         aligned(status, 4);
}

inline bool names_ok(const void* conn_of, size_t npackets, const void* names_out, const void* name_lens) {
  return conn_of && aligned(conn_of, 4) && npackets <= kMaxPackets && names_out && aligned(names_out, 16) &&
         name_lens && aligned(name_lens, 4);
}

inline bool entries_ok(const void* out, size_t cap) {
  return out && aligned(out, 16) && cap >= 1 && cap <= UGO_LISTEN_MAX_CONN;
}

}  // namespace listenargs
}  // namespace ugo
