// ack_args.hpp -- the host half of the receive histories (include/ugo_ack.h)
// that needs no device: the argument rules of every ugo_fec_ack_* entry point
// and the build of a set's member table.  Kept apart from ugo_ack.cpp so that
// a stand-alone program can run it under a sanitizer (tools/ack_args_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../ack_kernels.hpp"
#include "member_list.hpp"

namespace ugo {
namespace ackargs {

inline bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

inline bool window_ok(size_t window_packets) {
  return window_packets >= UGO_ACK_MIN_WINDOW && window_packets <= UGO_ACK_MAX_WINDOW &&
         (window_packets & (window_packets - 1)) == 0;
}

// What a set needs to know of a member: its device memory and its context.
struct Member {
  const void* ctx;
  uint64_t* bits;
  kern::AckRecord* rec;
  size_t window_packets;
};

// The rules of ugo_fec_ack_set_create; members[i] null for a NULL handle.
inline bool members_ok(const void* ctx, const Member* const* members, size_t nconn) {
  // (a history listed twice would be advanced twice)
  if (nconn > kern::kAckSetMaxConn || !ugo::members::list_ok(ctx, members, nconn)) return false;
  for (size_t i = 0; i < nconn; ++i)
    if (!window_ok(members[i]->window_packets)) return false;
  return true;
}

// One table entry per member, in set order.
inline std::vector<kern::AckEntry> build_table(const Member* const* members, size_t nconn) {
  std::vector<kern::AckEntry> t(nconn);
  for (size_t i = 0; i < nconn; ++i) {
    t[i].bits = members[i]->bits;
    t[i].rec = members[i]->rec;
    t[i].wp = static_cast<uint32_t>(members[i]->window_packets);
    t[i].reserved = 0;
  }
  return t;
}

inline bool receive_ok(const void* info, const void* conn_of, size_t npackets, const void* seg_status,
                       size_t max_segments) {
  return info && conn_of && aligned(info, 16) && aligned(conn_of, 4) && npackets <= (size_t(1) << 31) &&
         max_segments <= 0xffff && !(seg_status && max_segments == 0);
}

inline bool attach_ok(const void* first_packet, const void* n_packets, const void* total, size_t max_packets,
                      const void* info, const void* ranges, size_t max_ranges, const void* conn_of,
                      const void* total_out, const void* attached) {
  return first_packet && n_packets && total && total_out && attached && aligned(first_packet, 8) &&
         aligned(n_packets, 4) && aligned(total, 8) && aligned(total_out, 8) && max_packets <= (size_t(1) << 31) &&
         max_ranges <= 0xffff && !(max_packets && (!info || !conn_of)) && !(max_packets && max_ranges && !ranges) &&
         aligned(info, 16) && aligned(ranges, 8) && aligned(conn_of, 4);
}

}  // namespace ackargs
}  // namespace ugo
