// sent_args.hpp -- the host half of the sent histories (include/ugo_sent.h)
// that needs no device: the argument rules of every ugo_fec_sent_* entry point,
// the layout of a history's device block and the build of a set's member and
// chunk tables.  Kept apart from ugo_sent.cpp so that a stand-alone program can
// run it under a sanitizer (tools/sent_args_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../sent_kernels.hpp"
#include "member_list.hpp"

namespace ugo {
namespace sentargs {

inline bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

inline bool window_ok(size_t window_packets) {
  return window_packets >= UGO_SENT_MIN_WINDOW && window_packets <= UGO_SENT_MAX_WINDOW &&
         (window_packets & (window_packets - 1)) == 0;
}

inline bool seg_cap_ok(size_t seg_cap) { return seg_cap >= 1 && seg_cap <= UGO_SENT_MAX_SEG_CAP; }

// A history is one device block: record | slots | segment rows | difference ring | claim ring.
struct Layout {
  size_t rec, slots, segs, diff, claim, bytes;
};
constexpr size_t kRecordRoom = 256;  // the record's share of the block: keeps the slots 32-B aligned

inline Layout layout(size_t ws, size_t seg_cap) {
  Layout l{};
  l.rec = 0;
  l.slots = kRecordRoom;
  l.segs = l.slots + ws * sizeof(kern::SentSlot);
  l.diff = l.segs + ws * seg_cap * sizeof(ugo_stream_tx_rq_entry);
  l.claim = l.diff + ws * sizeof(int32_t);
  l.bytes = l.claim + ws * sizeof(uint32_t);
  return l;
}

// What a set needs to know of a member: its device block and its context.
struct Member {
  const void* ctx;
  unsigned char* block;
  size_t window_packets;
  size_t seg_cap;
};

// The rules of ugo_fec_sent_set_create; members[i] null for a NULL handle.
inline bool members_ok(const void* ctx, const Member* const* members, size_t nconn) {
  // (a history listed twice would be advanced twice)
  if (nconn > kern::kSentSetMaxConn || !ugo::members::list_ok(ctx, members, nconn)) return false;
  uint64_t chunks = 0;
  for (size_t i = 0; i < nconn; ++i) {
    if (!members[i]->block || !window_ok(members[i]->window_packets) || !seg_cap_ok(members[i]->seg_cap)) return false;
    chunks += members[i]->window_packets / kern::kSentChunk;
  }
  return chunks <= (uint64_t(1) << 30);  // one block per chunk in a grid
}

// One table entry per member, in set order, and the member of every chunk.
inline std::vector<kern::SentEntry> build_table(const Member* const* members, size_t nconn,
                                                std::vector<uint32_t>& chunk_member, size_t& min_seg_cap) {
  std::vector<kern::SentEntry> t(nconn);
  chunk_member.clear();
  min_seg_cap = UGO_SENT_MAX_SEG_CAP;
  for (size_t i = 0; i < nconn; ++i) {
    const Member& m = *members[i];
    const Layout l = layout(m.window_packets, m.seg_cap);
    t[i].rec = reinterpret_cast<kern::SentRecord*>(m.block + l.rec);
    t[i].slots = reinterpret_cast<kern::SentSlot*>(m.block + l.slots);
    t[i].segs = reinterpret_cast<ugo_stream_tx_rq_entry*>(m.block + l.segs);
    t[i].diff = reinterpret_cast<int32_t*>(m.block + l.diff);
    t[i].claim = reinterpret_cast<uint32_t*>(m.block + l.claim);
    t[i].ws = static_cast<uint32_t>(m.window_packets);
    t[i].seg_cap = static_cast<uint32_t>(m.seg_cap);
    t[i].chunk_base = static_cast<uint32_t>(chunk_member.size());
    t[i].reserved = 0;
    chunk_member.insert(chunk_member.end(), m.window_packets / kern::kSentChunk, static_cast<uint32_t>(i));
    min_seg_cap = std::min(min_seg_cap, m.seg_cap);
  }
  return t;
}

inline bool record_ok(const void* info, const void* segs, size_t max_segments, size_t min_seg_cap,
                      const void* conn_of, const void* wire_lens, const void* status, size_t npackets) {
  return info && segs && conn_of && wire_lens && status && aligned(info, 16) && aligned(segs, 16) &&
         aligned(conn_of, 4) && aligned(wire_lens, 2) && npackets <= (size_t(1) << 31) && max_segments >= 1 &&
         max_segments <= min_seg_cap;
}

inline bool ack_ok(const void* info, const void* ranges, size_t max_ranges, const void* conn_of, size_t npackets,
                   const void* events) {
  return events && aligned(events, 8) && npackets <= (size_t(1) << 31) && max_ranges <= 0xffff &&
         !(npackets && (!info || !conn_of)) && !(npackets && max_ranges && !ranges) && aligned(info, 16) &&
         aligned(ranges, 8) && aligned(conn_of, 4);
}

inline bool rto_ok(const void* delay_us, const void* fired) { return delay_us && fired && aligned(delay_us, 8); }

inline bool drain_ok(size_t max_entries, const void* conn_of, const void* offset, const void* len,
                     const void* n_entries, const void* touch, const void* upto) {
  return n_entries && touch && upto && aligned(n_entries, 8) && aligned(upto, 8) &&
         max_entries <= (size_t(1) << 31) && !(max_entries && (!conn_of || !offset || !len)) && aligned(conn_of, 4) &&
         aligned(offset, 8) && aligned(len, 4);
}

inline bool attach_ok(const void* first_packet, const void* n_packets, size_t max_packets, const void* info,
                      const void* attached) {
  return first_packet && n_packets && attached && aligned(first_packet, 8) && aligned(n_packets, 4) &&
         max_packets <= (size_t(1) << 31) && !(max_packets && !info) && aligned(info, 16);
}

}  // namespace sentargs
}  // namespace ugo
