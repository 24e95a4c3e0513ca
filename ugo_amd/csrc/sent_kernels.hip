// sent_kernels.hip -- sent histories on gfx950 (include/ugo_sent.h): batch
// packetSender for a set of connections.
//   sentPacket, receivedAck, ackPacket, nackPacket,
//   queuePacketForRetransmission, checkRTO,
//   dequeuePacketForRetransmission                  ugo/packet_sender.go:66-358
//   stopWaitingManager                              ugo/stop_waiting.go
//
// record  five launches:
//           k_sent_rec_first   per packet, k_sent_rec_adopt per member: a
//                              history that has stored nothing starts below
//                              the lowest number of its first packets
//           k_sent_rec_claim   per packet: who takes part; the lowest batch
//                              index that names a number claims its ring entry
//           k_sent_rec_store   per packet: stale / duplicate / error / store
//                              the slot and its segment row
//           k_sent_rec_commit  per member: the call's sums into the record
// ack     five launches, THE RULE's phases:
//           k_sent_ack_scan    per packet: valid, the largest w, the largest
//                              la, and the claim of every candidate la
//           k_sent_ack_marks   per packet: an accepted ACK (it holds its la's
//                              claim) adds +1 / -1 at the ends of what it
//                              acknowledges into its member's difference ring
//           k_sent_ack_sum     per chunk of 1,024 numbers of a member's
//                              [n0, last_sent]: the chunk's sum of the ring
//           k_sent_ack_apply   per chunk: the sums of the chunks before it, a
//                              scan inside it, and acked / nacks for every
//                              slot: free, count missing, queue
//           k_sent_ack_finish  per member: the record, the event row
//         ugo_fec_cc_sent_ack (include/ugo_cc.h) is the same five, apply and
//         finish in a second instantiation that also gathers the member's
//         ugo_cc_row: the highest number lost, the highest freed, and the
//         freed at or below split[c].
//         The time is (ACKs + their rows) + (the members' outstanding spans),
//         never their product, and a member with a long span gets one block
//         per 1,024 numbers of it.  An accepted ACK that acknowledges from the
//         bottom up is counted per member (n_pref) instead of adding to the
//         ring's first entry, which every such ACK would share, and the lanes
//         of a wave that add to one word of the ring add once (wave_add).
// rto     one wave per member.
// drain   six launches: the members' entry counts scanned (two levels, as
//         ugo_fec_ack_set_attach's slots), then per chunk the queued slots'
//         segment counts summed, scanned and written out, per member the
//         record, and the NO_CONN tail.
// attach  one thread per member.
//
// No block waits on another inside a kernel: the phases are launches.  The
// per-packet kernels combine, inside a wave and then inside a block of 1,024,
// what the lanes of one member add, before anything atomic leaves the block.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "sent_device.hpp"
#include "sent_kernels.hpp"

namespace ugo {
namespace kern {

namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kPkBlock = 1024;  // packets per block of the per-packet kernels
constexpr uint32_t kChThreads = 256; // threads of a chunk's block: kSentChunk / 4 numbers each
constexpr uint32_t kChRounds = kSentChunk / kChThreads;

static_assert(sizeof(SentSlot) == 32 && sizeof(SentRecord) == 160 && sizeof(ugo_sent_event) == 64 &&
                  sizeof(SentCall) == 128 && sizeof(SentEntry) == 56 && sizeof(ugo_stream_tx_rq_entry) == 16 &&
                  sizeof(SentCcCall) == 32 && sizeof(ugo_cc_row) == 32,
              "layouts");

// ---------------------------------------------------------------- wave helpers (wave64)
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v |= __shfl_xor(v, d, 64);
  return v;
}

// Inclusive scan of two ints over a block of kChThreads; tot = the block's sums.
__device__ __forceinline__ int2 block_incl2(int a, int b, int2* lds, int2& tot) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int oa = __shfl_up(a, d, 64), ob = __shfl_up(b, d, 64);
    if (lane_id() >= static_cast<uint32_t>(d)) {
      a += oa;
      b += ob;
    }
  }
  const uint32_t w = threadIdx.x >> 6;
  if (lane_id() == 63) lds[w] = make_int2(a, b);
  __syncthreads();
  int2 pre = make_int2(0, 0);
  tot = make_int2(0, 0);
#pragma unroll
  for (uint32_t k = 0; k < kChThreads / 64; ++k) {
    const int2 v = lds[k];
    if (k < w) {
      pre.x += v.x;
      pre.y += v.y;
    }
    tot.x += v.x;
    tot.y += v.y;
  }
  __syncthreads();
  return make_int2(a + pre.x, b + pre.y);
}

// Every lane with a non-null address adds v to it.  The lanes of the wave that
// name one address add their sum once, for the first few addresses: that takes
// the words a connection's ACKs share (one to four values a wave).  What is
// left after that is taken to be distinct and goes lane by lane, which is
// correct either way.  Called by all lanes of the wave.
__device__ __forceinline__ void wave_add(int32_t* addr, int v) {
  u64 todo = __ballot(addr != nullptr);
  for (int round = 0; round < 4 && todo; ++round) {
    const int leader = __ffsll(todo) - 1;
    const u64 la = __shfl(reinterpret_cast<u64>(addr), leader, 64);
    const bool same = addr != nullptr && reinterpret_cast<u64>(addr) == la;
    const u64 grp = __ballot(same);
    if (static_cast<int>(lane_id()) == leader) atomicAdd(addr, v * static_cast<int>(__popcll(grp)));
    if (same) addr = nullptr;
    todo &= ~grp;
  }
  if (addr != nullptr) atomicAdd(addr, v);
}

// The first number a member's scans look at: nothing occupied lies below it.
// set_ack starts no higher than lio + 1: a gap in the stored numbers can leave
// scan_from above it, and an accepted la (> lio) may lie in that gap -- its
// claim and the ends of its intervals must be inside the span that is scanned
// and cleared.  Either way the span [start, last_sent] has at most ws numbers.
__device__ __forceinline__ u64 scan_start(const SentRecord& r, uint32_t ws, bool for_ack) {
  const u64 w = r.last_sent >= ws ? r.last_sent - ws + 1 : 1;
  u64 from = r.scan_from;
  if (for_ack && r.lio + 1 < from) from = r.lio + 1;
  return from > w ? from : w;
}

__device__ __forceinline__ bool in_flight(const SentSlot& s, u64 n) {
  return s.packet_number == n && s.state == UGO_SENT_IN_FLIGHT;
}

// ---------------------------------------------------------------- record
// kind of packet i: 0 no part, 1 stale, 2 past the window, 3 inside it.
__device__ __forceinline__ uint32_t rec_kind(const SentRecordArgs& a, u64 i, uint32_t& c, const SentEntry*& e, u64& n,
                                             u64x2& tail) {
  c = a.conn_of[i];
  if (c >= a.nconn || a.status[i] != 0 || a.wire_lens[i] == 0) return 0;
  const u64x2* rec = reinterpret_cast<const u64x2*>(a.info + i);
  n = rec[0].x;
  if (n == 0) return 0;
  tail = {rec[0].y, rec[3].x};  // stop_waiting | n_ranges, n_segments, flags
  e = a.table + c;
  const SentRecord* r = e->rec;
  if (r->err) return 0;
  const u64 lio = r->lio;
  if (n <= lio) return 1;
  return n - lio > e->ws ? 2u : 3u;
}

// A history that has stored nothing adopts the lowest number of its first
// packets: lio = that number - 1 (a connection need not start at 1).
__global__ __launch_bounds__(256) void k_sent_rec_first(SentRecordArgs a) {
  const u64 i = blockIdx.x * 256ull + threadIdx.x;
  uint32_t c = 0;
  u64 inv = 0;
  const SentEntry* e = nullptr;
  if (i < a.npk) {
    c = a.conn_of[i];
    if (c < a.nconn && a.status[i] == 0 && a.wire_lens[i] != 0) {
      e = a.table + c;
      const SentRecord* r = e->rec;
      const u64 n = a.info[i].packet_number;
      if (n != 0 && !r->err && r->last_sent == 0 && r->lio == 0) inv = ~n;
    }
  }
  u64 act = __ballot(inv != 0);
  while (act) {  // per member of the wave: one atomicMax
    const int leader = __ffsll(act) - 1;
    const uint32_t cl = __shfl(c, leader, 64);
    const bool mine = inv != 0 && c == cl;
    const u64 grp = __ballot(mine);
    u64 m = mine ? inv : 0;
    if (grp & (grp - 1)) m = wave_max(m);
    if (static_cast<int>(lane_id()) == leader) atomicMax(&a.call[cl].first_inflight_inv, m);
    act &= ~grp;
  }
}

__global__ __launch_bounds__(256) void k_sent_rec_adopt(SentRecordArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  const u64 inv = a.call[c].first_inflight_inv;
  if (inv == 0) return;
  SentRecord* r = a.table[c].rec;
  r->lio = ~inv - 1;
  r->least_unacked = ~inv;
  r->scan_from = ~inv;
  a.call[c].first_inflight_inv = 0;
}

// A plan names a number once, so the claims of a wave go to 64 addresses; the
// copies of a number (a caller's mistake) are not combined first.
__global__ __launch_bounds__(256) void k_sent_rec_claim(SentRecordArgs a) {
  const u64 i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= a.npk) return;
  uint32_t c;
  const SentEntry* e;
  u64 n;
  u64x2 tail;
  if (rec_kind(a, i, c, e, n, tail) == 3)
    atomicMax(e->claim + (static_cast<uint32_t>(n) & (e->ws - 1u)), ~static_cast<uint32_t>(i));
}

__global__ __launch_bounds__(kPkBlock) void k_sent_rec_store(SentRecordArgs a) {
  __shared__ uint32_t blk_key, blk_stale, blk_dup, blk_stored, blk_flags;
  __shared__ u64 blk_bytes, blk_max;
  const u64 i = blockIdx.x * static_cast<u64>(kPkBlock) + threadIdx.x;
  if (threadIdx.x == 0) {
    blk_stale = blk_dup = blk_stored = blk_flags = 0;
    blk_bytes = blk_max = 0;
    blk_key = a.conn_of[i];  // i < npk: the grid has no empty block
  }
  __syncthreads();
  // what: 0 nothing, 1 stale, 2 duplicate, 3 stored, 4 error
  uint32_t what = 0, c = 0, len = 0;
  u64 n = 0;
  if (i < a.npk) {
    const SentEntry* e;
    u64x2 tail;
    const uint32_t kind = rec_kind(a, i, c, e, n, tail);
    if (kind == 1) {
      what = 1;
    } else if (kind == 2) {
      what = 4;
    } else if (kind == 3) {
      const uint32_t pos = static_cast<uint32_t>(n) & (e->ws - 1u);
      SentSlot* slot = e->slots + pos;
      const bool winner = e->claim[pos] == ~static_cast<uint32_t>(i);
      const u64 held = *reinterpret_cast<volatile u64*>(&slot->packet_number);
      if (held != 0 && held != n) {
        what = 4;
      } else if (!winner || held == n) {
        what = 2;
      } else {
        what = 3;
        len = a.wire_lens[i];
        uint32_t ns = static_cast<uint32_t>(tail.y >> 16) & 0xffffu;
        if (ns > a.max_segments) ns = a.max_segments;  // <= seg_cap: an argument rule
        const ugo_pkt_segment* src = a.segs + i * a.max_segments;
        ugo_stream_tx_rq_entry* row = e->segs + static_cast<u64>(pos) * e->seg_cap;
        u64 lowest = ~0ull;
        for (uint32_t j = 0; j < e->seg_cap; ++j) {
          ugo_stream_tx_rq_entry q{};
          if (j < ns) {
            q.offset = src[j].offset;
            q.len = src[j].len;
            lowest = q.offset < lowest ? q.offset : lowest;
          }
          row[j] = q;
        }
        SentSlot s{};
        s.packet_number = n;
        s.sent_us = a.now_us;
        s.min_offset = lowest;
        s.len = len;
        s.state = UGO_SENT_IN_FLIGHT;
        s.n_segments = static_cast<uint8_t>(ns);
        s.bits = static_cast<uint8_t>((((tail.y >> 32) & 0x80u) ? 0x80u : 0u) | (tail.x ? 0x40u : 0u));
        *slot = s;
      }
      if (winner) e->claim[pos] = 0;  // the others compare with their own index: 0 is as good as the winner's
    }
  }
  u64 act = __ballot(what != 0);
  while (act) {
    const int leader = __ffsll(act) - 1;
    const uint32_t cl = __shfl(c, leader, 64);
    const bool mine = what != 0 && c == cl;
    const u64 grp = __ballot(mine);
    const uint32_t n_stale = __popcll(__ballot(mine && what == 1)), n_dup = __popcll(__ballot(mine && what == 2)),
                   n_st = __popcll(__ballot(mine && what == 3));
    const bool any_err = __ballot(mine && what == 4) != 0;
    u64 by = mine && what == 3 ? len : 0, mx = mine && what == 3 ? n : 0;
    if (grp & (grp - 1)) {
      by = wave_sum64(by);
      mx = wave_max(mx);
    }
    if (static_cast<int>(lane_id()) == leader) {
      const bool in_lds = cl == blk_key;
      SentCall* k = a.call + cl;
      if (n_stale) atomicAdd(in_lds ? &blk_stale : &k->stale, n_stale);
      if (n_dup) atomicAdd(in_lds ? &blk_dup : &k->dup, n_dup);
      if (n_st) {
        atomicAdd(in_lds ? &blk_stored : &k->stored, n_st);
        atomicAdd(in_lds ? &blk_bytes : &k->bytes, by);
        atomicMax(in_lds ? &blk_max : &k->max_n, mx);
      }
      if (any_err) atomicOr(in_lds ? &blk_flags : &k->flags, kCallErr);
    }
    act &= ~grp;
  }
  __syncthreads();
  if (threadIdx.x == 0 && (blk_stale | blk_dup | blk_stored | blk_flags)) {  // then blk_key is a member
    SentCall* k = a.call + blk_key;
    if (blk_stale) atomicAdd(&k->stale, blk_stale);
    if (blk_dup) atomicAdd(&k->dup, blk_dup);
    if (blk_stored) {
      atomicAdd(&k->stored, blk_stored);
      atomicAdd(&k->bytes, blk_bytes);
      atomicMax(&k->max_n, blk_max);
    }
    if (blk_flags) atomicOr(&k->flags, blk_flags);
  }
}

__global__ __launch_bounds__(256) void k_sent_rec_commit(SentRecordArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  const SentCall k = a.call[c];
  if (!(k.stale | k.dup | k.stored | k.flags)) return;
  SentRecord* r = a.table[c].rec;
  if (k.stale) r->stale += k.stale;
  if (k.dup) r->duplicates += k.dup;
  if (k.stored) {
    r->bytes_in_flight += k.bytes;
    r->tracked += k.stored;
    if (k.max_n > r->last_sent) r->last_sent = k.max_n;
    r->last_sent_us = a.now_us;
  }
  if (k.flags & kCallErr) r->err = UGO_SENT_TOO_MANY_TRACKED;
  a.call[c] = SentCall{};
}

// ---------------------------------------------------------------- ack, per packet
struct AckPk {
  const SentEntry* e;
  u64 la, lio_a, w, delay;
  uint32_t c, nr, pos;
  bool carries, valid, unsent, cand;
};

__device__ __forceinline__ AckPk ack_classify(const SentAckArgs& a, u64 i) {
  AckPk p{};
  const u64x2* rec = reinterpret_cast<const u64x2*>(a.info + i);
  const u64x2 q2 = rec[2], q3 = rec[3];  // delay_us, status | n_ranges, n_segments, flags ..
  p.c = a.conn_of[i];
  if (static_cast<uint32_t>(q2.y) != UGO_PKT_OK || !((q3.x >> 32) & 0x80u) || p.c >= a.nconn) return p;
  p.e = a.table + p.c;
  const SentRecord* r = p.e->rec;
  if (r->err) return p;
  p.carries = true;
  const u64x2 q0 = rec[0], q1 = rec[1];
  p.w = q0.x;
  p.la = q1.x;
  p.lio_a = q1.y;
  p.delay = q2.x;
  p.nr = static_cast<uint32_t>(q3.x) & 0xffffu;
  if (p.nr > a.max_ranges) p.nr = a.max_ranges;
  if (p.la > r->last_sent) {
    p.unsent = true;
    return p;
  }
  if (p.w != 0 && p.w <= r->largest_with_ack) return p;
  p.valid = true;
  const u64 thr = r->largest_acked > r->lio ? r->largest_acked : r->lio;
  p.cand = p.la > thr;  // then la is in (lio, last_sent]: one ring entry per value
  p.pos = static_cast<uint32_t>(p.la) & (p.e->ws - 1u);
  return p;
}

__global__ __launch_bounds__(kPkBlock) void k_sent_ack_scan(SentAckArgs a) {
  __shared__ uint32_t blk_key, blk_unsent;
  __shared__ u64 blk_w, blk_la;
  const u64 i = blockIdx.x * static_cast<u64>(kPkBlock) + threadIdx.x;
  if (threadIdx.x == 0) {
    blk_unsent = 0;
    blk_w = blk_la = 0;
    blk_key = a.conn_of[i];
  }
  __syncthreads();
  AckPk p{};
  if (i < a.npk) p = ack_classify(a, i);
  const bool part = p.valid || p.unsent;
  u64 act = __ballot(part);
  while (act) {
    const int leader = __ffsll(act) - 1;
    const uint32_t cl = __shfl(p.c, leader, 64);
    const bool mine = part && p.c == cl;
    const u64 grp = __ballot(mine);
    const uint32_t n_uns = __popcll(__ballot(mine && p.unsent));
    u64 w = mine && p.valid ? p.w : 0, la = mine && p.cand ? p.la : 0;
    if (grp & (grp - 1)) {
      w = wave_max(w);
      la = wave_max(la);
    }
    // per ring entry of this member: the lowest lane has the lowest index
    u64 cands = __ballot(mine && p.cand);
    while (cands) {
      const int l2 = __ffsll(cands) - 1;
      const uint32_t pl = __shfl(p.pos, l2, 64);
      const u64 g2 = __ballot(mine && p.cand && p.pos == pl);
      if (static_cast<int>(lane_id()) == l2) atomicMax(p.e->claim + pl, ~static_cast<uint32_t>(i));
      cands &= ~g2;
    }
    if (static_cast<int>(lane_id()) == leader) {
      const bool in_lds = cl == blk_key;
      SentCall* k = a.call + cl;
      if (n_uns) atomicAdd(in_lds ? &blk_unsent : &k->unsent, n_uns);
      if (w) atomicMax(in_lds ? &blk_w : &k->w_max, w);
      if (la) atomicMax(in_lds ? &blk_la : &k->max_n, la);
    }
    act &= ~grp;
  }
  __syncthreads();
  if (threadIdx.x == 0 && (blk_unsent || blk_w || blk_la)) {
    SentCall* k = a.call + blk_key;
    if (blk_unsent) atomicAdd(&k->unsent, blk_unsent);
    if (blk_w) atomicMax(&k->w_max, blk_w);
    if (blk_la) atomicMax(&k->max_n, blk_la);
  }
}

__global__ __launch_bounds__(kPkBlock) void k_sent_ack_marks(SentAckArgs a) {
  __shared__ uint32_t blk_key, blk_acc, blk_pref;
  const u64 i = blockIdx.x * static_cast<u64>(kPkBlock) + threadIdx.x;
  if (threadIdx.x == 0) {
    blk_acc = blk_pref = 0;
    blk_key = a.conn_of[i];
  }
  __syncthreads();
  AckPk p{};
  if (i < a.npk) p = ack_classify(a, i);
  // An accepted ACK holds its la's claim.  The lanes of a wave walk their rows
  // in step, and the lanes that add to one word of a difference ring add once:
  // the ACKs of one connection share lio_a, the {lio, lio} row and the older
  // holes, and with a SACK on every packet those would be same-address atomics
  // by the hundred thousand.
  const bool acc = p.cand && p.e->claim[p.pos] == ~static_cast<uint32_t>(i);
  bool pref = false;
  uint32_t mask = 0, nr = 0;
  int32_t* diff = nullptr;
  const uint64_t* row = nullptr;
  u64 n0 = 0, lam = 0, minf = 0;
  if (acc) {
    mask = p.e->ws - 1u;
    diff = p.e->diff;
    n0 = scan_start(*p.e->rec, p.e->ws, true);  // n0 <= every occupied number and every candidate la
    lam = a.call[p.c].max_n;                     // la <= lam
    nr = p.nr;
    row = a.ranges + i * a.max_ranges * 2u;
    minf = p.la + 1;
  }
  const uint32_t nr_max = static_cast<uint32_t>(wave_max(nr));
  for (uint32_t k = 0; k < nr_max; ++k) {
    int32_t *up = nullptr, *down = nullptr;
    if (acc && k < nr && minf != 0) {
      const u64 f = row[2u * k], l = row[2u * k + 1u];
      const u64 hi = l < minf - 1 ? l : minf - 1, lo = f > n0 ? f : n0;
      if (lo <= hi) {  // n0 <= lo <= hi <= la <= lam: inside the ring's span
        up = diff + (static_cast<uint32_t>(lo) & mask);
        if (hi < lam) down = diff + (static_cast<uint32_t>(hi + 1) & mask);
      }
      if (f < minf) minf = f;
    }
    wave_add(up, 1);
    wave_add(down, -1);
  }
  {
    int32_t* down = nullptr;
    if (acc) {
      const bool has_pref = nr == 0 || minf != 0;
      const u64 pref_hi = nr == 0 ? p.la : (p.lio_a < minf - 1 ? p.lio_a : minf - 1);
      if (has_pref && pref_hi >= n0) {  // [n0, pref_hi]: counted per member, its end in the ring
        pref = true;
        if (pref_hi < lam) down = diff + (static_cast<uint32_t>(pref_hi + 1) & mask);
      }
    }
    wave_add(down, -1);
  }
  u64 act = __ballot(acc);
  while (act) {
    const int leader = __ffsll(act) - 1;
    const uint32_t cl = __shfl(p.c, leader, 64);
    const bool mine = acc && p.c == cl;
    const u64 grp = __ballot(mine);
    const uint32_t n_acc = __popcll(grp), n_pref = __popcll(__ballot(mine && pref));
    if (static_cast<int>(lane_id()) == leader) {
      const bool in_lds = cl == blk_key;
      atomicAdd(in_lds ? &blk_acc : &a.call[cl].n_acc, n_acc);
      if (n_pref) atomicAdd(in_lds ? &blk_pref : &a.call[cl].n_pref, n_pref);
    }
    act &= ~grp;
  }
  __syncthreads();
  if (threadIdx.x == 0 && blk_acc) {
    atomicAdd(&a.call[blk_key].n_acc, blk_acc);
    if (blk_pref) atomicAdd(&a.call[blk_key].n_pref, blk_pref);
  }
}

// ---------------------------------------------------------------- ack, per chunk
// Chunk b of the grid is chunk b - chunk_base of its member: the numbers
// [n0 + 1024 (b - chunk_base), ...] up to last_sent.  false: nothing there.
__device__ __forceinline__ bool chunk_geo(const SentEntry& e, const SentRecord& r, uint32_t b, bool for_ack, u64& first,
                                          u64& last) {
  const u64 n0 = scan_start(r, e.ws, for_ack);
  first = n0 + static_cast<u64>(b - e.chunk_base) * kSentChunk;
  last = r.last_sent;
  return first <= last;
}

__global__ __launch_bounds__(kChThreads) void k_sent_ack_sum(SentAckArgs a) {
  __shared__ int2 lds[kChThreads / 64];
  const uint32_t b = blockIdx.x, c = a.chunk_member[b];
  const SentCall* k = a.call + c;
  if (k->n_acc == 0) return;
  const SentEntry e = a.table[c];
  u64 first, last;
  if (!chunk_geo(e, *e.rec, b, true, first, last)) return;
  const u64 lam = k->max_n;
  int d = 0, ends = 0;
  for (uint32_t r = 0; r < kChRounds; ++r) {
    const u64 n = first + r * kChThreads + threadIdx.x;
    if (n <= lam) {
      const uint32_t pos = static_cast<uint32_t>(n) & (e.ws - 1u);
      d += e.diff[pos];
      ends += e.claim[pos] != 0;
    }
  }
  int2 tot;
  block_incl2(d, ends, lds, tot);
  if (threadIdx.x == 0) a.chunk_sum[b] = tot;
}

struct ChunkAcc {  // a block's sums before they leave it
  u64 bytes, acked_bytes, lost_bytes, first_inv, low_inv, upto_inv;
  uint32_t acked_pk, lost_pk, lost_segs, qfreed, qfreed_segs, flags;
};

struct CcAcc {  // the same, for what ugo_fec_cc_sent_ack adds (include/ugo_cc.h)
  u64 max_lost, max_acked;
  uint32_t acked_le;
};

// kCc: the body of ugo_fec_cc_sent_ack, which also gathers the member's
// ugo_cc_row; the plain instantiation is the kernel ugo_fec_sent_set_ack had.
template <bool kCc>
__global__ __launch_bounds__(kChThreads) void k_sent_ack_apply(SentAckArgs a) {
  __shared__ int2 lds[kChThreads / 64];
  __shared__ ChunkAcc acc;
  __shared__ CcAcc cacc;
  const uint32_t b = blockIdx.x, c = a.chunk_member[b];
  SentCall* k = a.call + c;
  const uint32_t n_acc = k->n_acc;
  if (n_acc == 0) return;
  const SentEntry e = a.table[c];
  const SentRecord* rec = e.rec;
  u64 first, last;
  if (!chunk_geo(e, *rec, b, true, first, last)) return;
  if (threadIdx.x == 0) acc = ChunkAcc{};
  u64 split = 0;
  CcAcc ct{};
  if constexpr (kCc) {
    if (threadIdx.x == 0) cacc = CcAcc{};
    split = a.split[c];
  }
  const u64 lam = k->max_n, lio0 = rec->lio;
  // the sums of the member's chunks before this one
  int cd = 0, ce = 0;
  for (uint32_t j = e.chunk_base + threadIdx.x; j < b; j += kChThreads) {
    const int2 v = a.chunk_sum[j];
    cd += v.x;
    ce += v.y;
  }
  int2 tot;
  block_incl2(cd, ce, lds, tot);  // its barriers also publish acc
  int run_d = static_cast<int>(k->n_pref) + tot.x, run_e = tot.y;

  ChunkAcc t{};
  for (uint32_t r = 0; r < kChRounds; ++r) {
    const u64 n = first + r * kChThreads + threadIdx.x;
    const uint32_t pos = static_cast<uint32_t>(n) & (e.ws - 1u);
    const bool live = n <= last, marked = n <= lam;
    int d = 0, end = 0;
    uint32_t claim = 0;
    if (marked) {
      d = e.diff[pos];
      claim = e.claim[pos];
      end = claim != 0;
      if (d) e.diff[pos] = 0;
      if (claim) e.claim[pos] = 0;
    }
    const int2 inc = block_incl2(d, end, lds, tot);
    if (live) {
      SentSlot s = e.slots[pos];
      if (s.packet_number == n) {
        bool occupied = true;
        if (marked) {
          const int cnt_ack = run_d + inc.x;                                    // accepted ACKs that acknowledge n
          const int cnt_le = static_cast<int>(n_acc) - (run_e + inc.y - end);  // accepted ACKs with n <= la
          if (n == lam) {  // the RTT sample, before the slot goes
            k->rtt_us = a.now_us > s.sent_us ? a.now_us - s.sent_us : 0;
            const uint32_t src = ~claim;  // lam is accepted: claim holds its ACK's index
            k->delay_us = claim != 0 && src < a.npk ? a.info[src].delay_us : 0;
            t.flags |= kCallRtt;
          }
          if (cnt_ack > 0) {
            occupied = false;
            e.slots[pos] = SentSlot{};
            t.acked_pk++;
            t.acked_bytes += s.len;
            if constexpr (kCc) {
              if (n > ct.max_acked) ct.max_acked = n;
              ct.acked_le += n <= split;
            }
            if (s.state == UGO_SENT_IN_FLIGHT) {
              t.bytes += s.len;
            } else {
              t.qfreed++;
              t.qfreed_segs += s.n_segments;
            }
          } else {
            const int nacks = cnt_le > cnt_ack ? cnt_le - cnt_ack : 0;
            const uint32_t m = s.missing + static_cast<uint32_t>(nacks);
            const uint8_t m8 = static_cast<uint8_t>(m > 255u ? 255u : m);
            const bool lose = m8 > UGO_SENT_RETRANSMIT_THRESHOLD && s.state == UGO_SENT_IN_FLIGHT;
            if (lose) {
              s.state = UGO_SENT_QUEUED;
              t.bytes += s.len;
              t.lost_pk++;
              t.lost_bytes += s.len;
              t.lost_segs += s.n_segments;
              if constexpr (kCc) {
                if (n > ct.max_lost) ct.max_lost = n;
              }
            }
            if (m8 != s.missing || lose) {
              s.missing = m8;
              e.slots[pos].state = s.state;
              e.slots[pos].missing = m8;
            }
          }
        }
        if (occupied) {
          if (~n > t.low_inv) t.low_inv = ~n;
          if (s.state == UGO_SENT_IN_FLIGHT && n > lio0 && ~n > t.first_inv) t.first_inv = ~n;
        }
      }
    }
    run_d += tot.x;
    run_e += tot.y;
  }
  // one value per wave into LDS, one per block out
  t.bytes = wave_sum64(t.bytes);
  t.acked_bytes = wave_sum64(t.acked_bytes);
  t.lost_bytes = wave_sum64(t.lost_bytes);
  t.first_inv = wave_max(t.first_inv);
  t.low_inv = wave_max(t.low_inv);
  t.acked_pk = wave_sum(t.acked_pk);
  t.lost_pk = wave_sum(t.lost_pk);
  t.lost_segs = wave_sum(t.lost_segs);
  t.qfreed = wave_sum(t.qfreed);
  t.qfreed_segs = wave_sum(t.qfreed_segs);
  t.flags = wave_or(t.flags);
  if (lane_id() == 0) {
    if (t.bytes) atomicAdd(&acc.bytes, t.bytes);
    if (t.acked_bytes) atomicAdd(&acc.acked_bytes, t.acked_bytes);
    if (t.lost_bytes) atomicAdd(&acc.lost_bytes, t.lost_bytes);
    if (t.first_inv) atomicMax(&acc.first_inv, t.first_inv);
    if (t.low_inv) atomicMax(&acc.low_inv, t.low_inv);
    if (t.acked_pk) atomicAdd(&acc.acked_pk, t.acked_pk);
    if (t.lost_pk) atomicAdd(&acc.lost_pk, t.lost_pk);
    if (t.lost_segs) atomicAdd(&acc.lost_segs, t.lost_segs);
    if (t.qfreed) atomicAdd(&acc.qfreed, t.qfreed);
    if (t.qfreed_segs) atomicAdd(&acc.qfreed_segs, t.qfreed_segs);
    if (t.flags) atomicOr(&acc.flags, t.flags);
  }
  if constexpr (kCc) {
    ct.max_lost = wave_max(ct.max_lost);
    ct.max_acked = wave_max(ct.max_acked);
    ct.acked_le = wave_sum(ct.acked_le);
    if (lane_id() == 0) {
      if (ct.max_lost) atomicMax(&cacc.max_lost, ct.max_lost);
      if (ct.max_acked) atomicMax(&cacc.max_acked, ct.max_acked);
      if (ct.acked_le) atomicAdd(&cacc.acked_le, ct.acked_le);
    }
  }
  __syncthreads();
  if constexpr (kCc) {
    if (threadIdx.x == 0) {
      SentCcCall* kc = a.cc_call + c;
      if (cacc.max_lost) atomicMax(&kc->max_lost, cacc.max_lost);
      if (cacc.max_acked) atomicMax(&kc->max_acked, cacc.max_acked);
      if (cacc.acked_le) atomicAdd(&kc->acked_le, cacc.acked_le);
    }
  }
  if (threadIdx.x == 0) {
    if (acc.bytes) atomicAdd(&k->bytes, acc.bytes);
    if (acc.acked_bytes) atomicAdd(&k->acked_bytes, acc.acked_bytes);
    if (acc.lost_bytes) atomicAdd(&k->lost_bytes, acc.lost_bytes);
    if (acc.first_inv) atomicMax(&k->first_inflight_inv, acc.first_inv);
    if (acc.low_inv) atomicMax(&k->lowest_occ_inv, acc.low_inv);
    if (acc.acked_pk) atomicAdd(&k->acked_pk, acc.acked_pk);
    if (acc.lost_pk) atomicAdd(&k->lost_pk, acc.lost_pk);
    if (acc.lost_segs) atomicAdd(&k->lost_segs, acc.lost_segs);
    if (acc.qfreed) atomicAdd(&k->qfreed, acc.qfreed);
    if (acc.qfreed_segs) atomicAdd(&k->qfreed_segs, acc.qfreed_segs);
    if (acc.flags) atomicOr(&k->flags, acc.flags);
  }
}

template <bool kCc>
__global__ __launch_bounds__(256) void k_sent_ack_finish(SentAckArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  const SentCall k = a.call[c];
  SentRecord* rec = a.table[c].rec;
  ugo_sent_event ev{};
  if constexpr (kCc) {  // the member's row, whole; all zero with no accepted ACK
    ugo_cc_row row{};
    if (k.n_acc) {
      const SentCcCall kc = a.cc_call[c];
      row.max_lost = kc.max_lost;
      row.max_acked = kc.max_acked;
      row.acked_le = kc.acked_le;
      if (kc.max_lost | kc.max_acked) a.cc_call[c] = SentCcCall{};
    }
    a.rows[c] = row;
  }
  if (k.unsent) rec->unsent_acks += k.unsent;
  if (k.w_max > rec->largest_with_ack) rec->largest_with_ack = k.w_max;
  if (k.n_acc) {
    SentRecord r = *rec;
    r.largest_acked = k.max_n;
    ev.accepted = 1;
    if (k.flags & kCallRtt) {
      ev.has_rtt = 1;
      ev.rtt_us = k.rtt_us;
      ev.delay_us = k.delay_us;
      r.rto_count = 0;
    }
    ev.acked_packets = k.acked_pk;
    ev.acked_bytes = k.acked_bytes;
    ev.lost_packets = k.lost_pk;
    ev.lost_bytes = k.lost_bytes;
    r.acked_packets += k.acked_pk;
    r.acked_bytes += k.acked_bytes;
    r.lost_packets += k.lost_pk;
    r.lost_bytes += k.lost_bytes;
    r.bytes_in_flight -= k.bytes;
    r.tracked -= k.acked_pk;
    r.queued += k.lost_pk - k.qfreed;
    r.queued_segments += k.lost_segs - k.qfreed_segs;
    if (k.lost_pk) r.sw_pending = 1;
    r.lio = k.first_inflight_inv ? ~k.first_inflight_inv - 1 : r.last_sent;
    r.least_unacked = r.lio + 1;
    r.scan_from = k.lowest_occ_inv ? ~k.lowest_occ_inv : r.last_sent + 1;
    *rec = r;
  }
  ev.bytes_in_flight = rec->bytes_in_flight;
  ev.largest_acked = rec->largest_acked;
  a.events[c] = ev;
  if (k.unsent | k.n_acc || k.w_max || k.max_n) a.call[c] = SentCall{};
}

// ---------------------------------------------------------------- rto (one wave per member)
__global__ __launch_bounds__(256) void k_sent_rto(SentRtoArgs a) {
  const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (c >= a.nconn) return;
  const SentEntry e = a.table[c];
  SentRecord* rec = e.rec;
  bool due = false;
  if (!rec->err && rec->last_sent_us != 0) {
    const u64 rto = sent_rto_us(a.delay_us[c], rec->rto_count);
    const u64 at = rec->last_sent_us + rto;
    due = at >= rto && a.now_us >= at;  // a deadline past 2^64 never comes
  }
  // the first two in-flight numbers of (lio, last_sent]: the one to queue, and where lio stops
  const u64 last = rec->last_sent;
  u64 f1 = 0, f2 = 0;
  if (due) {
    for (u64 base = rec->lio + 1; base <= last && f2 == 0; base += 64) {
      const u64 n = base + lane_id();
      bool hit = false;
      if (n <= last) hit = in_flight(e.slots[static_cast<uint32_t>(n) & (e.ws - 1u)], n);
      u64 m = __ballot(hit);
      if (m && f1 == 0) {
        f1 = base + (__ffsll(m) - 1);
        m &= m - 1;
      }
      if (m) f2 = base + (__ffsll(m) - 1);
      if (last - base < 64) break;  // base + 64 may wrap
    }
  }
  if (lane_id() != 0) return;
  if (f1 == 0) {
    a.fired[c] = 0;
    return;
  }
  SentSlot* s = e.slots + (static_cast<uint32_t>(f1) & (e.ws - 1u));
  s->state = UGO_SENT_QUEUED;
  rec->bytes_in_flight -= s->len;
  rec->lost_packets += 1;
  rec->lost_bytes += s->len;
  rec->queued += 1;
  rec->queued_segments += s->n_segments;
  rec->sw_pending = 1;
  rec->lio = f2 ? f2 - 1 : last;
  rec->least_unacked = rec->lio + 1;
  rec->last_sent_us = a.now_us;
  rec->rto_count += 1;
  a.fired[c] = 1;
}

// ---------------------------------------------------------------- drain
__device__ __forceinline__ u64 drain_count(const SentRecord& r) { return r.err ? 0u : r.queued_segments; }

__global__ __launch_bounds__(kSentScanBlock) void k_sent_drain_scan_members(SentDrainArgs a) {
  __shared__ uint32_t wave_tot[kSentScanBlock / 64];
  const uint32_t c = blockIdx.x * kSentScanBlock + threadIdx.x;
  const uint32_t v = c < a.nconn ? static_cast<uint32_t>(drain_count(*a.table[c].rec)) : 0u;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane_id() >= static_cast<uint32_t>(d)) incl += o;
  }
  const uint32_t w = threadIdx.x >> 6;
  if (lane_id() == 63) wave_tot[w] = incl;
  __syncthreads();
  u64 before = 0, total = 0;
  for (uint32_t k = 0; k < kSentScanBlock / 64; ++k) {
    if (k < w) before += wave_tot[k];
    total += wave_tot[k];
  }
  // a block's entries fit 32 bits: 1,024 members of at most 2^20 slots of at most 16 segments do not,
  // but a sum past 2^32 - 1 is past max_entries <= 2^31 as well: saturate
  const u64 sl = before + incl - v;
  if (c < a.nconn) a.start_local[c] = sl > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(sl);
  if (threadIdx.x == 0) a.block_start[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSentScanBlock) void k_sent_drain_scan_blocks(SentDrainArgs a, uint32_t n) {
  __shared__ u64 s[kSentScanBlock];
  const uint32_t t = threadIdx.x;
  const u64 v = t < n ? a.block_start[t] : 0;
  s[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kSentScanBlock; d <<= 1) {
    const u64 add = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  if (t < n) a.block_start[t] = s[t] - v;
  if (t == 0) *a.n_written = 0;
}

// Does member c drain, and from which entry?
__device__ __forceinline__ bool drains(const SentDrainArgs& a, uint32_t c, const SentRecord& r, u64& start) {
  start = a.block_start[c / kSentScanBlock] + a.start_local[c];
  return !r.err && r.queued != 0 && start + r.queued_segments <= a.max_entries;
}

__global__ __launch_bounds__(kChThreads) void k_sent_drain_sum(SentDrainArgs a) {
  __shared__ int2 lds[kChThreads / 64];
  const uint32_t b = blockIdx.x, c = a.chunk_member[b];
  const SentEntry e = a.table[c];
  const SentRecord* rec = e.rec;
  u64 start, first, last;
  if (!drains(a, c, *rec, start) || !chunk_geo(e, *rec, b, false, first, last)) return;
  int segs = 0;
  for (uint32_t r = 0; r < kChRounds; ++r) {
    const u64 n = first + r * kChThreads + threadIdx.x;
    if (n <= last) {
      const SentSlot s = e.slots[static_cast<uint32_t>(n) & (e.ws - 1u)];
      if (s.packet_number == n && s.state == UGO_SENT_QUEUED) segs += s.n_segments;
    }
  }
  int2 tot;
  block_incl2(segs, 0, lds, tot);
  if (threadIdx.x == 0) a.chunk_sum[b] = tot;
}

__global__ __launch_bounds__(kChThreads) void k_sent_drain_apply(SentDrainArgs a) {
  __shared__ int2 lds[kChThreads / 64];
  __shared__ ChunkAcc acc;
  const uint32_t b = blockIdx.x, c = a.chunk_member[b];
  const SentEntry e = a.table[c];
  const SentRecord* rec = e.rec;
  u64 start, first, last;
  if (rec->err || !chunk_geo(e, *rec, b, false, first, last)) return;
  const bool dr = drains(a, c, *rec, start);
  if (threadIdx.x == 0) acc = ChunkAcc{};
  int cs = 0;
  if (dr)
    for (uint32_t j = e.chunk_base + threadIdx.x; j < b; j += kChThreads) cs += a.chunk_sum[j].x;
  int2 tot;
  block_incl2(cs, 0, lds, tot);
  u64 run = start + static_cast<u64>(static_cast<uint32_t>(tot.x));

  ChunkAcc t{};
  for (uint32_t r = 0; r < kChRounds; ++r) {
    const u64 n = first + r * kChThreads + threadIdx.x;
    const uint32_t pos = static_cast<uint32_t>(n) & (e.ws - 1u);
    SentSlot s{};
    bool occ = false, out = false;
    if (n <= last) {
      s = e.slots[pos];
      occ = s.packet_number == n;
      out = occ && dr && s.state == UGO_SENT_QUEUED;
    }
    const int mine = out ? s.n_segments : 0;
    const int2 inc = block_incl2(mine, 0, lds, tot);
    if (out) {
      const ugo_stream_tx_rq_entry* row = e.segs + static_cast<u64>(pos) * e.seg_cap;
      u64 at = run + static_cast<u64>(static_cast<uint32_t>(inc.x - mine));
      for (int j = 0; j < mine && j < static_cast<int>(e.seg_cap); ++j, ++at) {
        if (at >= a.max_entries) break;  // never: start + queued_segments <= max_entries
        a.conn_of[at] = c;
        a.offset[at] = row[j].offset;
        a.len[at] = row[j].len;
      }
      e.slots[pos] = SentSlot{};
      t.qfreed++;
      if (s.bits & 0x80u) t.flags |= kCallTouch;
      if (s.bits & 0x40u) t.flags |= kCallStop;
    } else if (occ) {
      if (~n > t.low_inv) t.low_inv = ~n;
      if (~s.min_offset > t.upto_inv) t.upto_inv = ~s.min_offset;
    }
    run += static_cast<u64>(static_cast<uint32_t>(tot.x));
  }
  t.low_inv = wave_max(t.low_inv);
  t.upto_inv = wave_max(t.upto_inv);
  t.qfreed = wave_sum(t.qfreed);
  t.flags = wave_or(t.flags);
  if (lane_id() == 0) {
    if (t.low_inv) atomicMax(&acc.low_inv, t.low_inv);
    if (t.upto_inv) atomicMax(&acc.upto_inv, t.upto_inv);
    if (t.qfreed) atomicAdd(&acc.qfreed, t.qfreed);
    if (t.flags) atomicOr(&acc.flags, t.flags);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    SentCall* k = a.call + c;
    if (acc.low_inv) atomicMax(&k->lowest_occ_inv, acc.low_inv);
    if (acc.upto_inv) atomicMax(&k->upto_inv, acc.upto_inv);
    if (acc.qfreed) atomicAdd(&k->qfreed, acc.qfreed);
    if (acc.flags) atomicOr(&k->flags, acc.flags);
  }
}

__global__ __launch_bounds__(256) void k_sent_drain_finish(SentDrainArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  SentRecord* rec = a.table[c].rec;
  if (rec->err) {
    a.touch[c] = 0;
    a.upto[c] = 0;
    return;
  }
  const SentCall k = a.call[c];
  u64 start;
  if (drains(a, c, *rec, start)) {
    atomicMax(a.n_written, start + rec->queued_segments);
    rec->tracked -= k.qfreed;
    rec->queued = 0;
    rec->queued_segments = 0;
    if (k.flags & kCallStop) rec->sw_pending = 1;
  }
  const u64 low = k.lowest_occ_inv ? ~k.lowest_occ_inv : rec->last_sent + 1;
  if (rec->scan_from != low) rec->scan_from = low;
  a.touch[c] = (k.flags & kCallTouch) ? 1 : 0;
  a.upto[c] = ~k.upto_inv;
  if (k.lowest_occ_inv | k.upto_inv | k.qfreed | k.flags) a.call[c] = SentCall{};
}

__global__ __launch_bounds__(256) void k_sent_drain_tail(SentDrainArgs a) {
  const u64 j = blockIdx.x * 256ull + threadIdx.x;
  const u64 n = *a.n_written;
  if (j == 0) *a.n_entries = n;
  if (j >= n && j < a.max_entries) a.conn_of[j] = UGO_STREAM_NO_CONN;
}

// ---------------------------------------------------------------- attach, gather
__global__ __launch_bounds__(256) void k_sent_attach(SentAttachArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  SentRecord* rec = a.table[c].rec;
  uint8_t did = 0;
  if (rec->sw_pending && !rec->err && a.n_packets[c] > 0) {
    const u64 t = a.first_packet[c];
    if (t < a.max_packets) {
      a.info[t].stop_waiting = rec->least_unacked;
      rec->sw_pending = 0;
      did = 1;
    }
  }
  a.attached[c] = did;
}

__global__ __launch_bounds__(256) void k_sent_gather(const SentEntry* table, uint32_t nconn, ugo_sent_state* out) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c < nconn) out[c] = *table[c].rec;
}

}  // namespace

hipError_t launch_sent_record(const SentRecordArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const dim3 per_packet(static_cast<uint32_t>((a.npk + 255u) / 256u)), per_member((a.nconn + 255u) / 256u);
  launch(kKSent, k_sent_rec_first, per_packet, dim3(256), 0, s, a);
  launch(kKSent, k_sent_rec_adopt, per_member, dim3(256), 0, s, a);
  launch(kKSent, k_sent_rec_claim, per_packet, dim3(256), 0, s, a);
  launch(kKSent, k_sent_rec_store, dim3(static_cast<uint32_t>((a.npk + kPkBlock - 1u) / kPkBlock)), dim3(kPkBlock), 0,
         s, a);
  launch(kKSent, k_sent_rec_commit, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sent_ack(const SentAckArgs& a, hipStream_t s) {
  const bool cc = a.rows != nullptr;
  const uint32_t kid = cc ? kKCc : kKSent;
  if (a.npk != 0) {
    const dim3 per_packet(static_cast<uint32_t>((a.npk + kPkBlock - 1u) / kPkBlock));
    launch(kid, k_sent_ack_scan, per_packet, dim3(kPkBlock), 0, s, a);
    launch(kid, k_sent_ack_marks, per_packet, dim3(kPkBlock), 0, s, a);
    launch(kid, k_sent_ack_sum, dim3(a.nchunks), dim3(kChThreads), 0, s, a);
    launch(kid, cc ? k_sent_ack_apply<true> : k_sent_ack_apply<false>, dim3(a.nchunks), dim3(kChThreads), 0, s, a);
  }
  launch(kid, cc ? k_sent_ack_finish<true> : k_sent_ack_finish<false>, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s,
         a);
  return hipGetLastError();
}

hipError_t launch_sent_rto(const SentRtoArgs& a, hipStream_t s) {
  launch(kKSent, k_sent_rto, dim3((a.nconn + 3u) / 4u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sent_drain(const SentDrainArgs& a, hipStream_t s) {
  const uint32_t sblocks = (a.nconn + kSentScanBlock - 1) / kSentScanBlock;  // <= kSentScanBlock
  launch(kKSent, k_sent_drain_scan_members, dim3(sblocks), dim3(kSentScanBlock), 0, s, a);
  launch(kKSent, k_sent_drain_scan_blocks, dim3(1), dim3(kSentScanBlock), 0, s, a, sblocks);
  launch(kKSent, k_sent_drain_sum, dim3(a.nchunks), dim3(kChThreads), 0, s, a);
  launch(kKSent, k_sent_drain_apply, dim3(a.nchunks), dim3(kChThreads), 0, s, a);
  launch(kKSent, k_sent_drain_finish, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s, a);
  const uint64_t tail = a.max_entries ? a.max_entries : 1;
  launch(kKSent, k_sent_drain_tail, dim3(static_cast<uint32_t>((tail + 255u) / 256u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sent_attach(const SentAttachArgs& a, hipStream_t s) {
  launch(kKSent, k_sent_attach, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sent_gather(const SentEntry* table, uint32_t nconn, ugo_sent_state* out, hipStream_t s) {
  launch(kKSent, k_sent_gather, dim3((nconn + 255u) / 256u), dim3(256), 0, s, table, nconn, out);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
