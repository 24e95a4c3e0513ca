// ack_kernels.hip -- receive histories on gfx950 (include/ugo_ack.h): batch
// packetReceiver.receivedPacket / receivedStopWaiting and buildSack for a set
// of connections.
//   receivedPacket, receivedStopWaiting, buildSack   ugo/packet_receiver.go:39-163
//   recvHistory                                      ugo/recv_history.go:24-117
//
// receive  four launches, THE RULE's phases.  A number above lio_old + Wp
//          would alias a bit the floor has yet to clear, so the floor is down
//          before a bit is placed:
//            k_ack_scan_packets  per packet: who takes part, the largest
//                                stop-waiting per member
//            k_ack_floor         one wave per member: ipb, lio, bits <= lio cleared
//            k_ack_place         per packet: old / out of window / set the bit
//            k_ack_advance       one wave per member: lio over the set bits,
//                                outstanding recounted, the record committed
//          The per-packet kernels combine, inside a wave, the lanes that name
//          the same member (and the same bitmap word) before anything atomic:
//          one atomicMax per member and one 64-bit atomicOr per word per wave
//          -- with one connection and in-order traffic a whole wave lands on
//          one or two words of the member's bitmap.  No counter is added to
//          per wave either, or every wave of a one-connection grid would add
//          to the same words: fresh and lo are read off the bitmap by the
//          advance pass (its population before and after, its highest bit),
//          and old / out_of_window of the member a block of k_ack_place
//          begins with are summed in LDS and added once per block (DESIGN
//          §3.10 has the measurements).
// attach   three launches: the members that need an ACK-only slot are counted
//          per block of 1,024 and those counts scanned (k_tx_scan_budget /
//          k_tx_scan_blocks' two levels), then one wave per member walks its
//          bitmap from lo downwards and writes the range rows highest first.
//
// The bitmap as a member's wave reads it: "logical bit" i is packet number
// lio + 1 + i, ring bit (lio + 1 + i) & (Wp - 1); logical chunk j is the 64
// logical bits from 64 j, put together from two ring words.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ack_kernels.hpp"
#include "launch.hpp"

namespace ugo {
namespace kern {

namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kAckPlaceBlock = 1024;  // packets per block of k_ack_place: one add per counter and block
constexpr uint32_t kAckDepth = 8;          // bitmap words a lane of a per-member wave loads before it uses one

static_assert(sizeof(AckRecord) == 64 && sizeof(ugo_pkt_info) == 64 && sizeof(AckCall) == 24, "layouts");

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

__device__ __forceinline__ u64 wave_or(u64 v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v |= __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// exclusive prefix sum over the lanes, lane 0 first
__device__ __forceinline__ uint32_t wave_excl(uint32_t v, uint32_t& total) {
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane_id() >= static_cast<uint32_t>(d)) incl += o;
  }
  total = __shfl(incl, 63, 64);
  return incl - v;
}

// The bits of ring word wi (bits [64 wi, 64 wi + 64)) inside the linear range [a, e).
__device__ __forceinline__ u64 lin_mask(uint32_t wi, uint32_t a, uint32_t e) {
  const uint32_t B = wi * 64u;
  const uint32_t lo = a > B ? a : B, hi = e < B + 64u ? e : B + 64u;
  if (hi <= lo) return 0;
  const uint32_t n = hi - lo;
  return (n == 64u ? ~0ull : ((1ull << n) - 1ull)) << (lo - B);
}

// The bits of ring word wi inside the circular range of `count` (< wp) bits from ring bit s.
__device__ __forceinline__ u64 ring_mask(uint32_t wi, uint32_t s, uint32_t count, uint32_t wp) {
  const uint32_t e = s + count;  // <= 2 wp - 1: no overflow for wp <= 2^20
  return e <= wp ? lin_mask(wi, s, e) : (lin_mask(wi, s, wp) | lin_mask(wi, 0, e - wp));
}

// Logical chunk j of the stream that starts at ring bit p0.
__device__ __forceinline__ u64 load_chunk(const uint64_t* bits, uint32_t nwords, uint32_t p0, uint32_t j) {
  const uint32_t w0 = ((p0 >> 6) + j) & (nwords - 1u), sh = p0 & 63u;
  const u64 a = bits[w0];
  if (sh == 0) return a;
  const u64 b = bits[(w0 + 1u) & (nwords - 1u)];
  return (a >> sh) | (b << (64u - sh));
}

// Logical bit i of that stream, 0 outside [0, wp).
__device__ __forceinline__ u64 load_bit(const uint64_t* bits, uint32_t wp, uint32_t p0, int64_t i) {
  if (i < 0 || i >= static_cast<int64_t>(wp)) return 0;
  const uint32_t p = (p0 + static_cast<uint32_t>(i)) & (wp - 1u);
  return (bits[p >> 6] >> (p & 63u)) & 1ull;
}

// One wave: clear the `count` (<= wp) ring bits from s, return the set bits
// left and, in `top`, one more than the highest of them counted from ring bit
// s + count (0 if none is left): lio + top is the largest number recorded.
__device__ uint32_t clear_and_count(uint64_t* bits, uint32_t wp, uint32_t s, uint32_t count, uint32_t& top) {
  const uint32_t nwords = wp >> 6;
  const uint32_t o = (s + count) & (wp - 1u), ow = o >> 6, osh = o & 63u;  // the new origin
  uint32_t left = 0, hi = 0;
  // one wave walks a window of up to 128 KiB: kAckDepth loads in flight per lane
  for (uint32_t base = lane_id(); base < nwords; base += 64u * kAckDepth) {
    u64 w[kAckDepth];
#pragma unroll
    for (uint32_t u = 0; u < kAckDepth; ++u) {
      const uint32_t wi = base + 64u * u;
      w[u] = wi < nwords ? bits[wi] : 0;
    }
#pragma unroll
    for (uint32_t u = 0; u < kAckDepth; ++u) {
      const uint32_t wi = base + 64u * u;
      if (wi >= nwords) continue;
      const u64 m = count >= wp ? ~0ull : ring_mask(wi, s, count, wp);
      const u64 nw = w[u] & ~m;
      if (nw != w[u]) bits[wi] = nw;
      left += __popcll(nw);
      if (nw) {
        // the origin's own word holds the window's top in its bits below the origin
        const u64 low = wi == ow ? nw & ((1ull << osh) - 1ull) : 0;
        const uint32_t b = 63u - static_cast<uint32_t>(__clzll(low ? low : nw));
        const uint32_t at = ((wi * 64u + b - o) & (wp - 1u)) + 1u;
        hi = at > hi ? at : hi;
      }
    }
  }
  top = static_cast<uint32_t>(wave_max(hi));
  return wave_sum(left);
}

// ---------------------------------------------------------------- receive, per packet
// What THE RULE's four tests make of packet i: 0 = no part, 1 = takes part,
// 2 = fails the seg_status test only.  c is its member when the result is not 0.
__device__ __forceinline__ uint32_t take_part(const AckReceiveArgs& a, u64 i, const u64x2& tail, uint32_t& c,
                                              const AckEntry*& e, u64& lio) {
  // info[i] bytes [32, 64): delay_us | status, payload_off | n_ranges, n_segments, flags ...
  const uint32_t status = static_cast<uint32_t>(tail.x);
  c = a.conn_of[i];
  if (status != UGO_PKT_OK || c >= a.nconn) return 0;
  e = a.table + c;
  const u64x2* rec = reinterpret_cast<const u64x2*>(e->rec);
  const u64x2 head = rec[0], last = rec[3];  // lio, lo | out_of_window, {outstanding, changed, err}
  if ((last.y >> 40) & 0xffu) return 0;       // err: the member is inert
  lio = head.x;
  if (a.seg_status) {
    uint32_t ns = static_cast<uint32_t>(tail.y >> 16) & 0xffffu;
    if (ns > a.max_segments) ns = a.max_segments;
    const uint8_t* st = a.seg_status + i * a.max_segments;
    for (uint32_t j = 0; j < ns; ++j)
      if (st[j] == UGO_STREAM_OUT_OF_WINDOW) return 2;
  }
  return 1;
}

__global__ __launch_bounds__(256) void k_ack_scan_packets(AckReceiveArgs a) {
  const u64 i = blockIdx.x * 256ull + threadIdx.x;
  uint32_t part = 0, c = 0;
  u64 sw = 0;
  if (i < a.npk) {
    const u64x2* rec = reinterpret_cast<const u64x2*>(a.info + i);
    const u64x2 nums = rec[0], tail = {rec[2].y, rec[3].x};  // packet_number, stop_waiting | status.., n_ranges..
    const AckEntry* e;
    u64 lio;
    part = take_part(a, i, tail, c, e, lio);
    sw = part == 1 ? nums.y : 0;
  }
  // per member of the wave: one flag store, one atomicMax
  u64 act = __ballot(part == 1);
  while (act) {
    const int leader = __ffsll(act) - 1;
    const uint32_t cl = __shfl(c, leader, 64);
    const bool mine = part == 1 && c == cl;
    const u64 grp = __ballot(mine);
    u64 m = mine ? sw : 0;
    if (grp & (grp - 1)) m = wave_max(m);
    if (static_cast<int>(lane_id()) == leader) {
      AckCall* k = a.call + cl;
      if (!k->touched) k->touched = 1;  // every writer stores 1; a stale 0 costs one more store
      if (m) atomicMax(&k->sw_max, m);
    }
    act &= ~grp;
  }
}

// old and out_of_window of the member the block's first packet names are
// summed in LDS and added once per block: with one connection every wave of
// the grid would otherwise add to the same two words.  fresh needs no count
// (the advance pass has the bitmap's population before and after).
__global__ __launch_bounds__(kAckPlaceBlock) void k_ack_place(AckReceiveArgs a) {
  __shared__ uint32_t blk_old, blk_oow, blk_key;
  const u64 i = blockIdx.x * static_cast<u64>(kAckPlaceBlock) + threadIdx.x;
  if (threadIdx.x == 0) {
    blk_old = blk_oow = 0;
    blk_key = a.conn_of[i];  // i < npk: the grid has no empty block
  }
  __syncthreads();
  // kind: 0 nothing to count, 1 old, 2 out of window, 3 inside the window
  uint32_t kind = 0, c = 0, word = 0;
  u64 n = 0, bit = 0;
  const AckEntry* e = nullptr;
  if (i < a.npk) {
    const u64x2* rec = reinterpret_cast<const u64x2*>(a.info + i);
    const u64x2 nums = rec[0], tail = {rec[2].y, rec[3].x};
    u64 lio = 0;
    const uint32_t part = take_part(a, i, tail, c, e, lio);
    n = nums.x;
    if (part == 2) {
      kind = 2;
    } else if (part == 1 && n != 0) {
      const uint32_t wp = e->wp;
      if (n <= lio) {
        kind = 1;
      } else if (n - lio > wp) {
        kind = 2;
      } else {
        kind = 3;
        const uint32_t p = static_cast<uint32_t>(n) & (wp - 1u);
        word = p >> 6;
        bit = 1ull << (p & 63u);
      }
    }
  }
  u64 act = __ballot(kind != 0);
  while (act) {
    const int leader = __ffsll(act) - 1;
    const uint32_t cl = __shfl(c, leader, 64);
    const bool mine = kind != 0 && c == cl;
    const u64 grp = __ballot(mine);
    uint32_t n_old = __popcll(__ballot(mine && kind == 1));
    const uint32_t n_oow = __popcll(__ballot(mine && kind == 2));
    u64 inw = __ballot(mine && kind == 3);
    // per bitmap word of this member: one atomicOr
    while (inw) {
      const int l2 = __ffsll(inw) - 1;
      const uint32_t wl = __shfl(word, l2, 64);
      const bool same = mine && kind == 3 && word == wl;
      const u64 g2 = __ballot(same);
      u64 comb = same ? bit : 0;
      if (g2 & (g2 - 1)) comb = wave_or(comb);
      uint32_t fr = 0;
      if (static_cast<int>(lane_id()) == l2) {
        const u64 before = atomicOr(reinterpret_cast<u64*>(e->bits) + wl, comb);
        fr = __popcll(comb & ~before);
      }
      fr = __shfl(fr, l2, 64);
      n_old += __popcll(g2) - fr;  // present before, or a second copy inside this wave
      inw &= ~g2;
    }
    if (static_cast<int>(lane_id()) == leader) {
      const bool in_lds = cl == blk_key;
      if (n_old) atomicAdd(in_lds ? &blk_old : &a.call[cl].old, n_old);
      if (n_oow) atomicAdd(in_lds ? &blk_oow : &a.call[cl].oow, n_oow);
    }
    act &= ~grp;
  }
  __syncthreads();
  if (threadIdx.x == 0 && (blk_old | blk_oow)) {  // then blk_key is a member: only a leader's cl gets here
    if (blk_old) atomicAdd(&a.call[blk_key].old, blk_old);
    if (blk_oow) atomicAdd(&a.call[blk_key].oow, blk_oow);
  }
}

// ---------------------------------------------------------------- receive, per member (one wave each)
__global__ __launch_bounds__(256) void k_ack_floor(AckReceiveArgs a) {
  const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (c >= a.nconn) return;
  const u64 m = a.call[c].sw_max;
  if (m == 0) return;
  const AckEntry e = a.table[c];
  const u64 ipb = e.rec->ignore_below, lio = e.rec->largest_in_order;
  if (m <= ipb) return;
  const u64 nlio = m - 1 > lio ? m - 1 : lio;
  uint32_t left = e.rec->outstanding, top;
  if (nlio != lio) {
    const u64 d = nlio - lio;
    left = clear_and_count(e.bits, e.wp, static_cast<uint32_t>(lio + 1) & (e.wp - 1u),
                           d >= e.wp ? e.wp : static_cast<uint32_t>(d), top);
  }
  if (lane_id() == 0) {
    e.rec->ignore_below = m - 1;
    e.rec->largest_in_order = nlio;
    e.rec->outstanding = left;  // the bitmap's population: the advance pass takes fresh from its growth
    e.rec->changed = 1;
  }
}

__global__ __launch_bounds__(256) void k_ack_advance(AckReceiveArgs a) {
  const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (c >= a.nconn) return;
  const AckCall k = a.call[c];
  if (!k.touched && !k.oow) return;  // no packet of this member: bit for bit
  const AckEntry e = a.table[c];
  AckRecord r = *e.rec;
  if (k.touched) {
    const uint32_t nwords = e.wp >> 6, nchunks = nwords;
    const uint32_t p0 = static_cast<uint32_t>(r.largest_in_order + 1) & (e.wp - 1u);
    // the set bits from logical bit 0 up to the first clear one: 4,096 bits per
    // ballot, kAckDepth ballots' loads in flight
    uint32_t run = 0;
    bool found = false;
    for (uint32_t base = 0; base < nchunks && !found; base += 64u * kAckDepth) {
      u64 w[kAckDepth];
#pragma unroll
      for (uint32_t u = 0; u < kAckDepth; ++u) {
        const uint32_t j = base + 64u * u + lane_id();
        w[u] = j < nchunks ? load_chunk(e.bits, nwords, p0, j) : 0;
      }
#pragma unroll
      for (uint32_t u = 0; u < kAckDepth; ++u) {
        if (found || base + 64u * u >= nchunks) continue;
        const u64 open = __ballot(w[u] != ~0ull);
        if (open) {
          const int f = __ffsll(open) - 1;
          const u64 wf = __shfl(w[u], f, 64);
          run += 64u * f + static_cast<uint32_t>(__ffsll(~wf) - 1);
          found = true;
        } else {
          run += 64u * 64u;
        }
      }
    }
    uint32_t top;
    const uint32_t left = clear_and_count(e.bits, e.wp, p0, run, top);
    const uint32_t fresh = left + run - r.outstanding;  // r.outstanding: the set bits before the packets were placed
    const u64 lo_was = r.largest_observed;
    r.largest_in_order += run;
    if (r.largest_in_order + top > r.largest_observed) r.largest_observed = r.largest_in_order + top;
    if (r.largest_observed > lo_was) r.lo_time_us = a.now_us;
    r.outstanding = left;
    r.fresh += fresh;
    r.old += k.old;
    if (fresh) r.changed = 1;
    if (left > UGO_ACK_MAX_OUTSTANDING) r.err = UGO_ACK_TOO_MANY_OUTSTANDING;
  }
  r.out_of_window += k.oow;
  if (lane_id() == 0) {
    *e.rec = r;
    a.call[c] = AckCall{};
  }
}

__global__ __launch_bounds__(256) void k_ack_touch(const AckEntry* table, uint32_t nconn, const uint8_t* flags) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c < nconn && flags[c]) table[c].rec->changed = 1;
}

// ---------------------------------------------------------------- attach
// Does member c get an ACK-only slot if there is room?
__device__ __forceinline__ bool wants_slot(const AckAttachArgs& a, uint32_t c, const AckRecord& r) {
  return r.changed && !r.err && a.n_packets[c] == 0 && a.may_ack_only && a.may_ack_only[c];
}

__global__ __launch_bounds__(kAckScanBlock) void k_ack_scan_slots(AckAttachArgs a) {
  __shared__ uint32_t wave_tot[kAckScanBlock / 64];
  const uint32_t c = blockIdx.x * kAckScanBlock + threadIdx.x;
  const bool want = c < a.nconn && wants_slot(a, c, *a.table[c].rec);
  const u64 b = __ballot(want);
  const uint32_t w = threadIdx.x >> 6;
  if (lane_id() == 0) wave_tot[w] = __popcll(b);
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (uint32_t k = 0; k < kAckScanBlock / 64; ++k) {
    if (k < w) before += wave_tot[k];
    total += wave_tot[k];
  }
  if (c < a.nconn) a.slot_local[c] = before + __popcll(b & ((1ull << lane_id()) - 1ull));
  if (threadIdx.x == 0) a.block_slots[blockIdx.x] = total;
}

// block_slots[0 .. n) (n <= kAckScanBlock) to their exclusive scan; *total is
// kept for the members' pass and *total_out written.
__global__ __launch_bounds__(kAckScanBlock) void k_ack_scan_blocks(AckAttachArgs a, uint32_t n) {
  __shared__ u64 s[kAckScanBlock];
  const uint32_t t = threadIdx.x;
  const u64 v = t < n ? a.block_slots[t] : 0;
  s[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kAckScanBlock; d <<= 1) {
    const u64 add = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  if (t < n) a.block_slots[t] = s[t] - v;
  if (t == 0) {
    const u64 total = *a.total, want = s[kAckScanBlock - 1];
    const u64 room = total < a.max_packets ? a.max_packets - total : 0;
    *a.total_in = total;
    *a.total_out = total + (want < room ? want : room);
  }
}

__global__ __launch_bounds__(256) void k_ack_attach(AckAttachArgs a) {
  const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (c >= a.nconn) return;
  const uint32_t lane = lane_id();
  const AckEntry e = a.table[c];
  const AckRecord r = *e.rec;
  bool ack_only = false, have = false;
  u64 t = 0;
  if (r.changed && !r.err) {
    if (a.n_packets[c] > 0) {
      t = a.first_packet[c];
      have = true;
    } else if (wants_slot(a, c, r)) {
      t = *a.total_in + a.block_slots[c / kAckScanBlock] + a.slot_local[c];
      have = ack_only = true;
    }
    if (t >= a.max_packets) have = false;  // the clamp
  }
  if (!have) {
    if (lane == 0) a.attached[c] = UGO_ACK_NOT_ATTACHED;
    return;
  }
  const u64 lio = r.largest_in_order, lo = r.largest_observed;
  const uint32_t nwords = e.wp >> 6;
  const uint32_t p0 = static_cast<uint32_t>(lio + 1) & (e.wp - 1u);
  const uint32_t L = static_cast<uint32_t>(lo - lio);           // logical bits [0, L) can be set; L <= wp
  const uint32_t nchunks = (L + 63u) >> 6;
  const uint32_t keep = a.max_ranges ? a.max_ranges - 1u : 0u;  // runs a row has room for beside {lio, lio}
  uint64_t* row = a.ranges + t * a.max_ranges * 2u;
  // from the top chunk down, 64 chunks per pass, lane 0 the highest.  A run
  // ends at a set bit with a clear bit above it and starts at a set bit with a
  // clear bit below; the k-th end and the k-th start from the top are run k's.
  uint32_t ends_seen = 0, starts_seen = 0;
  for (uint32_t base = 0; base < nchunks; base += 64u) {
    const uint32_t q = base + lane;
    u64 w = 0, ends = 0, starts = 0;
    uint32_t j = 0;
    if (q < nchunks) {
      j = nchunks - 1u - q;
      w = load_chunk(e.bits, nwords, p0, j);
      const u64 above = load_bit(e.bits, e.wp, p0, 64ll * j + 64), below = load_bit(e.bits, e.wp, p0, 64ll * j - 1);
      ends = w & ~((w >> 1) | (above << 63));
      starts = w & ~((w << 1) | below);
    }
    uint32_t te, tst;
    uint32_t re = ends_seen + wave_excl(__popcll(ends), te);
    uint32_t rs = starts_seen + wave_excl(__popcll(starts), tst);
    for (; ends && re < keep; ++re) {  // highest bit first
      const int b = 63 - __clzll(ends);
      row[2u * re + 1u] = lio + 1 + 64ull * j + b;
      ends &= ~(1ull << b);
    }
    for (; starts && rs < keep; ++rs) {
      const int b = 63 - __clzll(starts);
      row[2u * rs] = lio + 1 + 64ull * j + b;
      starts &= ~(1ull << b);
    }
    ends_seen += te;
    starts_seen += tst;
    if (ends_seen > keep && starts_seen >= keep) break;  // truncated, and every kept run is written
  }
  if (lane != 0) return;
  const uint32_t runs = ends_seen;  // exact unless the walk stopped early, and then > keep too
  uint64_t largest_acked = lo;
  uint32_t n_ranges = 0;
  uint8_t how = UGO_ACK_ATTACHED;
  if (runs != 0) {
    if (runs > keep) how = UGO_ACK_TRUNCATED;
    if (a.max_ranges >= 2u) {
      const uint32_t kept = runs < keep ? runs : keep;
      row[2u * kept] = lio;
      row[2u * kept + 1u] = lio;
      n_ranges = kept + 1u;
    } else {
      largest_acked = lio;  // no row to say what is missing: acknowledge nothing above lio
    }
  }
  ugo_pkt_info* out = a.info + t;
  if (ack_only) {
    ugo_pkt_info o{};
    o.flags = 0x80;
    o.largest_acked = largest_acked;
    o.largest_in_order = lio;
    o.delay_us = a.now_us > r.lo_time_us ? a.now_us - r.lo_time_us : 0;
    o.n_ranges = static_cast<uint16_t>(n_ranges);
    *out = o;
    a.conn_of[t] = c;
  } else {
    out->flags |= 0x80;
    out->largest_acked = largest_acked;
    out->largest_in_order = lio;
    out->delay_us = a.now_us > r.lo_time_us ? a.now_us - r.lo_time_us : 0;
    out->n_ranges = static_cast<uint16_t>(n_ranges);
  }
  a.attached[c] = how;
  e.rec->changed = 0;
}

__global__ __launch_bounds__(256) void k_ack_gather(const AckEntry* table, uint32_t nconn, ugo_ack_state* out) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c < nconn) out[c] = *table[c].rec;
}

}  // namespace

hipError_t launch_ack_receive(const AckReceiveArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const dim3 per_packet(static_cast<uint32_t>((a.npk + 255u) / 256u)), per_member((a.nconn + 3u) / 4u);
  launch(kKAck, k_ack_scan_packets, per_packet, dim3(256), 0, s, a);
  launch(kKAck, k_ack_floor, per_member, dim3(256), 0, s, a);
  launch(kKAck, k_ack_place, dim3(static_cast<uint32_t>((a.npk + kAckPlaceBlock - 1u) / kAckPlaceBlock)),
         dim3(kAckPlaceBlock), 0, s, a);
  launch(kKAck, k_ack_advance, per_member, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ack_touch(const AckEntry* table, uint32_t nconn, const uint8_t* flags, hipStream_t s) {
  launch(kKAck, k_ack_touch, dim3((nconn + 255u) / 256u), dim3(256), 0, s, table, nconn, flags);
  return hipGetLastError();
}

hipError_t launch_ack_attach(const AckAttachArgs& a, hipStream_t s) {
  const uint32_t sblocks = (a.nconn + kAckScanBlock - 1) / kAckScanBlock;  // <= kAckScanBlock
  launch(kKAck, k_ack_scan_slots, dim3(sblocks), dim3(kAckScanBlock), 0, s, a);
  launch(kKAck, k_ack_scan_blocks, dim3(1), dim3(kAckScanBlock), 0, s, a, sblocks);
  launch(kKAck, k_ack_attach, dim3((a.nconn + 3u) / 4u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ack_gather(const AckEntry* table, uint32_t nconn, ugo_ack_state* out, hipStream_t s) {
  launch(kKAck, k_ack_gather, dim3((nconn + 255u) / 256u), dim3(256), 0, s, table, nconn, out);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
