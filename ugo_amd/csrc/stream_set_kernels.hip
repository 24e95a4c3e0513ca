// stream_set_kernels.hip -- stream delivery for a set of receive windows
// (ugo_fec_stream_set_*, include/ugo_stream.h): one batch holds the packets of
// many connections, interleaved as the listener received them, and conn_of[i]
// names the member of the set that packet i belongs to.
//
// The rule, the bitmaps and the seven-launch shape are those of
// stream_kernels.hip, whose kernels stay as they are and keep serving the
// single entry points; the helpers both files use are in stream_device.hpp.
// Per member the result is what ugo_fec_stream_deliver gives for the member's
// subsequence of the batch.  What changes once a block holds packets of
// several connections:
//
//   k_set_classify  16 lanes per packet; window, bitmaps and record come from
//                   table[conn_of[i]].  A packet of no connection (conn_of >=
//                   nconn) gets a zero row and is looked at by no later kernel.
//                   claim_end is reduced per connection of the block: the first
//                   group that holds a connection takes the maximum of that
//                   connection's groups to its record, and marks the record
//                   `touched`.
//   k_set_resolve   16 lanes per packet, as the single kernel.
//   k_set_apply     the connection on blockIdx.y (.z above 32,768), wblocks
//                   blocks each -- sized from the largest member window, not
//                   1024 -- and a block of an untouched connection leaves after
//                   one load.
//   k_set_ordered   one block per connection, at work only where n_contested !=
//                   0: it walks the batch's statuses in arrival order and takes
//                   the contested entries whose packet is its own.  done ==
//                   todo and the fatal stop are per connection; no block waits
//                   for another.
//   k_set_copy      64 packets per block.  Phase A (a thread per packet) reads
//                   fatal_idx, read_pos and cap of the packet's own connection
//                   and leaves window, cap, read_pos and fatal_idx in the
//                   packet's LDS descriptor, so that the copying lanes of phase
//                   B start on the bytes at once.  Counters, hi and
//                   accepted_data are summed per connection of the block, at
//                   the LDS slot of the connection's first packet (found with
//                   64 readlanes; skipped when the wave holds one connection),
//                   and that packet's thread takes them to the record.  The
//                   record of the wave's first packet is read with scalar loads.
//   k_set_scan      as apply.
//   k_set_finish    16 lanes per connection; clears `touched`.
// k_set_read is Conn.Read for every member: the connection on blockIdx.y,
// rblocks blocks each (the grid held near 4,096 blocks in all); ticket, scan_head and the last block's epilogue are the
// connection's own, and a connection with n[c] == 0 writes its two outputs and
// touches nothing of its record.  k_set_gather collects the public records for
// ugo_fec_stream_set_state.
//
// classify, resolve and copy read a packet's table entry and record through
// load_conn: scalar loads for the connection of the wave's first active lane,
// per-lane loads for the wave's other connections.
//
// group_any (classify, resolve) ballots within 16-lane groups; neighbouring
// groups of a wave now differ in connection and cap.  Every branch on the
// table entry is uniform over a group, so no lane leaves its group.
//
// gfx950, -O3, -Rpass-analysis=kernel-resource-usage (VGPRs / SGPRs / LDS bytes
// per block / waves per SIMD; no kernel uses scratch or spills):
//   k_set_classify 64 / 62 /  192 / 8     k_set_copy   94 / 77 / 5632 / 5
//   k_set_resolve  52 / 41 /    0 / 8     k_set_scan   20 / 32 /   16 / 8
//   k_set_apply    14 / 28 /    8 / 8     k_set_finish 15 / 14 /    0 / 8
//   k_set_ordered  68 / 104 / 4360 / 7    k_set_read   22 / 62 /   16 / 8
//   k_set_gather    8 / 14 /    0 / 8
// (k_stream_copy: 80 VGPRs; the 14 more are the per-packet window, cap,
// read_pos and fatal_idx that the single kernel keeps in SGPRs.)
// Measured: tools/stream_set_probe.py, DESIGN.md §3.8, profiles/stream_set/.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "stream_set_kernels.hpp"
#include "stream_device.hpp"

namespace ugo {
namespace kern {
namespace {

constexpr uint32_t kConnFold = 32768;  // connections on blockIdx.y; the rest go to blockIdx.z
constexpr uint32_t kFinishLanes = 16;

__device__ __forceinline__ uint32_t block_conn() { return blockIdx.z * kConnFold + blockIdx.y; }

dim3 conn_grid(uint32_t x, uint32_t nconn) {
  return dim3(x, nconn < kConnFold ? nconn : kConnFold, (nconn + kConnFold - 1) / kConnFold);
}

// One connection's view of the batch.
__device__ __forceinline__ StreamArgs view(const StreamSetArgs& g, const StreamSetEntry& e) {
  StreamArgs a;
  a.pkts = g.pkts;
  a.pad = g.pad;
  a.info = g.info;
  a.segs = g.segs;
  a.seg_status = g.seg_status;
  a.win = e.win;
  a.C = e.C;
  a.S = e.S;
  a.claim = e.claim;
  a.cont = e.cont;
  a.rec = e.rec;
  a.npk = g.npk;
  a.slot = g.slot;
  a.cap = e.cap;
  a.max_segments = g.max_segments;
  return a;
}

// What the lanes of a packet need of its connection: the table entry and the
// fields of the record that hold for the whole kernel.  c is a member's index
// or UGO_STREAM_NO_CONN (then nothing is loaded).  The connection of the wave's
// first active lane goes through a uniform index and a global-address-space
// pointer -- scalar loads, once for the wave, and all there is while a wave
// holds one connection -- the other connections of the wave per lane.  (Vector
// loads of a record that every block's atomics go to cost the copy kernel
// 0.5 ms at 852k packets of one connection; a load through a flat pointer is
// never scalar.)
struct ConnState {
  StreamSetEntry e;
  u64 rp, head, fatal;
  uint32_t inert;
  bool hv;
};

__device__ __forceinline__ ConnState load_conn(const StreamSetArgs& g, uint32_t c) {
  typedef const __attribute__((address_space(1))) StreamRecord* GlobalRecord;
  ConnState s{};
  const uint32_t cu = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(c)));
  if (cu != UGO_STREAM_NO_CONN) {
    s.e = g.table[cu];
    const GlobalRecord r = (GlobalRecord)s.e.rec;
    s.rp = r->pub.read_pos;
    s.head = r->pub.head_off;
    s.hv = r->pub.head_valid != 0;
    s.fatal = r->fatal_idx;
    s.inert = r->inert;
  }
  if (c != cu && c != UGO_STREAM_NO_CONN) {
    s.e = g.table[c];
    const StreamRecord* r = s.e.rec;
    s.rp = r->pub.read_pos;
    s.head = r->pub.head_off;
    s.hv = r->pub.head_valid != 0;
    s.fatal = r->fatal_idx;
    s.inert = r->inert;
  }
  return s;
}

// ------------------------------------------------------------ classify + claim
__global__ __launch_bounds__(256) void k_set_classify(StreamSetArgs g) {
  __shared__ uint32_t s_conn[kGroupsPerBlock];
  __shared__ u64 s_end[kGroupsPerBlock];
  const uint32_t grp = threadIdx.x / kGroupLanes, lane = threadIdx.x % kGroupLanes;
  const u64 i = blockIdx.x * static_cast<u64>(kGroupsPerBlock) + grp;
  const bool valid = i < g.npk;
  uint32_t c = valid ? g.conn_of[i] : UGO_STREAM_NO_CONN;
  if (c >= g.nconn) c = UGO_STREAM_NO_CONN;
  const ConnState cs = load_conn(g, c);
  uint8_t* st = g.seg_status + i * g.max_segments;
  u64 claim_end = 0;
  bool open = false;
  StreamRecord* rec = nullptr;
  if (c != UGO_STREAM_NO_CONN) {  // uniform over the group, like every branch on the entry below
    const StreamArgs a = view(g, cs.e);
    rec = cs.e.rec;
    open = cs.inert == 0;
    const bool live = open && a.info[i].status == UGO_PKT_OK;
    const uint32_t ns = live ? nseg_of(a, i) : 0u;
    for (uint32_t j = ns + lane; j < a.max_segments; j += kGroupLanes) st[j] = kNone;
    const u64 rp = cs.rp, head = cs.head, cap = a.cap;
    const bool hv = cs.hv;
    for (uint32_t j = 0; j < ns; ++j) {
      const Seg s = load_seg(a, i * a.max_segments + j);
      const bool indom = s.o >= rp && s.o - rp < cap;
      const u64 sbit = 1ull << (s.o & 63);
      uint32_t res;
      if ((hv && s.o == head) || (indom && (a.S[widx(s.o, cap)] & sbit))) {
        res = kDuplicate;
      } else if (s.len == 0) {
        res = indom ? kFinCand : kOutOfWindow;
        if (indom && lane == 0) {
          const u64 old = atomicOr(a.claim + widx(s.o, cap), sbit);
          if (old & sbit) atomicOr(a.cont + widx(s.o, cap), sbit);
        }
      } else if (s.o > rp + cap || s.len > rp + cap - s.o) {
        res = kOutOfWindow;
      } else if (s.o + s.len <= rp) {
        res = kDuplicate;
      } else {
        const u64 e2 = s.o + s.len, lo = s.o > rp ? s.o : rp;
        const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
        bool anyc = s.o < rp, anyu = false;
        for (u64 k = lane; k < nw; k += kGroupLanes) {
          const u64 p = p0 + 64 * k, m = range_mask(p, lo, e2), w = a.C[widx(p, cap)];
          anyc |= (w & m) != 0;
          anyu |= (~w & m) != 0;
        }
        anyc = group_any(anyc);
        anyu = group_any(anyu);
        if (!anyu) {
          res = kDuplicate;
        } else {
          for (u64 k = lane; k < nw; k += kGroupLanes) {
            const u64 p = p0 + 64 * k, wi = widx(p, cap);
            const u64 m = range_mask(p, lo, e2) & ~a.C[wi];
            if (m) {
              const u64 hit = atomicOr(a.claim + wi, m) & m;
              if (hit) atomicOr(a.cont + wi, hit);
            }
          }
          res = anyc ? kPartial : kCand;
          claim_end = e2 > claim_end ? e2 : claim_end;
        }
      }
      if (lane == 0) st[j] = static_cast<uint8_t>(res);
    }
  } else if (valid) {  // no connection: a zero row, and no later kernel looks at the packet
    for (uint32_t j = lane; j < g.max_segments; j += kGroupLanes) st[j] = kNone;
  }
  // Per connection of this block, the first group that holds it: the record is
  // touched, and how far k_set_apply has to look -- one atomic per block and
  // connection, spread over kEndShards words.
  if (lane == 0) {
    s_conn[grp] = open ? c : UGO_STREAM_NO_CONN;
    s_end[grp] = claim_end;
  }
  __syncthreads();
  if (lane == 0 && open) {
    bool leader = true;
    u64 end = 0;
    for (uint32_t k = 0; k < kGroupsPerBlock; ++k) {
      if (s_conn[k] != c) continue;
      leader &= k >= grp;
      end = s_end[k] > end ? s_end[k] : end;
    }
    if (leader) {
      rec->touched = 1;
      if (end != 0) atomicMax(&rec->claim_end[blockIdx.x % kEndShards], end);
    }
  }
}

// -------------------------------------------------------------------- resolve
__global__ __launch_bounds__(256) void k_set_resolve(StreamSetArgs g) {
  const u64 i = blockIdx.x * static_cast<u64>(kGroupsPerBlock) + threadIdx.x / kGroupLanes;
  const uint32_t lane = threadIdx.x % kGroupLanes;
  if (i >= g.npk) return;
  const uint32_t c = g.conn_of[i];
  if (c >= g.nconn) return;
  const ConnState cs = load_conn(g, c);
  const StreamArgs a = view(g, cs.e);
  StreamRecord& R = *cs.e.rec;
  if (cs.inert != 0 || a.info[i].status != UGO_PKT_OK) return;
  const uint32_t ns = nseg_of(a, i);
  uint8_t* st = a.seg_status + i * a.max_segments;
  const u64 rp = cs.rp, cap = a.cap;
  for (uint32_t j = 0; j < ns; ++j) {
    const uint32_t code = st[j];
    if (code < kPartial) continue;
    const Seg s = load_seg(a, i * a.max_segments + j);
    const u64 sw = widx(s.o, cap), sbit = 1ull << (s.o & 63);
    bool contested = code == kPartial;
    if (code == kFinCand) {
      contested = (a.cont[sw] & sbit) != 0;
    } else if (code == kCand) {
      const u64 e2 = s.o + s.len, lo = s.o;  // a candidate lies at or above read_pos
      const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
      bool hit = false;
      for (u64 k = lane; k < nw; k += kGroupLanes) {
        const u64 p = p0 + 64 * k;
        hit |= (a.cont[widx(p, cap)] & range_mask(p, lo, e2)) != 0;
      }
      contested = group_any(hit);
    }
    // as k_stream_resolve: an accepted segment's claim stays for k_set_apply,
    // everyone else takes the claim back
    if (code == kFinCand) {
      if (lane == 0) atomicAnd(a.claim + sw, ~sbit);
    } else if (contested) {
      const u64 e2 = s.o + s.len, lo = s.o > rp ? s.o : rp;
      const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
      for (u64 k = lane; k < nw; k += kGroupLanes) {
        const u64 p = p0 + 64 * k, wi = widx(p, cap);
        const u64 m = range_mask(p, lo, e2) & ~a.C[wi];  // what it claimed: C has not changed since
        if (m) atomicAnd(a.claim + wi, ~m);
      }
    }
    if (lane == 0) {
      if (contested) {
        atomicAdd(&R.n_contested, 1u);
      } else {
        atomicOr(a.S + sw, sbit);
      }
      st[j] = static_cast<uint8_t>(contested ? kContested : kAccepted);
    }
  }
}

// ---------------------------------------------------------------------- apply
__global__ __launch_bounds__(256) void k_set_apply(StreamSetArgs g) {
  const uint32_t c = block_conn();
  if (c >= g.nconn) return;
  const StreamSetEntry e = g.table[c];
  const StreamRecord& R = *e.rec;
  if (R.touched == 0) return;
  __shared__ u64 s_end;
  if (threadIdx.x == 0) s_end = 0;
  __syncthreads();
  if (threadIdx.x < kEndShards && R.claim_end[threadIdx.x] != 0) atomicMax(&s_end, R.claim_end[threadIdx.x]);
  __syncthreads();
  const u64 rp = R.pub.read_pos, end = s_end, cap = e.cap;
  if (end <= rp) return;
  const u64 p0 = rp & ~63ull, nw = words_of(rp, end);
  for (u64 k = blockIdx.x * 256ull + threadIdx.x; k < nw; k += 256ull * gridDim.x) {
    const u64 wi = widx(p0 + 64 * k, cap);
    const u64 cl = e.claim[wi];
    if (cl == 0) continue;
    e.claim[wi] = 0;
    e.C[wi] = cl == ~0ull ? cl : (e.C[wi] | cl);
  }
}

// --------------------------------------------------------------- ordered pass
// One block per connection; k_stream_ordered's walk over the whole batch, taking
// the contested entries of this connection's packets only.
__global__ __launch_bounds__(kOrderedThreads) void k_set_ordered(StreamSetArgs g) {
  const uint32_t c = block_conn();
  if (c >= g.nconn) return;
  const StreamSetEntry e = g.table[c];
  StreamRecord& R = *e.rec;
  if (R.touched == 0) return;
  const uint32_t todo = R.n_contested;
  if (todo == 0) return;
  const StreamArgs a = view(g, e);
  __shared__ uint32_t s_mask[kOrderedThreads];
  __shared__ uint32_t s_stop;
  const u64 rp = R.pub.read_pos, head = R.pub.head_off;
  const bool hv = R.pub.head_valid != 0;
  const u64 total = a.npk * a.max_segments;
  const uint32_t tid = threadIdx.x;
  const bool aligned16 = (reinterpret_cast<uintptr_t>(a.seg_status) & 15u) == 0;
  uint32_t done = 0;  // wave 0's count
  for (u64 base = 0; base < total; base += 16ull * kOrderedThreads) {
    const u64 first = base + 16ull * tid;
    uint32_t mask = 0;
    if (aligned16 && first + 16 <= total) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(a.seg_status + first);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t b = 0; b < 16; ++b)
        if (((w[b >> 2] >> (8u * (b & 3u))) & 0xffu) == kContested) mask |= 1u << b;
    } else {
      for (uint32_t b = 0; b < 16; ++b)
        if (first + b < total && a.seg_status[first + b] == kContested) mask |= 1u << b;
    }
    // of these, this connection's (contested entries are rare)
    for (uint32_t m = mask; m != 0; m &= m - 1) {
      const uint32_t b = static_cast<uint32_t>(__builtin_ctz(m));
      if (g.conn_of[(first + b) / a.max_segments] != c) mask &= ~(1u << b);
    }
    s_mask[tid] = mask;
    if (tid == 0) s_stop = 0;
    if (!__syncthreads_or(mask != 0)) continue;
    if (tid < 64) {
      bool stop = false;
      for (uint32_t t0 = 0; t0 < kOrderedThreads && !stop; t0 += 64) {
        const uint32_t mine = s_mask[t0 + tid];
        u64 bal = __ballot(mine != 0);
        while (bal != 0 && !stop) {
          const uint32_t t = static_cast<uint32_t>(__builtin_ctzll(bal));
          bal &= bal - 1;
          uint32_t mt = __shfl(mine, static_cast<int>(t));
          while (mt != 0 && !stop) {
            const uint32_t b = static_cast<uint32_t>(__builtin_ctz(mt));
            mt &= mt - 1;
            const bool fatal = ordered_one(a, base + 16ull * (t0 + t) + b, tid, rp, head, hv);
            ++done;
            stop = fatal || done == todo;
          }
        }
      }
      if (tid == 0 && stop) s_stop = 1;
    }
    __syncthreads();
    if (s_stop != 0) break;
    __syncthreads();  // s_stop is rewritten at the top of the next tile
  }
  if (tid == 0) R.pub.ordered_segments += done;
}

// ------------------------------------------------ counters, undo, clear, copy
__global__ __launch_bounds__(256) void k_set_copy(StreamSetArgs g) {
  constexpr uint32_t P = kCopyPacketsPerBlock;
  static_assert(P == 64, "phase A is one wave: the readlane search below relies on it");
  // what B needs of a packet: its first segment and its connection's window, so
  // that its lanes start on the bytes at once
  __shared__ ugo_pkt_segment s_seg0[P];
  __shared__ uint32_t s_ns[P], s_code0[P], s_conn[P];
  __shared__ uint8_t* s_win[P];
  __shared__ u64 s_cap[P], s_rp[P], s_fatal[P];
  // per connection of the block, at the slot of its first packet: accepted,
  // duplicate, out of window, skipped packets, accepted data; hi
  __shared__ uint32_t s_cnt[P][5];
  __shared__ u64 s_hi[P];
  const uint32_t t = threadIdx.x;
  if (t < P) {
    s_ns[t] = 0;  // no packet, no connection, an inert connection or a skipped packet
    s_hi[t] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) s_cnt[t][k] = 0;
  }
  __syncthreads();
  const u64 first = blockIdx.x * static_cast<u64>(P);
  uint32_t leader = t;
  StreamRecord* rec = nullptr;
  // A: one thread per packet takes the counters and hi from the statuses at or
  // before its connection's fatal segment
  if (t < P) {
    const u64 i = first + t;
    uint32_t c = i < g.npk ? g.conn_of[i] : UGO_STREAM_NO_CONN;
    if (c >= g.nconn) c = UGO_STREAM_NO_CONN;
    const ConnState cs = load_conn(g, c);
    const StreamSetEntry& e = cs.e;
    const u64 fatal = cs.fatal, rp = cs.rp;
    if (cs.inert != 0) c = UGO_STREAM_NO_CONN;
    rec = c != UGO_STREAM_NO_CONN ? e.rec : nullptr;
    // the first packet of the block with my connection
    if (!__all(c == static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(c))))) {
#pragma unroll
      for (int k = static_cast<int>(P) - 1; k >= 0; --k)
        if (static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(c), k)) == c) leader = k;
    } else {
      leader = 0;
    }
    if (c != UGO_STREAM_NO_CONN) {
      s_conn[t] = c;
      s_win[t] = e.win;
      s_cap[t] = e.cap;
      s_rp[t] = rp;
      s_fatal[t] = fatal;
      if (g.info[i].status != UGO_PKT_OK) {
        if (i * g.max_segments <= fatal) atomicAdd(&s_cnt[leader][3], 1u);
      } else {
        const uint32_t n = g.info[i].n_segments;
        const uint32_t ns = n < g.max_segments ? n : g.max_segments;
        s_ns[t] = ns;
        if (ns != 0) {
          s_code0[t] = g.seg_status[i * g.max_segments];
          s_seg0[t] = g.segs[i * g.max_segments];
        }
        uint32_t acc = 0, dup = 0, oow = 0;
        u64 hi = 0;
        for (uint32_t j = 0; j < ns; ++j) {
          const u64 idx = i * g.max_segments + j;
          if (idx > fatal) break;
          const uint32_t code = j == 0 ? s_code0[t] : g.seg_status[idx];
          if (code == kAccepted) {
            ++acc;
            const ugo_pkt_segment sg = j == 0 ? s_seg0[t] : g.segs[idx];
            if (sg.len != 0 && sg.offset + sg.len > hi) hi = sg.offset + sg.len;
          }
          dup += code == kDuplicate;
          oow += code == kOutOfWindow;
        }
        if (acc) atomicAdd(&s_cnt[leader][0], acc);
        if (dup) atomicAdd(&s_cnt[leader][1], dup);
        if (oow) atomicAdd(&s_cnt[leader][2], oow);
        if (hi) {
          atomicMax(&s_hi[leader], hi);
          s_cnt[leader][4] = 1;
        }
      }
    }
  }
  __syncthreads();
  if (t < P && rec != nullptr && leader == t) {
    StreamRecord& R = *rec;
    if (s_cnt[t][0]) atomicAdd(reinterpret_cast<u64*>(&R.pub.accepted), static_cast<u64>(s_cnt[t][0]));
    if (s_cnt[t][1]) atomicAdd(reinterpret_cast<u64*>(&R.pub.duplicate), static_cast<u64>(s_cnt[t][1]));
    if (s_cnt[t][2]) atomicAdd(reinterpret_cast<u64*>(&R.pub.out_of_window), static_cast<u64>(s_cnt[t][2]));
    if (s_cnt[t][3]) atomicAdd(reinterpret_cast<u64*>(&R.pub.skipped_packets), static_cast<u64>(s_cnt[t][3]));
    if (s_hi[t]) atomicMax(reinterpret_cast<u64*>(&R.pub.hi), s_hi[t]);
    if (s_cnt[t][4]) R.accepted_data = 1;
  }
  // B: kCopyLanes lanes per packet
  constexpr uint32_t kGroups = 256u / kCopyLanes;
  const uint32_t grp = threadIdx.x / kCopyLanes, hl = threadIdx.x % kCopyLanes;
  StreamArgs a{};
  a.pkts = g.pkts;
  a.pad = g.pad;
  a.segs = g.segs;
  a.slot = g.slot;
  a.max_segments = g.max_segments;
  for (uint32_t p = grp; p < P; p += kGroups) {
    const u64 i = first + p;
    const uint32_t ns = s_ns[p];
    if (ns == 0) continue;
    const u64 fatal = s_fatal[p], rp = s_rp[p], cap = s_cap[p];
    a.win = s_win[p];
    a.cap = cap;
    for (uint32_t j = 0; j < ns; ++j) {
      const u64 idx = i * a.max_segments + j;
      const uint32_t code = j == 0 ? s_code0[p] : g.seg_status[idx];
      const Seg s = j == 0 ? to_seg(a, s_seg0[p]) : load_seg(a, idx);
      const bool indom = s.o >= rp && s.o - rp < cap;
      const u64 e2 = s.o + s.len, lo = s.o > rp ? s.o : rp;
      const bool ranged = s.len != 0 && !(s.o > rp + cap || s.len > rp + cap - s.o) && e2 > rp;
      const bool undo = idx > fatal && code == kAccepted;
      // only after a fatal: the contested it left behind still have their
      // contested bits, the accepted after it come out of C again
      const bool left = code == kContested;
      if (left || undo) {
        const StreamSetEntry e = g.table[s_conn[p]];
        if (left && s.len == 0 && indom && hl == 0) e.cont[widx(s.o, cap)] = 0;
        if (ranged) {
          const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
          for (u64 k = hl; k < nw; k += kCopyLanes) {
            const u64 q = p0 + 64 * k, wi = widx(q, cap);
            if (left) e.cont[wi] = 0;
            if (undo) atomicAnd(e.C + wi, ~range_mask(q, lo, e2));
          }
        }
        if (undo && hl == 0) atomicAnd(e.S + widx(s.o, cap), ~(1ull << (s.o & 63)));
      }
      if (idx > fatal) {
        if (hl == 0 && code != kNone) g.seg_status[idx] = kNone;
      } else if (code == kAccepted && s.len != 0) {
        copy_segment(a, i, s, hl);
      }
    }
  }
}

// -------------------------------------------------------------------- summary
__global__ __launch_bounds__(256) void k_set_scan(StreamSetArgs g) {
  const uint32_t c = block_conn();
  if (c >= g.nconn) return;
  const StreamSetEntry e = g.table[c];
  StreamRecord& R = *e.rec;
  if (R.touched == 0) return;
  const u64 rp = R.pub.read_pos, hi = R.pub.hi, cap = e.cap;
  if (hi <= rp) return;
  __shared__ uint32_t s_runs;
  __shared__ u64 s_u;
  if (threadIdx.x == 0) {
    s_runs = 0;
    s_u = ~0ull;
  }
  __syncthreads();
  const u64 p0 = rp & ~63ull, nw = words_of(rp, hi);
  uint32_t runs = 0;
  u64 u = ~0ull;
  for (u64 k = blockIdx.x * 256ull + threadIdx.x; k < nw; k += 256ull * gridDim.x) {
    const u64 p = p0 + 64 * k;
    const u64 unc = ~e.C[widx(p, cap)] & range_mask(p, rp, hi);
    if (unc == 0) continue;
    // a run starts at an uncovered byte whose predecessor is covered (or is below read_pos)
    const u64 prev_unc = p > rp ? (~e.C[widx(p - 64, cap)] >> 63) : 0ull;
    runs += static_cast<uint32_t>(__builtin_popcountll(unc & ~((unc << 1) | prev_unc)));
    const u64 pos = p + static_cast<u64>(__builtin_ctzll(unc));
    u = pos < u ? pos : u;
  }
  if (runs) atomicAdd(&s_runs, runs);
  if (u != ~0ull) atomicMin(&s_u, u);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_runs) atomicAdd(&R.scan_runs, s_runs);
    if (s_u != ~0ull) atomicMin(&R.scan_u, s_u);
  }
}

__global__ __launch_bounds__(256) void k_set_finish(StreamSetArgs g) {
  const uint32_t c = blockIdx.x * (256u / kFinishLanes) + threadIdx.x / kFinishLanes;
  const uint32_t lane = threadIdx.x % kFinishLanes;
  if (c >= g.nconn) return;
  const StreamSetEntry e = g.table[c];
  StreamRecord& R = *e.rec;
  if (R.touched == 0) return;  // no packet of this call: the record stays bit for bit (touched implies not inert)
  for (uint32_t k = lane; k < kEndShards; k += kFinishLanes) R.claim_end[k] = 0;
  if (lane != 0) return;
  const u64 rp = R.pub.read_pos, hi = R.pub.hi;
  const u64 u = R.scan_u < hi ? R.scan_u : (hi > rp ? hi : rp);
  R.pub.ngaps = R.scan_runs + 1u;
  R.pub.readable = u - rp;
  R.pub.eof = (u - rp < e.cap && ((e.S[widx(u, e.cap)] >> (u & 63)) & 1ull)) ? 1 : 0;
  if (R.pub.err == 0 && R.accepted_data != 0 && R.pub.ngaps > UGO_STREAM_MAX_GAPS)
    R.pub.err = UGO_STREAM_TOO_MANY_GAPS;
  if (R.pub.err != 0) R.inert = 1;
  R.fatal_idx = ~0ull;
  R.scan_u = ~0ull;
  R.scan_runs = 0;
  R.n_contested = 0;
  R.accepted_data = 0;
  R.touched = 0;
}

// ----------------------------------------------------------------------- read
__global__ __launch_bounds__(256) void k_set_read(StreamSetReadArgs g) {
  const uint32_t c = block_conn();
  if (c >= g.nconn) return;
  const u64 n = g.n[c];
  if (n == 0) {  // skipped: nothing of the record is read or written
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      g.n_read[c] = 0;
      if (g.eof) g.eof[c] = 0;
    }
    return;
  }
  const StreamSetEntry en = g.table[c];
  StreamRecord& R = *en.rec;
  uint8_t* dst = g.dst ? g.dst + g.dst_off[c] : nullptr;
  const u64 rp = R.pub.read_pos, readable = R.pub.readable, cap = en.cap, capm = en.cap - 1;
  const u64 m = n < readable ? n : readable;
  const u64 e = rp + m;
  __shared__ u64 s_head;
  __shared__ uint32_t s_last;
  if (threadIdx.x == 0) s_head = 0;
  __syncthreads();
  const u64 gtid = blockIdx.x * 256ull + threadIdx.x, gsz = 256ull * gridDim.x;
  if (m != 0) {
    // the bytes: whole 16-B chunks of the window, then the ends
    if (dst != nullptr) {
      const u64 c0 = (rp + 15) >> 4, c1 = e >> 4;
      for (u64 ch = c0 + gtid; ch < c1; ch += gsz) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(en.win + ((16 * ch) & capm)));
        *reinterpret_cast<u32x4u*>(dst + (16 * ch - rp)) = v;
      }
      if (blockIdx.x == 0 && threadIdx.x < 32) {
        const u64 head_end = e < 16 * c0 ? e : 16 * c0;
        const u64 tail_start = 16 * c1 > head_end ? 16 * c1 : head_end;
        const u64 x = threadIdx.x < 16 ? rp + threadIdx.x : tail_start + (threadIdx.x - 16);
        if (threadIdx.x < 16 ? x < head_end : x < e) dst[x - rp] = en.win[x & capm];
      }
    }
    // the bits: cleared, and the highest start bit among them noted
    const u64 p0 = rp & ~63ull, nw = words_of(rp, e);
    u64 best = 0;
    for (u64 k = gtid; k < nw; k += gsz) {
      const u64 p = p0 + 64 * k, wi = widx(p, cap), mk = range_mask(p, rp, e);
      u64 sb;
      if (mk == ~0ull) {
        sb = en.S[wi];
        if (sb) en.S[wi] = 0;
        en.C[wi] = 0;
      } else {
        sb = atomicAnd(en.S + wi, ~mk) & mk;
        atomicAnd(en.C + wi, ~mk);
      }
      if (sb) best = p + 64 - static_cast<u64>(__builtin_clzll(sb));  // 1 + position; k ascends
    }
    if (best) atomicMax(&s_head, best);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_head) atomicMax(&R.scan_head, s_head);
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = atomicAdd(&R.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;  // the connection's own blocks
  }
  __syncthreads();
  if (s_last == 0 || threadIdx.x != 0) return;
  // every block of this connection has read the record and cleared its bits: advance
  __threadfence();
  const u64 found = aload(&R.scan_head);
  if (m != 0) {
    const bool partly = m < readable && ((aload(en.S + widx(e, cap)) >> (e & 63)) & 1ull) == 0;
    if (!partly) {
      R.pub.head_valid = 0;
      R.pub.head_off = 0;
    } else if (found != 0) {
      R.pub.head_valid = 1;
      R.pub.head_off = found - 1;
    }
  }
  R.pub.read_pos = e;
  R.pub.readable = readable - m;
  g.n_read[c] = m;
  if (g.eof) g.eof[c] = (m == readable && R.pub.eof != 0) ? 1 : 0;
  R.scan_head = 0;
  R.ticket = 0;
}

// --------------------------------------------------------------------- gather
__global__ __launch_bounds__(256) void k_set_gather(const StreamSetEntry* table, uint32_t nconn, u64* out) {
  constexpr uint32_t kWords = sizeof(ugo_stream_rx_state) / sizeof(u64);
  const u64 gid = blockIdx.x * 256ull + threadIdx.x;
  const u64 c = gid / kWords, w = gid % kWords;
  if (c >= nconn) return;
  out[gid] = reinterpret_cast<const u64*>(&table[c].rec->pub)[w];
}

}  // namespace

uint32_t stream_set_wblocks(uint64_t max_cap) {
  const uint64_t b = (max_cap / 64 + 256 * 4 - 1) / (256 * 4);  // four bitmap words per thread
  return static_cast<uint32_t>(b < 1 ? 1 : (b > kScanBlocks ? kScanBlocks : b));
}

// Every block of k_set_read ends with a device-scope fence and its
// connection's ticket (about 55 ns a block, measured: 131,072 blocks took 3.6
// to 7 ms to clear bitmaps alone), so the whole grid stays near 4,096 blocks.
uint32_t stream_set_rblocks(uint64_t max_cap, uint32_t nconn) {
  const uint64_t by_window = (max_cap + 256 * 64 - 1) / (256 * 64);  // four 16-B chunks per thread
  const uint64_t by_grid = nconn >= 4096 ? 1 : 4096 / nconn;
  const uint64_t b = by_window < by_grid ? by_window : by_grid;
  return static_cast<uint32_t>(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

hipError_t launch_stream_set_deliver(const StreamSetArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const uint32_t gblocks = static_cast<uint32_t>((a.npk + kGroupsPerBlock - 1) / kGroupsPerBlock);
  const uint32_t cblocks = static_cast<uint32_t>((a.npk + kCopyPacketsPerBlock - 1) / kCopyPacketsPerBlock);
  const uint32_t fblocks = (a.nconn + 256 / kFinishLanes - 1) / (256 / kFinishLanes);
  launch(kKStreamDeliver, k_set_classify, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_set_resolve, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_set_apply, conn_grid(a.wblocks, a.nconn), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_set_ordered, conn_grid(1, a.nconn), dim3(kOrderedThreads), 0, s, a);
  launch(kKStreamDeliver, k_set_copy, dim3(cblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_set_scan, conn_grid(a.wblocks, a.nconn), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_set_finish, dim3(fblocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_set_read(const StreamSetReadArgs& a, hipStream_t s) {
  launch(kKStreamRead, k_set_read, conn_grid(a.rblocks, a.nconn), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_set_gather(const StreamSetEntry* table, uint32_t nconn, ugo_stream_rx_state* out,
                                    hipStream_t s) {
  const uint64_t words = static_cast<uint64_t>(nconn) * (sizeof(ugo_stream_rx_state) / sizeof(u64));
  launch(kKStreamRead, k_set_gather, dim3(static_cast<uint32_t>((words + 255) / 256)), dim3(256), 0, s, table, nconn,
         reinterpret_cast<u64*>(out));
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
