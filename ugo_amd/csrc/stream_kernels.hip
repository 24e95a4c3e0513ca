// stream_kernels.hip -- stream delivery on the device (include/ugo_stream.h):
// batch Conn.handleSegment / segmentSorter.push into a receive window, and
// Conn.Read out of it.
//
//   Conn.handleSegment   ugo/conn.go:473-490
//   segmentSorter.push   ugo/segment_sorter.go:31-98
//   Conn.Read            ugo/conn.go:149-245
//
// The reference keeps a linked list of gaps and a map of queued segments and
// pushes one segment at a time.  The rule that list implements is stated in
// the header over two bitmaps (C: byte received, S: a queued segment starts
// here), and over bitmaps it is order-independent for almost every segment:
//
//   * a segment that is a duplicate by the state before the call (start bit,
//     head_off, every byte covered) is a duplicate whatever else arrives:
//     coverage and start bits only grow within a call;
//   * a segment with an uncovered byte CLAIMS its uncovered bytes in a scratch
//     bitmap (atomicOr); a bit that was already claimed is ORed into the
//     CONTESTED bitmap.  A wholly uncovered segment whose range shows no
//     contested bit shares no byte with any other claimer of the batch, so it
//     is accepted whatever else arrives;
//   * what is left -- segments whose claims collided (the same packet twice,
//     the same offset with two lengths, an empty segment and data at one
//     offset) and partly covered segments, which claim too so that whatever
//     touches their uncovered part is contested with them -- only interacts
//     with each other and goes through the ORDERED pass: one wave that walks
//     them in arrival order and applies the rule literally.  It is a launch of
//     its own that exits at once when nothing is contested; it never waits
//     for another block.
//
// A fatal overlap can only be found by the ordered pass; it records its
// arrival index, and the last data kernel undoes (C, S, status) the accepts
// of the parallel passes that arrived after it, so nothing after a fatal is
// applied or copied.  hi and the counters are only taken there, from final
// statuses.
//
// Launches of one ugo_fec_stream_deliver, all kernel class kKStreamDeliver:
//   k_stream_classify  16 lanes per packet: statuses by the pre-call state, claims
//   k_stream_resolve   16 lanes per packet: accept the uncontested, mark the contested
//   k_stream_apply     a word per thread: C |= the accepted segments' claims, claims cleared
//   k_stream_ordered   one block; wave 0 applies the contested in arrival order
//   k_stream_copy      64 packets per block: counters, hi, undo after a fatal, then
//                      half a wave per packet copies the accepted bytes (the hot
//                      path, below)
//   k_stream_scan      gaps and the first uncovered byte of [read_pos, hi)
//   k_stream_finish    one thread: ngaps, readable, eof, the gap limit
// ugo_fec_stream_read is one kernel, k_stream_read (class kKStreamRead); the
// block that finishes last advances the record.
//
// Measured (tools/stream_deliver_probe.py, 851,968 packets with one 1400-B
// segment, slot 1488, RC4 pad, 2-GiB window; DESIGN.md §3.7,
// profiles/stream_deliver/): 1.28 ms per call in order -- classify 0.30,
// resolve 0.12, apply 0.07, copy 0.74, scan 0.05 -- against 0.37 ms for an nt
// copy of the same bytes; the ordered pass 1.84 us per contested segment.
// Setting C per segment in resolve (atomics on the end words) and clearing the
// scratch bitmaps per segment in the copy kernel: 1.64 ms.  A wave per packet
// in the copy: 0.77 against 0.67 ms on the same box.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "stream_kernels.hpp"
#include "stream_device.hpp"

namespace ugo {
namespace kern {

void stream_record_init(StreamRecord* r) {
  *r = StreamRecord{};
  r->pub.ngaps = 1;  // the gap list starts as one open gap (segment_sorter.go:27)
  r->fatal_idx = ~0ull;
  r->scan_u = ~0ull;
}

namespace {

// The statuses between the kernels, the clamped segment, the bitmap word
// arithmetic, ordered_one and copy_segment live in stream_device.hpp, shared
// with the set kernels (stream_set_kernels.hip).

// ------------------------------------------------------------ classify + claim
__global__ __launch_bounds__(256) void k_stream_classify(StreamArgs a) {
  __shared__ u64 s_end;
  if (threadIdx.x == 0) s_end = 0;
  __syncthreads();
  const u64 i = blockIdx.x * static_cast<u64>(kGroupsPerBlock) + threadIdx.x / kGroupLanes;
  const uint32_t lane = threadIdx.x % kGroupLanes;
  const bool valid = i < a.npk;
  const StreamRecord& R = *a.rec;
  const bool live = valid && R.inert == 0 && a.info[i].status == UGO_PKT_OK;
  const uint32_t ns = live ? nseg_of(a, i) : 0u;
  uint8_t* st = a.seg_status + i * a.max_segments;
  if (valid)
    for (uint32_t j = ns + lane; j < a.max_segments; j += kGroupLanes) st[j] = kNone;
  const u64 rp = R.pub.read_pos, head = R.pub.head_off, cap = a.cap;
  const bool hv = R.pub.head_valid != 0;
  u64 claim_end = 0;
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
      const u64 e = s.o + s.len, lo = s.o > rp ? s.o : rp;
      const u64 p0 = lo & ~63ull, nw = words_of(lo, e);
      bool anyc = s.o < rp, anyu = false;
      for (u64 k = lane; k < nw; k += kGroupLanes) {
        const u64 p = p0 + 64 * k, m = range_mask(p, lo, e), w = a.C[widx(p, cap)];
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
          const u64 m = range_mask(p, lo, e) & ~a.C[wi];
          if (m) {
            const u64 hit = atomicOr(a.claim + wi, m) & m;
            if (hit) atomicOr(a.cont + wi, hit);
          }
        }
        res = anyc ? kPartial : kCand;
        claim_end = e > claim_end ? e : claim_end;
      }
    }
    if (lane == 0) st[j] = static_cast<uint8_t>(res);
  }
  // how far k_stream_apply has to look: one atomic per block, spread over kEndShards words
  if (lane == 0 && claim_end != 0) atomicMax(&s_end, claim_end);
  __syncthreads();
  if (threadIdx.x == 0 && s_end != 0) atomicMax(&a.rec->claim_end[blockIdx.x % kEndShards], s_end);
}

// -------------------------------------------------------------------- resolve
__global__ __launch_bounds__(256) void k_stream_resolve(StreamArgs a) {
  const u64 i = blockIdx.x * static_cast<u64>(kGroupsPerBlock) + threadIdx.x / kGroupLanes;
  const uint32_t lane = threadIdx.x % kGroupLanes;
  if (i >= a.npk) return;
  StreamRecord& R = *a.rec;
  if (R.inert != 0 || a.info[i].status != UGO_PKT_OK) return;
  const uint32_t ns = nseg_of(a, i);
  uint8_t* st = a.seg_status + i * a.max_segments;
  const u64 rp = R.pub.read_pos, cap = a.cap;
  for (uint32_t j = 0; j < ns; ++j) {
    const uint32_t code = st[j];
    if (code < kPartial) continue;
    const Seg s = load_seg(a, i * a.max_segments + j);
    const u64 sw = widx(s.o, cap), sbit = 1ull << (s.o & 63);
    bool contested = code == kPartial;
    if (code == kFinCand) {
      contested = (a.cont[sw] & sbit) != 0;
    } else if (code == kCand) {
      const u64 e = s.o + s.len, lo = s.o;  // a candidate lies at or above read_pos
      const u64 p0 = lo & ~63ull, nw = words_of(lo, e);
      bool hit = false;
      for (u64 k = lane; k < nw; k += kGroupLanes) {
        const u64 p = p0 + 64 * k;
        hit |= (a.cont[widx(p, cap)] & range_mask(p, lo, e)) != 0;
      }
      contested = group_any(hit);
    }
    // An accepted segment's claim stays: k_stream_apply ORs what is left of the
    // claim bitmap into C a word at a time, without atomics.  Everyone else --
    // the contested, whose bytes the ordered pass decides, and empty segments,
    // whose claim is no byte -- takes the claim back (rare).
    if (code == kFinCand) {
      if (lane == 0) atomicAnd(a.claim + sw, ~sbit);
    } else if (contested) {
      const u64 e = s.o + s.len, lo = s.o > rp ? s.o : rp;
      const u64 p0 = lo & ~63ull, nw = words_of(lo, e);
      for (u64 k = lane; k < nw; k += kGroupLanes) {
        const u64 p = p0 + 64 * k, wi = widx(p, cap);
        const u64 m = range_mask(p, lo, e) & ~a.C[wi];  // what it claimed: C has not changed since
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
// What is left in the claim bitmap is exactly the accepted segments' bytes:
// C |= claim and claim = 0, a word per thread over [read_pos, highest claimed
// end), plain loads and stores.
__global__ __launch_bounds__(256) void k_stream_apply(StreamArgs a) {
  const StreamRecord& R = *a.rec;
  if (R.inert != 0) return;
  __shared__ u64 s_end;
  if (threadIdx.x == 0) s_end = 0;
  __syncthreads();
  if (threadIdx.x < kEndShards && R.claim_end[threadIdx.x] != 0) atomicMax(&s_end, R.claim_end[threadIdx.x]);
  __syncthreads();
  const u64 rp = R.pub.read_pos, end = s_end, cap = a.cap;
  if (end <= rp) return;
  const u64 p0 = rp & ~63ull, nw = words_of(rp, end);
  for (u64 k = blockIdx.x * 256ull + threadIdx.x; k < nw; k += 256ull * gridDim.x) {
    const u64 wi = widx(p0 + 64 * k, cap);
    const u64 c = a.claim[wi];
    if (c == 0) continue;
    a.claim[wi] = 0;
    a.C[wi] = c == ~0ull ? c : (a.C[wi] | c);
  }
}

// --------------------------------------------------------------- ordered pass
__global__ __launch_bounds__(kOrderedThreads) void k_stream_ordered(StreamArgs a) {
  StreamRecord& R = *a.rec;
  const uint32_t todo = R.n_contested;
  if (R.inert != 0 || todo == 0) return;
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
__global__ __launch_bounds__(256) void k_stream_copy(StreamArgs a) {
  StreamRecord& R = *a.rec;
  if (R.inert != 0) return;
  __shared__ u64 s_hi;
  __shared__ uint32_t s_cnt[5];  // accepted, duplicate, out of window, skipped packets, accepted data
  // what B needs of a packet's first segment, so that its lanes start on the bytes at once
  __shared__ ugo_pkt_segment s_seg0[kCopyPacketsPerBlock];
  __shared__ uint32_t s_ns[kCopyPacketsPerBlock], s_code0[kCopyPacketsPerBlock];
  if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_hi = 0;
  __syncthreads();
  const u64 first = blockIdx.x * static_cast<u64>(kCopyPacketsPerBlock);
  const u64 fatal = R.fatal_idx, rp = R.pub.read_pos, cap = a.cap;
  // A: one thread per packet takes the counters and hi from the statuses at or
  // before the fatal segment
  if (threadIdx.x < kCopyPacketsPerBlock) s_ns[threadIdx.x] = 0;  // no packet, or a skipped one
  if (threadIdx.x < kCopyPacketsPerBlock && first + threadIdx.x < a.npk) {
    const u64 i = first + threadIdx.x;
    if (a.info[i].status != UGO_PKT_OK) {
      if (i * a.max_segments <= fatal) atomicAdd(&s_cnt[3], 1u);
    } else {
      const uint32_t ns = nseg_of(a, i);
      s_ns[threadIdx.x] = ns;
      if (ns != 0) {
        s_code0[threadIdx.x] = a.seg_status[i * a.max_segments];
        s_seg0[threadIdx.x] = a.segs[i * a.max_segments];
      }
      uint32_t acc = 0, dup = 0, oow = 0;
      u64 hi = 0;
      for (uint32_t j = 0; j < ns; ++j) {
        const u64 idx = i * a.max_segments + j;
        if (idx > fatal) break;
        const uint32_t code = j == 0 ? s_code0[threadIdx.x] : a.seg_status[idx];
        if (code == kAccepted) {
          ++acc;
          const ugo_pkt_segment sg = j == 0 ? s_seg0[threadIdx.x] : a.segs[idx];
          if (sg.len != 0 && sg.offset + sg.len > hi) hi = sg.offset + sg.len;
        }
        dup += code == kDuplicate;
        oow += code == kOutOfWindow;
      }
      if (acc) atomicAdd(&s_cnt[0], acc);
      if (dup) atomicAdd(&s_cnt[1], dup);
      if (oow) atomicAdd(&s_cnt[2], oow);
      if (hi) {
        atomicMax(&s_hi, hi);
        s_cnt[4] = 1;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(reinterpret_cast<u64*>(&R.pub.accepted), static_cast<u64>(s_cnt[0]));
    if (s_cnt[1]) atomicAdd(reinterpret_cast<u64*>(&R.pub.duplicate), static_cast<u64>(s_cnt[1]));
    if (s_cnt[2]) atomicAdd(reinterpret_cast<u64*>(&R.pub.out_of_window), static_cast<u64>(s_cnt[2]));
    if (s_cnt[3]) atomicAdd(reinterpret_cast<u64*>(&R.pub.skipped_packets), static_cast<u64>(s_cnt[3]));
    if (s_hi) atomicMax(reinterpret_cast<u64*>(&R.pub.hi), s_hi);
    if (s_cnt[4]) R.accepted_data = 1;
  }
  // B: kCopyLanes lanes per packet
  constexpr uint32_t kGroups = 256u / kCopyLanes;
  const uint32_t grp = threadIdx.x / kCopyLanes, hl = threadIdx.x % kCopyLanes;
  for (uint32_t t = grp; t < kCopyPacketsPerBlock; t += kGroups) {
    const u64 i = first + t;
    const uint32_t ns = s_ns[t];
    for (uint32_t j = 0; j < ns; ++j) {
      const u64 idx = i * a.max_segments + j;
      const uint32_t code = j == 0 ? s_code0[t] : a.seg_status[idx];
      const Seg s = j == 0 ? to_seg(a, s_seg0[t]) : load_seg(a, idx);
      const bool indom = s.o >= rp && s.o - rp < cap;
      const u64 e = s.o + s.len, lo = s.o > rp ? s.o : rp;
      const bool ranged = s.len != 0 && !(s.o > rp + cap || s.len > rp + cap - s.o) && e > rp;
      const bool undo = idx > fatal && code == kAccepted;
      // only after a fatal: the contested it left behind still have their
      // contested bits, the accepted after it come out of C again
      const bool left = code == kContested;
      if (left && s.len == 0 && indom && hl == 0) a.cont[widx(s.o, cap)] = 0;
      if ((left || undo) && ranged) {
        const u64 p0 = lo & ~63ull, nw = words_of(lo, e);
        for (u64 k = hl; k < nw; k += kCopyLanes) {
          const u64 p = p0 + 64 * k, wi = widx(p, cap);
          if (left) a.cont[wi] = 0;
          if (undo) atomicAnd(a.C + wi, ~range_mask(p, lo, e));
        }
      }
      if (idx > fatal) {
        if (hl == 0) {
          if (undo) atomicAnd(a.S + widx(s.o, cap), ~(1ull << (s.o & 63)));
          if (code != kNone) a.seg_status[idx] = kNone;
        }
      } else if (code == kAccepted && s.len != 0) {
        copy_segment(a, i, s, hl);
      }
    }
  }
}

// -------------------------------------------------------------------- summary
__global__ __launch_bounds__(256) void k_stream_scan(StreamArgs a) {
  StreamRecord& R = *a.rec;
  if (R.inert != 0) return;
  const u64 rp = R.pub.read_pos, hi = R.pub.hi, cap = a.cap;
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
    const u64 unc = ~a.C[widx(p, cap)] & range_mask(p, rp, hi);
    if (unc == 0) continue;
    // a run starts at an uncovered byte whose predecessor is covered (or is below read_pos)
    const u64 prev_unc = p > rp ? (~a.C[widx(p - 64, cap)] >> 63) : 0ull;
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

__global__ void k_stream_finish(StreamArgs a) {
  StreamRecord& R = *a.rec;
  if (R.inert != 0) return;
  if (threadIdx.x < kEndShards) R.claim_end[threadIdx.x] = 0;
  if (threadIdx.x != 0) return;
  const u64 rp = R.pub.read_pos, hi = R.pub.hi;
  const u64 u = R.scan_u < hi ? R.scan_u : (hi > rp ? hi : rp);
  R.pub.ngaps = R.scan_runs + 1u;
  R.pub.readable = u - rp;
  R.pub.eof = (u - rp < a.cap && ((a.S[widx(u, a.cap)] >> (u & 63)) & 1ull)) ? 1 : 0;
  if (R.pub.err == 0 && R.accepted_data != 0 && R.pub.ngaps > UGO_STREAM_MAX_GAPS)
    R.pub.err = UGO_STREAM_TOO_MANY_GAPS;
  if (R.pub.err != 0) R.inert = 1;
  R.fatal_idx = ~0ull;
  R.scan_u = ~0ull;
  R.scan_runs = 0;
  R.n_contested = 0;
  R.accepted_data = 0;
}

// ----------------------------------------------------------------------- read
__global__ __launch_bounds__(256) void k_stream_read(StreamReadArgs a) {
  StreamRecord& R = *a.rec;
  const u64 rp = R.pub.read_pos, readable = R.pub.readable, cap = a.cap, capm = a.cap - 1;
  const u64 m = a.n < readable ? a.n : readable;
  const u64 e = rp + m;
  __shared__ u64 s_head;
  __shared__ uint32_t s_last;
  if (threadIdx.x == 0) s_head = 0;
  __syncthreads();
  const u64 gtid = blockIdx.x * 256ull + threadIdx.x, gsz = 256ull * gridDim.x;
  if (m != 0) {
    // the bytes: whole 16-B chunks of the window, then the ends
    if (a.dst != nullptr) {
      const u64 c0 = (rp + 15) >> 4, c1 = e >> 4;
      for (u64 c = c0 + gtid; c < c1; c += gsz) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.win + ((16 * c) & capm)));
        *reinterpret_cast<u32x4u*>(a.dst + (16 * c - rp)) = v;
      }
      if (blockIdx.x == 0 && threadIdx.x < 32) {
        const u64 head_end = e < 16 * c0 ? e : 16 * c0;
        const u64 tail_start = 16 * c1 > head_end ? 16 * c1 : head_end;
        const u64 x = threadIdx.x < 16 ? rp + threadIdx.x : tail_start + (threadIdx.x - 16);
        if (threadIdx.x < 16 ? x < head_end : x < e) a.dst[x - rp] = a.win[x & capm];
      }
    }
    // the bits: cleared, and the highest start bit among them noted
    const u64 p0 = rp & ~63ull, nw = words_of(rp, e);
    u64 best = 0;
    for (u64 k = gtid; k < nw; k += gsz) {
      const u64 p = p0 + 64 * k, wi = widx(p, cap), mk = range_mask(p, rp, e);
      u64 sb;
      if (mk == ~0ull) {
        sb = a.S[wi];
        if (sb) a.S[wi] = 0;
        a.C[wi] = 0;
      } else {
        sb = atomicAnd(a.S + wi, ~mk) & mk;
        atomicAnd(a.C + wi, ~mk);
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
    s_last = atomicAdd(&R.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (s_last == 0 || threadIdx.x != 0) return;
  // every block has read the record and cleared its bits: advance
  __threadfence();
  const u64 found = aload(&R.scan_head);
  if (m != 0) {
    const bool partly = m < readable && ((aload(a.S + widx(e, cap)) >> (e & 63)) & 1ull) == 0;
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
  *a.n_read = m;
  if (a.eof) *a.eof = (m == readable && R.pub.eof != 0) ? 1 : 0;
  R.scan_head = 0;
  R.ticket = 0;
}

}  // namespace

hipError_t launch_stream_deliver(const StreamArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const uint32_t gblocks = static_cast<uint32_t>((a.npk + kGroupsPerBlock - 1) / kGroupsPerBlock);
  const uint32_t cblocks = static_cast<uint32_t>((a.npk + kCopyPacketsPerBlock - 1) / kCopyPacketsPerBlock);
  launch(kKStreamDeliver, k_stream_classify, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_stream_resolve, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_stream_apply, dim3(kScanBlocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_stream_ordered, dim3(1), dim3(kOrderedThreads), 0, s, a);
  launch(kKStreamDeliver, k_stream_copy, dim3(cblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_stream_scan, dim3(kScanBlocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_stream_finish, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_read(const StreamReadArgs& a, hipStream_t s) {
  const uint64_t want = a.n < a.cap ? a.n : a.cap;
  uint64_t blocks = (want + 256 * 64 - 1) / (256 * 64);  // 4 chunks per thread
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  launch(kKStreamRead, k_stream_read, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
