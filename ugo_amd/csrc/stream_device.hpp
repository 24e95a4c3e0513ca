// stream_device.hpp -- device helpers of the stream-delivery kernels
// (stream_kernels.hip): the statuses between the kernels of a call, the clamped
// segment, the bitmap word arithmetic, one segment of the ordered pass and the
// realigning copy of one segment.  The helpers that need the batch take it as
// `b` (pkts, pad, info, segs, seg_status, slot, max_segments: StreamArgs and
// StreamSetArgs name these alike) and the connection as `e` (win, C, S, claim,
// cont, rec, cap: StreamArgs itself for the single entry points, a
// StreamSetEntry for a member of a set).  Device code only: include from a .hip
// file, after stream_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "stream_kernels.hpp"

namespace ugo {
namespace kern {
namespace {

typedef unsigned long long u64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

constexpr uint32_t kGroupLanes = 16;  // lanes per packet in classify / resolve
constexpr uint32_t kGroupsPerBlock = 256 / kGroupLanes;
constexpr uint32_t kCopyLanes = 32;        // lanes per packet in the copy
constexpr uint32_t kCopyPacketsPerBlock = 64;
constexpr uint32_t kScanBlocks = 1024;
constexpr uint32_t kOrderedThreads = 1024;
constexpr uint32_t kEndShards = 64;
static_assert(kEndShards == sizeof(StreamRecord::claim_end) / sizeof(unsigned long long), "one word per shard");

// statuses between the kernels of one call (never left in seg_status)
enum : uint32_t {
  kNone = UGO_STREAM_NONE,
  kAccepted = UGO_STREAM_ACCEPTED,
  kDuplicate = UGO_STREAM_DUPLICATE,
  kOutOfWindow = UGO_STREAM_OUT_OF_WINDOW,
  kOverlap = UGO_STREAM_OVERLAP,
  kPartial = 0xFC,    // partly covered before the call: always ordered
  kFinCand = 0xFD,    // empty segment that claimed its offset
  kCand = 0xFE,       // wholly uncovered before the call, claimed its range
  kContested = 0xFF,  // for the ordered pass
};

struct Seg {
  u64 o;
  uint32_t data_off, len, avail;
};

template <class B>
__device__ __forceinline__ Seg to_seg(const B& b, const ugo_pkt_segment& s) {
  Seg r;
  r.o = s.offset;
  r.data_off = s.data_off;
  r.len = s.len;
  uint32_t av = s.avail < s.len ? s.avail : s.len;
  const u64 room = s.data_off < b.slot ? b.slot - s.data_off : 0;  // never read past the slot
  r.avail = av < room ? av : static_cast<uint32_t>(room);
  return r;
}
template <class B>
__device__ __forceinline__ Seg load_seg(const B& b, u64 idx) {
  return to_seg(b, b.segs[idx]);
}

// The word that holds stream positions [p, p + 64) (p a multiple of 64): the
// bits of [max(p, lo), min(p + 64, e)).  lo < p + 64 and e > p.
__device__ __forceinline__ u64 range_mask(u64 p, u64 lo, u64 e) {
  const u64 a = lo > p ? lo - p : 0;
  const u64 b = e - p;
  const u64 hi = b >= 64 ? ~0ull : ((1ull << b) - 1ull);
  return hi & ~((1ull << a) - 1ull);
}
__device__ __forceinline__ u64 widx(u64 p, u64 cap) { return (p & (cap - 1)) >> 6; }
__device__ __forceinline__ u64 words_of(u64 lo, u64 e) { return (e - (lo & ~63ull) + 63) >> 6; }
__device__ __forceinline__ u64 aload(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// "any lane of my 16-lane group": the groups of a wave branch apart, but the
// lanes of one group never do, so the group's ballot bits are all its own.
__device__ __forceinline__ bool group_any(bool v) {
  const u64 b = __ballot(v);
  const uint32_t g = (threadIdx.x & 63u) / kGroupLanes;
  return ((b >> (g * kGroupLanes)) & ((1u << kGroupLanes) - 1u)) != 0;
}

template <class B>
__device__ __forceinline__ uint32_t nseg_of(const B& b, u64 i) {
  const uint32_t n = b.info[i].n_segments;
  return n < b.max_segments ? n : b.max_segments;
}

// --------------------------------------------------------------- ordered pass
// One contested segment, by the 64 lanes of wave 0: steps 2-7 of the rule
// against the bitmaps as they are now.  Reads and writes go to L2 (atomics), and
// a fence ends each segment, so the next one sees this one's bits.
template <class B, class E>
__device__ bool ordered_one(const B& b, const E& e, u64 idx, uint32_t lane, u64 rp, u64 head, bool hv) {
  const u64 cap = e.cap;
  const Seg s = load_seg(b, idx);
  const bool indom = s.o >= rp && s.o - rp < cap;
  u64* sw = e.S + widx(s.o, cap);
  const u64 sbit = 1ull << (s.o & 63);
  uint32_t res;
  if ((hv && s.o == head) || (indom && (aload(sw) & sbit))) {
    res = kDuplicate;
  } else if (s.len == 0) {
    if (lane == 0) atomicOr(sw, sbit);
    res = kAccepted;
  } else {
    const u64 e2 = s.o + s.len, lo = s.o > rp ? s.o : rp;
    const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
    bool anyc = s.o < rp, anyu = false;
    for (u64 k = lane; k < nw; k += 64) {
      const u64 p = p0 + 64 * k, m = range_mask(p, lo, e2), w = aload(e.C + widx(p, cap));
      anyc |= (w & m) != 0;
      anyu |= (~w & m) != 0;
    }
    anyc = __any(anyc);
    anyu = __any(anyu);
    if (!anyc) {
      for (u64 k = lane; k < nw; k += 64) {
        const u64 p = p0 + 64 * k;
        atomicOr(e.C + widx(p, cap), range_mask(p, lo, e2));
      }
      if (lane == 0) atomicOr(sw, sbit);
      res = kAccepted;
    } else if (!anyu) {
      res = kDuplicate;
    } else {
      res = kOverlap;
      if (lane == 0) {
        e.rec->pub.err = UGO_STREAM_OVERLAP;
        e.rec->pub.err_packet = idx / b.max_segments;
        e.rec->pub.err_segment = static_cast<uint32_t>(idx % b.max_segments);
        e.rec->fatal_idx = idx;
      }
    }
  }
  // its contested bits have served (k_resolve read them)
  if (s.len == 0) {
    if (lane == 0) *(e.cont + widx(s.o, cap)) = 0;
  } else {
    const u64 e2 = s.o + s.len, lo = s.o > rp ? s.o : rp;
    const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
    for (u64 k = lane; k < nw; k += 64) e.cont[widx(p0 + 64 * k, cap)] = 0;
  }
  if (lane == 0) b.seg_status[idx] = static_cast<uint8_t>(res);
  __threadfence();
  return res == kOverlap;
}

// ----------------------------------------------------------------------- copy
__device__ __forceinline__ u32x4 ldu16(const uint8_t* p) { return *reinterpret_cast<const u32x4u*>(p); }

__device__ __forceinline__ uint32_t seg_byte(const uint8_t* src, const uint8_t* padp, uint32_t k, uint32_t avail) {
  if (k >= avail) return 0u;
  uint32_t v = src[k];
  if (padp) v ^= padp[k];
  return v;
}

// The accepted segment's bytes into the window, by kCopyLanes lanes.  Whole
// 16-B chunks of the stream (they are whole chunks of the window too, and none
// straddles the wrap): one unaligned 16-B load, the pad XOR, one aligned
// nontemporal 16-B store.  The up-to-15 bytes on either side: byte stores, one
// per lane.  No byte outside [o, o + len) is written.
template <class B>
__device__ __forceinline__ void copy_segment(const B& b, uint8_t* win, u64 cap, u64 i, const Seg& s, uint32_t hl) {
  const uint8_t* src = b.pkts + i * b.slot + s.data_off;
  const uint8_t* padp = b.pad ? b.pad + s.data_off : nullptr;
  const u64 o = s.o, e = s.o + s.len, capm = cap - 1;
  const u64 c0 = (o + 15) >> 4, c1 = e >> 4;  // whole chunks [c0, c1)
  for (u64 c = c0 + hl; c < c1; c += 4ull * kCopyLanes) {
    u32x4 v[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const u64 cc = c + q * kCopyLanes;
      if (cc < c1) {
        const uint32_t k = static_cast<uint32_t>(16 * cc - o);
        if (k + 16u <= s.avail) {
          v[q] = ldu16(src + k);
          if (padp) v[q] ^= ldu16(padp + k);
        } else {  // the chunk where a truncated segment ends, and its zero tail
          uint32_t w[4] = {0u, 0u, 0u, 0u};
          if (k < s.avail)
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b) w[b >> 2] |= seg_byte(src, padp, k + b, s.avail) << (8u * (b & 3u));
          v[q] = u32x4{w[0], w[1], w[2], w[3]};
        }
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const u64 cc = c + q * kCopyLanes;
      if (cc < c1) __builtin_nontemporal_store(v[q], reinterpret_cast<u32x4*>(win + ((16 * cc) & capm)));
    }
  }
  const u64 head_end = e < 16 * c0 ? e : 16 * c0;                   // head bytes [o, head_end)
  const u64 tail_start = 16 * c1 > head_end ? 16 * c1 : head_end;  // tail bytes [tail_start, e)
  const u64 x = hl < 16 ? o + hl : tail_start + (hl - 16);
  if (hl < 16 ? x < head_end : x < e)
    win[x & capm] = static_cast<uint8_t>(seg_byte(src, padp, static_cast<uint32_t>(x - o), s.avail));
}

}  // namespace
}  // namespace kern
}  // namespace ugo
