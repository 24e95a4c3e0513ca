// stream_kernels.hip -- stream delivery on the device (include/ugo_stream.h):
// batch Conn.handleSegment / segmentSorter.push into a receive window, and
// Conn.Read out of it -- for one window (ugo_fec_stream_deliver / _read) and
// for a set of windows whose packets share a batch (ugo_fec_stream_set_*).
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
// Every kernel is one body, a template on a connection policy, instantiated
// twice: k_*<One> over StreamArgs / StreamReadArgs for the single entry
// points, k_*<Many> over StreamSetArgs / StreamSetReadArgs for a set, where
// conn_of[i] names the member packet i belongs to.  Per member a set call
// gives what the single call gives for the member's subsequence of the batch.
// The policies (below) answer what differs; the rule per segment, the bitmap
// loops, the tile walk, the copy's loops and the read are written once.
//
// Launches of one deliver call, all kernel class kKStreamDeliver:
//   k_classify  16 lanes per packet: statuses by the pre-call state, claims.
//               Many: window, bitmaps and record come from table[conn_of[i]]; a
//               packet of no connection (conn_of >= nconn) gets a zero row and
//               is looked at by no later kernel; claim_end is reduced per
//               connection of the block, and the record is marked `touched`.
//   k_resolve   16 lanes per packet: accept the uncontested, mark the contested
//   k_apply     a word per thread: C |= the accepted segments' claims, claims
//               cleared.  One: kScanBlocks blocks.  Many: the connection on
//               blockIdx.y (.z above 32,768), wblocks blocks each -- sized from
//               the largest member window -- and a block of an untouched
//               connection leaves after one load.
//   k_ordered   one block per connection; wave 0 applies the contested in
//               arrival order.  Many: at work only where n_contested != 0; it
//               walks the batch's statuses and takes the contested entries
//               whose packet is its own.  done == todo and the fatal stop are
//               per connection; no block waits for another.
//   k_copy      64 packets per block: counters, hi, undo after a fatal, then
//               half a wave per packet copies the accepted bytes (the hot
//               path).  Many: phase A (a thread per packet) reads fatal_idx,
//               read_pos and cap of the packet's own connection and leaves
//               them with the window in the packet's LDS descriptor, so that
//               the copying lanes of phase B start on the bytes at once;
//               counters, hi and accepted_data are summed per connection of
//               the block, at the LDS slot of the connection's first packet
//               (found with 64 readlanes; skipped when the wave holds one
//               connection), and that packet's thread takes them to the record.
//   k_scan      gaps and the first uncovered byte of [read_pos, hi); grid as apply
//   k_finish    ngaps, readable, eof, the gap limit.  One: one block of 64
//               threads.  Many: 16 lanes per connection; clears `touched`.
// A read is one kernel, k_read (class kKStreamRead); the block of a connection
// that finishes last advances the record.  Many: the connection on blockIdx.y,
// rblocks blocks each (the grid held near 4,096 blocks in all); ticket,
// scan_head and the epilogue are the connection's own, and a connection with
// n[c] == 0 writes its two outputs and touches nothing of its record.
// k_set_gather collects the public records for ugo_fec_stream_set_state.
//
// k_classify<Many>, k_resolve<Many> and k_copy<Many> read a packet's table
// entry and record through Many::load_conn: scalar loads for the connection of
// the wave's first active lane, per-lane loads for the wave's other
// connections.  group_any (classify, resolve) ballots within 16-lane groups;
// neighbouring groups of a wave differ in connection and cap there.  Every
// branch on the table entry is uniform over a group, so no lane leaves its
// group.
//
// gfx950, -O3, -Rpass-analysis=kernel-resource-usage (VGPRs / SGPRs / LDS bytes
// per block / waves per SIMD; no kernel uses scratch or spills):
//                 <One>                   <Many>
//   k_classify    48 /  72 /    8 / 8     64 /  60 /  192 / 8
//   k_resolve     36 /  55 /    0 / 8     52 /  41 /    0 / 8
//   k_apply       14 /  22 /    8 / 8     14 /  28 /    8 / 8
//   k_ordered     62 / 106 / 4360 / 7     68 / 104 / 4360 / 7
//   k_copy        80 /  93 / 1568 / 6     94 /  77 / 5632 / 5
//   k_scan        20 /  32 /   16 / 8     20 /  32 /   16 / 8
//   k_finish       6 /  21 /    0 / 8     15 /  14 /    0 / 8
//   k_read        21 /  58 /   16 / 8     22 /  62 /   16 / 8
//   k_set_gather                           8 /  14 /    0 / 8
// (k_copy: the 14 VGPRs more of <Many> are the per-packet window, cap, read_pos
// and fatal_idx that <One> keeps in SGPRs.)
//
// Measured, one window (tools/stream_deliver_probe.py, 851,968 packets with one
// 1400-B segment, slot 1488, RC4 pad, 2-GiB window; DESIGN.md §3.7,
// profiles/stream_deliver/): 1.28 ms per call in order -- classify 0.30,
// resolve 0.12, apply 0.07, copy 0.74, scan 0.05 -- against 0.37 ms for an nt
// copy of the same bytes; the ordered pass 1.84 us per contested segment.
// Setting C per segment in resolve (atomics on the end words) and clearing the
// scratch bitmaps per segment in the copy kernel: 1.64 ms.  A wave per packet
// in the copy: 0.77 against 0.67 ms on the same box.  Sets:
// tools/stream_set_probe.py, DESIGN.md §3.8, profiles/stream_set/; both forms
// before and after the two files became one: profiles/stream_unify/.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "stream_kernels.hpp"
#include "stream_set_kernels.hpp"
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

constexpr uint32_t kConnFold = 32768;  // connections on blockIdx.y; the rest go to blockIdx.z

__device__ __forceinline__ uint32_t block_conn() { return blockIdx.z * kConnFold + blockIdx.y; }

dim3 conn_grid(uint32_t x, uint32_t nconn) {
  return dim3(x, nconn < kConnFold ? nconn : kConnFold, (nconn + kConnFold - 1) / kConnFold);
}

// What the lanes of a packet need of its connection (classify, resolve, copy)
// is the policy's Conn: the connection part `e` (win, C, S, claim, cont, rec,
// cap) and the fields of the record that hold for the whole kernel -- inert(),
// rp(), head(), hv(), fatal().

// What phase B of the copy needs of a packet's connection.
struct CopyDesc {
  uint8_t* win;
  u64 cap, rp, fatal;
};

// ------------------------------------------------------ the connection policy
// What differs between the two forms.  The kernels that work per packet
// (classify, resolve, copy; ordered's filter) ask an object of the policy.  The
// kernels that work per connection (apply, ordered, scan, finish, read) find
// their connection in their first lines under `if constexpr (P::kMany)`, and so
// does classify's claim_end reduction: a kernel that hands its argument struct
// to a function by reference is compiled without the proof that the pointers
// loaded from the table are global and not clobbered, and its loads of the
// record turn from scalar into flat ones (k_scan<Many>: 22 VGPRs for 20,
// k_read<Many>: 31 for 22).
//
// One: the single entry points.  The arguments are the connection; its record
// is read uniformly, with no conn_of and no table in front of it.
struct One {
  typedef StreamArgs Args;
  typedef StreamReadArgs ReadArgs;
  struct Conn {  // read from the record where the body asks, uniformly
    const StreamArgs& e;
    __device__ __forceinline__ uint32_t inert() const { return e.rec->inert; }
    __device__ __forceinline__ u64 rp() const { return e.rec->pub.read_pos; }
    __device__ __forceinline__ u64 head() const { return e.rec->pub.head_off; }
    __device__ __forceinline__ bool hv() const { return e.rec->pub.head_valid != 0; }
    __device__ __forceinline__ u64 fatal() const { return e.rec->fatal_idx; }
  };
  typedef StreamArgs Entry;  // the connection part of the arguments: the arguments
  typedef StreamReadArgs ReadEntry;
  static constexpr bool kMany = false;
  static constexpr uint32_t kCopySlots = 1;     // the block sums its counters in one place
  static constexpr uint32_t kFinishLanes = 64;  // one block of 64 threads finishes the connection
  static constexpr bool kBlockGated = true;     // the copy's blocks leave together when the connection is inert
  struct EndLds {
    u64 end;
  };
  struct CopyStash {};

  const StreamArgs& a;
  __device__ __forceinline__ explicit One(const StreamArgs& a_) : a(a_) {}

  // a packet's connection, and what its lanes need of it
  __device__ __forceinline__ uint32_t packet_conn(u64, bool valid) const { return valid ? 0u : UGO_STREAM_NO_CONN; }
  __device__ __forceinline__ Conn load_conn(uint32_t) const { return {a}; }

  // a block of apply / ordered / scan / finish: whether its connection has work
  __device__ __forceinline__ static uint32_t finish_conn() { return threadIdx.x / kFinishLanes; }
  __device__ __forceinline__ static bool idle(const StreamRecord& R) { return R.inert != 0; }
  __device__ __forceinline__ static void finished(StreamRecord&) {}

  // ordered: every contested entry is this connection's
  __device__ __forceinline__ uint32_t own(uint32_t mask, u64, uint32_t) const { return mask; }

  // copy
  __device__ __forceinline__ bool block_idle() const { return a.rec->inert != 0; }
  __device__ __forceinline__ static uint32_t leader(uint32_t, uint32_t) { return 0; }
  __device__ __forceinline__ static void stash(CopyStash&, uint32_t, uint32_t, const CopyDesc&) {}
  __device__ __forceinline__ static CopyDesc fetch(const CopyStash&, uint32_t, const CopyDesc& mine) { return mine; }
  __device__ __forceinline__ const StreamArgs& stashed_entry(const CopyStash&, uint32_t) const { return a; }
};

// Many: the receive-window sets.  A packet's connection is table[conn_of[i]].
struct Many {
  typedef StreamSetArgs Args;
  typedef StreamSetReadArgs ReadArgs;
  struct Conn {  // loaded once per packet by load_conn
    StreamSetEntry e;
    u64 rp_, head_, fatal_;
    uint32_t inert_;
    bool hv_;
    __device__ __forceinline__ uint32_t inert() const { return inert_; }
    __device__ __forceinline__ u64 rp() const { return rp_; }
    __device__ __forceinline__ u64 head() const { return head_; }
    __device__ __forceinline__ bool hv() const { return hv_; }
    __device__ __forceinline__ u64 fatal() const { return fatal_; }
  };
  typedef StreamSetEntry Entry;
  typedef StreamSetEntry ReadEntry;
  static constexpr bool kMany = true;
  static constexpr uint32_t kCopySlots = kCopyPacketsPerBlock;  // counters at the slot of a connection's first packet
  static constexpr uint32_t kFinishLanes = 16;
  static constexpr bool kBlockGated = false;
  struct EndLds {
    u64 end[kGroupsPerBlock];
    uint32_t conn[kGroupsPerBlock];
  };
  struct CopyStash {
    uint8_t* win[kCopyPacketsPerBlock];
    u64 cap[kCopyPacketsPerBlock], rp[kCopyPacketsPerBlock], fatal[kCopyPacketsPerBlock];
    uint32_t conn[kCopyPacketsPerBlock];
  };

  const StreamSetArgs& g;
  __device__ __forceinline__ explicit Many(const StreamSetArgs& g_) : g(g_) {}

  // conn_of[i], or UGO_STREAM_NO_CONN for no packet and for anything >= nconn
  __device__ __forceinline__ uint32_t packet_conn(u64 i, bool valid) const {
    const uint32_t c = valid ? g.conn_of[i] : UGO_STREAM_NO_CONN;
    return c < g.nconn ? c : UGO_STREAM_NO_CONN;
  }
  // c is a member's index or UGO_STREAM_NO_CONN (then nothing is loaded).  The
  // connection of the wave's first active lane goes through a uniform index and
  // a global-address-space pointer -- scalar loads, once for the wave, and all
  // there is while a wave holds one connection -- the other connections of the
  // wave per lane.  (Vector loads of a record that every block's atomics go to
  // cost the copy kernel 0.5 ms at 852k packets of one connection; a load
  // through a flat pointer is never scalar.)
  __device__ __forceinline__ Conn load_conn(uint32_t c) const {
    typedef const __attribute__((address_space(1))) StreamRecord* GlobalRecord;
    Conn s{};
    const uint32_t cu = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(c)));
    if (cu != UGO_STREAM_NO_CONN) {
      s.e = g.table[cu];
      const GlobalRecord r = (GlobalRecord)s.e.rec;
      s.rp_ = r->pub.read_pos;
      s.head_ = r->pub.head_off;
      s.hv_ = r->pub.head_valid != 0;
      s.fatal_ = r->fatal_idx;
      s.inert_ = r->inert;
    }
    if (c != cu && c != UGO_STREAM_NO_CONN) {
      s.e = g.table[c];
      const StreamRecord* r = s.e.rec;
      s.rp_ = r->pub.read_pos;
      s.head_ = r->pub.head_off;
      s.hv_ = r->pub.head_valid != 0;
      s.fatal_ = r->fatal_idx;
      s.inert_ = r->inert;
    }
    return s;
  }

  __device__ __forceinline__ static uint32_t finish_conn() {
    return blockIdx.x * (256u / kFinishLanes) + threadIdx.x / kFinishLanes;
  }
  // no packet of this call: the record stays bit for bit (touched implies not inert)
  __device__ __forceinline__ static bool idle(const StreamRecord& R) { return R.touched == 0; }
  __device__ __forceinline__ static void finished(StreamRecord& R) { R.touched = 0; }

  // ordered: of a thread's 16 entries from `first`, this connection's (contested entries are rare)
  __device__ __forceinline__ uint32_t own(uint32_t mask, u64 first, uint32_t c) const {
    for (uint32_t m = mask; m != 0; m &= m - 1) {
      const uint32_t b = static_cast<uint32_t>(__builtin_ctz(m));
      if (g.conn_of[(first + b) / g.max_segments] != c) mask &= ~(1u << b);
    }
    return mask;
  }

  // copy.  leader: the first packet of the block with my connection (phase A is wave 0)
  __device__ __forceinline__ bool block_idle() const { return false; }
  __device__ __forceinline__ static uint32_t leader(uint32_t c, uint32_t t) {
    static_assert(kCopyPacketsPerBlock == 64, "phase A is one wave: the readlane search relies on it");
    if (__all(c == static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(c))))) return 0;
    uint32_t l = t;
#pragma unroll
    for (int k = static_cast<int>(kCopyPacketsPerBlock) - 1; k >= 0; --k)
      if (static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(c), k)) == c) l = k;
    return l;
  }
  __device__ __forceinline__ static void stash(CopyStash& L, uint32_t t, uint32_t c, const CopyDesc& mine) {
    L.conn[t] = c;
    L.win[t] = mine.win;
    L.cap[t] = mine.cap;
    L.rp[t] = mine.rp;
    L.fatal[t] = mine.fatal;
  }
  __device__ __forceinline__ static CopyDesc fetch(const CopyStash& L, uint32_t p, const CopyDesc&) {
    return {L.win[p], L.cap[p], L.rp[p], L.fatal[p]};
  }
  __device__ __forceinline__ const StreamSetEntry& stashed_entry(const CopyStash& L, uint32_t p) const {
    return g.table[L.conn[p]];
  }
};

// ------------------------------------------------------------ classify + claim
template <class P>
__global__ __launch_bounds__(256) void k_classify(typename P::Args a) {
  __shared__ typename P::EndLds s_end;
  const P pol(a);
  if constexpr (!P::kMany) {
    if (threadIdx.x == 0) s_end.end = 0;
    __syncthreads();
  }
  const u64 i = blockIdx.x * static_cast<u64>(kGroupsPerBlock) + threadIdx.x / kGroupLanes;
  const uint32_t lane = threadIdx.x % kGroupLanes;
  const bool valid = i < a.npk;
  const uint32_t c = pol.packet_conn(i, valid);
  const typename P::Conn cs = pol.load_conn(c);
  // c, and with it every branch on the connection below, is uniform over the
  // group.  No connection: a zero row, and no later kernel looks at the packet.
  const auto& e = cs.e;
  const bool open = c != UGO_STREAM_NO_CONN && cs.inert() == 0;
  const bool live = open && a.info[i].status == UGO_PKT_OK;
  const uint32_t ns = live ? nseg_of(a, i) : 0u;
  uint8_t* st = a.seg_status + i * a.max_segments;
  if (valid)
    for (uint32_t j = ns + lane; j < a.max_segments; j += kGroupLanes) st[j] = kNone;
  const u64 rp = cs.rp(), head = cs.head(), cap = e.cap;
  const bool hv = cs.hv();
  u64 claim_end = 0;
  {
    for (uint32_t j = 0; j < ns; ++j) {
      const Seg s = load_seg(a, i * a.max_segments + j);
      const bool indom = s.o >= rp && s.o - rp < cap;
      const u64 sbit = 1ull << (s.o & 63);
      uint32_t res;
      if ((hv && s.o == head) || (indom && (e.S[widx(s.o, cap)] & sbit))) {
        res = kDuplicate;
      } else if (s.len == 0) {
        res = indom ? kFinCand : kOutOfWindow;
        if (indom && lane == 0) {
          const u64 old = atomicOr(e.claim + widx(s.o, cap), sbit);
          if (old & sbit) atomicOr(e.cont + widx(s.o, cap), sbit);
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
          const u64 p = p0 + 64 * k, m = range_mask(p, lo, e2), w = e.C[widx(p, cap)];
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
            const u64 m = range_mask(p, lo, e2) & ~e.C[wi];
            if (m) {
              const u64 hit = atomicOr(e.claim + wi, m) & m;
              if (hit) atomicOr(e.cont + wi, hit);
            }
          }
          res = anyc ? kPartial : kCand;
          claim_end = e2 > claim_end ? e2 : claim_end;
        }
      }
      if (lane == 0) st[j] = static_cast<uint8_t>(res);
    }
  }
  // How far k_apply has to look, spread over kEndShards words of the record.
  if constexpr (!P::kMany) {  // one atomic per block
    if (lane == 0 && claim_end != 0) atomicMax(&s_end.end, claim_end);
    __syncthreads();
    if (threadIdx.x == 0 && s_end.end != 0) atomicMax(&a.rec->claim_end[blockIdx.x % kEndShards], s_end.end);
  } else {  // one per connection of the block, by the first group that holds it; the record is touched
    const uint32_t grp = threadIdx.x / kGroupLanes;
    if (lane == 0) {
      s_end.conn[grp] = open ? c : UGO_STREAM_NO_CONN;
      s_end.end[grp] = claim_end;
    }
    __syncthreads();
    if (lane == 0 && open) {
      bool first = true;
      u64 end = 0;
      for (uint32_t k = 0; k < kGroupsPerBlock; ++k) {
        if (s_end.conn[k] != c) continue;
        first &= k >= grp;
        end = s_end.end[k] > end ? s_end.end[k] : end;
      }
      if (first) {
        e.rec->touched = 1;
        if (end != 0) atomicMax(&e.rec->claim_end[blockIdx.x % kEndShards], end);
      }
    }
  }
}

// -------------------------------------------------------------------- resolve
template <class P>
__global__ __launch_bounds__(256) void k_resolve(typename P::Args a) {
  const u64 i = blockIdx.x * static_cast<u64>(kGroupsPerBlock) + threadIdx.x / kGroupLanes;
  const uint32_t lane = threadIdx.x % kGroupLanes;
  if (i >= a.npk) return;
  const P pol(a);
  const uint32_t c = pol.packet_conn(i, true);
  if (c == UGO_STREAM_NO_CONN) return;
  const typename P::Conn cs = pol.load_conn(c);
  const auto& e = cs.e;
  StreamRecord& R = *e.rec;
  if (cs.inert() != 0 || a.info[i].status != UGO_PKT_OK) return;
  const uint32_t ns = nseg_of(a, i);
  uint8_t* st = a.seg_status + i * a.max_segments;
  const u64 rp = cs.rp(), cap = e.cap;
  for (uint32_t j = 0; j < ns; ++j) {
    const uint32_t code = st[j];
    if (code < kPartial) continue;
    const Seg s = load_seg(a, i * a.max_segments + j);
    const u64 sw = widx(s.o, cap), sbit = 1ull << (s.o & 63);
    bool contested = code == kPartial;
    if (code == kFinCand) {
      contested = (e.cont[sw] & sbit) != 0;
    } else if (code == kCand) {
      const u64 e2 = s.o + s.len, lo = s.o;  // a candidate lies at or above read_pos
      const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
      bool hit = false;
      for (u64 k = lane; k < nw; k += kGroupLanes) {
        const u64 p = p0 + 64 * k;
        hit |= (e.cont[widx(p, cap)] & range_mask(p, lo, e2)) != 0;
      }
      contested = group_any(hit);
    }
    // An accepted segment's claim stays: k_apply ORs what is left of the claim
    // bitmap into C a word at a time, without atomics.  Everyone else -- the
    // contested, whose bytes the ordered pass decides, and empty segments,
    // whose claim is no byte -- takes the claim back (rare).
    if (code == kFinCand) {
      if (lane == 0) atomicAnd(e.claim + sw, ~sbit);
    } else if (contested) {
      const u64 e2 = s.o + s.len, lo = s.o > rp ? s.o : rp;
      const u64 p0 = lo & ~63ull, nw = words_of(lo, e2);
      for (u64 k = lane; k < nw; k += kGroupLanes) {
        const u64 p = p0 + 64 * k, wi = widx(p, cap);
        const u64 m = range_mask(p, lo, e2) & ~e.C[wi];  // what it claimed: C has not changed since
        if (m) atomicAnd(e.claim + wi, ~m);
      }
    }
    if (lane == 0) {
      if (contested) {
        atomicAdd(&R.n_contested, 1u);
      } else {
        atomicOr(e.S + sw, sbit);
      }
      st[j] = static_cast<uint8_t>(contested ? kContested : kAccepted);
    }
  }
}

// ---------------------------------------------------------------------- apply
// What is left in the claim bitmap is exactly the accepted segments' bytes:
// C |= claim and claim = 0, a word per thread over [read_pos, highest claimed
// end), plain loads and stores.
template <class P>
__global__ __launch_bounds__(256) void k_apply(typename P::Args a) {
  const uint32_t c = P::kMany ? block_conn() : 0;
  typename P::Entry e;
  if constexpr (P::kMany) {
    if (c >= a.nconn) return;
    e = a.table[c];
  } else {
    e = a;
  }
  const StreamRecord& R = *e.rec;
  if (P::idle(R)) return;
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
// One block per connection: a walk over the whole batch's statuses in tiles of
// 16 entries per thread, wave 0 taking the connection's contested entries in
// arrival order.
template <class P>
__global__ __launch_bounds__(kOrderedThreads) void k_ordered(typename P::Args a) {
  const uint32_t c = P::kMany ? block_conn() : 0;
  typename P::Entry e;
  if constexpr (P::kMany) {
    if (c >= a.nconn) return;
    e = a.table[c];
  } else {
    e = a;
  }
  StreamRecord& R = *e.rec;
  if (P::kMany && P::idle(R)) return;  // a block of an untouched connection leaves after the one load
  const uint32_t todo = R.n_contested;
  if (P::idle(R) || todo == 0) return;
  const P pol(a);
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
    mask = pol.own(mask, first, c);
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
            const bool fatal = ordered_one(a, e, base + 16ull * (t0 + t) + b, tid, rp, head, hv);
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
template <class P>
__global__ __launch_bounds__(256) void k_copy(typename P::Args a) {
  constexpr uint32_t N = kCopyPacketsPerBlock;
  const P pol(a);
  if (pol.block_idle()) return;
  // per connection of the block (P::kCopySlots: one, or the slot of the
  // connection's first packet): accepted, duplicate, out of window, skipped
  // packets, accepted data; hi
  __shared__ u64 s_hi[P::kCopySlots];
  __shared__ uint32_t s_cnt[P::kCopySlots][5];
  // what B needs of a packet, so that its lanes start on the bytes at once: its
  // first segment, and what the policy stashes of its connection
  __shared__ ugo_pkt_segment s_seg0[N];
  __shared__ uint32_t s_ns[N], s_code0[N];
  __shared__ typename P::CopyStash s_conn;
  const uint32_t t = threadIdx.x;
  for (uint32_t k = t; k < 5 * P::kCopySlots; k += 256) (&s_cnt[0][0])[k] = 0;
  if (t < P::kCopySlots) s_hi[t] = 0;
  __syncthreads();
  const u64 first = blockIdx.x * static_cast<u64>(N);
  uint32_t leader = 0;
  // A: one thread per packet takes the counters and hi from the statuses at or
  // before its connection's fatal segment
  if (t < N) s_ns[t] = 0;  // no packet, no connection, an inert connection or a skipped packet
  const u64 i = first + t;
  uint32_t c = t < N ? pol.packet_conn(i, i < a.npk) : UGO_STREAM_NO_CONN;
  const typename P::Conn cs = pol.load_conn(c);  // nothing is loaded for the waves past the first
  const CopyDesc mine = {cs.e.win, cs.e.cap, cs.rp(), cs.fatal()};
  if (t < N) {
    const u64 fatal = mine.fatal;
    if (!P::kBlockGated && cs.inert() != 0) c = UGO_STREAM_NO_CONN;
    leader = P::leader(c, t);
    if (c != UGO_STREAM_NO_CONN) {
      P::stash(s_conn, t, c, mine);
      if (a.info[i].status != UGO_PKT_OK) {
        if (i * a.max_segments <= fatal) atomicAdd(&s_cnt[leader][3], 1u);
      } else {
        const uint32_t ns = nseg_of(a, i);
        s_ns[t] = ns;
        if (ns != 0) {
          s_code0[t] = a.seg_status[i * a.max_segments];
          s_seg0[t] = a.segs[i * a.max_segments];
        }
        uint32_t acc = 0, dup = 0, oow = 0;
        u64 hi = 0;
        for (uint32_t j = 0; j < ns; ++j) {
          const u64 idx = i * a.max_segments + j;
          if (idx > fatal) break;
          const uint32_t code = j == 0 ? s_code0[t] : a.seg_status[idx];
          if (code == kAccepted) {
            ++acc;
            const ugo_pkt_segment sg = j == 0 ? s_seg0[t] : a.segs[idx];
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
  if (t < N && c != UGO_STREAM_NO_CONN && leader == t) {
    StreamRecord& R = *cs.e.rec;
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
  for (uint32_t p = grp; p < N; p += kGroups) {
    const u64 ip = first + p;
    const uint32_t ns = s_ns[p];
    if (ns == 0) continue;
    const CopyDesc d = P::fetch(s_conn, p, mine);
    const u64 fatal = d.fatal, rp = d.rp, cap = d.cap;
    for (uint32_t j = 0; j < ns; ++j) {
      const u64 idx = ip * a.max_segments + j;
      const uint32_t code = j == 0 ? s_code0[p] : a.seg_status[idx];
      const Seg s = j == 0 ? to_seg(a, s_seg0[p]) : load_seg(a, idx);
      const bool indom = s.o >= rp && s.o - rp < cap;
      const u64 e2 = s.o + s.len, lo = s.o > rp ? s.o : rp;
      const bool ranged = s.len != 0 && !(s.o > rp + cap || s.len > rp + cap - s.o) && e2 > rp;
      const bool undo = idx > fatal && code == kAccepted;
      // only after a fatal: the contested it left behind still have their
      // contested bits, the accepted after it come out of C again
      const bool left = code == kContested;
      if (left || undo) {
        const auto e = pol.stashed_entry(s_conn, p);
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
        if (hl == 0 && code != kNone) a.seg_status[idx] = kNone;
      } else if (code == kAccepted && s.len != 0) {
        copy_segment(a, d.win, cap, ip, s, hl);
      }
    }
  }
}

// -------------------------------------------------------------------- summary
template <class P>
__global__ __launch_bounds__(256) void k_scan(typename P::Args a) {
  const uint32_t c = P::kMany ? block_conn() : 0;
  typename P::Entry e;
  if constexpr (P::kMany) {
    if (c >= a.nconn) return;
    e = a.table[c];
  } else {
    e = a;
  }
  StreamRecord& R = *e.rec;
  if (P::idle(R)) return;
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

// P::kFinishLanes lanes per connection
template <class P>
__global__ __launch_bounds__(256) void k_finish(typename P::Args a) {
  const uint32_t c = P::finish_conn(), lane = threadIdx.x % P::kFinishLanes;
  typename P::Entry e;
  if constexpr (P::kMany) {
    if (c >= a.nconn) return;
    e = a.table[c];
  } else {
    if (c != 0) return;
    e = a;
  }
  StreamRecord& R = *e.rec;
  if (P::idle(R)) return;
  for (uint32_t k = lane; k < kEndShards; k += P::kFinishLanes) R.claim_end[k] = 0;
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
  P::finished(R);
}

// ----------------------------------------------------------------------- read
template <class P>
__global__ __launch_bounds__(256) void k_read(typename P::ReadArgs a) {
  // the connection, and where n and dst come from; n_read and eof go to a.n_read[c] and a.eof[c]
  const uint32_t c = P::kMany ? block_conn() : 0;
  typename P::ReadEntry en;
  u64 n;
  uint8_t* dst;
  if constexpr (P::kMany) {
    if (c >= a.nconn) return;
    n = a.n[c];
    if (n == 0) {  // skipped: nothing of the record is read or written
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.n_read[c] = 0;
        if (a.eof) a.eof[c] = 0;
      }
      return;
    }
    en = a.table[c];
    dst = a.dst ? a.dst + a.dst_off[c] : nullptr;
  } else {  // no skip: a zero-length read still reports end of stream by the rule
    n = a.n;
    en = a;
    dst = a.dst;
  }
  StreamRecord& R = *en.rec;
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
  a.n_read[c] = m;
  if (a.eof) a.eof[c] = (m == readable && R.pub.eof != 0) ? 1 : 0;
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

// Every block of k_read<Many> ends with a device-scope fence and its
// connection's ticket (about 55 ns a block, measured: 131,072 blocks took 3.6
// to 7 ms to clear bitmaps alone), so the whole grid stays near 4,096 blocks.
uint32_t stream_set_rblocks(uint64_t max_cap, uint32_t nconn) {
  const uint64_t by_window = (max_cap + 256 * 64 - 1) / (256 * 64);  // four 16-B chunks per thread
  const uint64_t by_grid = nconn >= 4096 ? 1 : 4096 / nconn;
  const uint64_t b = by_window < by_grid ? by_window : by_grid;
  return static_cast<uint32_t>(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

hipError_t launch_stream_deliver(const StreamArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const uint32_t gblocks = static_cast<uint32_t>((a.npk + kGroupsPerBlock - 1) / kGroupsPerBlock);
  const uint32_t cblocks = static_cast<uint32_t>((a.npk + kCopyPacketsPerBlock - 1) / kCopyPacketsPerBlock);
  launch(kKStreamDeliver, k_classify<One>, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_resolve<One>, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_apply<One>, dim3(kScanBlocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_ordered<One>, dim3(1), dim3(kOrderedThreads), 0, s, a);
  launch(kKStreamDeliver, k_copy<One>, dim3(cblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_scan<One>, dim3(kScanBlocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_finish<One>, dim3(1), dim3(One::kFinishLanes), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_read(const StreamReadArgs& a, hipStream_t s) {
  const uint64_t want = a.n < a.cap ? a.n : a.cap;
  uint64_t blocks = (want + 256 * 64 - 1) / (256 * 64);  // 4 chunks per thread
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  launch(kKStreamRead, k_read<One>, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_set_deliver(const StreamSetArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const uint32_t gblocks = static_cast<uint32_t>((a.npk + kGroupsPerBlock - 1) / kGroupsPerBlock);
  const uint32_t cblocks = static_cast<uint32_t>((a.npk + kCopyPacketsPerBlock - 1) / kCopyPacketsPerBlock);
  const uint32_t fblocks = (a.nconn + 256 / Many::kFinishLanes - 1) / (256 / Many::kFinishLanes);
  launch(kKStreamDeliver, k_classify<Many>, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_resolve<Many>, dim3(gblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_apply<Many>, conn_grid(a.wblocks, a.nconn), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_ordered<Many>, conn_grid(1, a.nconn), dim3(kOrderedThreads), 0, s, a);
  launch(kKStreamDeliver, k_copy<Many>, dim3(cblocks), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_scan<Many>, conn_grid(a.wblocks, a.nconn), dim3(256), 0, s, a);
  launch(kKStreamDeliver, k_finish<Many>, dim3(fblocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_set_read(const StreamSetReadArgs& a, hipStream_t s) {
  launch(kKStreamRead, k_read<Many>, conn_grid(a.rblocks, a.nconn), dim3(256), 0, s, a);
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
