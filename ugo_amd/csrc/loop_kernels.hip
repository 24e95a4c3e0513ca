// loop_kernels.hip -- the connection loop on gfx950 (include/ugo_loop.h): the
// timers, FIN / RST and the exits of a set of connections.
//   the top of handlePacket   ugo/conn.go:388-444
//   Close, resetConn          ugo/conn.go:283-302, 500-512
//   the top of sendPacket     ugo/conn.go:521-552, 582-593, 632
//   resetTimer                ugo/conn.go:358-385
//
// receive  three launches:
//            k_loop_rx_scan   per packet: the lowest batch index of a packet
//                             of each kind (any, ending, numbered, FIN) by
//                             atomicMin on the member's four words.  A block
//                             of 1,024 packets that all name one member
//                             combines in LDS and lowers the words once; else
//                             the lanes of a wave that name one member combine,
//                             so a member costs a wave one atomic per word; a lane
//                             whose index is not below what the word already
//                             holds sends none.  The words only fall, so a
//                             stale read costs an atomic, never a result.
//            k_loop_rx_mask   per packet: conn_of of what lies at or past E, or
//                             belongs to an exited member; dropped by one
//                             atomic per block if it drops of one member only,
//                             else per wave and member
//            k_loop_rx_apply  per member: THE RULE, and the words back to idle
//          No lane waits for another lane's store: what mask and apply read of
//          scan lies behind a kernel boundary.
// close    one lane per member.
// check    one lane per member; it reads the four neighbouring records.
// append   two launches: pending members counted per block of 1,024, then
//          ranked (the blocks' counts scanned by every block, the members by a
//          block scan) and written.
// sent     two launches: per member the origin reset and the deadline terms
//          (wave and block minimum, one 64-bit atomicMin a block on a word of
//          the set), the unreported exits and the live members counted per
//          block; then ranked and written as in append.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "loop_kernels.hpp"
#include "sent_device.hpp"

namespace ugo {
namespace kern {

namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

static_assert(sizeof(LoopRecord) == 64 && sizeof(LoopCall) == 16 && sizeof(ugo_pkt_info) == 64 &&
                  sizeof(ugo_pkt_segment) == 16 && sizeof(ugo_loop_params) == 24,
              "layouts");

constexpr u64 kNever = ~0ull;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

union RecIO {
  LoopRecord s;
  u64x2 v[4];
  __device__ RecIO() {}
};

__device__ __forceinline__ LoopRecord load_rec(const LoopRecord* p) {
  RecIO io;
  const u64x2* src = reinterpret_cast<const u64x2*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) io.v[i] = src[i];
  return io.s;
}

__device__ __forceinline__ void store_rec(LoopRecord* p, const LoopRecord& s) {
  RecIO io;
  io.s = s;
  u64x2* dst = reinterpret_cast<u64x2*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[i] = io.v[i];
}

// status and flags of a decoded record: the pieces at 32 and 48
__device__ __forceinline__ void info_tail(const ugo_pkt_info* rec, uint32_t& status, uint32_t& flags) {
  const u64x2* v = reinterpret_cast<const u64x2*>(rec);
  status = static_cast<uint32_t>(v[2].y);
  flags = static_cast<uint32_t>(v[3].x >> 32) & 0xffu;
}

// 0 no, 1 ACK|FIN, 2 RST, 3 decode error
__device__ __forceinline__ uint32_t end_kind(uint32_t status, uint32_t flags) {
  if (status >= 1u && status <= 5u) return 3u;
  if (status != UGO_PKT_OK && status != UGO_PKT_CAPACITY) return 0u;
  if (flags == 0x90u) return 1u;
  if (flags == 0x08u) return 2u;
  return 0u;
}

__device__ __forceinline__ void exit_member(LoopRecord& s, uint8_t reason, bool rst, u64 now) {
  s.exited = 1;
  s.reason = reason;
  s.exit_us = now;
  if (rst) s.pending = UGO_LOOP_PENDING_RST;
}

__device__ __forceinline__ u64 sat_add(u64 a, u64 b) { return a + b < a ? kNever : a + b; }

// atomicMin unless the word is seen at or below v already
__device__ __forceinline__ void lower(uint32_t* w, uint32_t v) {
  if (*w > v) atomicMin(w, v);
}

constexpr uint32_t kScanBlock = 1024;         // packets per block of k_loop_rx_scan
constexpr uint32_t kMixed = 0xfffffffeu;      // a wave whose lanes name more than one member

// ---------------------------------------------------------------- receive
__global__ __launch_bounds__(kScanBlock) void k_loop_rx_scan(LoopReceiveArgs a) {
  __shared__ uint32_t wave_c[kScanBlock / 64];
  __shared__ uint32_t wave_min[kScanBlock / 64][4];
  const u64 i = blockIdx.x * static_cast<u64>(kScanBlock) + threadIdx.x;
  uint32_t c = kLoopIdle;
  bool ending = false, pn = false, fin = false;
  if (i < a.npk) {
    c = a.conn_of[i];
    if (c < a.t.nconn) {
      const u64x2* v = reinterpret_cast<const u64x2*>(a.info + i);
      uint32_t status, flags;
      info_tail(a.info + i, status, flags);
      ending = end_kind(status, flags) != 0;
      pn = v[0].x != 0;
      fin = (flags & 0x10u) != 0;
    } else {
      c = kLoopIdle;
    }
  }
  const uint32_t idx = static_cast<uint32_t>(i);
  const uint32_t base = idx - lane_id();
  bool todo_me = c != kLoopIdle;
  u64 todo = __ballot(todo_me);
  // A block whose packets all name one member (a ring of few connections) combines in LDS first:
  // its lowest indices go to the member's words once a block, not once a wave.
  {
    const uint32_t cf = __shfl(c, todo ? __ffsll(todo) - 1 : 0, 64);
    const bool one = todo != 0 && __ballot(todo_me && c == cf) == todo;
    const u64 me = __ballot(todo_me && ending), mp = __ballot(todo_me && pn), mf = __ballot(todo_me && fin);
    const uint32_t w = threadIdx.x >> 6;
    if (lane_id() == 0) {
      wave_c[w] = todo == 0 ? kLoopIdle : one ? cf : kMixed;
      wave_min[w][0] = todo ? base + (__ffsll(todo) - 1) : kLoopIdle;
      wave_min[w][1] = me ? base + (__ffsll(me) - 1) : kLoopIdle;
      wave_min[w][2] = mp ? base + (__ffsll(mp) - 1) : kLoopIdle;
      wave_min[w][3] = mf ? base + (__ffsll(mf) - 1) : kLoopIdle;
    }
    __syncthreads();
    uint32_t member = kLoopIdle;
    bool uniform = true;
#pragma unroll
    for (uint32_t k = 0; k < kScanBlock / 64; ++k) {
      const uint32_t x = wave_c[k];
      if (x == kLoopIdle) continue;
      if (x == kMixed || (member != kLoopIdle && x != member)) uniform = false;
      member = x;
    }
    if (uniform) {  // the same answer in every thread of the block
      if (threadIdx.x < 4 && member != kLoopIdle) {
        uint32_t m = kLoopIdle;
#pragma unroll
        for (uint32_t k = 0; k < kScanBlock / 64; ++k) m = wave_min[k][threadIdx.x] < m ? wave_min[k][threadIdx.x] : m;
        uint32_t* word = &a.t.call[member].first + threadIdx.x;  // first, end, pn, fin
        if (m != kLoopIdle) lower(word, m);
      }
      return;
    }
  }
  for (int round = 0; round < 4 && todo; ++round) {  // the members a wave's lanes share, one at a time
    const int leader = __ffsll(todo) - 1;
    const uint32_t cl = __shfl(c, leader, 64);
    const bool mine = todo_me && c == cl;
    const u64 grp = __ballot(mine);
    const u64 me = __ballot(mine && ending), mp = __ballot(mine && pn), mf = __ballot(mine && fin);
    if (static_cast<int>(lane_id()) == leader) {
      LoopCall* k = a.t.call + cl;
      lower(&k->first, idx);
      if (me) lower(&k->end, base + (__ffsll(me) - 1));
      if (mp) lower(&k->pn, base + (__ffsll(mp) - 1));
      if (mf) lower(&k->fin, base + (__ffsll(mf) - 1));
    }
    if (mine) todo_me = false;
    todo &= ~grp;
  }
  if (todo_me) {  // what is left is taken to be distinct
    LoopCall* k = a.t.call + c;
    lower(&k->first, idx);
    if (ending) lower(&k->end, idx);
    if (pn) lower(&k->pn, idx);
    if (fin) lower(&k->fin, idx);
  }
}

__global__ __launch_bounds__(kScanBlock) void k_loop_rx_mask(LoopReceiveArgs a) {
  __shared__ uint32_t wave_c[kScanBlock / 64];
  __shared__ uint32_t wave_n[kScanBlock / 64];
  const u64 i = blockIdx.x * static_cast<u64>(kScanBlock) + threadIdx.x;
  uint32_t c = kLoopIdle;
  bool drop = false;
  if (i < a.npk) {
    c = a.conn_of[i];
    if (c < a.t.nconn) {
      drop = a.t.recs[c].exited != 0 || static_cast<uint32_t>(i) >= a.t.call[c].end;
      if (drop) a.conn_of[i] = UGO_STREAM_NO_CONN;
    }
  }
  u64 todo = __ballot(drop);
  {  // a block that drops packets of one member only counts them in LDS and adds once
    const uint32_t cf = __shfl(c, todo ? __ffsll(todo) - 1 : 0, 64);
    const bool one = todo != 0 && __ballot(drop && c == cf) == todo;
    const uint32_t w = threadIdx.x >> 6;
    if (lane_id() == 0) {
      wave_c[w] = todo == 0 ? kLoopIdle : one ? cf : kMixed;
      wave_n[w] = static_cast<uint32_t>(__popcll(todo));
    }
    __syncthreads();
    uint32_t member = kLoopIdle, n = 0;
    bool uniform = true;
#pragma unroll
    for (uint32_t k = 0; k < kScanBlock / 64; ++k) {
      const uint32_t x = wave_c[k];
      if (x == kLoopIdle) continue;
      if (x == kMixed || (member != kLoopIdle && x != member)) uniform = false;
      member = x;
      n += wave_n[k];
    }
    if (uniform) {
      if (threadIdx.x == 0 && member != kLoopIdle)
        atomicAdd(reinterpret_cast<u64*>(&a.t.recs[member].dropped), static_cast<u64>(n));
      return;
    }
  }
  for (int round = 0; round < 4 && todo; ++round) {
    const int leader = __ffsll(todo) - 1;
    const uint32_t cl = __shfl(c, leader, 64);
    const bool mine = drop && c == cl;
    const u64 grp = __ballot(mine);
    if (static_cast<int>(lane_id()) == leader)
      atomicAdd(reinterpret_cast<u64*>(&a.t.recs[cl].dropped), static_cast<u64>(__popcll(grp)));
    if (mine) drop = false;
    todo &= ~grp;
  }
  if (drop) atomicAdd(reinterpret_cast<u64*>(&a.t.recs[c].dropped), 1ull);
}

__global__ __launch_bounds__(256) void k_loop_rx_apply(LoopReceiveArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.t.nconn) return;
  const LoopCall k = a.t.call[c];
  if (k.first == kLoopIdle) return;  // no packet names the member: the other words are idle too
  a.t.call[c] = LoopCall{kLoopIdle, kLoopIdle, kLoopIdle, kLoopIdle};
  LoopRecord s = load_rec(a.t.recs + c);
  if (s.exited) return;
  s.last_activity_us = a.now_us;
  if (s.origin_ack_us == 0 && k.pn < k.end) s.origin_ack_us = a.now_us;
  uint32_t kind = 0;
  if (k.end != kLoopIdle && k.end < a.npk) {
    uint32_t status, flags;
    info_tail(a.info + k.end, status, flags);
    kind = end_kind(status, flags);
  }
  if (k.fin < k.end || kind == 1u) s.fin_rcvd = 1;
  if (kind == 1u) exit_member(s, UGO_LOOP_PEER_ACK_FIN, false, a.now_us);
  if (kind == 2u) exit_member(s, UGO_LOOP_PEER_RST, false, a.now_us);
  if (kind == 3u) exit_member(s, UGO_LOOP_BAD_PACKET, true, a.now_us);
  store_rec(a.t.recs + c, s);
}

// ---------------------------------------------------------------- close
__global__ __launch_bounds__(256) void k_loop_close(LoopCloseArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.t.nconn) return;
  const uint32_t how = a.how[c];
  if ((how & 15u) == 0) return;
  LoopRecord s = load_rec(a.t.recs + c);
  if (s.exited) return;
  if (how & UGO_LOOP_HOW_NODELAY_ON) s.ack_no_delay = 1;
  if (how & UGO_LOOP_HOW_NODELAY_OFF) s.ack_no_delay = 0;
  if (s.closed) {
    // Close on a closed connection returns before it looks at linger (conn.go:284-286)
  } else if (how & UGO_LOOP_HOW_ABORT) {
    exit_member(s, UGO_LOOP_ABORT, true, a.now_us);
  } else if (how & UGO_LOOP_HOW_CLOSE) {
    s.closed = 1;
    const u64 linger = a.linger_us ? a.linger_us[c] : 0;
    if (linger > 0) s.linger_deadline_us = sat_add(a.now_us, linger);
  }
  store_rec(a.t.recs + c, s);
}

// ---------------------------------------------------------------- check
__global__ __launch_bounds__(256) void k_loop_check(LoopCheckArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.t.nconn) return;
  LoopRecord s = load_rec(a.t.recs + c);
  if (!s.exited) {
    const SentRecord* sr = a.t.sent_tx[c].rec;
    const uint32_t before = (static_cast<uint32_t>(s.pending) << 8) | s.exited;
    uint8_t reason = 0;
    if (a.t.stream_rx[c].rec->pub.err)
      reason = UGO_LOOP_STREAM_ERR;
    else if (a.t.ack_rx[c].rec->err)
      reason = UGO_LOOP_ACK_ERR;
    else if (sr->err)
      reason = UGO_LOOP_SENT_ERR;
    else if (sr->rto_count > a.t.p.max_retries)
      reason = UGO_LOOP_FAILURES;
    else if (s.closed && s.linger_deadline_us != 0 && a.now_us >= s.linger_deadline_us)
      reason = UGO_LOOP_LINGER;
    else if (a.now_us >= s.last_activity_us && a.now_us - s.last_activity_us >= a.t.p.idle_us)
      reason = UGO_LOOP_IDLE;
    if (reason) {
      exit_member(s, reason, true, a.now_us);
    } else if (s.closed) {
      if (!s.fin_sent && s.pending == 0) {
        const StreamTxRecord* tr = a.t.stream_tx[c].rec;
        if (tr->tail == tr->write_pos && tr->rq_len == 0 && sr->tracked == 0) s.pending = UGO_LOOP_PENDING_FIN;
      }
      if (s.fin_rcvd && (s.fin_sent || s.pending == UGO_LOOP_PENDING_FIN))
        exit_member(s, UGO_LOOP_CLOSED, false, a.now_us);
    }
    if (before != ((static_cast<uint32_t>(s.pending) << 8) | s.exited)) store_rec(a.t.recs + c, s);
  }
  if (s.exited || s.fin_sent || s.pending != 0) a.budget[c] = 0;
  uint8_t may = 0;
  if (!s.exited)
    may = s.ack_no_delay || s.origin_ack_us == 0 ||
          (a.now_us > s.origin_ack_us && a.now_us - s.origin_ack_us > a.t.p.ack_delay_us);
  a.may_ack_only[c] = may;
}

// ---------------------------------------------------------------- ranks over the members
// Exclusive scan of v over a block of kLoopScanBlock; tot = the block's sum.
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* lds, uint32_t& tot) {
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane_id() >= static_cast<uint32_t>(d)) incl += o;
  }
  const uint32_t w = threadIdx.x >> 6;
  if (lane_id() == 63) lds[w] = incl;
  __syncthreads();
  uint32_t pre = 0;
  tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < kLoopScanBlock / 64; ++k) {
    const uint32_t x = lds[k];
    if (k < w) pre += x;
    tot += x;
  }
  __syncthreads();
  return pre + incl - v;
}

// The sum of counts[0 .. nblocks) and of those before block b, by one block.
__device__ __forceinline__ u64 blocks_before(const uint32_t* counts, uint32_t nblocks, uint32_t b, uint32_t* lds,
                                             u64& all) {
  const uint32_t v = threadIdx.x < nblocks ? counts[threadIdx.x] : 0u;
  // a block's count is at most 1,024 and there are at most 1,024 blocks: 32 bits hold the sums
  uint32_t tot;
  const uint32_t excl = block_excl(v, lds, tot);
  __shared__ uint32_t mine;
  if (threadIdx.x == b) mine = excl;
  __syncthreads();
  all = tot;
  const u64 r = mine;
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------- append
__global__ __launch_bounds__(kLoopScanBlock) void k_loop_append_count(LoopAppendArgs a) {
  __shared__ uint32_t lds[kLoopScanBlock / 64];
  const uint32_t c = blockIdx.x * kLoopScanBlock + threadIdx.x;
  const uint32_t v = c < a.t.nconn && a.t.recs[c].pending != 0 ? 1u : 0u;
  uint32_t tot;
  (void)block_excl(v, lds, tot);
  if (threadIdx.x == 0) {
    a.t.block_a[blockIdx.x] = tot;
    if (blockIdx.x == 0) a.t.words[0] = *a.total;  // total_out may be total
  }
}

__global__ __launch_bounds__(kLoopScanBlock) void k_loop_append_write(LoopAppendArgs a) {
  __shared__ uint32_t lds[kLoopScanBlock / 64];
  const uint32_t c = blockIdx.x * kLoopScanBlock + threadIdx.x;
  u64 all;
  const u64 before = blocks_before(a.t.block_a, gridDim.x, blockIdx.x, lds, all);
  const u64 total = a.t.words[0];
  const uint32_t pending = c < a.t.nconn ? a.t.recs[c].pending : 0u;
  uint32_t tot;
  const uint32_t rank = block_excl(pending != 0 ? 1u : 0u, lds, tot);
  const u64 room = total < a.max_packets ? a.max_packets - total : 0;
  if (c == 0) *a.total_out = total + (all < room ? all : room);
  if (c >= a.t.nconn) return;
  uint8_t done = 0;
  if (pending != 0 && before + rank < room) {
    const u64 t = total + before + rank;
    const bool fin = pending == UGO_LOOP_PENDING_FIN;
    u64x2* rec = reinterpret_cast<u64x2*>(a.info + t);
    const u64x2 zero = {0, 0};
    rec[0] = zero;
    rec[1] = zero;
    rec[2] = zero;
    // n_ranges | n_segments << 16 | flags << 32
    rec[3] = u64x2{fin ? (1ull << 16) | (0x10ull << 32) : (0x08ull << 32), 0};
    a.conn_of[t] = c;
    LoopRecord s = load_rec(a.t.recs + c);
    if (fin) {
      const StreamTxEntry e = a.t.stream_tx[c];
      const u64 off = e.rec->write_pos;
      a.segs[t * a.max_segments] = ugo_pkt_segment{off, static_cast<uint32_t>(off & (e.cap - 1)), 0, 0};
      s.fin_sent = 1;
      s.linger_deadline_us = 0;
    }
    s.pending = 0;
    store_rec(a.t.recs + c, s);
    done = fin ? 1 : 2;
  }
  a.appended[c] = done;
}

// ---------------------------------------------------------------- sent
__global__ __launch_bounds__(kLoopScanBlock) void k_loop_sent_count(LoopSentArgs a) {
  __shared__ uint32_t lds[kLoopScanBlock / 64];
  __shared__ u64 lds_min[kLoopScanBlock / 64];
  const uint32_t c = blockIdx.x * kLoopScanBlock + threadIdx.x;
  u64 dl = kNever;
  uint32_t unreported = 0, live = 0;
  if (c < a.t.nconn) {
    LoopRecord* rec = a.t.recs + c;
    LoopRecord s = load_rec(rec);
    if (s.exited) {
      unreported = s.reported ? 0u : 1u;
    } else {
      live = 1;
      if (s.origin_ack_us != 0 && (a.n_packets[c] > 0 || a.attached[c] != 0)) {
        s.origin_ack_us = 0;
        rec->origin_ack_us = 0;
      }
      dl = sat_add(s.last_activity_us, a.t.p.idle_us);
      if (s.origin_ack_us != 0) {
        const u64 t = sat_add(s.origin_ack_us, a.t.p.ack_delay_us);
        dl = t < dl ? t : dl;
      }
      if (s.linger_deadline_us != 0 && s.linger_deadline_us < dl) dl = s.linger_deadline_us;
      const SentRecord* sr = a.t.sent_tx[c].rec;
      if (sr->last_sent_us != 0) {
        const u64 t = sat_add(sr->last_sent_us, sent_rto_us(a.delay_us ? a.delay_us[c] : 0ull, sr->rto_count));
        if (t > a.now_us && t < dl) dl = t;
      }
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_xor(dl, d, 64);
    dl = o < dl ? o : dl;
  }
  if (lane_id() == 0) lds_min[threadIdx.x >> 6] = dl;
  uint32_t tot_u, tot_l;
  (void)block_excl(unreported, lds, tot_u);  // its barriers also order lds_min
  (void)block_excl(live, lds, tot_l);
  if (threadIdx.x == 0) {
    a.t.block_a[blockIdx.x] = tot_u;
    a.t.block_b[blockIdx.x] = tot_l;
    u64 m = kNever;
    for (uint32_t k = 0; k < kLoopScanBlock / 64; ++k) m = lds_min[k] < m ? lds_min[k] : m;
    if (m != kNever) atomicMin(a.t.words + 1, m);
  }
}

__global__ __launch_bounds__(kLoopScanBlock) void k_loop_sent_write(LoopSentArgs a) {
  __shared__ uint32_t lds[kLoopScanBlock / 64];
  const uint32_t c = blockIdx.x * kLoopScanBlock + threadIdx.x;
  u64 all_u, all_l;
  const u64 before_u = blocks_before(a.t.block_a, gridDim.x, blockIdx.x, lds, all_u);
  const u64 before_l = blocks_before(a.t.block_b, gridDim.x, blockIdx.x, lds, all_l);
  uint32_t unreported = 0, live = 0;
  uint8_t reason = 0;
  if (c < a.t.nconn) {
    const LoopRecord* rec = a.t.recs + c;
    live = rec->exited ? 0u : 1u;
    unreported = rec->exited && !rec->reported ? 1u : 0u;
    reason = rec->reason;
  }
  uint32_t tot;
  const uint32_t rank_u = block_excl(unreported, lds, tot);
  const uint32_t rank_l = block_excl(live, lds, tot);
  if (c == 0) {
    *a.n_exits = all_u;
    if (a.nconn_new) *a.nconn_new = all_l;
    *a.deadline_us = a.t.words[1];
    a.t.words[1] = kNever;  // idle again: the atomics on it lie behind a kernel boundary
  }
  if (c >= a.t.nconn) return;
  if (unreported && before_u + rank_u < a.max_exits) {
    const u64 k = before_u + rank_u;
    a.exits[k] = c;
    a.reasons[k] = reason;
    a.t.recs[c].reported = 1;
  }
  if (a.new_index) a.new_index[c] = live ? static_cast<uint32_t>(before_l + rank_l) : UGO_STREAM_NO_CONN;
}

inline dim3 per_member(uint32_t nconn) { return dim3((nconn + 255u) / 256u); }
inline dim3 per_scan_block(uint32_t nconn) { return dim3((nconn + kLoopScanBlock - 1u) / kLoopScanBlock); }

}  // namespace

hipError_t launch_loop_receive(const LoopReceiveArgs& a, hipStream_t s) {
  const dim3 per_scan(static_cast<uint32_t>((a.npk + kScanBlock - 1u) / kScanBlock));
  launch(kKLoop, k_loop_rx_scan, per_scan, dim3(kScanBlock), 0, s, a);
  launch(kKLoop, k_loop_rx_mask, per_scan, dim3(kScanBlock), 0, s, a);
  launch(kKLoop, k_loop_rx_apply, per_member(a.t.nconn), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_loop_close(const LoopCloseArgs& a, hipStream_t s) {
  launch(kKLoop, k_loop_close, per_member(a.t.nconn), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_loop_check(const LoopCheckArgs& a, hipStream_t s) {
  launch(kKLoop, k_loop_check, per_member(a.t.nconn), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_loop_append(const LoopAppendArgs& a, hipStream_t s) {
  launch(kKLoop, k_loop_append_count, per_scan_block(a.t.nconn), dim3(kLoopScanBlock), 0, s, a);
  launch(kKLoop, k_loop_append_write, per_scan_block(a.t.nconn), dim3(kLoopScanBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_loop_sent(const LoopSentArgs& a, hipStream_t s) {
  launch(kKLoop, k_loop_sent_count, per_scan_block(a.t.nconn), dim3(kLoopScanBlock), 0, s, a);
  launch(kKLoop, k_loop_sent_write, per_scan_block(a.t.nconn), dim3(kLoopScanBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
