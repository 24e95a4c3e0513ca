// stream_tx_kernels.hip -- send windows on gfx950 (include/ugo_stream.h, "send
// windows"): batch Conn.Write, segmentSender.PopSegments and the
// lastPacketNumber++ loop of Conn.sendPacket for a set of connections.
//   Conn.Write              ugo/conn.go:247-275
//   getDataForWriting       ugo/conn.go:753-779
//   PopSegments and below   ugo/segment_sender.go:18-99
//   the sendPacket loop     ugo/conn.go:521-640
// The encoder that reads the windows is k_packet_encode's window form
// (pkt_kernels.hip).
//
// write    two launches: the copy (blocks per connection, 16-B chunks aligned
//          on the window, unaligned loads from src, byte stores for the up to
//          15 bytes at either end, so nothing outside [tail, tail+m) is
//          touched), then one thread per connection moves tail.  The copy
//          only reads the record, so no block can see a moved tail.
// plan     the retransmission queue makes a connection's first packets
//          serial, everything after the queue runs empty is arithmetic in
//          write_pos, pending, M and the packet's index.  Six launches:
//          budgets scanned (two levels of 1024), one thread per connection
//          walks its queue without changing anything and counts its packets,
//          the counts are scanned, one thread per connection walks again,
//          writes the packets that drew from the queue and commits the
//          record, and one thread per packet fills the arithmetic ones.
// release, retransmit, gather: one thread per connection (or per list group).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "stream_tx_kernels.hpp"

namespace ugo {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

constexpr uint32_t kKStreamTx = 11;  // UGO_FEC_KERNEL_STREAM_TX

__device__ __forceinline__ uint64_t write_len(const StreamTxRecord& r, uint64_t cap, uint64_t n) {
  const uint64_t room = cap - (r.tail - r.base);
  return n < room ? n : room;
}

// ---------------------------------------------------------------- write
__global__ __launch_bounds__(256) void k_tx_write_copy(StreamTxWriteArgs a) {
  const uint32_t c = blockIdx.x / a.wblocks, part = blockIdx.x % a.wblocks;
  const uint64_t n = a.n[c];
  if (n == 0) return;
  const StreamTxEntry e = a.table[c];
  const uint64_t tail = e.rec->tail;
  const uint64_t m = write_len(*e.rec, e.cap, n);
  if (m == 0) return;
  const uint64_t mask = e.cap - 1;
  const uint8_t* src = a.src + a.src_off[c];
  uint64_t head = (16u - (tail & 15u)) & 15u;  // up to the window's next 16-B boundary
  if (head > m) head = m;
  const uint64_t nch = (m - head) >> 4;
  const uint64_t rest = m - head - (nch << 4);
  if (part == 0) {
    if (threadIdx.x < head) e.win[(tail + threadIdx.x) & mask] = src[threadIdx.x];
    if (threadIdx.x >= 32u && threadIdx.x - 32u < rest) {
      const uint64_t k = head + (nch << 4) + (threadIdx.x - 32u);
      e.win[(tail + k) & mask] = src[k];
    }
  }
  // a chunk is 16-B aligned on the window and cap % 16 == 0: it never crosses the wrap
  for (uint64_t ch = part * 256ull + threadIdx.x; ch < nch; ch += a.wblocks * 256ull) {
    const uint64_t k = head + (ch << 4);
    const u32x4 v = *reinterpret_cast<const u32x4u*>(src + k);
    *reinterpret_cast<u32x4*>(e.win + ((tail + k) & mask)) = v;
  }
}

__global__ __launch_bounds__(256) void k_tx_write_commit(StreamTxWriteArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  const uint64_t n = a.n[c];
  uint64_t m = 0;
  if (n != 0) {
    const StreamTxEntry e = a.table[c];
    m = write_len(*e.rec, e.cap, n);
    if (m != 0) e.rec->tail += m;
  }
  a.n_written[c] = m;
}

// ---------------------------------------------------------------- release
__global__ __launch_bounds__(256) void k_tx_release(const StreamTxEntry* table, uint32_t nconn, const uint64_t* upto) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= nconn) return;
  const StreamTxEntry e = table[c];
  const StreamTxRecord r = *e.rec;
  uint64_t lo = upto[c] < r.write_pos ? upto[c] : r.write_pos;
  uint32_t h = r.rq_head;
  for (uint32_t k = 0; k < r.rq_len; ++k) {
    const uint64_t o = e.rq[h].offset;
    if (o < lo) lo = o;
    h = h + 1u == e.rq_cap ? 0u : h + 1u;
  }
  if (lo > r.base) e.rec->base = lo;
}

// ---------------------------------------------------------------- retransmit
__global__ __launch_bounds__(1024) void k_tx_rq_check(StreamTxRetransmitArgs a) {
  int bad = 0;
  for (uint64_t j = threadIdx.x + 1ull; j < a.m; j += 1024u)
    if (a.conn_of[j] < a.conn_of[j - 1]) bad = 1;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) *a.unsorted = bad ? 1u : 0u;
}

// The first entry of each connection's group appends the whole group, in list order.
__global__ __launch_bounds__(256) void k_tx_rq_apply(StreamTxRetransmitArgs a) {
  const uint64_t j0 = blockIdx.x * 256ull + threadIdx.x;
  if (j0 >= a.m) return;
  if (*a.unsorted) {
    a.status[j0] = UGO_STREAM_TX_RQ_UNSORTED;
    return;
  }
  const uint32_t c = a.conn_of[j0];
  if (j0 != 0 && a.conn_of[j0 - 1] == c) return;
  if (c >= a.nconn) {
    for (uint64_t j = j0; j < a.m && a.conn_of[j] == c; ++j) a.status[j] = UGO_STREAM_TX_RQ_REJECTED;
    return;
  }
  const StreamTxEntry e = a.table[c];
  const StreamTxRecord r = *e.rec;
  uint32_t qlen = r.rq_len;
  uint64_t refused = 0;
  bool full = false;
  for (uint64_t j = j0; j < a.m && a.conn_of[j] == c; ++j) {
    const uint64_t o = a.offset[j];
    const uint64_t l = a.len[j];
    uint8_t st;
    if (full) {
      st = UGO_STREAM_TX_RQ_FULL;
    } else if (l == 0 || l > 0xffffu || o < r.base || o > r.write_pos || l > r.write_pos - o) {
      st = UGO_STREAM_TX_RQ_REJECTED;
    } else if (qlen == e.rq_cap) {
      st = UGO_STREAM_TX_RQ_FULL;
      full = true;
    } else {
      const uint32_t at = static_cast<uint32_t>((static_cast<uint64_t>(r.rq_head) + qlen) % e.rq_cap);
      e.rq[at].offset = o;
      e.rq[at].len = static_cast<uint32_t>(l);
      e.rq[at].reserved = 0;
      ++qlen;
      st = UGO_STREAM_TX_RQ_QUEUED;
    }
    if (st != UGO_STREAM_TX_RQ_QUEUED) ++refused;
    a.status[j] = st;
  }
  if (qlen != r.rq_len) e.rec->rq_len = qlen;
  if (refused) e.rec->rq_rejected = r.rq_rejected + refused;
}

// ---------------------------------------------------------------- plan
// Exclusive scan of one value per thread over a block of kTxScanBlock threads.
__device__ uint64_t block_excl_scan(uint64_t v, uint64_t& total) {
  __shared__ uint64_t s[kTxScanBlock];
  const uint32_t t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kTxScanBlock; d <<= 1) {
    const uint64_t add = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  total = s[kTxScanBlock - 1];
  const uint64_t incl = s[t];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(kTxScanBlock) void k_tx_scan_budget(StreamTxPlanArgs a) {
  const uint32_t c = blockIdx.x * kTxScanBlock + threadIdx.x;
  uint64_t total;
  const uint64_t ex = block_excl_scan(c < a.nconn ? a.budget[c] : 0u, total);
  if (c < a.nconn) a.scratch[c].budget_start = ex;
  if (threadIdx.x == 0) a.block_budget[blockIdx.x] = total;
}

// sums[0 .. n) (n <= kTxScanBlock) to their exclusive scan, the grand total to *total
__global__ __launch_bounds__(kTxScanBlock) void k_tx_scan_blocks(uint64_t* sums, uint32_t n,
                                                                 unsigned long long* total_out) {
  uint64_t total;
  const uint64_t ex = block_excl_scan(threadIdx.x < n ? sums[threadIdx.x] : 0u, total);
  if (threadIdx.x < n) sums[threadIdx.x] = ex;
  if (threadIdx.x == 0 && total_out) *total_out = total;
}

__device__ __forceinline__ void put_segment(ugo_pkt_segment* sg, uint64_t offset, uint32_t len, uint64_t mask) {
  ugo_pkt_segment s;
  s.offset = offset;
  s.data_off = static_cast<uint32_t>(offset & mask);
  s.len = static_cast<uint16_t>(len);
  s.avail = static_cast<uint16_t>(len);
  *sg = s;
}

__device__ __forceinline__ void put_info(ugo_pkt_info* out, uint64_t packet_number, uint32_t n_segments) {
  ugo_pkt_info o{};
  o.packet_number = packet_number;
  o.n_segments = static_cast<uint16_t>(n_segments);
  *out = o;
}

// THE RULE for connection c with budget_eff packets, its packets starting at
// batch index `first`.  kEmit false: nothing is changed, only sc is filled
// (n_packets, n_queue and where the arithmetic packets start).  kEmit true:
// the packets that drew from the queue are written and the record committed.
template <bool kEmit>
__device__ void tx_walk(const StreamTxPlanArgs& a, const StreamTxEntry& e, uint32_t c, uint32_t budget_eff,
                        uint64_t first, StreamTxPlanScratch& sc) {
  const StreamTxRecord r = *e.rec;
  const uint32_t M = a.max_payload, H = kTxHeader;
  const uint64_t mask = e.cap - 1;
  uint32_t head = r.rq_head, qlen = r.rq_len;
  uint64_t wp = r.write_pos, pn = r.last_packet_number;
  uint64_t fo = 0;  // the queue's front entry, once loaded (a split shortens it)
  uint32_t fl = 0;
  bool have_front = false, front_dirty = false;
  uint32_t k = 0;
  uint64_t nseg = 0, bytes_new = 0, bytes_rtx = 0;
  while (k < budget_eff && qlen > 0) {
    uint32_t cur = 0, ns = 0;
    ugo_pkt_segment* sg = a.segs + (first + k) * a.max_segments;
    while (qlen > 0 && ns < a.max_segments) {
      if (cur + H >= M) break;  // deviation (a)
      cur += H;
      if (!have_front) {
        fo = e.rq[head].offset;
        fl = e.rq[head].len;
        have_front = true;
      }
      const uint32_t room = M - cur;
      if (fl > room) {  // maybeSplitOffFrame
        if (kEmit) put_segment(sg + ns, fo, room, mask);
        fo += room;
        fl -= room;
        front_dirty = true;
        cur += room;
        bytes_rtx += room;
        ++ns;
        break;
      }
      if (kEmit) put_segment(sg + ns, fo, fl, mask);
      cur += fl;
      bytes_rtx += fl;
      ++ns;
      head = head + 1u == e.rq_cap ? 0u : head + 1u;
      --qlen;
      have_front = front_dirty = false;
    }
    const uint32_t rem = M - cur;
    const uint64_t pending = r.tail - wp;
    if (rem > H && pending > 0 && ns < a.max_segments) {  // deviation (a)
      const uint32_t n = pending < rem - H ? static_cast<uint32_t>(pending) : rem - H;
      if (kEmit) put_segment(sg + ns, wp, n, mask);
      wp += n;
      bytes_new += n;
      ++ns;
    }
    // ns > 0: the queue was not empty and M >= 16 leaves room for a byte of its front
    ++pn;
    if (kEmit) {
      put_info(a.info + first + k, pn, ns);
      a.conn_of[first + k] = c;
    }
    nseg += ns;
    ++k;
  }
  const uint64_t pending = r.tail - wp, step = M - H;
  uint64_t nf = (pending + step - 1) / step;
  if (nf > budget_eff - k) nf = budget_eff - k;
  sc.n_packets = k + static_cast<uint32_t>(nf);
  sc.n_queue = k;
  sc.fresh_pos = wp;
  sc.fresh_pending = pending;
  sc.fresh_pn = pn;
  if (kEmit && sc.n_packets != 0) {
    if (front_dirty) {
      e.rq[head].offset = fo;
      e.rq[head].len = fl;
    }
    const uint64_t fresh = pending < nf * step ? pending : nf * step;
    StreamTxRecord w = r;
    w.write_pos = wp + fresh;
    w.last_packet_number = pn + nf;
    w.rq_head = head;
    w.rq_len = qlen;
    w.packets += sc.n_packets;
    w.segments += nseg + nf;
    w.bytes_new += bytes_new + fresh;
    w.bytes_retransmitted += bytes_rtx;
    *e.rec = w;
  }
}

__global__ __launch_bounds__(kTxScanBlock) void k_tx_plan_count(StreamTxPlanArgs a) {
  const uint32_t c = blockIdx.x * kTxScanBlock + threadIdx.x;
  uint32_t np = 0;
  if (c < a.nconn) {
    StreamTxPlanScratch sc = a.scratch[c];
    const uint64_t start = sc.budget_start + a.block_budget[blockIdx.x];
    const uint64_t b = a.budget[c];
    sc.budget_eff = start >= a.max_packets ? 0u
                                           : static_cast<uint32_t>(b < a.max_packets - start ? b : a.max_packets - start);
    tx_walk<false>(a, a.table[c], c, sc.budget_eff, 0, sc);
    a.scratch[c] = sc;
    np = sc.n_packets;
  }
  uint64_t total;
  const uint64_t ex = block_excl_scan(np, total);
  if (c < a.nconn) a.scratch[c].first = ex;
  if (threadIdx.x == 0) a.block_first[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_tx_plan_conn(StreamTxPlanArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  StreamTxPlanScratch sc = a.scratch[c];
  const uint64_t first = sc.first + a.block_first[c / kTxScanBlock];
  a.first_dense[c] = first;
  a.first_packet[c] = first;
  a.n_packets[c] = sc.n_packets;
  if (sc.n_packets == 0) return;  // idle: the record stays bit for bit
  tx_walk<true>(a, a.table[c], c, sc.budget_eff, first, sc);
}

// One thread per packet slot of the caller's arrays: the packets after a
// connection's queue ran empty carry M - H new bytes each (the last one what
// is left), at write_pos + f * (M - H).
__global__ __launch_bounds__(256) void k_tx_plan_fill(StreamTxPlanArgs a) {
  const uint64_t* first_dense = a.first_dense;
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= a.max_packets) return;
  if (i >= *a.total) {
    a.conn_of[i] = UGO_STREAM_NO_CONN;
    return;
  }
  // the last connection whose packets start at or before i: idle ones share
  // their start with the busy one after them
  uint32_t lo = 0, hi = a.nconn;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (first_dense[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t c = lo;
  const StreamTxPlanScratch& sc = a.scratch[c];
  const uint64_t k = i - first_dense[c];
  if (k < sc.n_queue) return;  // written by the connection's own pass
  const uint64_t f = k - sc.n_queue, step = a.max_payload - kTxHeader;
  const uint64_t left = sc.fresh_pending - f * step;
  put_segment(a.segs + i * a.max_segments, sc.fresh_pos + f * step, static_cast<uint32_t>(left < step ? left : step),
              a.table[c].cap - 1);
  put_info(a.info + i, sc.fresh_pn + f + 1, 1);
  a.conn_of[i] = c;
}

__global__ __launch_bounds__(256) void k_tx_gather(const StreamTxEntry* table, uint32_t nconn,
                                                   ugo_stream_tx_state* out) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c < nconn) out[c] = *table[c].rec;
}

}  // namespace

uint32_t stream_tx_wblocks(uint64_t max_cap, uint32_t nconn) {
  // 16 KiB per block and pass, and about 64k blocks at the most
  uint64_t by_cap = max_cap / 16384u, by_grid = 65536u / nconn;
  if (by_cap < 1) by_cap = 1;
  if (by_grid < 1) by_grid = 1;
  return static_cast<uint32_t>(by_cap < by_grid ? by_cap : by_grid);
}

hipError_t launch_stream_tx_write(const StreamTxWriteArgs& a, hipStream_t s) {
  launch(kKStreamTx, k_tx_write_copy, dim3(a.nconn * a.wblocks), dim3(256), 0, s, a);
  launch(kKStreamTx, k_tx_write_commit, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_tx_release(const StreamTxEntry* table, uint32_t nconn, const uint64_t* upto, hipStream_t s) {
  launch(kKStreamTx, k_tx_release, dim3((nconn + 255u) / 256u), dim3(256), 0, s, table, nconn, upto);
  return hipGetLastError();
}

hipError_t launch_stream_tx_retransmit(const StreamTxRetransmitArgs& a, hipStream_t s) {
  if (a.m == 0) return hipSuccess;
  launch(kKStreamTx, k_tx_rq_check, dim3(1), dim3(1024), 0, s, a);
  launch(kKStreamTx, k_tx_rq_apply, dim3(static_cast<uint32_t>((a.m + 255u) / 256u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_tx_plan(const StreamTxPlanArgs& a, hipStream_t s) {
  const uint32_t sblocks = (a.nconn + kTxScanBlock - 1) / kTxScanBlock;  // <= kTxScanBlock
  launch(kKStreamTx, k_tx_scan_budget, dim3(sblocks), dim3(kTxScanBlock), 0, s, a);
  launch(kKStreamTx, k_tx_scan_blocks, dim3(1), dim3(kTxScanBlock), 0, s, a.block_budget, sblocks,
         static_cast<unsigned long long*>(nullptr));
  launch(kKStreamTx, k_tx_plan_count, dim3(sblocks), dim3(kTxScanBlock), 0, s, a);
  launch(kKStreamTx, k_tx_scan_blocks, dim3(1), dim3(kTxScanBlock), 0, s, a.block_first, sblocks, a.total);
  launch(kKStreamTx, k_tx_plan_conn, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s, a);
  if (a.max_packets != 0)
    launch(kKStreamTx, k_tx_plan_fill, dim3(static_cast<uint32_t>((a.max_packets + 255u) / 256u)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stream_tx_gather(const StreamTxEntry* table, uint32_t nconn, ugo_stream_tx_state* out,
                                   hipStream_t s) {
  launch(kKStreamTx, k_tx_gather, dim3((nconn + 255u) / 256u), dim3(256), 0, s, table, nconn, out);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
