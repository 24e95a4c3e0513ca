// ugo_stream_tx.cpp -- C ABI of the send windows (include/ugo_stream.h): one
// window, and sets of them with write, release, retransmit, plan and encode.
// Host-side control plane only; the kernels are in stream_tx_kernels.hip and
// pkt_kernels.hip.
#include "host/set_call.hpp"
#include "pkt_kernels.hpp"

using namespace ugo::host;

extern "C" {

int ugo_fec_stream_tx_create(ugo_fec* c, size_t window_bytes, size_t rq_cap, uint64_t start_offset,
                             uint64_t start_packet_number, ugo_stream_tx** out) {
  static_assert(sizeof(ugo_stream_tx_state) == 80, "ugo_stream_tx_state is 80 bytes");
  static_assert(sizeof(ugo_stream_tx_rq_entry) == 16, "a queue entry is 16 bytes");
  static_assert(UGO_FEC_KERNEL_STREAM_TX == 11, "kernel class matches stream_tx_kernels.hip");
  if (out) *out = nullptr;
  if (!c || !out || window_bytes < UGO_STREAM_MIN_WINDOW || window_bytes > UGO_STREAM_TX_MAX_WINDOW ||
      (window_bytes & (window_bytes - 1)) != 0 || rq_cap == 0 || rq_cap > (size_t(1) << 24))
    return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  ugo_stream_tx* tx = new (std::nothrow) ugo_stream_tx();
  if (!tx) return UGO_FEC_ERR_HIP;
  tx->ctx = c;
  tx->cap = window_bytes;
  tx->rq_cap = rq_cap;
  ugo::kern::StreamTxRecord init{};
  init.base = init.write_pos = init.tail = start_offset;
  init.last_packet_number = start_packet_number;
  const size_t rq_bytes = rq_cap * sizeof(ugo_stream_tx_rq_entry);
  if (hipMalloc(&tx->win, window_bytes) != hipSuccess || hipMalloc(&tx->rq, rq_bytes) != hipSuccess ||
      hipMalloc(&tx->rec, sizeof(init)) != hipSuccess || hipMemset(tx->win, 0, window_bytes) != hipSuccess ||
      hipMemset(tx->rq, 0, rq_bytes) != hipSuccess ||
      hipMemcpy(tx->rec, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {  // the fills ran on the null stream
    (void)hipGetLastError();
    ugo_fec_stream_tx_destroy(tx);
    return UGO_FEC_ERR_HIP;
  }
  *out = tx;
  return UGO_FEC_OK;
}

void ugo_fec_stream_tx_destroy(ugo_stream_tx* tx) {
  if (!tx) return;
  {
    DeviceGuard g(tx->ctx->device);
    (void)sync_sets(tx);
    (void)hipFree(tx->win);
    (void)hipFree(tx->rq);
    (void)hipFree(tx->rec);
  }
  delete tx;
}

int ugo_fec_stream_tx_window(ugo_stream_tx* tx, uint8_t** window_dev, size_t* window_bytes) {
  if (!tx || !window_dev || !window_bytes) return UGO_FEC_ERR_INVALID_ARG;
  *window_dev = tx->win;
  *window_bytes = tx->cap;
  return UGO_FEC_OK;
}

int ugo_fec_stream_tx_queue(ugo_stream_tx* tx, ugo_stream_tx_rq_entry** rq_dev, size_t* rq_cap) {
  if (!tx || !rq_dev || !rq_cap) return UGO_FEC_ERR_INVALID_ARG;
  *rq_dev = tx->rq;
  *rq_cap = tx->rq_cap;
  return UGO_FEC_OK;
}

int ugo_fec_stream_tx_set_create(ugo_fec* c, ugo_stream_tx* const* txs, size_t nconn, ugo_stream_tx_set** out) {
  static_assert(sizeof(ugo::kern::StreamTxEntry) == 40, "a table entry is 40 bytes");
  if (out) *out = nullptr;
  if (!c || !txs || !out || nconn == 0 || nconn > ugo::kern::kTxSetMaxConn) return UGO_FEC_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    // (a window listed twice would be planned twice from one record)
    if (!ugo::members::list_ok(c, txs, nconn)) return UGO_FEC_ERR_INVALID_ARG;
    if (c->poisoned) return UGO_FEC_ERR_HIP;
    DeviceGuard g(c->device);
    if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
    std::vector<ugo::kern::StreamTxEntry> host(nconn);
    size_t max_cap = 0;
    for (size_t i = 0; i < nconn; ++i) {
      ugo_stream_tx* tx = txs[i];
      host[i] = {tx->win, tx->rq, tx->rec, tx->cap, static_cast<uint32_t>(tx->rq_cap), 0u};
      max_cap = std::max(max_cap, tx->cap);
    }
    ugo_stream_tx_set* set = new (std::nothrow) ugo_stream_tx_set();
    if (!set) return UGO_FEC_ERR_HIP;
    set->ctx = c;
    set->wblocks = ugo::kern::stream_tx_wblocks(max_cap, static_cast<uint32_t>(nconn));
    const size_t nwords = 2 * ugo::kern::kTxScanBlock + nconn + 1;
    if (hipMalloc(&set->table, nconn * sizeof(host[0])) != hipSuccess ||
        hipMalloc(&set->gathered, nconn * sizeof(ugo_stream_tx_state)) != hipSuccess ||
        hipMalloc(&set->scratch, nconn * sizeof(ugo::kern::StreamTxPlanScratch)) != hipSuccess ||
        hipMalloc(&set->words, nwords * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(set->words, 0, nwords * sizeof(uint64_t)) != hipSuccess ||
        hipMemcpy(set->table, host.data(), nconn * sizeof(host[0]), hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
      (void)hipGetLastError();
      ugo_fec_stream_tx_set_destroy(set);
      return UGO_FEC_ERR_HIP;
    }
    set_register(set, txs, nconn, ugo_fec_stream_tx_set_destroy);
    *out = set;
    return UGO_FEC_OK;
  });
}

void ugo_fec_stream_tx_set_destroy(ugo_stream_tx_set* set) {
  set_destroy(set, [set] {
    (void)hipFree(set->table);
    (void)hipFree(set->gathered);
    (void)hipFree(set->scratch);
    (void)hipFree(set->words);
  });
}

int ugo_fec_stream_tx_set_write(ugo_stream_tx_set* set, const uint8_t* src, const uint64_t* src_off,
                                const uint64_t* n, uint64_t* n_written, void* stream) {
  const auto rule = [&] {
    return !(!src || !src_off || !n || !n_written || reinterpret_cast<uintptr_t>(src_off) % 8 ||
             reinterpret_cast<uintptr_t>(n) % 8 || reinterpret_cast<uintptr_t>(n_written) % 8);
  };
  SetCall call(set, false, rule, stream, src, src_off, n, n_written);
  if (!call.go) return call.status;
  ugo::kern::StreamTxWriteArgs a{};
  a.table = set->table;
  a.src = src;
  a.src_off = src_off;
  a.n = n;
  a.n_written = reinterpret_cast<unsigned long long*>(n_written);
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.wblocks = set->wblocks;
  return hip_status(ugo::kern::launch_stream_tx_write(a, call.s));
}

int ugo_fec_stream_tx_set_release(ugo_stream_tx_set* set, const uint64_t* upto, void* stream) {
  SetCall call(set, false, [&] { return upto && reinterpret_cast<uintptr_t>(upto) % 8 == 0; }, stream, upto);
  if (!call.go) return call.status;
  return hip_status(ugo::kern::launch_stream_tx_release(set->table, static_cast<uint32_t>(set->members.size()), upto,
                                                        call.s));
}

int ugo_fec_stream_tx_set_retransmit(ugo_stream_tx_set* set, const uint32_t* conn_of, const uint64_t* offset,
                                     const uint32_t* len, size_t m, uint8_t* status, void* stream) {
  const auto rule = [&] {
    return !(!conn_of || !offset || !len || !status || m > (size_t(1) << 31) ||
             reinterpret_cast<uintptr_t>(conn_of) % 4 || reinterpret_cast<uintptr_t>(offset) % 8 ||
             reinterpret_cast<uintptr_t>(len) % 4);
  };
  SetCall call(set, m == 0, rule, stream, conn_of, offset, len, status);
  if (!call.go) return call.status;
  const size_t nconn = set->members.size();
  ugo::kern::StreamTxRetransmitArgs a{};
  a.table = set->table;
  a.conn_of = conn_of;
  a.offset = offset;
  a.len = len;
  a.status = status;
  a.unsorted = reinterpret_cast<uint32_t*>(set->words + 2 * ugo::kern::kTxScanBlock + nconn);
  a.m = m;
  a.nconn = static_cast<uint32_t>(nconn);
  return hip_status(ugo::kern::launch_stream_tx_retransmit(a, call.s));
}

int ugo_fec_stream_tx_set_plan(ugo_stream_tx_set* set, const uint32_t* budget, size_t max_payload,
                               size_t max_segments, size_t max_packets, ugo_pkt_info* info, ugo_pkt_segment* segs,
                               uint32_t* conn_of, uint64_t* first_packet, uint32_t* n_packets, uint64_t* total,
                               void* stream) {
  const auto rule = [&] {
    return !(!budget || !first_packet || !n_packets || !total || max_payload < 16 || max_payload > 0xffff ||
             max_segments == 0 || max_segments > 0xffff || max_packets > (size_t(1) << 31) ||
             (max_packets && (!info || !segs || !conn_of)) || reinterpret_cast<uintptr_t>(budget) % 4 ||
             reinterpret_cast<uintptr_t>(info) % 8 || reinterpret_cast<uintptr_t>(segs) % 8 ||
             reinterpret_cast<uintptr_t>(conn_of) % 4 || reinterpret_cast<uintptr_t>(first_packet) % 8 ||
             reinterpret_cast<uintptr_t>(n_packets) % 4 || reinterpret_cast<uintptr_t>(total) % 8);
  };
  SetCall call(set, false, rule, stream, budget, info, segs, conn_of, first_packet, n_packets, total);
  if (!call.go) return call.status;
  ugo::kern::StreamTxPlanArgs a{};
  a.table = set->table;
  a.budget = budget;
  a.info = info;
  a.segs = segs;
  a.conn_of = conn_of;
  a.first_packet = reinterpret_cast<unsigned long long*>(first_packet);
  a.n_packets = n_packets;
  a.total = reinterpret_cast<unsigned long long*>(total);
  a.scratch = set->scratch;
  a.block_budget = set->words;
  a.block_first = set->words + ugo::kern::kTxScanBlock;
  a.first_dense = set->words + 2 * ugo::kern::kTxScanBlock;
  a.max_packets = max_packets;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.max_payload = static_cast<uint32_t>(max_payload);
  a.max_segments = static_cast<uint32_t>(max_segments);
  return hip_status(ugo::kern::launch_stream_tx_plan(a, call.s));
}

int ugo_fec_stream_tx_set_encode(ugo_stream_tx_set* set, const ugo_pkt_info* info, const uint64_t* ranges,
                                 size_t max_ranges, const ugo_pkt_segment* segs, size_t max_segments,
                                 const uint32_t* conn_of, size_t npk, const uint8_t* pad, unsigned flags,
                                 uint8_t* wire, size_t slot, uint16_t* wire_lens, uint8_t* status, void* stream) {
  const auto rule = [&] {
    return !(!info || !conn_of || !wire || !wire_lens || !status || slot % 16 || slot == 0 || slot > 0xffff ||
             reinterpret_cast<uintptr_t>(wire) % 16 || (pad && reinterpret_cast<uintptr_t>(pad) % 16) ||
             reinterpret_cast<uintptr_t>(conn_of) % 4 || (max_ranges && !ranges) || (max_segments && !segs) ||
             max_ranges > 0xffff || max_segments > 0xffff || (flags & ~UGO_PKT_FEC_FRAMED) ||
             ((flags & UGO_PKT_FEC_FRAMED) && pad) || npk > (size_t(1) << 31));
  };
  SetCall call(set, npk == 0, rule, stream, info, ranges, segs, conn_of, pad, wire, wire_lens, status);
  if (!call.go) return call.status;
  ugo::kern::PktEncSetArgs a{};
  a.info = info;
  a.ranges = ranges;
  a.segs = segs;
  a.pad = pad;
  a.wire = wire;
  a.wire_lens = wire_lens;
  a.status = status;
  a.npk = npk;
  a.slot = slot;
  a.max_ranges = static_cast<uint32_t>(max_ranges);
  a.max_segments = static_cast<uint32_t>(max_segments);
  a.framed = flags & UGO_PKT_FEC_FRAMED;
  a.conn_of = conn_of;
  a.table = set->table;
  a.nconn = static_cast<uint32_t>(set->members.size());
  return hip_status(ugo::kern::launch_packet_encode_set(a, call.s));
}

int ugo_fec_stream_tx_set_state(ugo_stream_tx_set* set, ugo_stream_tx_state* host_out) {
  return set_state(set, host_out, ugo::kern::launch_stream_tx_gather);  // departs from SetCall: no poisoned test
}

}  // extern "C"
