// ugo_stream_rx.cpp -- C ABI of stream delivery (include/ugo_stream.h): one
// receive window, and sets of them.  Host-side control plane only; the kernels
// are in stream_kernels.hip.
#include "host/set_call.hpp"

using namespace ugo::host;

namespace {
// A window as the kernels take it: rx->bits holds C | S | claim | contested,
// cap / 64 words each.
ugo::kern::StreamSetEntry stream_rx_entry(const ugo_stream_rx* rx) {
  const size_t words = rx->cap / 64;
  return {rx->win, rx->bits, rx->bits + words, rx->bits + 2 * words, rx->bits + 3 * words, rx->rec, rx->cap};
}

// The argument rule ugo_fec_stream_deliver and ugo_fec_stream_set_deliver share; conn_of is the set
// form's and stays null for a single window.  Both check poisoned before the batch, SetCall's order.
bool stream_deliver_ok(const uint8_t* pkts, size_t slot, const uint8_t* pad, const ugo_pkt_info* info,
                       const ugo_pkt_segment* segs, size_t max_segments, size_t npk, bool set,
                       const uint32_t* conn_of, const uint8_t* seg_status) {
  return !(!pkts || !info || !segs || (set && !conn_of) || !seg_status || slot % 16 || slot == 0 || slot > 0xffff ||
           reinterpret_cast<uintptr_t>(pkts) % 16 || (pad && reinterpret_cast<uintptr_t>(pad) % 16) ||
           reinterpret_cast<uintptr_t>(conn_of) % 4 || max_segments == 0 || max_segments > 0xffff ||
           npk > (size_t(1) << 31));
}
}  // namespace

extern "C" {

int ugo_fec_stream_rx_create(ugo_fec* c, size_t window_bytes, ugo_stream_rx** out) {
  static_assert(sizeof(ugo_stream_rx_state) == 96, "ugo_stream_rx_state is 96 bytes");
  static_assert(UGO_FEC_KERNEL_STREAM_DELIVER == ugo::kern::kKStreamDeliver &&
                    UGO_FEC_KERNEL_STREAM_READ == ugo::kern::kKStreamRead,
                "kernel classes match the header");
  if (out) *out = nullptr;
  if (!c || !out || window_bytes < UGO_STREAM_MIN_WINDOW || (window_bytes & (window_bytes - 1)) != 0)
    return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  ugo_stream_rx* rx = new (std::nothrow) ugo_stream_rx();
  if (!rx) return UGO_FEC_ERR_HIP;
  rx->ctx = c;
  rx->cap = window_bytes;
  const size_t bitmap_bytes = window_bytes / 8;
  ugo::kern::StreamRecord init;
  ugo::kern::stream_record_init(&init);
  if (hipMalloc(&rx->win, window_bytes) != hipSuccess || hipMalloc(&rx->bits, 4 * bitmap_bytes) != hipSuccess ||
      hipMalloc(&rx->rec, sizeof(init)) != hipSuccess || hipMemset(rx->win, 0, window_bytes) != hipSuccess ||
      hipMemset(rx->bits, 0, 4 * bitmap_bytes) != hipSuccess ||
      hipMemcpy(rx->rec, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {  // the fills ran on the null stream
    (void)hipGetLastError();
    ugo_fec_stream_rx_destroy(rx);
    return UGO_FEC_ERR_HIP;
  }
  *out = rx;
  return UGO_FEC_OK;
}

void ugo_fec_stream_rx_destroy(ugo_stream_rx* rx) {
  if (!rx) return;
  {
    DeviceGuard g(rx->ctx->device);
    if (rx->use.last) (void)hipStreamSynchronize(rx->use.last);
    (void)sync_sets(rx);
    (void)hipFree(rx->win);
    (void)hipFree(rx->bits);
    (void)hipFree(rx->rec);
  }
  delete rx;
}

int ugo_fec_stream_deliver(ugo_stream_rx* rx, const uint8_t* pkts, size_t slot, const uint8_t* pad,
                           const ugo_pkt_info* info, const ugo_pkt_segment* segs, size_t max_segments, size_t npk,
                           uint8_t* seg_status, void* stream) {
  const auto rule = [&] {
    return stream_deliver_ok(pkts, slot, pad, info, segs, max_segments, npk, false, nullptr, seg_status);
  };
  SetCall call(rx, npk == 0, rule, stream, pkts, pad, info, segs, seg_status);
  if (!call.go) return call.status;
  const ugo::kern::StreamSetEntry e = stream_rx_entry(rx);
  ugo::kern::StreamArgs a{};
  a.pkts = pkts;
  a.pad = pad;
  a.info = info;
  a.segs = segs;
  a.seg_status = seg_status;
  a.win = e.win;
  a.C = e.C;
  a.S = e.S;
  a.claim = e.claim;
  a.cont = e.cont;
  a.rec = e.rec;
  a.npk = npk;
  a.slot = slot;
  a.cap = e.cap;
  a.max_segments = static_cast<uint32_t>(max_segments);
  return hip_status(ugo::kern::launch_stream_deliver(a, call.s));
}

int ugo_fec_stream_read(ugo_stream_rx* rx, uint8_t* dst, size_t n, uint64_t* n_read, uint8_t* eof, void* stream) {
  if (!rx || !n_read) return UGO_FEC_ERR_INVALID_ARG;  // departs from SetCall: the rule comes before poisoned
  SetCall call(rx, false, [] { return true; }, stream, dst, n_read, eof);
  if (!call.go) return call.status;
  const ugo::kern::StreamSetEntry e = stream_rx_entry(rx);
  ugo::kern::StreamReadArgs a{};
  a.win = e.win;
  a.C = e.C;
  a.S = e.S;
  a.rec = e.rec;
  a.dst = dst;
  a.n_read = reinterpret_cast<unsigned long long*>(n_read);
  a.eof = eof;
  a.n = n;
  a.cap = e.cap;
  return hip_status(ugo::kern::launch_stream_read(a, call.s));
}

int ugo_fec_stream_rx_state(ugo_stream_rx* rx, ugo_stream_rx_state* host_out) {
  if (!rx || !host_out) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(rx->ctx->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  // departs from StreamUse::wait: `last` is synchronised whether used or not
  if (hipStreamSynchronize(rx->use.last) != hipSuccess || sync_sets(rx) != hipSuccess) return UGO_FEC_ERR_HIP;
  return hip_status(hipMemcpy(host_out, &rx->rec->pub, sizeof(*host_out), hipMemcpyDeviceToHost));
}

int ugo_fec_stream_rx_window(ugo_stream_rx* rx, uint8_t** window_dev, size_t* window_bytes) {
  if (!rx || !window_dev || !window_bytes) return UGO_FEC_ERR_INVALID_ARG;
  *window_dev = rx->win;
  *window_bytes = rx->cap;
  return UGO_FEC_OK;
}

// ---------------------------------------------------------------- receive-window sets
int ugo_fec_stream_set_create(ugo_fec* c, ugo_stream_rx* const* rxs, size_t nconn, ugo_stream_rx_set** out) {
  static_assert(sizeof(ugo::kern::StreamSetEntry) == 56, "a table entry is 56 bytes");
  if (out) *out = nullptr;
  if (!c || !rxs || !out || nconn == 0 || nconn > ugo::kern::kSetMaxConn) return UGO_FEC_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    // (a window listed twice: two table entries over one record would make the rule's atomics meaningless)
    if (!ugo::members::list_ok(c, rxs, nconn)) return UGO_FEC_ERR_INVALID_ARG;
    if (c->poisoned) return UGO_FEC_ERR_HIP;
    DeviceGuard g(c->device);
    if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
    std::vector<ugo::kern::StreamSetEntry> host(nconn);
    size_t max_cap = 0;
    for (size_t i = 0; i < nconn; ++i) {
      host[i] = stream_rx_entry(rxs[i]);
      max_cap = std::max(max_cap, rxs[i]->cap);
    }
    ugo_stream_rx_set* set = new (std::nothrow) ugo_stream_rx_set();
    if (!set) return UGO_FEC_ERR_HIP;
    set->ctx = c;
    set->wblocks = ugo::kern::stream_set_wblocks(max_cap);
    set->rblocks = ugo::kern::stream_set_rblocks(max_cap, static_cast<uint32_t>(nconn));
    if (hipMalloc(&set->table, nconn * sizeof(host[0])) != hipSuccess ||
        hipMalloc(&set->gathered, nconn * sizeof(ugo_stream_rx_state)) != hipSuccess ||
        hipMemcpy(set->table, host.data(), nconn * sizeof(host[0]), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      ugo_fec_stream_set_destroy(set);
      return UGO_FEC_ERR_HIP;
    }
    set_register(set, rxs, nconn, ugo_fec_stream_set_destroy);
    *out = set;
    return UGO_FEC_OK;
  });
}

void ugo_fec_stream_set_destroy(ugo_stream_rx_set* set) {
  set_destroy(set, [set] {
    (void)hipFree(set->table);
    (void)hipFree(set->gathered);
  });
}

int ugo_fec_stream_set_deliver(ugo_stream_rx_set* set, const uint8_t* pkts, size_t slot, const uint8_t* pad,
                               const ugo_pkt_info* info, const ugo_pkt_segment* segs, size_t max_segments,
                               size_t npk, const uint32_t* conn_of, uint8_t* seg_status, void* stream) {
  const auto rule = [&] {
    return stream_deliver_ok(pkts, slot, pad, info, segs, max_segments, npk, true, conn_of, seg_status);
  };
  SetCall call(set, npk == 0, rule, stream, pkts, pad, info, segs, conn_of, seg_status);
  if (!call.go) return call.status;
  ugo::kern::StreamSetArgs a{};
  a.pkts = pkts;
  a.pad = pad;
  a.info = info;
  a.segs = segs;
  a.seg_status = seg_status;
  a.conn_of = conn_of;
  a.table = set->table;
  a.npk = npk;
  a.slot = slot;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.max_segments = static_cast<uint32_t>(max_segments);
  a.wblocks = set->wblocks;
  return hip_status(ugo::kern::launch_stream_set_deliver(a, call.s));
}

int ugo_fec_stream_set_read(ugo_stream_rx_set* set, uint8_t* dst, const uint64_t* dst_off, const uint64_t* n,
                            uint64_t* n_read, uint8_t* eof, void* stream) {
  // departs from SetCall: the rule comes before poisoned
  if (!set || !n || !n_read || (dst && !dst_off) || reinterpret_cast<uintptr_t>(n) % 8 ||
      reinterpret_cast<uintptr_t>(n_read) % 8 || reinterpret_cast<uintptr_t>(dst_off) % 8)
    return UGO_FEC_ERR_INVALID_ARG;
  if (!dst) dst_off = nullptr;
  SetCall call(set, false, [] { return true; }, stream, dst, dst_off, n, n_read, eof);
  if (!call.go) return call.status;
  ugo::kern::StreamSetReadArgs a{};
  a.table = set->table;
  a.dst = dst;
  a.dst_off = dst_off;
  a.n = n;
  a.n_read = reinterpret_cast<unsigned long long*>(n_read);
  a.eof = eof;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.rblocks = set->rblocks;
  return hip_status(ugo::kern::launch_stream_set_read(a, call.s));
}

int ugo_fec_stream_set_state(ugo_stream_rx_set* set, ugo_stream_rx_state* host_out) {
  return set_state(set, host_out, ugo::kern::launch_stream_set_gather);  // departs from SetCall: no poisoned test
}

}  // extern "C"
