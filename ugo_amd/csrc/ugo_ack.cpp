// ugo_ack.cpp -- C ABI of the receive histories (include/ugo_ack.h).  Host-side
// control plane only: the argument rules are host/ack_args.hpp, the kernels
// ack_kernels.hip.
#include "host/set_call.hpp"

using namespace ugo::host;

extern "C" {

int ugo_fec_ack_rx_create(ugo_fec* c, size_t window_packets, ugo_ack_rx** out) {
  static_assert(sizeof(ugo_ack_state) == 64, "ugo_ack_state is 64 bytes");
  static_assert(sizeof(ugo::kern::AckEntry) == 24, "a table entry is 24 bytes");
  static_assert(UGO_FEC_KERNEL_ACK == ugo::kern::kKAck, "kernel class matches ack_kernels.hpp");
  if (out) *out = nullptr;
  if (!c || !out || !ugo::ackargs::window_ok(window_packets)) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  ugo_ack_rx* rx = new (std::nothrow) ugo_ack_rx();
  if (!rx) return UGO_FEC_ERR_HIP;
  rx->ctx = c;
  rx->m.ctx = c;
  rx->m.window_packets = window_packets;
  const size_t bitmap_bytes = window_packets / 8;
  if (hipMalloc(&rx->m.bits, bitmap_bytes) != hipSuccess || hipMalloc(&rx->m.rec, sizeof(ugo_ack_state)) != hipSuccess ||
      hipMemset(rx->m.bits, 0, bitmap_bytes) != hipSuccess ||
      hipMemset(rx->m.rec, 0, sizeof(ugo_ack_state)) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {  // the fills ran on the null stream
    (void)hipGetLastError();
    ugo_fec_ack_rx_destroy(rx);
    return UGO_FEC_ERR_HIP;
  }
  *out = rx;
  return UGO_FEC_OK;
}

void ugo_fec_ack_rx_destroy(ugo_ack_rx* rx) {
  if (!rx) return;
  {
    DeviceGuard g(rx->ctx->device);
    (void)sync_sets(rx);
    (void)hipFree(rx->m.bits);
    (void)hipFree(rx->m.rec);
  }
  delete rx;
}

int ugo_fec_ack_rx_state(ugo_ack_rx* rx, ugo_ack_state* host_out) {
  if (!rx || !host_out) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(rx->ctx->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (sync_sets(rx) != hipSuccess) return UGO_FEC_ERR_HIP;
  return hip_status(hipMemcpy(host_out, rx->m.rec, sizeof(*host_out), hipMemcpyDeviceToHost));
}

int ugo_fec_ack_rx_bitmap(ugo_ack_rx* rx, uint64_t** bitmap_dev, size_t* window_packets) {
  if (!rx || !bitmap_dev || !window_packets) return UGO_FEC_ERR_INVALID_ARG;
  *bitmap_dev = rx->m.bits;
  *window_packets = rx->m.window_packets;
  return UGO_FEC_OK;
}

int ugo_fec_ack_set_create(ugo_fec* c, ugo_ack_rx* const* rxs, size_t nconn, ugo_ack_rx_set** out) {
  if (out) *out = nullptr;
  if (!c || !rxs || !out || nconn == 0 || nconn > ugo::kern::kAckSetMaxConn) return UGO_FEC_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::vector<const ugo::ackargs::Member*> ms(nconn);
    for (size_t i = 0; i < nconn; ++i) ms[i] = rxs[i] ? &rxs[i]->m : nullptr;
    if (!ugo::ackargs::members_ok(c, ms.data(), nconn)) return UGO_FEC_ERR_INVALID_ARG;
    if (c->poisoned) return UGO_FEC_ERR_HIP;
    const std::vector<ugo::kern::AckEntry> host = ugo::ackargs::build_table(ms.data(), nconn);
    DeviceGuard g(c->device);
    if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
    ugo_ack_rx_set* set = new (std::nothrow) ugo_ack_rx_set();
    if (!set) return UGO_FEC_ERR_HIP;
    set->ctx = c;
    const size_t nwords = ugo::kern::kAckScanBlock + 1;
    if (hipMalloc(&set->table, nconn * sizeof(host[0])) != hipSuccess ||
        hipMalloc(&set->gathered, nconn * sizeof(ugo_ack_state)) != hipSuccess ||
        hipMalloc(&set->call, nconn * sizeof(ugo::kern::AckCall)) != hipSuccess ||
        hipMalloc(&set->slot_local, nconn * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&set->words, nwords * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(set->call, 0, nconn * sizeof(ugo::kern::AckCall)) != hipSuccess ||
        hipMemset(set->slot_local, 0, nconn * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(set->words, 0, nwords * sizeof(uint64_t)) != hipSuccess ||
        hipMemcpy(set->table, host.data(), nconn * sizeof(host[0]), hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
      (void)hipGetLastError();
      ugo_fec_ack_set_destroy(set);
      return UGO_FEC_ERR_HIP;
    }
    set_register(set, rxs, nconn, ugo_fec_ack_set_destroy);
    *out = set;
    return UGO_FEC_OK;
  });
}

void ugo_fec_ack_set_destroy(ugo_ack_rx_set* set) {
  set_destroy(set, [set] {
    (void)hipFree(set->table);
    (void)hipFree(set->gathered);
    (void)hipFree(set->call);
    (void)hipFree(set->slot_local);
    (void)hipFree(set->words);
  });
}

int ugo_fec_ack_set_receive(ugo_ack_rx_set* set, const ugo_pkt_info* info, const uint32_t* conn_of, size_t npk,
                            const uint8_t* seg_status, size_t max_segments, uint64_t now_us, void* stream) {
  const auto rule = [&] { return ugo::ackargs::receive_ok(info, conn_of, npk, seg_status, max_segments); };
  SetCall call(set, npk == 0, rule, stream, info, conn_of, seg_status);
  if (!call.go) return call.status;
  ugo::kern::AckReceiveArgs a{};
  a.table = set->table;
  a.call = set->call;
  a.info = info;
  a.conn_of = conn_of;
  a.seg_status = seg_status;
  a.npk = npk;
  a.now_us = now_us;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.max_segments = static_cast<uint32_t>(max_segments);
  return hip_status(ugo::kern::launch_ack_receive(a, call.s));
}

int ugo_fec_ack_set_touch(ugo_ack_rx_set* set, const uint8_t* flags, void* stream) {
  SetCall call(set, false, [&] { return flags != nullptr; }, stream, flags);
  if (!call.go) return call.status;
  return hip_status(
      ugo::kern::launch_ack_touch(set->table, static_cast<uint32_t>(set->members.size()), flags, call.s));
}

int ugo_fec_ack_set_attach(ugo_ack_rx_set* set, uint64_t now_us, const uint64_t* first_packet,
                           const uint32_t* n_packets, const uint64_t* total, const uint8_t* may_ack_only,
                           size_t max_packets, ugo_pkt_info* info, uint64_t* ranges, size_t max_ranges,
                           uint32_t* conn_of, uint64_t* total_out, uint8_t* attached, void* stream) {
  const auto rule = [&] {
    return ugo::ackargs::attach_ok(first_packet, n_packets, total, max_packets, info, ranges, max_ranges, conn_of,
                                   total_out, attached);
  };
  SetCall call(set, false, rule, stream, first_packet, n_packets, total, may_ack_only, info, ranges, conn_of,
               total_out, attached);
  if (!call.go) return call.status;
  ugo::kern::AckAttachArgs a{};
  a.table = set->table;
  a.first_packet = reinterpret_cast<const unsigned long long*>(first_packet);
  a.n_packets = n_packets;
  a.total = reinterpret_cast<const unsigned long long*>(total);
  a.may_ack_only = may_ack_only;
  a.info = info;
  a.ranges = ranges;
  a.conn_of = conn_of;
  a.total_out = reinterpret_cast<unsigned long long*>(total_out);
  a.attached = attached;
  a.slot_local = set->slot_local;
  a.block_slots = set->words;
  a.total_in = set->words + ugo::kern::kAckScanBlock;
  a.now_us = now_us;
  a.max_packets = max_packets;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.max_ranges = static_cast<uint32_t>(max_ranges);
  return hip_status(ugo::kern::launch_ack_attach(a, call.s));
}

int ugo_fec_ack_set_state(ugo_ack_rx_set* set, ugo_ack_state* host_out) {
  return set_state(set, host_out, ugo::kern::launch_ack_gather);  // departs from SetCall: no poisoned test
}

}  // extern "C"
