// ugo_loop.cpp -- C ABI of the connection loop (include/ugo_loop.h): one record
// per member of four neighbouring sets.  Host-side control plane only: the
// argument rules are host/loop_args.hpp, the kernels loop_kernels.hip.
#include "host/loop_args.hpp"
#include "host/set_call.hpp"

using namespace ugo::host;

namespace {
int loop_set_build(ugo_fec* c, ugo_stream_rx_set* srx, ugo_ack_rx_set* arx, ugo_stream_tx_set* stx,
                   ugo_sent_tx_set* sent, const ugo_loop_params& p, uint64_t now_us, ugo_loop_set** out) {
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  const size_t nconn = sent->members.size();
  const std::vector<ugo_loop_state> init(nconn, ugo::loopargs::initial(now_us));
  const std::vector<uint32_t> idle(4 * nconn, ugo::kern::kLoopIdle);
  const unsigned long long words[2] = {0ull, ~0ull};
  srx->loop_sets.reserve(srx->loop_sets.size() + 1);  // what may throw comes before the set exists
  arx->loop_sets.reserve(arx->loop_sets.size() + 1);
  stx->loop_sets.reserve(stx->loop_sets.size() + 1);
  sent->loop_sets.reserve(sent->loop_sets.size() + 1);
  ugo_loop_set* set = new (std::nothrow) ugo_loop_set();
  if (!set) return UGO_FEC_ERR_HIP;
  set->ctx = c;
  set->stream_rx = srx;
  set->ack_rx = arx;
  set->stream_tx = stx;
  set->sent_tx = sent;
  srx->loop_sets.push_back(set);
  arx->loop_sets.push_back(set);
  stx->loop_sets.push_back(set);
  sent->loop_sets.push_back(set);
  ugo::kern::LoopTables& t = set->t;
  t.stream_rx = srx->table;
  t.ack_rx = arx->table;
  t.stream_tx = stx->table;
  t.sent_tx = sent->table;
  t.p = p;
  t.nconn = static_cast<uint32_t>(nconn);
  const size_t nblock = ugo::kern::kLoopScanBlock * sizeof(uint32_t);
  if (hipMalloc(&t.recs, nconn * sizeof(ugo_loop_state)) != hipSuccess ||
      hipMalloc(&t.call, nconn * sizeof(ugo::kern::LoopCall)) != hipSuccess ||
      hipMalloc(&t.block_a, nblock) != hipSuccess || hipMalloc(&t.block_b, nblock) != hipSuccess ||
      hipMalloc(&t.words, sizeof(words)) != hipSuccess || hipMemset(t.block_a, 0, nblock) != hipSuccess ||
      hipMemset(t.block_b, 0, nblock) != hipSuccess ||
      hipMemcpy(t.recs, init.data(), nconn * sizeof(ugo_loop_state), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(t.call, idle.data(), nconn * sizeof(ugo::kern::LoopCall), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(t.words, words, sizeof(words), hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipGetLastError();
    ugo_fec_loop_set_destroy(set);
    return UGO_FEC_ERR_HIP;
  }
  *out = set;
  return UGO_FEC_OK;
}
}  // namespace

extern "C" {

int ugo_fec_loop_set_create(ugo_fec* c, ugo_stream_rx_set* srx, ugo_ack_rx_set* arx, ugo_stream_tx_set* stx,
                            ugo_sent_tx_set* sent, const ugo_loop_params* params, uint64_t now_us,
                            ugo_loop_set** out) {
  static_assert(sizeof(ugo_loop_state) == 64 && sizeof(ugo_loop_params) == 24, "the layouts ugo_loop.h states");
  static_assert(UGO_FEC_KERNEL_LOOP == ugo::kern::kKLoop, "kernel class matches loop_kernels.hpp");
  if (out) *out = nullptr;
  if (!c || !srx || !arx || !stx || !sent || !out || srx->ctx != c || arx->ctx != c || stx->ctx != c ||
      sent->ctx != c)
    return UGO_FEC_ERR_INVALID_ARG;
  if (!ugo::loopargs::nconn_ok(srx->members.size(), arx->members.size(), stx->members.size(), sent->members.size()))
    return UGO_FEC_ERR_INVALID_ARG;
  const ugo_loop_params p = params ? *params : ugo::loopargs::defaults();
  if (!ugo::loopargs::params_ok(p)) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  return guarded([&] { return loop_set_build(c, srx, arx, stx, sent, p, now_us, out); });
}

void ugo_fec_loop_set_destroy(ugo_loop_set* set) {
  if (!set) return;
  {
    DeviceGuard g(set->ctx->device);
    (void)set->use.wait();
    (void)hipFree(set->t.recs);
    (void)hipFree(set->t.call);
    (void)hipFree(set->t.block_a);
    (void)hipFree(set->t.block_b);
    (void)hipFree(set->t.words);
  }
  loop_set_detach(set);
  delete set;
}

int ugo_fec_loop_set_receive(ugo_loop_set* set, const ugo_pkt_info* info, uint32_t* conn_of, size_t npk,
                             uint64_t now_us, void* stream) {
  SetCall call(set, npk == 0, [&] { return ugo::loopargs::receive_ok(info, conn_of, npk); }, stream, info, conn_of);
  if (!call.go) return call.status;
  ugo::kern::LoopReceiveArgs a{};
  a.t = set->t;
  a.info = info;
  a.conn_of = conn_of;
  a.npk = npk;
  a.now_us = now_us;
  return hip_status(ugo::kern::launch_loop_receive(a, call.s));
}

int ugo_fec_loop_set_close(ugo_loop_set* set, const uint8_t* how, const uint64_t* linger_us, uint64_t now_us,
                           void* stream) {
  SetCall call(set, false, [&] { return ugo::loopargs::close_ok(how, linger_us); }, stream, how, linger_us);
  if (!call.go) return call.status;
  ugo::kern::LoopCloseArgs a{};
  a.t = set->t;
  a.how = how;
  a.linger_us = reinterpret_cast<const unsigned long long*>(linger_us);
  a.now_us = now_us;
  return hip_status(ugo::kern::launch_loop_close(a, call.s));
}

int ugo_fec_loop_set_check(ugo_loop_set* set, uint64_t now_us, uint32_t* budget, uint8_t* may_ack_only,
                           void* stream) {
  SetCall call(set, false, [&] { return ugo::loopargs::check_ok(budget, may_ack_only); }, stream, budget,
               may_ack_only);
  if (!call.go) return call.status;
  ugo::kern::LoopCheckArgs a{};
  a.t = set->t;
  a.budget = budget;
  a.may_ack_only = may_ack_only;
  a.now_us = now_us;
  return hip_status(ugo::kern::launch_loop_check(a, call.s));
}

int ugo_fec_loop_set_append(ugo_loop_set* set, const uint64_t* total, size_t max_packets, ugo_pkt_info* info,
                            ugo_pkt_segment* segs, size_t max_segments, uint32_t* conn_of, uint64_t* total_out,
                            uint8_t* appended, void* stream) {
  const auto rule = [&] {
    return ugo::loopargs::append_ok(total, max_packets, info, segs, max_segments, conn_of, total_out, appended);
  };
  SetCall call(set, false, rule, stream, total, info, segs, conn_of, total_out, appended);
  if (!call.go) return call.status;
  ugo::kern::LoopAppendArgs a{};
  a.t = set->t;
  a.total = reinterpret_cast<const unsigned long long*>(total);
  a.info = info;
  a.segs = segs;
  a.conn_of = conn_of;
  a.total_out = reinterpret_cast<unsigned long long*>(total_out);
  a.appended = appended;
  a.max_packets = max_packets;
  a.max_segments = max_segments;
  return hip_status(ugo::kern::launch_loop_append(a, call.s));
}

int ugo_fec_loop_set_sent(ugo_loop_set* set, const uint32_t* n_packets, const uint8_t* attached,
                          const uint64_t* delay_us, uint64_t now_us, uint64_t* deadline_us, uint32_t* exits,
                          uint8_t* reasons, size_t max_exits, uint64_t* n_exits, uint32_t* new_index,
                          uint64_t* nconn_new, void* stream) {
  const auto rule = [&] {
    return ugo::loopargs::sent_ok(n_packets, attached, delay_us, deadline_us, exits, reasons, max_exits, n_exits,
                                  new_index, nconn_new);
  };
  SetCall call(set, false, rule, stream, n_packets, attached, delay_us, deadline_us, exits, reasons, n_exits,
               new_index, nconn_new);
  if (!call.go) return call.status;
  ugo::kern::LoopSentArgs a{};
  a.t = set->t;
  a.n_packets = n_packets;
  a.attached = attached;
  a.delay_us = reinterpret_cast<const unsigned long long*>(delay_us);
  a.deadline_us = reinterpret_cast<unsigned long long*>(deadline_us);
  a.exits = exits;
  a.reasons = reasons;
  a.n_exits = reinterpret_cast<unsigned long long*>(n_exits);
  a.new_index = new_index;
  a.nconn_new = reinterpret_cast<unsigned long long*>(nconn_new);
  a.max_exits = max_exits;
  a.now_us = now_us;
  return hip_status(ugo::kern::launch_loop_sent(a, call.s));
}

int ugo_fec_loop_set_state(ugo_loop_set* set, ugo_loop_state* host_out) {
  if (!set || !host_out) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(set->ctx->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (set->use.wait() != hipSuccess) return UGO_FEC_ERR_HIP;
  return hip_status(
      hipMemcpy(host_out, set->t.recs, set->t.nconn * sizeof(*host_out), hipMemcpyDeviceToHost));
}

}  // extern "C"
