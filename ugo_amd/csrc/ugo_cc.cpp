// ugo_cc.cpp -- C ABI of congestion control (include/ugo_cc.h): a set of
// controllers over a set of sent histories.  ugo_fec_cc_sent_ack, a call on the
// sent set, is in ugo_sent.cpp.  Host-side control plane only: the argument
// rules are host/cc_args.hpp, the kernels cc_kernels.hip.
#include "host/cc_args.hpp"
#include "host/set_call.hpp"

using namespace ugo::host;

namespace {
int cc_set_build(ugo_fec* c, ugo_sent_tx_set* sent, const ugo_cc_params& p, ugo_cc_set** out) {
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  const std::vector<ugo_cc_state> init(sent->members.size(), ugo::ccargs::initial(p));
  sent->cc_sets.reserve(sent->cc_sets.size() + 1);  // what may throw comes before the set exists
  ugo_cc_set* set = new (std::nothrow) ugo_cc_set();
  if (!set) return UGO_FEC_ERR_HIP;
  set->ctx = c;
  set->params = p;
  set->nconn = init.size();
  sent->cc_sets.push_back(set);
  set->sent = sent;
  if (hipMalloc(&set->recs, set->nconn * sizeof(ugo_cc_state)) != hipSuccess ||
      hipMalloc(&set->cutback, set->nconn * sizeof(uint64_t)) != hipSuccess ||
      hipMemset(set->cutback, 0, set->nconn * sizeof(uint64_t)) != hipSuccess ||
      hipMemcpy(set->recs, init.data(), set->nconn * sizeof(ugo_cc_state), hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipGetLastError();
    ugo_fec_cc_set_destroy(set);
    return UGO_FEC_ERR_HIP;
  }
  *out = set;
  return UGO_FEC_OK;
}
}  // namespace

extern "C" {

int ugo_fec_cc_set_create(ugo_fec* c, ugo_sent_tx_set* sent, const ugo_cc_params* params, ugo_cc_set** out) {
  static_assert(sizeof(ugo_cc_state) == 192 && sizeof(ugo_cc_row) == 32 && sizeof(ugo_cc_params) == 20,
                "the layouts ugo_cc.h states");
  static_assert(UGO_FEC_KERNEL_CC == ugo::kern::kKCc, "kernel class matches sent_kernels.hpp");
  if (out) *out = nullptr;
  if (!c || !sent || !out || sent->ctx != c) return UGO_FEC_ERR_INVALID_ARG;
  const ugo_cc_params p = params ? *params : ugo::ccargs::defaults();
  if (!ugo::ccargs::params_ok(p)) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  return guarded([&] { return cc_set_build(c, sent, p, out); });
}

void ugo_fec_cc_set_destroy(ugo_cc_set* set) {
  if (!set) return;
  {
    DeviceGuard g(set->ctx->device);
    (void)set->use.wait();
    (void)hipFree(set->recs);
    (void)hipFree(set->cutback);
  }
  if (set->sent)
    set->sent->cc_sets.erase(std::remove(set->sent->cc_sets.begin(), set->sent->cc_sets.end(), set),
                             set->sent->cc_sets.end());
  delete set;
}

int ugo_fec_cc_set_cutback(ugo_cc_set* set, const uint64_t** dev) {
  if (!set || !dev) return UGO_FEC_ERR_INVALID_ARG;
  *dev = reinterpret_cast<const uint64_t*>(set->cutback);
  return UGO_FEC_OK;
}

int ugo_fec_cc_set_ack(ugo_cc_set* set, const ugo_sent_event* events, const ugo_cc_row* rows, uint64_t now_us,
                       uint64_t* delay_us, void* stream) {
  SetCall call(set, false, [&] { return ugo::ccargs::ack_ok(events, rows, delay_us); }, stream, events, rows,
               delay_us);
  if (!call.go) return call.status;
  ugo::kern::CcAckArgs a{};
  a.table = set->sent->table;
  a.recs = set->recs;
  a.cutback = set->cutback;
  a.events = events;
  a.rows = rows;
  a.delay_us = reinterpret_cast<unsigned long long*>(delay_us);
  a.now_us = now_us;
  a.p = set->params;
  a.nconn = static_cast<uint32_t>(set->nconn);
  return hip_status(ugo::kern::launch_cc_ack(a, call.s));
}

int ugo_fec_cc_set_rto(ugo_cc_set* set, const uint8_t* fired, size_t packet_bytes, size_t max_budget,
                       uint32_t* budget, void* stream) {
  SetCall call(set, false, [&] { return ugo::ccargs::rto_ok(fired, packet_bytes, max_budget, budget); }, stream, fired,
               budget);
  if (!call.go) return call.status;
  ugo::kern::CcRtoArgs a{};
  a.table = set->sent->table;
  a.recs = set->recs;
  a.cutback = set->cutback;
  a.fired = fired;
  a.budget = budget;
  a.packet_bytes = packet_bytes;
  a.max_budget = max_budget;
  a.p = set->params;
  a.nconn = static_cast<uint32_t>(set->nconn);
  return hip_status(ugo::kern::launch_cc_rto(a, call.s));
}

int ugo_fec_cc_set_state(ugo_cc_set* set, ugo_cc_state* host_out) {
  if (!set || !host_out) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(set->ctx->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (set->use.wait() != hipSuccess) return UGO_FEC_ERR_HIP;
  return hip_status(hipMemcpy(host_out, set->recs, set->nconn * sizeof(*host_out), hipMemcpyDeviceToHost));
}

}  // extern "C"
