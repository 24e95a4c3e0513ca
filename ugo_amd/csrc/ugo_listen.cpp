// ugo_listen.cpp -- C ABI of the connection table (include/ugo_listen.h).
// Host-side control plane only: the argument rules are host/listen_args.hpp,
// the kernels listen_kernels.hip.
#include "host/listen_args.hpp"
#include "host/set_call.hpp"

using namespace ugo::host;

extern "C" {

int ugo_fec_listen_create(ugo_fec* c, size_t max_conn, ugo_listen_table** out) {
  static_assert(sizeof(ugo_listen_state) == 80 && sizeof(ugo_listen_accept) == 48 && sizeof(ugo_listen_entry) == 32,
                "the layouts ugo_listen.h states");
  static_assert(UGO_FEC_KERNEL_LISTEN == ugo::kern::kKListen, "kernel class matches listen_kernels.hpp");
  if (out) *out = nullptr;
  if (!c || !out || !ugo::listenargs::max_conn_ok(max_conn)) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  ugo_listen_table* table = new (std::nothrow) ugo_listen_table();
  if (!table) return UGO_FEC_ERR_HIP;
  table->ctx = c;
  ugo::kern::ListenTable& t = table->t;
  t.max_conn = static_cast<uint32_t>(max_conn);
  t.n_slots = ugo::listenargs::slots_for(max_conn);
  if (hipMalloc(&t.slots, size_t(t.n_slots) * sizeof(ugo::kern::ListenSlot)) != hipSuccess ||
      hipMalloc(&t.claim, size_t(t.n_slots) * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&t.names, max_conn * UGO_LISTEN_NAME_BYTES) != hipSuccess ||
      hipMalloc(&t.tmp_names, max_conn * UGO_LISTEN_NAME_BYTES) != hipSuccess ||
      hipMalloc(&t.member_slot, max_conn * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&t.mark, max_conn * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&t.block_count, ugo::kern::kListenScanBlocks * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&t.st, sizeof(ugo_listen_state)) != hipSuccess ||
      hipMalloc(&t.call, sizeof(ugo::kern::ListenCall)) != hipSuccess ||
      hipMemset(t.tmp_names, 0, max_conn * UGO_LISTEN_NAME_BYTES) != hipSuccess ||
      hipMemset(t.block_count, 0, ugo::kern::kListenScanBlocks * sizeof(uint32_t)) != hipSuccess ||
      ugo::kern::launch_listen_init(t, nullptr) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipGetLastError();
    ugo_fec_listen_destroy(table);
    return UGO_FEC_ERR_HIP;
  }
  *out = table;
  return UGO_FEC_OK;
}

void ugo_fec_listen_destroy(ugo_listen_table* table) {
  if (!table) return;
  {
    DeviceGuard g(table->ctx->device);
    (void)table->use.wait();
    ugo::kern::ListenTable& t = table->t;
    (void)hipFree(t.slots);
    (void)hipFree(t.claim);
    (void)hipFree(t.names);
    (void)hipFree(t.tmp_names);
    (void)hipFree(t.member_slot);
    (void)hipFree(t.mark);
    (void)hipFree(t.block_count);
    (void)hipFree(t.st);
    (void)hipFree(t.call);
  }
  delete table;
}

int ugo_fec_listen_state(ugo_listen_table* table, ugo_listen_state* host_out) {
  if (!table || !host_out) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(table->ctx->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (table->use.wait() != hipSuccess) return UGO_FEC_ERR_HIP;
  return hip_status(hipMemcpy(host_out, table->t.st, sizeof(*host_out), hipMemcpyDeviceToHost));
}

int ugo_fec_listen_route(ugo_listen_table* table, const uint8_t* names, const uint8_t* pkts, size_t slot,
                         const uint16_t* lens, size_t npk, uint32_t* conn_of, uint8_t* cls,
                         ugo_listen_accept* accepted, size_t max_accepted, uint32_t* n_accepted, void* stream) {
  const auto rule = [&] {
    return ugo::listenargs::route_ok(names, pkts, slot, lens, npk, conn_of, cls, accepted, max_accepted, n_accepted);
  };
  SetCall call(table, npk == 0, rule, stream, names, pkts, lens, conn_of, cls, accepted, n_accepted);
  if (!call.go) return call.status;
  ugo::kern::ListenRouteArgs a{};
  a.t = table->t;
  a.names = names;
  a.pkts = pkts;
  a.lens = lens;
  a.conn_of = conn_of;
  a.cls = cls;
  a.accepted = accepted;
  a.n_accepted = n_accepted;
  a.slot = static_cast<uint32_t>(slot);
  a.npackets = static_cast<uint32_t>(npk);
  a.max_accepted = static_cast<uint32_t>(max_accepted);
  return hip_status(ugo::kern::launch_listen_route(a, call.s));
}

int ugo_fec_listen_remap(ugo_listen_table* table, const uint32_t* new_index, size_t n_index, size_t nconn_new,
                         uint32_t* status, void* stream) {
  SetCall call(table, false, [&] { return ugo::listenargs::remap_ok(new_index, n_index, nconn_new, status); }, stream,
               new_index, status);
  if (!call.go) return call.status;
  ugo::kern::ListenRemapArgs a{};
  a.t = table->t;
  a.new_index = new_index;
  a.status = status;
  a.n_index = static_cast<uint32_t>(n_index);
  a.nconn_new = static_cast<uint32_t>(std::min<size_t>(nconn_new, size_t(table->t.max_conn) + 1));
  return hip_status(ugo::kern::launch_listen_remap(a, call.s));
}

int ugo_fec_listen_names(ugo_listen_table* table, const uint32_t* conn_of, size_t npk, uint8_t* names_out,
                         uint32_t* name_lens, void* stream) {
  SetCall call(table, npk == 0, [&] { return ugo::listenargs::names_ok(conn_of, npk, names_out, name_lens); }, stream,
               conn_of, names_out, name_lens);
  if (!call.go) return call.status;
  ugo::kern::ListenNamesArgs a{};
  a.t = table->t;
  a.conn_of = conn_of;
  a.names_out = names_out;
  a.name_lens = name_lens;
  a.npackets = static_cast<uint32_t>(npk);
  return hip_status(ugo::kern::launch_listen_names(a, call.s));
}

int ugo_fec_listen_entries(ugo_listen_table* table, ugo_listen_entry* out, size_t cap, void* stream) {
  SetCall call(table, false, [&] { return ugo::listenargs::entries_ok(out, cap); }, stream, out);
  if (!call.go) return call.status;
  return hip_status(ugo::kern::launch_listen_entries(table->t, out, static_cast<uint32_t>(cap), call.s));
}

}  // extern "C"
