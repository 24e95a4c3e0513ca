// set_call.hpp -- what the entry points of every set, of the controllers, the
// loop and the connection table do alike, written once: the prologue of a
// per-call entry point, the state call of a set, and the life of a set among
// its members.  The device-free member rule is host/member_list.hpp.
#pragma once
#include <algorithm>
#include <new>
#include <optional>

#include "handles.hpp"
#include "member_list.hpp"

namespace ugo {
namespace host __attribute__((visibility("hidden"))) {

// The prologue of one per-call entry point on handle h; it holds the device guard and the timer scope
// for the rest of the call.  The order of the checks is behaviour: it decides which status a call with
// two faults returns.
//   1. a NULL (or, for loop and cc, closed) handle   INVALID_ARG
//   2. a poisoned context                            ERR_HIP
//   3. an empty batch                                OK
//   4. the argument rule, rule()                     INVALID_ARG
//   5. the context's device                          NO_DEVICE
//   6. the device view of every pointer in ptrs      INVALID_ARG
//   7. the timer scope and the stream bookkeeping; the caller launches on `s`
// Use:  SetCall call(set, npk == 0, [&] { return rule_ok(...); }, stream, ptr, ptr, ...);
//       if (!call.go) return call.status;
template <class H>
struct SetCall {
  int status = UGO_FEC_OK;  // what the entry point returns when !go
  bool go = false;
  hipStream_t s = nullptr;
  std::optional<DeviceGuard> guard;
  std::optional<TimerScope> timer;

  template <class Rule, class... P>
  SetCall(H* h, bool empty, Rule rule, void* stream, P*&... ptrs) {
    status = enter(h, empty, rule, stream, ptrs...);
  }

 private:
  template <class Rule, class... P>
  int enter(H* h, bool empty, Rule rule, void* stream, P*&... ptrs) {
    if (!is_open(h)) return UGO_FEC_ERR_INVALID_ARG;
    ugo_fec* c = h->ctx;
    if (c->poisoned) return UGO_FEC_ERR_HIP;
    if (empty) return UGO_FEC_OK;
    if (!rule()) return UGO_FEC_ERR_INVALID_ARG;
    guard.emplace(c->device);
    if (!guard->ok) return UGO_FEC_ERR_NO_DEVICE;
    if (!(device_view(ptrs) && ...)) return UGO_FEC_ERR_INVALID_ARG;
    timer.emplace(c);
    s = h->use.record(stream);
    go = true;
    return UGO_FEC_OK;
  }
};

// ugo_fec_*_set_state: gathers the members' records on the set's last stream and copies them out.
// Departs from SetCall on purpose: no poisoned test, and `last` whether used or not.
template <class Set, class Rec, class Gather>
int set_state(Set* set, Rec* host_out, Gather gather) {
  if (!set || !host_out) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(set->ctx->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  const uint32_t nconn = static_cast<uint32_t>(set->members.size());
  if (gather(set->table, nconn, set->gathered, set->use.last) != hipSuccess ||
      hipStreamSynchronize(set->use.last) != hipSuccess)
    return UGO_FEC_ERR_HIP;
  return hip_status(hipMemcpy(host_out, set->gathered, nconn * sizeof(*host_out), hipMemcpyDeviceToHost));
}

// The calls made on a member through the sets it belongs to: its destroy and its state wait for them.
template <class M>
hipError_t sync_sets(const M* m) {
  hipError_t e = hipSuccess;
  for (const auto* set : m->sets)
    if (e == hipSuccess) e = set->use.wait();
  return e;
}

// The body of a create, whose host containers may throw std::bad_alloc: nothing throws through the C boundary.
template <class Build>
int guarded(Build build) {
  try {
    return build();
  } catch (const std::bad_alloc&) {
    return UGO_FEC_ERR_HIP;
  }
}

// The last step of a set's create: the set learns its members and they learn of it.  A set that fails
// halfway goes through its destroy, which takes it out of the members that had it already.
template <class Set, class M, class Destroy>
void set_register(Set* set, M* const* members, size_t nconn, Destroy destroy) {
  try {
    set->members.assign(members, members + nconn);
    for (M* m : set->members) m->sets.push_back(set);
  } catch (const std::bad_alloc&) {
    destroy(set);
    throw;
  }
}

// A set's destroy: waits for its calls, closes the loop sets that read its table, frees its device
// arrays (release()) and takes it out of its members' lists.
template <class Set, class Release>
void set_destroy(Set* set, Release release) {
  if (!set) return;
  {
    DeviceGuard g(set->ctx->device);
    (void)set->use.wait();
    loop_sets_close(set->loop_sets);
    release();
  }
  for (auto* m : set->members) m->sets.erase(std::remove(m->sets.begin(), m->sets.end(), set), m->sets.end());
  delete set;
}

}  // namespace host
}  // namespace ugo
