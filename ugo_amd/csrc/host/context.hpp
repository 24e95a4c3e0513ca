// context.hpp -- the context behind every handle of the C ABI (struct ugo_fec)
// and what each unit of the ABI needs around a call on it: the device guard,
// the launch-timer scope, device views of caller pointers and the HIP status.
// Internal to ugo_amd/csrc/ugo_*.cpp; nothing here is exported.
#pragma once
#include "../../../include/ugo_fec.h"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../fec_kernels.hpp"
#include "../launch.hpp"

namespace ugo {
// What the units of the C ABI share.  Hidden: libugofec.so exports the C ABI, not its plumbing.
namespace host __attribute__((visibility("hidden"))) {

constexpr int kStreams = 3;

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace host
}  // namespace ugo

struct ugo_fec {
  int device = 0;
  int d = 0, p = 0, n = 0;
  std::vector<uint8_t> M;  // n x d
  uint32_t dpad = 0, epad = 0, desc_stride = 0;
  int table_max = 16;       // d+p <= table_max -> host-built pattern table (MODE 1)
  uint8_t* d_M = nullptr;
  uint8_t* d_gf = nullptr;  // exp[512] | log[256] | pad | gf::perm_tables at +1024
  uint8_t* d_encdesc = nullptr;
  uint8_t* d_table = nullptr;
  // stream-ordered scratch (MODE 2 descriptors, RX claim words): allocated and
  // freed on the call's own stream, so calls on different streams never share
  // a workspace
  hipMemPool_t pool = nullptr;
  std::vector<std::pair<hipStream_t, hipEvent_t>> scratch_ev;  // per stream: behind its last scratch free
  // host-path staging
  hipStream_t streams[ugo::host::kStreams] = {};
  uint8_t* d_stage[ugo::host::kStreams] = {};
  uint64_t* d_mask[ugo::host::kStreams] = {};
  int8_t* d_status[ugo::host::kStreams] = {};
  uint64_t* d_zc_mask = nullptr;  // zero-copy host reconstruct: presence masks / status of the batch,
  int8_t* d_zc_status = nullptr;   // pinned host memory the kernels read / write through its mapping
  // RX: k_rx_begin's record of calls that found a presence bit set (atomicMax of
  // the call id), and this context's call counter
  unsigned long long* d_rxseen = nullptr;
  unsigned long long rx_calls = 0;
  // one-launch lossy list (k_lossy_list1): per stream, the tiles' epoch-tagged
  // count words (context-owned, zeroed once) and that stream's call epoch
  struct LossyWords {
    hipStream_t s;
    uint64_t* words;
    size_t tiles;
    uint32_t epoch;
  };
  std::vector<LossyWords> lossy_words;
  size_t zc_groups = 0;
  // d+p > 64: decode descriptors built on the host, one per erasure pattern
  // (klauspost caches its inversions per pattern the same way)
  std::unordered_map<std::string, std::vector<uint8_t>> wide_cache;
  int tx_route = 0;  // host TX wire route (ugo_fec_set_tx_host_route): 0 D2H copy, 1 mapped write
#ifndef UGO_COPY_QUEUE_DEFAULT
#define UGO_COPY_QUEUE_DEFAULT 1
#endif
  bool host_copy_queue = UGO_COPY_QUEUE_DEFAULT != 0;  // ugo_fec_set_host_copy_queue: streams[1] low priority
  bool streams_shared = false;  // streams[1] is the process-wide low-priority copy stream (not ours to destroy)
  size_t stage_groups = 0;  // groups per staging buffer
  size_t stage_pitch = 0;
  // launch timing (ugo_fec_timing_begin/end)
  bool timing = false;
  ugo::kern::LaunchTimer timer;
  // per-call service (ugo_fec_service_start): mailbox in coherent pinned memory
  bool svc_on = false;
  uint64_t svc_idle_ticks = 0;
  ugo::kern::SvcBox* svc_box = nullptr;   // host address
  ugo::kern::SvcBox* svc_dbox = nullptr;  // device view
  hipStream_t svc_stream = nullptr;
  uint32_t svc_seq = 0;                 // the last seq posted on the mailbox line
  uint32_t svc_timeout_ms = 5000;       // watchdog: a call's wait for an answer
  uint32_t svc_grace_ms = 5000;         // then: the wait for the block to leave
  uint32_t svc_stall_us = 0;            // tests only (ugo_fec_service_config)
  uint64_t svc_khz = 100000;            // wall_clock64's rate (100 MHz on gfx950)
  // the service block did not leave within the grace period: it may still read
  // the mailbox and tables and write a caller's batch, so every call fails and
  // destroy leaks what the block reads
  bool poisoned = false;
};

namespace ugo {
namespace host __attribute__((visibility("hidden"))) {

// Makes the context's launch timer (if on) the one the launchers of this
// thread see, for the duration of one ABI call.
struct TimerScope {
  ugo::kern::LaunchTimer* prev;
  explicit TimerScope(ugo_fec* c) : prev(ugo::kern::current_timer()) {
    ugo::kern::current_timer() = (c && c->timing) ? &c->timer : nullptr;
  }
  ~TimerScope() { ugo::kern::current_timer() = prev; }
};

inline int hip_status(hipError_t e) { return e == hipSuccess ? UGO_FEC_OK : UGO_FEC_ERR_HIP; }

// Device view of a buffer a kernel will touch: device (or managed) memory as
// is, pinned host memory through its device mapping (the kernel then reads or
// writes it over PCIe: zero-copy, e.g. a recvmmsg ring), anything else --
// pageable host memory the GPU cannot reach, or another GPU's memory -- rejected
// instead of faulting.  Called under the context's DeviceGuard, so the current
// device is the one the kernels run on.
template <typename T>
bool device_view(T*& p) {
  if (!p) return true;
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeUnified) return true;
  if (at.type == hipMemoryTypeDevice) {
    int cur = -1;
    return hipGetDevice(&cur) == hipSuccess && at.device == cur;
  }
  if (at.type != hipMemoryTypeHost || !at.devicePointer) return false;  // unregistered (pageable) memory
  if (at.devicePointer == at.hostPointer) return true;  // one address for host and device (ROCm)
  auto* base = static_cast<uint8_t*>(at.devicePointer);
  if (at.hostPointer) base += reinterpret_cast<const uint8_t*>(p) - static_cast<const uint8_t*>(at.hostPointer);
  p = reinterpret_cast<T*>(base);
  return true;
}

}  // namespace host
}  // namespace ugo
