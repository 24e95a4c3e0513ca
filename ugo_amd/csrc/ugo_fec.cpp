// ugo_fec.cpp -- C-ABI (include/ugo_fec.h) of the MI355X FEC engine: the
// context and the calls on device memory.  The per-call service and the
// host-memory paths are ugo_fec_host.cpp, RX/TX assembly and the packet codec
// ugo_pkt.cpp, each later family its own ugo_*.cpp.
//
// Host-side control plane only: geometry validation (reedsolomon.New as called
// at ugo/fec.go:59), the code matrix, the decode-descriptor table (the analogue
// of klauspost's inversion-tree cache, built once per context instead of per
// erasure pattern on first use), argument checks mirroring checkShards, and
// launch selection.  All byte arithmetic runs in the gfx950 kernels of
// fec_kernels.hip; there is no CPU compute path for shard bytes.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <new>

#include "gf256.hpp"
#include "host/fec_core.hpp"
#include "host/rc4.hpp"

namespace ugo {
namespace host __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxItems = 0x7fffffffu;

// Groups per launch: a launch's work-item count is a uint32.  The vector
// kernels may pad every group to a whole number of waves (k_apply_qa: rows
// rounded up to 64 chunks), so a slice is sized from the padded count --
// otherwise a short-row code (e.g. 1 chunk per row, padded to 64) would wrap
// groups * 64 past 2^32 and leave most of the slice unwritten.
inline size_t slice_groups(uint32_t chunks, bool fast) {
  const size_t per_group = fast ? round_up(chunks, 64) : chunks;
  return std::max<size_t>(1, kMaxItems / per_group);
}

void timer_release(ugo_fec* c) {
  ugo::kern::LaunchTimer& t = c->timer;
  for (size_t i = 0; i < 2 * t.cap; ++i)
    if (t.ev[i]) (void)hipEventDestroy(t.ev[i]);
  delete[] t.ev;
  delete[] t.kid;
  t = ugo::kern::LaunchTimer{};
  c->timing = false;
}

// Decode descriptor for one presence mask (layout: fec_kernels.hip).
// Survivors = first d present rows in index order (klauspost Reconstruct),
// outputs = erased data rows then erased parity rows, coefficients
// Dinv[r] (data row r) or M[r] * Dinv (parity row r).
// Presence words per group: one for d+p <= 64, ceil((d+p)/64) above (bit r of
// the pattern = bit r % 64 of word r / 64).
size_t mask_words(const ugo_fec* c) { return (size_t(c->n) + 63) / 64; }

int build_desc_bits(const ugo_fec* c, const uint64_t* w, uint8_t* out) {
  const int d = c->d, n = c->n;
  auto present = [w](int r) { return (w[r >> 6] >> (r & 63)) & 1; };
  std::memset(out, 0, c->desc_stride);
  int np = 0;
  for (int r = 0; r < n; ++r) np += present(r);
  if (np == n) return UGO_FEC_OK;  // e = 0: nothing to rebuild
  if (np < d) {
    out[2] = UGO_FEC_ERR_TOO_FEW_SHARDS;
    return UGO_FEC_OK;
  }
  std::vector<uint8_t> sub(size_t(d) * d), inv(size_t(d) * d), work(size_t(2) * d * d);
  std::vector<int> surv, outr;
  for (int r = 0; r < n; ++r) {
    if (present(r)) {
      if (int(surv.size()) < d) surv.push_back(r);
    } else {
      outr.push_back(r);
    }
  }
  for (int i = 0; i < d; ++i) std::memcpy(&sub[size_t(i) * d], &c->M[size_t(surv[i]) * d], d);
  if (!ugo::gf::invert(d, sub.data(), inv.data(), work.data())) {
    out[2] = UGO_FEC_ERR_SINGULAR;
    return UGO_FEC_ERR_SINGULAR;
  }
  int e_data = 0;
  for (int r : outr) e_data += r < d;
  out[0] = static_cast<uint8_t>(outr.size());
  out[1] = static_cast<uint8_t>(e_data);
  for (int i = 0; i < d; ++i) out[4 + i] = static_cast<uint8_t>(surv[i]);
  for (size_t i = 0; i < outr.size(); ++i) out[4 + c->dpad + i] = static_cast<uint8_t>(outr[i]);
  uint8_t* coef = out + 4 + c->dpad + c->epad;
  for (size_t i = 0; i < outr.size(); ++i) {
    const int r = outr[i];
    for (int k = 0; k < d; ++k) {
      uint8_t v;
      if (r < d) {
        v = inv[size_t(r) * d + k];
      } else {
        v = 0;
        for (int j = 0; j < d; ++j) v ^= ugo::gf::mul(c->M[size_t(r) * d + j], inv[size_t(j) * d + k]);
      }
      coef[i * c->dpad + k] = v;
    }
  }
  return UGO_FEC_OK;
}

int build_desc(const ugo_fec* c, uint64_t mask, uint8_t* out) { return build_desc_bits(c, &mask, out); }

void free_ctx(ugo_fec* c) {
  if (!c) return;
  DeviceGuard g(c->device);
  // the resident block leaves before its mailbox and tables go
  if (c->poisoned || svc_stop(c) != UGO_FEC_OK) {
    // poisoned: a block that never left may still read the mailbox and tables
    // and write a caller's batch.  Every device-side release -- hipFree,
    // hipHostFree, stream and pool destruction -- synchronizes with the device
    // and would wait for that block (forever, if it never leaves), so all of
    // it is leaked; only the host-side object goes.
    delete c;
    return;
  }
  (void)hipHostFree(c->svc_box);
  (void)hipFree(c->d_M);
  (void)hipFree(c->d_gf);
  (void)hipFree(c->d_encdesc);
  (void)hipFree(c->d_table);
  (void)hipFree(c->d_rxseen);
  for (auto& lw : c->lossy_words) (void)hipFree(lw.words);
  timer_release(c);
  (void)hipHostFree(c->d_zc_mask);
  (void)hipHostFree(c->d_zc_status);
  for (int i = 0; i < kStreams; ++i) {
    (void)hipFree(c->d_stage[i]);
    (void)hipFree(c->d_mask[i]);
    (void)hipFree(c->d_status[i]);
    if (c->streams[i] && !is_shared_stream(c, i)) (void)hipStreamDestroy(c->streams[i]);
  }
  // this context's async scratch frees still queued on the callers' streams
  for (auto& se : c->scratch_ev) {
    (void)hipEventSynchronize(se.second);
    (void)hipEventDestroy(se.second);
  }
  if (c->pool) (void)hipMemPoolDestroy(c->pool);
  delete c;
}

Layout interleaved(const ugo_fec* c, size_t pitch) { return Layout{pitch, uint64_t(c->n) * pitch}; }

// The 16-B vector kernels need aligned rows; every d runs on them (d <= 32:
// register-array kernels, d > 32: the streaming kernels, which take any row
// length and output count).  Unaligned layouts run the byte kernel.
bool fast_layout(const ugo_fec*, const uint8_t* shards, const Layout& L, size_t) {
  return (reinterpret_cast<uintptr_t>(shards) % 16 == 0) && (L.rstride % 16 == 0) && (L.gstride % 16 == 0);
}

ugo::kern::Batch base_batch(const ugo_fec* c, uint8_t* shards, size_t S, const Layout& L) {
  ugo::kern::Batch a{};
  a.base = shards;
  a.gstride = L.gstride;
  a.rstride = L.rstride;
  a.nmask = c->n >= 64 ? ~0ull : ((1ull << c->n) - 1);
  a.S = static_cast<uint32_t>(S);
  a.desc_stride = c->desc_stride;
  a.d = static_cast<uint32_t>(c->d);
  a.dpad = c->dpad;
  a.epad = c->epad;
  a.mult = reinterpret_cast<const uint32_t*>(c->d_gf + 1024);
  return a;
}

// Bytes spanned by `rows` x `groups` slots of S bytes (row r of group g at
// g*gstride + r*rstride).
size_t extent(size_t S, size_t rstride, size_t rows, size_t gstride, size_t groups) {
  if (rows == 0 || groups == 0) return 0;
  return (groups - 1) * gstride + (rows - 1) * rstride + S;
}

// True if those slots are pairwise disjoint: sorted by stride, the smaller
// stride is >= S and the larger one clears a whole run of the smaller.
bool layout_disjoint(size_t S, size_t rstride, size_t rows, size_t gstride, size_t groups) {
  size_t small = rstride, ns = rows, large = gstride, nl = groups;
  if (ns <= 1 || (nl > 1 && gstride < rstride)) {
    std::swap(small, large);
    std::swap(ns, nl);
  }
  if (ns > 1 && small < S) return false;
  if (nl > 1 && large < (ns - 1) * small + S) return false;
  return true;
}

int check_batch(const ugo_fec* c, const void* shards, size_t groups, size_t S, const Layout& L) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (S == 0) return UGO_FEC_ERR_SHARD_NO_DATA;  // checkShards: all shards empty
  if (S > 0xffffffffu) return UGO_FEC_ERR_INVALID_ARG;
  if (groups == 0) return UGO_FEC_OK;  // an empty batch has no layout to check
  // no two shard slots may overlap: kernels write rows other lanes read
  if (!layout_disjoint(S, L.rstride, size_t(c->n), L.gstride, groups)) return UGO_FEC_ERR_INVALID_ARG;
  if (groups && !shards) return UGO_FEC_ERR_INVALID_ARG;
  return UGO_FEC_OK;
}

// Dense planar batch: groups packed back to back in each row (group stride ==
// S, no padding), rows 16-B aligned.  Encode is column-wise and every group
// uses the same matrix, so k = 16 / gcd(S, 16) consecutive groups form one
// pseudo-group of k*S bytes, a whole number of 16-B chunks: the vector kernels
// then read and write exactly the batch's bytes, with no padding and no
// partial chunk except at the batch's end.
bool dense_rows(const uint8_t* shards, size_t S, const Layout& L) {
  return L.gstride == S && S % 16 != 0 && reinterpret_cast<uintptr_t>(shards) % 16 == 0 && L.rstride % 16 == 0 &&
         S <= 0xffffffffu / 16;
}

int encode_dev(ugo_fec* c, uint8_t* shards, size_t groups, size_t S, const Layout& L, hipStream_t s) {
  if (c->p == 0 || groups == 0) return UGO_FEC_OK;
  if (groups > 1 && dense_rows(shards, S, L)) {
    size_t k = 16;
    while (S % (16 / k * 2) == 0) k /= 2;  // k = 16 / gcd(S, 16)
    const size_t full = groups / k, tail = groups % k;
    int st = full ? encode_dev(c, shards, full, k * S, Layout{L.rstride, k * S}, s) : UGO_FEC_OK;
    if (st == UGO_FEC_OK && tail)  // one pseudo-group (its group stride is never used)
      st = encode_dev(c, shards + full * k * S, 1, tail * S, Layout{L.rstride, round_up(tail * S, 16)}, s);
    return st;
  }
  const bool fast = fast_layout(c, shards, L, S);
  ugo::kern::Batch a = base_batch(c, shards, S, L);
  a.desc = c->d_encdesc;
  a.chunks = static_cast<uint32_t>(fast ? (S + 15) / 16 : (S + 3) / 4);
  const size_t per = slice_groups(a.chunks, fast);
  for (size_t g0 = 0; g0 < groups; g0 += per) {
    const size_t gn = std::min(per, groups - g0);
    a.g0 = g0;
    a.items = static_cast<uint32_t>(gn * a.chunks);
    hipError_t e;
    if (fast && ugo::kern::has_const_encode(c->d, c->p))
      e = ugo::kern::launch_encode_const(c->d, c->p, a, s);
    else if (fast)
      e = ugo::kern::launch_apply(0, ugo::kern::apply_dmax(c->d), a, s);
    else
      e = ugo::kern::launch_apply_bytes(0, a, s);
    if (e != hipSuccess) return UGO_FEC_ERR_HIP;
  }
  return UGO_FEC_OK;
}

// Scratch of `bytes` on stream s, from the context's memory pool (created on
// first use; memory is kept in the pool between calls, so after the first call
// an allocation is a host-side bookkeeping step).  Free with scratch_free on
// the same stream.
int scratch_alloc(ugo_fec* c, size_t bytes, hipStream_t s, void** out) {
  *out = nullptr;
  if (!c->pool) {
    hipMemPoolProps props{};
    props.allocType = hipMemAllocationTypePinned;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = c->device;
    if (hipMemPoolCreate(&c->pool, &props) != hipSuccess) {
      c->pool = nullptr;
      return UGO_FEC_ERR_HIP;
    }
    uint64_t keep = ~0ull;
    (void)hipMemPoolSetAttribute(c->pool, hipMemPoolAttrReleaseThreshold, &keep);
  }
  return hip_status(hipMallocFromPoolAsync(out, bytes ? bytes : 16, c->pool, s));
}

// Frees scratch on its stream and records, per stream, an event behind the
// free: destroying the context waits for exactly those events (its own
// scratch frees), not for every stream on the device -- other contexts'
// in-flight batches do not stall a destroy.
int scratch_free(ugo_fec* c, void* ptr, hipStream_t s) {
  if (!ptr) return UGO_FEC_OK;
  if (hipFreeAsync(ptr, s) != hipSuccess) return UGO_FEC_ERR_HIP;
  hipEvent_t ev = nullptr;
  for (auto& se : c->scratch_ev)
    if (se.first == s) ev = se.second;
  if (!ev) {
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return UGO_FEC_ERR_HIP;
    c->scratch_ev.emplace_back(s, ev);
  }
  return hip_status(hipEventRecord(ev, s));
}

bool fast_out(const OutBatch& O) {
  return !O.base || (reinterpret_cast<uintptr_t>(O.base) % 16 == 0 && O.L.rstride % 16 == 0 && O.L.gstride % 16 == 0);
}

constexpr size_t kWideCacheMax = 4096;  // patterns kept per context (d+p > 64)

// d+p > 64 (wider than one presence word): the decode descriptors are built on
// the host per erasure pattern (cached) and uploaded; the apply kernels run as
// for k_prepare's descriptors (MODE 2).  The masks are read on the host: from
// host_present when the caller has them there, else copied from the device
// (a synchronising copy -- wide codes are not ugo's geometry).
int reconstruct_wide(ugo_fec* c, uint8_t* shards, const uint64_t* present, size_t groups, size_t S,
                     const Layout& L, unsigned flags, int8_t* status, hipStream_t s, const OutBatch& O,
                     const uint64_t* host_present) {
  const size_t W = mask_words(c);
  std::vector<uint64_t> hm;
  if (!host_present) {
    hm.resize(groups * W);
    if (hipMemcpyAsync(hm.data(), present, hm.size() * sizeof(uint64_t), hipMemcpyDefault, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return UGO_FEC_ERR_HIP;
    host_present = hm.data();
  }
  const bool fast = fast_layout(c, shards, L, S) && fast_out(O);
  ugo::kern::Batch a = base_batch(c, shards, S, L);
  a.out = O.base;
  a.ogstride = O.L.gstride;
  a.orstride = O.L.rstride;
  a.status = status;
  a.data_only = (flags & UGO_FEC_RECONSTRUCT_DATA_ONLY) ? 1u : 0u;
  a.chunks = static_cast<uint32_t>(fast ? (S + 15) / 16 : (S + 3) / 4);
  const size_t per = std::min<size_t>(slice_groups(a.chunks, fast), 65536);
  const size_t stride = c->desc_stride;
  std::vector<uint8_t> hd(std::min(per, groups) * stride);
  uint8_t* work = nullptr;
  int st = scratch_alloc(c, hd.size() + 64, s, reinterpret_cast<void**>(&work));
  if (st) return st;
  struct Release {
    ugo_fec* c;
    uint8_t* p;
    hipStream_t s;
    ~Release() { (void)scratch_free(c, p, s); }
  } release{c, work, s};
  for (size_t g0 = 0; g0 < groups; g0 += per) {
    const size_t gn = std::min(per, groups - g0);
    for (size_t g = 0; g < gn; ++g) {
      const uint64_t* w = host_present + (g0 + g) * W;
      std::string key(reinterpret_cast<const char*>(w), W * sizeof(uint64_t));
      auto it = c->wide_cache.find(key);
      if (it == c->wide_cache.end()) {
        std::vector<uint8_t> dsc(stride);
        (void)build_desc_bits(c, w, dsc.data());  // a failure is the group's status byte
        if (c->wide_cache.size() >= kWideCacheMax) c->wide_cache.clear();
        it = c->wide_cache.emplace(std::move(key), std::move(dsc)).first;
      }
      std::memcpy(&hd[g * stride], it->second.data(), stride);
    }
    // hd is refilled for the next slice: the copy must have read it first
    if (hipMemcpyAsync(work, hd.data(), gn * stride, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return UGO_FEC_ERR_HIP;
    a.g0 = g0;
    a.items = static_cast<uint32_t>(gn * a.chunks);
    a.desc = work;
    a.g_desc0 = g0;
    const hipError_t e = fast ? ugo::kern::launch_apply(2, ugo::kern::apply_dmax(c->d), a, s)
                              : ugo::kern::launch_apply_bytes(2, a, s);
    if (e != hipSuccess) return UGO_FEC_ERR_HIP;
  }
  return UGO_FEC_OK;
}

int reconstruct_dev(ugo_fec* c, uint8_t* shards, const uint64_t* present, size_t groups, size_t S,
                    const Layout& L, unsigned flags, int8_t* status, hipStream_t s, const OutBatch& O,
                    const uint64_t* host_present) {
  if (groups == 0) return UGO_FEC_OK;
  if (!present) return UGO_FEC_ERR_INVALID_ARG;
  if (c->n > 64) return reconstruct_wide(c, shards, present, groups, S, L, flags, status, s, O, host_present);
  // A dense planar batch (group stride == S) runs k_apply_pd: lanes on the
  // rows' aligned 16-B chunks, the bytes of a chunk that straddles two groups
  // split between two lanes.  That kernel's shape: d <= 16, p <= 4, S >= 1009.
  const bool dense = dense_rows(shards, S, L) && ugo::kern::apply_dmax(c->d) > 0 &&
                     ugo::kern::apply_dmax(c->d) <= 16 && c->epad == 4 && S >= ugo::kern::kDenseMinS;
  const bool fast = (fast_layout(c, shards, L, S) && fast_out(O)) || dense;
  const int mode = c->d_table ? 1 : 2;
  ugo::kern::Batch a = base_batch(c, shards, S, L);
  a.out = O.base;
  a.ogstride = O.L.gstride;
  a.orstride = O.L.rstride;
  a.present = present;
  a.status = status;
  a.data_only = (flags & UGO_FEC_RECONSTRUCT_DATA_ONLY) ? 1u : 0u;
  a.chunks = static_cast<uint32_t>(fast ? (S + 15) / 16 : (S + 3) / 4);
  size_t per = slice_groups(a.chunks, fast);
  if (dense) {  // slices start on 16-B aligned bytes: a multiple of 16 / gcd(S, 16) groups
    per = std::max<size_t>(16, per / 16 * 16);
  }
  uint8_t* work = nullptr;
  if (mode == 2) {
    // per-group descriptors, bounded workspace (<= 64 Ki groups per slice)
    per = std::min<size_t>(per, 65536);
    const int st = scratch_alloc(c, std::min(per, groups) * c->desc_stride + 64, s, reinterpret_cast<void**>(&work));
    if (st) return st;
  }
  struct Release {  // the workspace goes back to the pool after this call's kernels
    ugo_fec* c;
    uint8_t* p;
    hipStream_t s;
    ~Release() { (void)scratch_free(c, p, s); }
  } release{c, work, s};
  for (size_t g0 = 0; g0 < groups; g0 += per) {
    const size_t gn = std::min(per, groups - g0);
    a.g0 = g0;
    a.items = static_cast<uint32_t>(gn * a.chunks);
    if (mode == 1) {
      a.desc = c->d_table;
    } else {
      ugo::kern::Prep pr{};
      pr.desc = work;
      pr.present = present;
      pr.M = c->d_M;
      pr.gf_exp = c->d_gf;
      pr.gf_log = c->d_gf + 512;
      pr.g0 = g0;
      pr.g_desc0 = g0;
      pr.nmask = a.nmask;
      pr.desc_stride = c->desc_stride;
      pr.d = static_cast<uint32_t>(c->d);
      pr.n = static_cast<uint32_t>(c->n);
      pr.dpad = c->dpad;
      pr.epad = c->epad;
      if (ugo::kern::launch_prepare(pr, static_cast<uint32_t>(gn), s) != hipSuccess) return UGO_FEC_ERR_HIP;
      a.desc = work;
      a.g_desc0 = g0;
    }
    hipError_t e;
    if (dense) {
      ugo::kern::Batch b = a;
      b.base = shards + g0 * S;
      b.n = static_cast<uint32_t>(gn);
      b.items = static_cast<uint32_t>((gn * S + 15) / 16);
      e = ugo::kern::launch_apply_dense(mode, ugo::kern::apply_dmax(c->d), b, s);
    } else {
      e = fast ? ugo::kern::launch_apply(mode, ugo::kern::apply_dmax(c->d), a, s)
               : ugo::kern::launch_apply_bytes(mode, a, s);
    }
    if (e != hipSuccess) return UGO_FEC_ERR_HIP;
  }
  return UGO_FEC_OK;
}

// ugo_fec_lossy_groups on device views: one launch (k_lossy_list1), or the
// two-launch form (k_lossy_count -> k_lossy_write) in A/B builds.
#ifndef UGO_LOSSY_ONE_LAUNCH
#define UGO_LOSSY_ONE_LAUNCH 1
#endif
constexpr bool kLossyOneLaunch = UGO_LOSSY_ONE_LAUNCH != 0;
int lossy_list_dev(ugo_fec* c, const uint64_t* present, size_t groups, unsigned flags, uint32_t* list,
                   uint32_t* count, hipStream_t s, uint32_t* rowoff, uint32_t* rows) {
  if (groups == 0) {
    if (rows && hipMemsetAsync(rows, 0, sizeof(uint32_t), s) != hipSuccess) return UGO_FEC_ERR_HIP;
    return hip_status(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
  }
  const uint64_t nmask = c->n >= 64 ? ~0ull : ((1ull << c->n) - 1);
  const uint64_t dmask =
      (flags & UGO_FEC_RECONSTRUCT_DATA_ONLY) && c->d < 64 ? ((1ull << c->d) - 1) : ~0ull;  // d = 64: p = 0
  const size_t blocks = (groups + ugo::kern::kLossyPerBlock - 1) / ugo::kern::kLossyPerBlock;
  if (kLossyOneLaunch) {
    // the stream's count words (made, or grown, on first use; zeroed once, on the call's own stream so the
    // zeroing is ordered before the kernel -- hipMemset is asynchronous to a non-blocking stream -- and
    // epoch 0 is never used)
    ugo_fec::LossyWords* lw = nullptr;
    for (auto& e : c->lossy_words)
      if (e.s == s) lw = &e;
    if (!lw || lw->tiles < blocks || lw->epoch == 0xffffffffu) {
      if (lw && hipStreamSynchronize(s) != hipSuccess) return UGO_FEC_ERR_HIP;
      const size_t tiles = std::max<size_t>(blocks, lw ? 2 * lw->tiles : 64);
      uint64_t* w = nullptr;
      if (hipMalloc(&w, tiles * sizeof(uint64_t)) != hipSuccess) return UGO_FEC_ERR_HIP;
      if (hipMemsetAsync(w, 0, tiles * sizeof(uint64_t), s) != hipSuccess) {
        (void)hipFree(w);
        return UGO_FEC_ERR_HIP;
      }
      if (lw) {
        (void)hipFree(lw->words);
        *lw = ugo_fec::LossyWords{s, w, tiles, 0};
      } else {
        c->lossy_words.push_back(ugo_fec::LossyWords{s, w, tiles, 0});
        lw = &c->lossy_words.back();
      }
    }
    const uint32_t epoch = ++lw->epoch;
    return hip_status(ugo::kern::launch_lossy_list1(present, groups, nmask, dmask, static_cast<uint32_t>(c->d), list,
                                                    count, rowoff, rows, lw->words, epoch, s));
  }
  void* work = nullptr;
  int st = scratch_alloc(c, 2 * blocks * sizeof(uint32_t), s, &work);
  if (st) return st;
  st = hip_status(ugo::kern::launch_lossy_list(present, groups, nmask, dmask, static_cast<uint32_t>(c->d), list,
                                               count, rowoff, rows, static_cast<uint32_t*>(work), s));
  const int fr = scratch_free(c, work, s);
  return st ? st : fr;
}

// ugo_fec_reconstruct_list on device views (arguments checked by the caller).
int reconstruct_list_dev(ugo_fec* c, const uint8_t* shards, const uint64_t* present, const uint32_t* list,
                         const uint32_t* count, size_t max_entries, size_t S, const Layout& L, uint8_t* out,
                         size_t out_row_stride, size_t out_entry_stride, unsigned flags, int8_t* status,
                         hipStream_t s, const uint32_t* rowoff, uint32_t* rowid, uint32_t max_rows) {
  ugo::kern::Batch a = base_batch(c, const_cast<uint8_t*>(shards), S, L);
  a.rowoff = rowoff;  // row-compact outputs (rx_recover_host, ugo_fec_recover_data)
  a.rowid = rowid;
  a.max_rows = max_rows;
  a.n = static_cast<uint32_t>(c->n);
  a.out = out;
  a.ogstride = out_entry_stride;
  a.orstride = out_row_stride;
  a.present = present;
  a.status = status;
  a.data_only = (flags & UGO_FEC_RECONSTRUCT_DATA_ONLY) ? 1u : 0u;
  a.chunks = static_cast<uint32_t>((S + 15) / 16);
  a.desc = c->d_table;
  a.list = list;
  a.count = count;
  const size_t per = slice_groups(a.chunks, true);
  for (size_t g0 = 0; g0 < max_entries; g0 += per) {
    const size_t gn = std::min(per, max_entries - g0);
    a.g0 = g0;
    a.items = static_cast<uint32_t>(gn * a.chunks);
    if (ugo::kern::launch_apply_list(ugo::kern::apply_dmax(c->d), a, s) != hipSuccess) return UGO_FEC_ERR_HIP;
  }
  return UGO_FEC_OK;
}
}  // namespace host
}  // namespace ugo

using namespace ugo::host;

extern "C" {

int ugo_fec_abi_version(void) { return UGO_FEC_ABI_VERSION; }

const char* ugo_fec_strerror(int s) {
  switch (s) {
    case UGO_FEC_OK: return "ok";
    case UGO_FEC_ERR_INV_SHARD_NUM:
      return "cannot create Encoder with less than one data shard or less than zero parity shards";
    case UGO_FEC_ERR_MAX_SHARD_NUM: return "cannot create Encoder with more than 256 data+parity shards";
    case UGO_FEC_ERR_TOO_FEW_SHARDS: return "too few shards given";
    case UGO_FEC_ERR_SHARD_NO_DATA: return "no shard data";
    case UGO_FEC_ERR_SHARD_SIZE: return "shard sizes do not match";
    case UGO_FEC_ERR_INVALID_ARG: return "invalid argument";
    case UGO_FEC_ERR_SINGULAR: return "matrix is singular";
    case UGO_FEC_ERR_HIP: return "HIP runtime error";
    case UGO_FEC_ERR_NO_DEVICE: return "no usable gfx950 device";
    default: return "unknown status";
  }
}

int ugo_fec_check_shards(int n, const size_t* lens, int nil_ok, size_t* shard_size) {
  if (n <= 0 || !lens) return UGO_FEC_ERR_INVALID_ARG;
  size_t size = 0;
  for (int i = 0; i < n; ++i)
    if (lens[i]) {
      size = lens[i];
      break;
    }
  if (shard_size) *shard_size = size;
  if (size == 0) return UGO_FEC_ERR_SHARD_NO_DATA;
  for (int i = 0; i < n; ++i)
    if (lens[i] != size && (lens[i] != 0 || !nil_ok)) return UGO_FEC_ERR_SHARD_SIZE;
  return UGO_FEC_OK;
}

int ugo_fec_create(int device, int data_shards, int parity_shards, ugo_fec** out) {
  if (!out) return UGO_FEC_ERR_INVALID_ARG;
  *out = nullptr;
  if (data_shards <= 0 || parity_shards < 0) return UGO_FEC_ERR_INV_SHARD_NUM;
  if (data_shards + parity_shards > 256) return UGO_FEC_ERR_MAX_SHARD_NUM;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return UGO_FEC_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return UGO_FEC_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return UGO_FEC_ERR_NO_DEVICE;
  DeviceGuard guard(device);
  if (!guard.ok) return UGO_FEC_ERR_NO_DEVICE;

  ugo_fec* c = new (std::nothrow) ugo_fec();
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  c->device = device;
  c->d = data_shards;
  c->p = parity_shards;
  c->n = data_shards + parity_shards;
  if (const char* env = std::getenv("UGO_FEC_TABLE_MAX_SHARDS")) c->table_max = std::atoi(env);
  const int d = c->d, p = c->p, n = c->n;
  c->M.resize(size_t(n) * d);
  std::vector<uint8_t> scratch(size_t(n) * d + 3 * size_t(d) * d);
  if (!ugo::gf::build_matrix(d, p, c->M.data(), scratch.data())) {
    delete c;
    return UGO_FEC_ERR_SINGULAR;
  }
  const int dmax = ugo::kern::apply_dmax(d);
  c->dpad = static_cast<uint32_t>(round_up(std::max(d, dmax), 4));
  c->epad = static_cast<uint32_t>(round_up(std::max(p, 1), 4));
  c->desc_stride = static_cast<uint32_t>(round_up(4 + c->dpad + c->epad + size_t(p) * c->dpad, 16));

  int st = UGO_FEC_OK;
  auto fail = [&](int code) {
    free_ctx(c);
    return code;
  };
  if (hipMalloc(&c->d_M, c->M.size()) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
  if (hipMemcpy(c->d_M, c->M.data(), c->M.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
  {
    std::vector<uint8_t> gf(1024 + 256 * 32, 0);  // exp | log | pad | perm tables
    std::memcpy(gf.data(), ugo::gf::kTables.exp, 512);
    std::memcpy(gf.data() + 512, ugo::gf::kTables.log, 256);
    ugo::gf::perm_tables(gf.data() + 1024);
    if (hipMalloc(&c->d_gf, gf.size()) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
    if (hipMemcpy(c->d_gf, gf.data(), gf.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
  }
  {
    // MODE 0 encode descriptor: inputs = data rows, outputs = parity rows
    std::vector<uint8_t> ed(c->desc_stride + 64, 0);
    ed[0] = static_cast<uint8_t>(p);
    ed[1] = 0;
    for (int i = 0; i < d; ++i) ed[4 + i] = static_cast<uint8_t>(i);
    for (int i = 0; i < p; ++i) ed[4 + c->dpad + i] = static_cast<uint8_t>(d + i);
    for (int i = 0; i < p; ++i)
      for (int k = 0; k < d; ++k) ed[4 + c->dpad + c->epad + size_t(i) * c->dpad + k] = c->M[size_t(d + i) * d + k];
    if (hipMalloc(&c->d_encdesc, ed.size()) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
    if (hipMemcpy(c->d_encdesc, ed.data(), ed.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
    if (hipMalloc(&c->d_rxseen, sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(c->d_rxseen, 0, sizeof(unsigned long long)) != hipSuccess)
      return fail(UGO_FEC_ERR_HIP);
  }
  if (n <= c->table_max && n <= 20) {
    const size_t entries = size_t(1) << n;
    std::vector<uint8_t> tab(entries * c->desc_stride + 64, 0);
    for (size_t m = 0; m < entries; ++m) {
      st = build_desc(c, m, &tab[m * c->desc_stride]);
      if (st) return fail(st);
    }
    if (hipMalloc(&c->d_table, tab.size()) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
    if (hipMemcpy(c->d_table, tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(UGO_FEC_ERR_HIP);
  }
  *out = c;
  return UGO_FEC_OK;
}

void ugo_fec_destroy(ugo_fec* c) { free_ctx(c); }

int ugo_fec_geometry(const ugo_fec* c, int* d, int* p, int* device) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (d) *d = c->d;
  if (p) *p = c->p;
  if (device) *device = c->device;
  return UGO_FEC_OK;
}

int ugo_fec_matrix(const ugo_fec* c, uint8_t* out) {
  if (!c || !out) return UGO_FEC_ERR_INVALID_ARG;
  std::memcpy(out, c->M.data(), c->M.size());
  return UGO_FEC_OK;
}

int ugo_fec_encode_strided(ugo_fec* c, uint8_t* shards, size_t groups, size_t S, size_t row_stride,
                           size_t group_stride, void* stream) {
  const Layout L{row_stride, group_stride};
  int st = check_batch(c, shards, groups, S, L);
  if (st) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (groups == 0) return UGO_FEC_OK;  // nothing is touched (an empty tensor's pointer may be anything)
  if (!device_view(shards)) return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  return encode_dev(c, shards, groups, S, L, static_cast<hipStream_t>(stream));
}

int ugo_fec_encode(ugo_fec* c, uint8_t* shards, size_t groups, size_t S, size_t pitch, void* stream) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (pitch < S) return S == 0 ? UGO_FEC_ERR_SHARD_NO_DATA : UGO_FEC_ERR_INVALID_ARG;
  return ugo_fec_encode_strided(c, shards, groups, S, pitch, size_t(c->n) * pitch, stream);
}

int ugo_fec_reconstruct_strided(ugo_fec* c, uint8_t* shards, const uint64_t* present, size_t groups, size_t S,
                                size_t row_stride, size_t group_stride, unsigned flags, int8_t* status,
                                void* stream) {
  const Layout L{row_stride, group_stride};
  int st = check_batch(c, shards, groups, S, L);
  if (st) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (groups == 0) return UGO_FEC_OK;
  if (!device_view(shards) || !device_view(present) || !device_view(status)) return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  return reconstruct_dev(c, shards, present, groups, S, L, flags, status, static_cast<hipStream_t>(stream));
}

int ugo_fec_reconstruct_into(ugo_fec* c, const uint8_t* shards, const uint64_t* present, size_t groups, size_t S,
                             size_t row_stride, size_t group_stride, uint8_t* out, size_t out_row_stride,
                             size_t out_group_stride, unsigned flags, int8_t* status, void* stream) {
  const Layout L{row_stride, group_stride};
  int st = check_batch(c, shards, groups, S, L);
  if (st) return st;
  if (groups == 0) return UGO_FEC_OK;
  // p output slots of S bytes per group: no two slots may overlap (the smaller
  // stride must clear S, the larger one a whole run of the smaller), and the
  // output may not overlap the batch it reads (other lanes would read rows
  // being overwritten)
  if (!out || !layout_disjoint(S, out_row_stride, size_t(c->p), out_group_stride, groups)) return UGO_FEC_ERR_INVALID_ARG;
  {
    const size_t in_ext = extent(S, row_stride, size_t(c->n), group_stride, groups);
    const size_t out_ext = extent(S, out_row_stride, size_t(c->p), out_group_stride, groups);
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(shards), o0 = reinterpret_cast<uintptr_t>(out);
    if (o0 < i0 + in_ext && i0 < o0 + out_ext) return UGO_FEC_ERR_INVALID_ARG;
  }
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(shards) || !device_view(present) || !device_view(status) || !device_view(out))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  OutBatch O;
  O.base = out;
  O.L = Layout{out_row_stride, out_group_stride};
  return reconstruct_dev(c, const_cast<uint8_t*>(shards), present, groups, S, L, flags, status,
                         static_cast<hipStream_t>(stream), O);
}

int ugo_fec_lossy_groups(ugo_fec* c, const uint64_t* present, size_t groups, unsigned flags, uint32_t* list,
                         uint32_t* count, void* stream) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (!present || !list || !count || c->n > 64 || groups >= 0xffffffffull) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(present) || !device_view(list) || !device_view(count)) return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  return lossy_list_dev(c, present, groups, flags, list, count, static_cast<hipStream_t>(stream));
}

int ugo_fec_reconstruct_list(ugo_fec* c, const uint8_t* shards, const uint64_t* present, size_t groups,
                             const uint32_t* list, const uint32_t* count, size_t max_entries, size_t S,
                             size_t row_stride, size_t group_stride, uint8_t* out, size_t out_row_stride,
                             size_t out_entry_stride, unsigned flags, int8_t* status, void* stream) {
  const Layout L{row_stride, group_stride};
  int st = check_batch(c, shards, groups, S, L);
  if (st) return st;
  if (groups == 0 || max_entries == 0) return UGO_FEC_OK;
  if (!present || !list || !count || c->n > 16 || !c->d_table || max_entries > groups)
    return UGO_FEC_ERR_INVALID_ARG;
  if (!fast_layout(c, shards, L, S)) return UGO_FEC_ERR_INVALID_ARG;
  const size_t oslots = (flags & UGO_FEC_RECONSTRUCT_DATA_ONLY) ? size_t(std::min(c->d, c->p)) : size_t(c->p);
  if (out) {
    if (reinterpret_cast<uintptr_t>(out) % 16 || out_row_stride % 16 || out_entry_stride % 16 ||
        !layout_disjoint(S, out_row_stride, oslots, out_entry_stride, max_entries))
      return UGO_FEC_ERR_INVALID_ARG;
    const size_t in_ext = extent(S, row_stride, size_t(c->n), group_stride, groups);
    const size_t out_ext = extent(S, out_row_stride, oslots, out_entry_stride, max_entries);
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(shards), o0 = reinterpret_cast<uintptr_t>(out);
    if (o0 < i0 + in_ext && i0 < o0 + out_ext) return UGO_FEC_ERR_INVALID_ARG;
  }
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(shards) || !device_view(present) || !device_view(list) || !device_view(count) ||
      !device_view(status) || !device_view(out))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  return reconstruct_list_dev(c, shards, present, list, count, max_entries, S, L, out, out_row_stride,
                              out_entry_stride, flags, status, static_cast<hipStream_t>(stream));
}

int ugo_fec_recover_data(ugo_fec* c, const uint8_t* shards, const uint64_t* present, size_t groups, size_t S,
                         size_t row_stride, size_t group_stride, uint8_t* out, size_t out_row_stride, size_t max_rows,
                         uint32_t* index, uint32_t* count, void* stream) {
  const Layout L{row_stride, group_stride};
  int st = check_batch(c, shards, groups, S, L);
  if (st) return st;
  if (!present || !count || c->n > 16 || !c->d_table || groups * size_t(c->n) >= 0xffffffffull ||
      max_rows > 0xffffffffull || (max_rows && (!out || !index)))
    return UGO_FEC_ERR_INVALID_ARG;
  if (!fast_layout(c, shards, L, S)) return UGO_FEC_ERR_INVALID_ARG;
  if (max_rows) {
    if (reinterpret_cast<uintptr_t>(out) % 16 || out_row_stride % 16 || out_row_stride < round_up(S, 16))
      return UGO_FEC_ERR_INVALID_ARG;
    const size_t in_ext = extent(S, row_stride, size_t(c->n), group_stride, groups);
    const size_t out_ext = (max_rows - 1) * out_row_stride + S;
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(shards), o0 = reinterpret_cast<uintptr_t>(out);
    if (o0 < i0 + in_ext && i0 < o0 + out_ext) return UGO_FEC_ERR_INVALID_ARG;
  }
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(shards) || !device_view(present) || !device_view(out) || !device_view(index) ||
      !device_view(count))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (groups == 0) return hip_status(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
  // scratch: the lossy-group list | each entry's first output row | the entry count
  void* scratch = nullptr;
  st = scratch_alloc(c, groups * 8 + 16, s, &scratch);
  if (st) return st;
  uint32_t* list = static_cast<uint32_t*>(scratch);
  uint32_t* rowoff = list + groups;
  uint32_t* entries = rowoff + groups;
  st = lossy_list_dev(c, present, groups, UGO_FEC_RECONSTRUCT_DATA_ONLY, list, entries, s, rowoff, count);
  if (!st && max_rows)
    st = reconstruct_list_dev(c, shards, present, list, entries, groups, S, L, out, out_row_stride, 0,
                              UGO_FEC_RECONSTRUCT_DATA_ONLY, nullptr, s, rowoff, index,
                              static_cast<uint32_t>(max_rows));
  const int fr = scratch_free(c, scratch, s);
  return st ? st : fr;
}

int ugo_fec_reconstruct(ugo_fec* c, uint8_t* shards, const uint64_t* present, size_t groups, size_t S,
                        size_t pitch, unsigned flags, int8_t* status, void* stream) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (pitch < S) return S == 0 ? UGO_FEC_ERR_SHARD_NO_DATA : UGO_FEC_ERR_INVALID_ARG;
  return ugo_fec_reconstruct_strided(c, shards, present, groups, S, pitch, size_t(c->n) * pitch, flags, status,
                                     stream);
}

int ugo_fec_reconstruct_rows(ugo_fec* c, const uint8_t* const* rows, const uint64_t* present, size_t groups,
                             size_t S, uint8_t* out, size_t out_row_stride, size_t out_group_stride, unsigned flags,
                             int8_t* status, void* stream) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (S == 0) return UGO_FEC_ERR_SHARD_NO_DATA;
  if (groups == 0) return UGO_FEC_OK;
  if (S > 0xffffffffu || c->n > 64 || !rows || !present || !out) return UGO_FEC_ERR_INVALID_ARG;
  // output slots per group: p, or with DATA_ONLY min(d, p) (at most that many data rows are erased)
  const size_t oslots = (flags & UGO_FEC_RECONSTRUCT_DATA_ONLY) ? size_t(std::min(c->d, c->p)) : size_t(c->p);
  if (reinterpret_cast<uintptr_t>(out) % 16 || out_row_stride % 16 || out_group_stride % 16 ||
      !layout_disjoint(S, out_row_stride, oslots, out_group_stride, groups))
    return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(rows) || !device_view(present) || !device_view(status) || !device_view(out))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int mode = c->d_table ? 1 : 2;
  ugo::kern::Batch a = base_batch(c, nullptr, S, Layout{0, 0});
  a.rows = reinterpret_cast<const uint64_t*>(rows);
  a.n = static_cast<uint32_t>(c->n);
  a.out = out;
  a.ogstride = out_group_stride;
  a.orstride = out_row_stride;
  a.present = present;
  a.status = status;
  a.data_only = (flags & UGO_FEC_RECONSTRUCT_DATA_ONLY) ? 1u : 0u;
  a.chunks = static_cast<uint32_t>((S + 15) / 16);
  size_t per = slice_groups(a.chunks, true);
  uint8_t* work = nullptr;
  if (mode == 2) {
    per = std::min<size_t>(per, 65536);
    const int st = scratch_alloc(c, std::min(per, groups) * c->desc_stride + 64, s, reinterpret_cast<void**>(&work));
    if (st) return st;
  }
  struct Release {
    ugo_fec* c;
    uint8_t* p;
    hipStream_t s;
    ~Release() { (void)scratch_free(c, p, s); }
  } release{c, work, s};
  for (size_t g0 = 0; g0 < groups; g0 += per) {
    const size_t gn = std::min(per, groups - g0);
    a.g0 = g0;
    a.items = static_cast<uint32_t>(gn * a.chunks);
    if (mode == 1) {
      a.desc = c->d_table;
    } else {
      ugo::kern::Prep pr{};
      pr.desc = work;
      pr.present = present;
      pr.M = c->d_M;
      pr.gf_exp = c->d_gf;
      pr.gf_log = c->d_gf + 512;
      pr.g0 = g0;
      pr.g_desc0 = g0;
      pr.nmask = a.nmask;
      pr.desc_stride = c->desc_stride;
      pr.d = static_cast<uint32_t>(c->d);
      pr.n = static_cast<uint32_t>(c->n);
      pr.dpad = c->dpad;
      pr.epad = c->epad;
      if (ugo::kern::launch_prepare(pr, static_cast<uint32_t>(gn), s) != hipSuccess) return UGO_FEC_ERR_HIP;
      a.desc = work;
      a.g_desc0 = g0;
    }
    if (ugo::kern::launch_apply_rows(mode, a, s) != hipSuccess) return UGO_FEC_ERR_HIP;
  }
  return UGO_FEC_OK;
}

int ugo_fec_device_address(const ugo_fec* c, const void* p, void** dev) {
  if (!c || !dev) return UGO_FEC_ERR_INVALID_ARG;
  *dev = nullptr;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  const uint8_t* q = static_cast<const uint8_t*>(p);
  if (!q || !device_view(q)) return UGO_FEC_ERR_INVALID_ARG;
  *dev = const_cast<uint8_t*>(q);
  return UGO_FEC_OK;
}

int ugo_fec_rc4_keystream(const uint8_t* key, size_t key_len, uint8_t* out, size_t n) {
  if (!key || key_len == 0 || key_len > 256 || (n && !out)) return UGO_FEC_ERR_INVALID_ARG;
  ugo::rc4_keystream(key, key_len, out, n);
  return UGO_FEC_OK;
}

int ugo_fec_timing_begin(ugo_fec* c, size_t max_launches) {
  if (c && c->poisoned) return UGO_FEC_ERR_HIP;
  if (!c || max_launches == 0 || max_launches > (size_t(1) << 20)) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  timer_release(c);
  ugo::kern::LaunchTimer& t = c->timer;
  t.ev = new (std::nothrow) hipEvent_t[2 * max_launches]();
  t.kid = new (std::nothrow) uint32_t[max_launches]();
  if (!t.ev || !t.kid) {
    timer_release(c);
    return UGO_FEC_ERR_INVALID_ARG;
  }
  t.cap = max_launches;
  for (size_t i = 0; i < 2 * max_launches; ++i)
    if (hipEventCreate(&t.ev[i]) != hipSuccess) {
      timer_release(c);
      return UGO_FEC_ERR_HIP;
    }
  c->timing = true;
  return UGO_FEC_OK;
}

int ugo_fec_timing_end(ugo_fec* c, ugo_fec_launch_time* out, size_t cap, size_t* n_out, size_t* n_untimed) {
  if (!c || (cap && !out)) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  ugo::kern::LaunchTimer& t = c->timer;
  int st = UGO_FEC_OK;
  size_t n = 0;
  for (size_t i = 0; i < t.used; ++i) {
    if (hipEventSynchronize(t.ev[2 * i + 1]) != hipSuccess) {
      st = UGO_FEC_ERR_HIP;
      break;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]) != hipSuccess) {
      st = UGO_FEC_ERR_HIP;
      break;
    }
    if (n < cap) out[n++] = ugo_fec_launch_time{t.kid[i], ms};
  }
  if (n_out) *n_out = n;
  if (n_untimed) *n_untimed = t.dropped;
  timer_release(c);
  return st;
}

// Fault injection for tests (ugo_fec_set_host_alloc_limit): pinned
// allocations larger than the limit fail, as on a host out of pinnable memory.
// An explicit call rather than an environment variable read on the allocation
// path (a stray variable in deployment would fail every allocation
// silently, and getenv races a concurrent setenv).
static std::atomic<unsigned long long> g_host_alloc_limit{0};

int ugo_fec_set_host_alloc_limit(size_t bytes) {
  g_host_alloc_limit.store(bytes, std::memory_order_relaxed);
  return UGO_FEC_OK;
}

int ugo_fec_host_alloc(size_t bytes, void** out) {
  if (!out) return UGO_FEC_ERR_INVALID_ARG;
  *out = nullptr;
  const unsigned long long lim = g_host_alloc_limit.load(std::memory_order_relaxed);
  if (lim && bytes > lim) return UGO_FEC_ERR_HIP;
  return hip_status(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
}

int ugo_fec_host_free(void* p) { return hip_status(hipHostFree(p)); }
}  // extern "C"
