// cc_kernels.hip -- congestion control on gfx950 (include/ugo_cc.h): the RTT
// filter, hybrid slow start and CUBIC of a set of connections.
//   cubicSender      ugo/congestion/cubic_sender.go
//   Cubic            ugo/congestion/cubic.go
//   RTTStats         ugo/congestion/rtt_stats.go:83-114
//   HybridSlowStart  ugo/congestion/hybrid_slow_start.go
//
// ack  one lane per member: UpdateRTT, OnCongestionEvent, the outputs.
// rto  one lane per member: checkRTO's two calls where fired, and the budget.
//
// A lane loads its record, its event row and its cc row as 16-byte vectors and
// stores the record the same way; no LDS, no atomics.  The work of a lane does
// not grow with the number of packets a call acknowledges (grow() below).
//
// The float32 lines of the reference are kept as written: every product and
// sum is rounded on its own.  hipcc would contract a * b + c into one fused
// operation, so contraction is off for the whole file; the division is the
// correctly rounded one (no flag relaxes it).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cc_kernels.hpp"
#include "launch.hpp"

#pragma clang fp contract(off)

namespace ugo {
namespace kern {

namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

static_assert(sizeof(CcRecord) == 192 && sizeof(ugo_cc_row) == 32 && sizeof(ugo_sent_event) == 64 &&
                  sizeof(ugo_cc_params) == 20,
              "layouts");

constexpr u64 kCubeFactor = (1ull << 40) / 410ull;  // cubeFactor
constexpr i64 kMaxCubicIntervalUs = 30000;          // maxCubicTimeInterval
constexpr uint32_t kHystartLowWindow = 16, kHystartMinSamples = 8;
constexpr u64 kHystartMinThresholdUs = 4000, kHystartMaxThresholdUs = 16000;

template <typename T, int N>
union VecIO {
  T s;
  u64x2 v[N];
  __device__ VecIO() {}
};

template <typename T, int N>
__device__ __forceinline__ T load16(const T* p) {
  static_assert(sizeof(T) == 16 * N, "whole vectors");
  VecIO<T, N> io;
  const u64x2* src = reinterpret_cast<const u64x2*>(p);
#pragma unroll
  for (int i = 0; i < N; ++i) io.v[i] = src[i];
  return io.s;
}

template <typename T, int N>
__device__ __forceinline__ void store16(T* p, const T& s) {
  VecIO<T, N> io;
  io.s = s;
  u64x2* dst = reinterpret_cast<u64x2*>(p);
#pragma unroll
  for (int i = 0; i < N; ++i) dst[i] = io.v[i];
}

// ---------------------------------------------------------------- Cubic
__device__ __forceinline__ float cc_beta(uint32_t n) {
  const float fn = static_cast<float>(n);
  return ((fn - 1.0f) + 0.7f) / fn;
}

__device__ __forceinline__ float cc_alpha(uint32_t n) {
  const float b = cc_beta(n), fn = static_cast<float>(n);
  return (((3.0f * fn) * fn) * (1.0f - b)) / (1.0f + b);
}

// The largest t with t^3 <= x.
__device__ __forceinline__ uint32_t icbrt(u64 x) {
  u64 t = 0;
#pragma unroll
  for (int b = 21; b >= 0; --b) {
    const u64 cand = t | (1ull << b);
    if (cand <= 2642245ull && cand * cand * cand <= x) t = cand;  // 2642245^3 < 2^64 <= 2642246^3
  }
  return static_cast<uint32_t>(t);
}

__device__ __forceinline__ void cubic_reset(CcRecord& s) {
  s.epoch_us = s.app_limited_us = s.last_update_us = 0;
  s.last_cwnd = s.last_max_cwnd = s.est_tcp_cwnd = s.origin_cwnd = s.last_target_cwnd = 0;
  s.acked_count = s.time_to_origin = 0;
}

// Cubic.CongestionWindowAfterPacketLoss
__device__ __forceinline__ u64 cubic_after_loss(CcRecord& s, const ugo_cc_params& p) {
  if (s.cwnd < s.last_max_cwnd)
    s.last_max_cwnd = static_cast<u64>(0.85f * static_cast<float>(s.cwnd));
  else
    s.last_max_cwnd = s.cwnd;
  s.epoch_us = 0;
  return static_cast<u64>(static_cast<float>(s.cwnd) * cc_beta(p.num_connections));
}

// onPacketLost for a number above cutback.
__device__ __forceinline__ void loss_reaction(CcRecord& s, const ugo_cc_params& p, u64 last_sent) {
  s.last_cutback_exited_slowstart = s.cwnd < s.ssthresh;
  u64 w = cubic_after_loss(s, p);
  if (w < p.min_cwnd) w = p.min_cwnd;
  s.cwnd = w;
  s.ssthresh = w;
  s.cutback = last_sent;
  s.cutbacks += 1;
}

// Cubic.CongestionWindowAfterAck; early = the step took the 30-ms return and
// changed nothing but acked_count.
__device__ __forceinline__ u64 cubic_after_ack(CcRecord& s, float alpha, u64 now, bool& early) {
  s.acked_count += 1;
  early = s.last_cwnd == s.cwnd && s.last_update_us != 0 &&
          static_cast<i64>(now - s.last_update_us) <= kMaxCubicIntervalUs;
  if (early) return s.last_target_cwnd > s.est_tcp_cwnd ? s.last_target_cwnd : s.est_tcp_cwnd;
  s.last_cwnd = s.cwnd;
  s.last_update_us = now;
  if (s.epoch_us == 0) {
    s.epoch_us = now;
    s.acked_count = 1;
    s.est_tcp_cwnd = s.cwnd;
    if (s.last_max_cwnd <= s.cwnd) {
      s.time_to_origin = 0;
      s.origin_cwnd = s.cwnd;
    } else {
      s.time_to_origin = icbrt(kCubeFactor * (s.last_max_cwnd - s.cwnd));
      s.origin_cwnd = s.last_max_cwnd;
    }
  } else if (s.app_limited_us != 0) {
    s.epoch_us += now - s.app_limited_us;
    s.app_limited_us = 0;
  }
  // Go's int64 arithmetic: the products wrap, the shift is the signed one
  const i64 elapsed = static_cast<i64>(((now + s.min_rtt_us) - s.epoch_us) << 10) / 1000000;
  const u64 off = static_cast<u64>(static_cast<i64>(s.time_to_origin) - elapsed);
  const u64 delta = static_cast<u64>(static_cast<i64>(410ull * off * off * off) >> 40);
  u64 target = s.origin_cwnd - delta;
  for (;;) {  // at most about sqrt(2 alpha acked_count) rounds: each takes est / alpha of the count
    const uint32_t required = static_cast<uint32_t>(static_cast<float>(s.est_tcp_cwnd) / alpha);
    if (s.acked_count < required) break;
    s.acked_count -= required;
    s.est_tcp_cwnd += 1;
  }
  s.last_target_cwnd = target;
  if (target < s.est_tcp_cwnd) target = s.est_tcp_cwnd;
  return target;
}

// isCwndLimited
__device__ __forceinline__ bool cwnd_limited(u64 cwnd, u64 ssthresh, u64 bif, u64 mss) {
  const u64 w = cwnd * mss;
  if (bif >= w) return true;
  const bool slow_start_limited = cwnd < ssthresh && bif > w / 2;
  return slow_start_limited || w - bif <= 3 * mss;
}

// g times maybeIncreaseCwnd at one instant, in a number of rounds that does
// not depend on g.  cwnd_limited falls with cwnd, so the slow-start steps up
// to the first of ssthresh, max_cwnd and the first window that is not limited
// are one addition; a CUBIC step that took the 30-ms return and left cwnd as
// it was is what every later step does, so the rest only counts.
__device__ __forceinline__ void grow(CcRecord& s, const ugo_cc_params& p, u64 g, u64 bif, u64 now) {
  const u64 mss = p.mss;
  const float alpha = cc_alpha(p.num_connections);
  while (g != 0) {
    if (!cwnd_limited(s.cwnd, s.ssthresh, bif, mss)) {  // OnApplicationLimited, and so is every later step
      if (s.app_limited_us == 0) s.app_limited_us = now;
      return;
    }
    if (s.cwnd >= p.max_cwnd) return;
    if (s.cwnd < s.ssthresh) {
      // in slow start a window c is not limited iff c mss >= 2 bif and c mss > bif + 3 mss
      const u64 q = bif / mss, r = bif % mss;
      const u64 twice = bif >> 62 ? ~0ull : 2 * q + (2 * r + mss - 1) / mss;  // ceil(2 bif / mss)
      const u64 above = q > ~0ull - 4 ? ~0ull : q + 4;
      u64 stop = twice > above ? twice : above;  // > cwnd: cwnd is limited
      if (stop > s.ssthresh) stop = s.ssthresh;
      if (stop > p.max_cwnd) stop = p.max_cwnd;
      const u64 k = stop - s.cwnd < g ? stop - s.cwnd : g;
      s.cwnd += k;
      g -= k;
      continue;
    }
    const u64 before = s.cwnd;
    bool early;
    const u64 t = cubic_after_ack(s, alpha, now, early);
    s.cwnd = t < p.max_cwnd ? t : p.max_cwnd;
    g -= 1;
    if (early && s.cwnd == before) {
      s.acked_count += static_cast<uint32_t>(g);  // wraps as the reference's uint32 does
      return;
    }
  }
}

// ---------------------------------------------------------------- RTTStats, HybridSlowStart
__device__ __forceinline__ void update_rtt(CcRecord& s, u64 send_delta, u64 ack_delay) {
  if (s.min_rtt_us == 0 || s.min_rtt_us > send_delta) s.min_rtt_us = send_delta;
  u64 sample = send_delta;
  if (sample > ack_delay) sample -= ack_delay;
  s.latest_rtt_us = sample;
  if (s.srtt_us == 0) {
    s.srtt_us = sample;
    s.mean_dev_us = sample / 2;
  } else {
    const u64 dev = s.srtt_us > sample ? s.srtt_us - sample : sample - s.srtt_us;
    const float md = 0.75f * static_cast<float>(s.mean_dev_us), dv = 0.25f * static_cast<float>(dev);
    s.mean_dev_us = static_cast<u64>(md + dv);
    const float sm = static_cast<float>(s.srtt_us) * 0.875f, sa = static_cast<float>(sample) * 0.125f;
    s.srtt_us = static_cast<u64>(sm + sa);
  }
}

__device__ __forceinline__ bool should_exit_slow_start(CcRecord& s, u64 last_sent) {
  if (!s.started) {  // StartReceiveRound
    s.end_packet_number = last_sent;
    s.current_min_rtt_us = 0;
    s.sample_count = 0;
    s.started = 1;
  }
  if (s.found) return true;
  s.sample_count += 1;
  if (s.sample_count <= kHystartMinSamples &&
      (s.current_min_rtt_us == 0 || s.current_min_rtt_us > s.latest_rtt_us))
    s.current_min_rtt_us = s.latest_rtt_us;
  if (s.sample_count == kHystartMinSamples) {
    u64 thr = s.min_rtt_us >> 3;
    if (thr > kHystartMaxThresholdUs) thr = kHystartMaxThresholdUs;
    if (thr < kHystartMinThresholdUs) thr = kHystartMinThresholdUs;
    if (s.current_min_rtt_us > s.min_rtt_us + thr) s.found = 1;
  }
  return s.cwnd >= kHystartLowWindow && s.found;
}

// ---------------------------------------------------------------- the two calls
__global__ __launch_bounds__(256) void k_cc_ack(CcAckArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  CcRecord s = load16<CcRecord, 12>(a.recs + c);
  const SentRecord* sr = a.table[c].rec;
  if (sr->err) {  // inert
    a.delay_us[c] = 0;
    a.cutback[c] = s.cutback;
    return;
  }
  const ugo_sent_event ev = load16<ugo_sent_event, 4>(a.events + c);
  const u64 last_sent = sr->last_sent, lio = sr->lio;
  if (ev.accepted) {
    const ugo_cc_row row = load16<ugo_cc_row, 2>(a.rows + c);
    if (ev.has_rtt && ev.rtt_us > 0) update_rtt(s, ev.rtt_us, ev.delay_us);
    if (ev.has_rtt && s.cwnd < s.ssthresh && should_exit_slow_start(s, last_sent)) s.ssthresh = s.cwnd;
    bool cut = false;
    if (ev.lost_packets > 0 && row.max_lost > s.cutback) {
      loss_reaction(s, a.p, last_sent);
      cut = true;
    }
    const u64 acked = ev.acked_packets, prior = s.largest_acked;
    if (row.max_acked > prior) s.largest_acked = row.max_acked;
    u64 in_recovery = cut ? acked : (prior > s.cutback ? 0 : row.acked_le);
    if (in_recovery > acked) in_recovery = acked;  // a row that is not this event's: never more than all
    const u64 g = acked - in_recovery;
    grow(s, a.p, g, ev.bytes_in_flight, a.now_us);
    if (g != 0 && s.cwnd < s.ssthresh && row.max_acked > s.end_packet_number) s.started = 0;
  }
  s.rto_candidate = lio == last_sent ? 0 : lio + 1;
  a.delay_us[c] = s.srtt_us == 0 ? 0 : s.srtt_us + 4 * s.mean_dev_us;
  a.cutback[c] = s.cutback;
  store16<CcRecord, 12>(a.recs + c, s);
}

__global__ __launch_bounds__(256) void k_cc_rto(CcRtoArgs a) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.nconn) return;
  const SentRecord* sr = a.table[c].rec;
  if (sr->err) {  // inert
    a.budget[c] = 0;
    return;
  }
  CcRecord s = load16<CcRecord, 12>(a.recs + c);
  if (a.fired[c]) {
    if (s.rto_candidate != 0 && s.rto_candidate > s.cutback) loss_reaction(s, a.p, sr->last_sent);
    s.cutback = 0;  // OnRetransmissionTimeout(true)
    s.started = s.found = 0;
    cubic_reset(s);
    s.ssthresh = s.cwnd / 2;
    s.cwnd = a.p.min_cwnd;
    s.rtos += 1;
    a.cutback[c] = 0;
    store16<CcRecord, 12>(a.recs + c, s);
  }
  const u64 w = s.cwnd * a.p.mss, bif = sr->bytes_in_flight;
  u64 b = 0;
  if (bif <= w) {
    b = (w - bif) / a.packet_bytes + 1;
    if (b > a.max_budget) b = a.max_budget;
  }
  a.budget[c] = static_cast<uint32_t>(b);
}

}  // namespace

hipError_t launch_cc_ack(const CcAckArgs& a, hipStream_t s) {
  launch(kKCc, k_cc_ack, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cc_rto(const CcRtoArgs& a, hipStream_t s) {
  launch(kKCc, k_cc_rto, dim3((a.nconn + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
