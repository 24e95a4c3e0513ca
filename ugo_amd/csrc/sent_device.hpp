// sent_device.hpp -- device functions of the sent histories that more than one
// kernel file uses (sent_kernels.hip, loop_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ugo_sent.h"

namespace ugo {
namespace kern {

// getRTO of packet_sender.go: the delay cc handed in (0: the default), clamped
// to [minimum, maximum], backed off by consecutiveRTOCount, clamped again.
__device__ __forceinline__ unsigned long long sent_rto_us(unsigned long long delay_us, uint32_t rto_count) {
  unsigned long long rto = delay_us;
  if (rto == 0) rto = UGO_SENT_RTO_DEFAULT_US;
  if (rto > UGO_SENT_RTO_MAX_US) rto = UGO_SENT_RTO_MAX_US;
  if (rto < UGO_SENT_RTO_MIN_US) rto = UGO_SENT_RTO_MIN_US;
  const uint32_t sh = rto_count < 16u ? rto_count : 16u;
  rto <<= sh;
  if (rto > UGO_SENT_RTO_MAX_US) rto = UGO_SENT_RTO_MAX_US;
  return rto;
}

}  // namespace kern
}  // namespace ugo
