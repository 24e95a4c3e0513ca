// cc_kernels.hpp -- internal interface of the congestion controllers of a set
// (ugo_fec_cc_set_*, include/ugo_cc.h).  ugo_fec_cc_sent_ack is the cc form of
// launch_sent_ack (sent_kernels.hpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/ugo_cc.h"
#include "sent_kernels.hpp"

namespace ugo {
namespace kern {

// The device form of a controller's record is the public struct; the records
// of a set are one dense array, 16-B aligned.
typedef ugo_cc_state CcRecord;

struct CcAckArgs {
  const SentEntry* table;          // the sent set's: the members' sent records
  CcRecord* recs;                  // [nconn]
  unsigned long long* cutback;     // [nconn], the dense copy of recs[c].cutback
  const ugo_sent_event* events;    // [nconn]
  const ugo_cc_row* rows;          // [nconn]
  unsigned long long* delay_us;    // [nconn], out
  uint64_t now_us;
  ugo_cc_params p;
  uint32_t nconn;
};
hipError_t launch_cc_ack(const CcAckArgs& a, hipStream_t s);

struct CcRtoArgs {
  const SentEntry* table;
  CcRecord* recs;
  unsigned long long* cutback;
  const uint8_t* fired;            // [nconn]
  uint32_t* budget;                // [nconn], out
  uint64_t packet_bytes;
  uint64_t max_budget;
  ugo_cc_params p;
  uint32_t nconn;
};
hipError_t launch_cc_rto(const CcRtoArgs& a, hipStream_t s);

}  // namespace kern
}  // namespace ugo
