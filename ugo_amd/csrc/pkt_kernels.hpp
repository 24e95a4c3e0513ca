// pkt_kernels.hpp -- internal interface of the packet wire codec (decoder and encoder).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/ugo_pkt.h"
#include "stream_tx_kernels.hpp"

namespace ugo {
namespace kern {

struct PktArgs {
  const uint8_t* pkts;     // packet i at pkts + i*slot (16-B aligned)
  const uint16_t* lens;
  const uint8_t* pad;      // nullable keystream, >= slot bytes
  ugo_pkt_info* info;
  uint64_t* ranges;        // [npk][max_ranges][2]
  ugo_pkt_segment* segs;   // [npk][max_segments]
  uint64_t npk;
  uint64_t slot;
  uint32_t max_ranges;
  uint32_t max_segments;
  uint32_t framed;
};

hipError_t launch_packet_decode(const PktArgs& a, hipStream_t s);

struct PktEncArgs {
  const ugo_pkt_info* info;
  const uint64_t* ranges;       // [npk][max_ranges][2]
  const ugo_pkt_segment* segs;  // [npk][max_segments]
  const uint8_t* payload;       // segment j's bytes at payload + i*payload_stride + data_off (any alignment)
  const uint8_t* pad;           // nullable keystream, >= slot bytes (null when framed)
  uint8_t* wire;                // packet i at wire + i*slot (16-B aligned)
  uint16_t* wire_lens;
  uint8_t* status;
  uint64_t npk;
  uint64_t slot;
  uint64_t payload_stride;
  uint32_t max_ranges;
  uint32_t max_segments;
  uint32_t framed;
};

hipError_t launch_packet_encode(const PktEncArgs& a, hipStream_t s);

// ugo_fec_stream_tx_set_encode: the segment bytes come from the send window of
// member conn_of[i] (payload and payload_stride are unused)
struct PktEncSetArgs : PktEncArgs {
  const uint32_t* conn_of;     // [npk]
  const StreamTxEntry* table;  // [nconn]
  uint32_t nconn;
};

hipError_t launch_packet_encode_set(const PktEncSetArgs& a, hipStream_t s);

}  // namespace kern
}  // namespace ugo
