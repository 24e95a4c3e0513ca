// ugo_pkt.cpp -- C ABI of RX / TX assembly (include/ugo_fec.h) and of the
// packet codec (include/ugo_pkt.h).  Host-side control plane only; the kernels
// are in rx_kernels.hip, tx_kernels.hip and pkt_kernels.hip.
#include <algorithm>

#include "host/fec_core.hpp"
#include "pkt_kernels.hpp"
#include "rx_kernels.hpp"
#include "tx_kernels.hpp"

namespace ugo {
namespace host __attribute__((visibility("hidden"))) {

// Bytes a placed row is written to.  The public calls write a frame row in
// [0, round_up(S + 6, 16)) and nowhere else (include/ugo_fec.h), whatever the
// alignment of the base and the strides: a caller may own no byte past that,
// inside a wider pitch or behind the batch's last row.  own_lines: the caller
// is the engine itself, the rows are its own scratch on 64-B aligned slots that
// span round_up(S + 6, 64), and it asks for whole 64-B lines -- a row then ends
// on a whole line instead of leaving its last one partially written (which the
// neighbouring row's writer completes at another time).  Requested, never
// inferred from pointer arithmetic: aligned, disjoint slots do not prove that
// the bytes behind a row are the caller's.
size_t rx_row_fill(size_t S, bool frame, bool own_lines) {
  return round_up(frame ? S + 6 : S, frame && own_lines ? 64 : 16);
}

// Stream-ordered scratch of one rx_assemble call: presence snapshot [groups] u64 | claim words
// [groups][n] u32 | dup flag.
size_t rx_scratch_bytes(const ugo_fec* c, size_t groups) {
  return groups * sizeof(uint64_t) + (groups * size_t(c->n) + 16) * sizeof(uint32_t);
}

// rx_assemble on device views (arguments checked by the caller).
int rx_assemble_dev(ugo_fec* c, const uint8_t* wire, size_t slot_stride, const uint16_t* lens, size_t npk,
                    const uint8_t* pad, uint64_t first_group, size_t groups, uint8_t* shards, size_t S,
                    size_t row_stride, size_t group_stride, uint64_t* present, uint32_t* stats, hipStream_t s,
                    bool frame, void* call_scratch, bool own_lines) {
  ugo::kern::RxArgs a{};
  a.frame = frame ? 1u : 0u;
  // the frame kernels' pass count follows this (launch_rx_scatter)
  a.fill = static_cast<uint32_t>(rx_row_fill(S, frame, own_lines));
  a.wire = wire;
  a.lens = lens;
  a.pad = pad;
  a.shards = shards;
  a.present = present;
  a.stats = stats;
  a.npk = npk;
  a.slot = slot_stride;
  a.first_group = first_group;
  a.groups = groups;
  a.rstride = row_stride;
  a.gstride = group_stride;
  a.S = static_cast<uint32_t>(S);
  a.n = static_cast<uint32_t>(c->n);
  // First arrival in ring order wins (ugo/fec.go:123-129), optimistically
  // (rx_kernels.hip): place everything, flag a (group, row) taken twice, and
  // only then -- gated on the flag, on the device -- claim and re-place.
  // scratch: presence snapshot [groups] u64 | claim words [groups][n] u32 | dup flag
  const uint64_t words = groups * uint64_t(c->n);
  // call_scratch: the caller's (rx_recover_host: one block for all its chunk calls, which run in order on s),
  // rx_scratch_bytes(c, groups) of it
  void* scratch = call_scratch;
  int st = call_scratch ? UGO_FEC_OK : scratch_alloc(c, rx_scratch_bytes(c, groups), s, &scratch);
  if (st) return st;
  uint64_t* prev = static_cast<uint64_t*>(scratch);
  uint32_t* win = reinterpret_cast<uint32_t*>(prev + groups);
  uint32_t* dup = win + words;
  // call entry, one launch: dup = 0, the presence snapshot -- a (group, row)
  // an earlier call placed keeps that call's copy (ugo/fec.go:123-129 keeps the
  // first) -- the claim words, and whether any presence bit was set at all (if
  // none was, the place pass skips its per-packet snapshot lookups)
  const unsigned long long call = ++c->rx_calls;
  st = hip_status(ugo::kern::launch_rx_begin(present, prev, groups, dup, win, words, c->d_rxseen, call, s));
  a.dup = dup;
  a.prev = prev;
  a.seen = c->d_rxseen;
  a.call = call;
  ugo::kern::RxArgs f = a;  // the gated claim and re-place of the first copies
  f.win = win;
  f.gate = dup;
  f.dup = nullptr;
  f.stats = nullptr;
  f.fixup = 1;
  if (!st) st = hip_status(ugo::kern::launch_rx_scatter(a, s));
  if (!st) st = hip_status(ugo::kern::launch_rx_claim(f, s));
  if (!st) st = hip_status(ugo::kern::launch_rx_scatter(f, s));
  const int fr = call_scratch ? UGO_FEC_OK : scratch_free(c, scratch, s);
  return st ? st : fr;
}

// ugo_fec_rx_assemble / _frames: argument checks, device views, launch.  A
// frame row spans S + 6 bytes (the packet's header columns, then the payload).
int rx_assemble_abi(ugo_fec* c, const uint8_t* wire, size_t slot_stride, const uint16_t* lens, size_t npk,
                    const uint8_t* pad, uint64_t first_group, size_t groups, uint8_t* shards, size_t S,
                    size_t row_stride, size_t group_stride, uint64_t* present, uint32_t* stats, void* stream,
                    bool frame) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (S == 0) return UGO_FEC_ERR_SHARD_NO_DATA;
  if (npk == 0) return UGO_FEC_OK;
  if (!wire || !lens || !shards || !present || groups == 0 || c->n > 64 || npk >= 0xffffffffull)
    return UGO_FEC_ERR_INVALID_ARG;
  if (slot_stride % 16 || slot_stride < 16 || reinterpret_cast<uintptr_t>(wire) % 16 ||
      reinterpret_cast<uintptr_t>(shards) % 16 || row_stride % 16 || group_stride % 16 ||
      (pad && reinterpret_cast<uintptr_t>(pad) % 16) || S > 0xffffffffu - 22)
    return UGO_FEC_ERR_INVALID_ARG;
  const size_t span = frame ? S + 6 : S;
  if (!layout_disjoint(span, row_stride, size_t(c->n), group_stride, groups)) return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(wire) || !device_view(lens) || !device_view(pad) || !device_view(shards) ||
      !device_view(present) || !device_view(stats))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  return rx_assemble_dev(c, wire, slot_stride, lens, npk, pad, first_group, groups, shards, S, row_stride,
                         group_stride, present, stats, static_cast<hipStream_t>(stream), frame);
}
}  // namespace host
}  // namespace ugo

using namespace ugo::host;

extern "C" {

int ugo_fec_rx_assemble(ugo_fec* c, const uint8_t* wire, size_t slot_stride, const uint16_t* lens, size_t npk,
                        const uint8_t* pad, uint64_t first_group, size_t groups, uint8_t* shards, size_t S,
                        size_t row_stride, size_t group_stride, uint64_t* present, uint32_t* stats,
                        void* stream) {
  return rx_assemble_abi(c, wire, slot_stride, lens, npk, pad, first_group, groups, shards, S, row_stride,
                         group_stride, present, stats, stream, false);
}

int ugo_fec_rx_assemble_frames(ugo_fec* c, const uint8_t* wire, size_t slot_stride, const uint16_t* lens,
                               size_t npk, const uint8_t* pad, uint64_t first_group, size_t groups, uint8_t* shards,
                               size_t S, size_t row_stride, size_t group_stride, uint64_t* present, uint32_t* stats,
                               void* stream) {
  return rx_assemble_abi(c, wire, slot_stride, lens, npk, pad, first_group, groups, shards, S, row_stride,
                         group_stride, present, stats, stream, true);
}

int ugo_fec_tx_assemble(ugo_fec* c, const uint8_t* pkts, size_t slot_in, const uint16_t* lens, size_t groups,
                        uint32_t first_seq, const uint8_t* pad, size_t max_len, uint8_t* wire, size_t slot_out,
                        uint16_t* wire_lens, int8_t* status, void* stream) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (groups == 0) return UGO_FEC_OK;
  const uint64_t n = static_cast<uint64_t>(c->n);
  const uint32_t paws = static_cast<uint32_t>((0xffffffffull / n - 1) * n);  // ugo/fec.go:58
  const size_t need = round_up(max_len, 16);
  if (!pkts || !lens || !wire || !wire_lens || c->d > 32 || max_len < 6 || max_len > 0xffff ||
      slot_in % 16 || slot_out % 16 || slot_in < need || slot_out < need ||
      reinterpret_cast<uintptr_t>(pkts) % 16 || reinterpret_cast<uintptr_t>(wire) % 16 ||
      (pad && reinterpret_cast<uintptr_t>(pad) % 16) || first_seq % n || first_seq >= paws)
    return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(pkts) || !device_view(lens) || !device_view(pad) || !device_view(wire) ||
      !device_view(wire_lens) || !device_view(status))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  ugo::kern::TxArgs a{};
  a.pkts = pkts;
  a.lens = lens;
  a.pad = pad;
  a.desc = c->d_encdesc;
  a.wire = wire;
  a.wire_lens = wire_lens;
  a.status = status;
  a.slot_in = slot_in;
  a.slot_out = slot_out;
  a.first_seq = first_seq;
  a.paws = paws;
  a.max_len = static_cast<uint32_t>(max_len);
  a.chunks = static_cast<uint32_t>(need / 16);
  a.d = static_cast<uint32_t>(c->d);
  a.p = static_cast<uint32_t>(c->p);
  a.dpad = c->dpad;
  a.epad = c->epad;
  const int dmax = ugo::kern::has_const_encode(c->d, c->p) ? 0 : ugo::kern::apply_dmax(c->d);
  const uint64_t per_launch = (1ull << 31) / a.chunks;  // items of one launch fit 32 bits
  for (uint64_t g0 = 0; g0 < groups; g0 += per_launch) {
    a.g0 = g0;
    a.groups = std::min<uint64_t>(per_launch, groups - g0);
    const int st = hip_status(ugo::kern::launch_tx_assemble(dmax, a, static_cast<hipStream_t>(stream)));
    if (st != UGO_FEC_OK) return st;
  }
  return UGO_FEC_OK;
}

int ugo_fec_packet_decode(ugo_fec* c, const uint8_t* pkts, size_t slot, const uint16_t* lens, size_t npk,
                          const uint8_t* pad, unsigned flags, ugo_pkt_info* info, uint64_t* ranges,
                          size_t max_ranges, ugo_pkt_segment* segs, size_t max_segments, void* stream) {
  static_assert(sizeof(ugo_pkt_info) == 64, "ugo_pkt_info is 64 bytes");
  static_assert(sizeof(ugo_pkt_segment) == 16, "ugo_pkt_segment is 16 bytes");
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;  // a service block that never left (svc_retire)
  if (npk == 0) return UGO_FEC_OK;
  if (!pkts || !lens || !info || slot % 16 || slot == 0 || slot > 0xffff ||
      reinterpret_cast<uintptr_t>(pkts) % 16 || (pad && reinterpret_cast<uintptr_t>(pad) % 16) ||
      (max_ranges && !ranges) || (max_segments && !segs) || max_ranges > 0xffff || max_segments > 0xffff ||
      (flags & ~UGO_PKT_FEC_FRAMED))
    return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(pkts) || !device_view(lens) || !device_view(pad) || !device_view(info) ||
      !device_view(ranges) || !device_view(segs))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  ugo::kern::PktArgs a{};
  a.pkts = pkts;
  a.lens = lens;
  a.pad = pad;
  a.info = info;
  a.ranges = ranges;
  a.segs = segs;
  a.npk = npk;
  a.slot = slot;
  a.max_ranges = static_cast<uint32_t>(max_ranges);
  a.max_segments = static_cast<uint32_t>(max_segments);
  a.framed = flags & UGO_PKT_FEC_FRAMED;
  return hip_status(ugo::kern::launch_packet_decode(a, static_cast<hipStream_t>(stream)));
}

int ugo_fec_packet_encode(ugo_fec* c, const ugo_pkt_info* info, const uint64_t* ranges, size_t max_ranges,
                          const ugo_pkt_segment* segs, size_t max_segments, const uint8_t* payload,
                          size_t payload_stride, size_t npk, const uint8_t* pad, unsigned flags, uint8_t* wire,
                          size_t slot, uint16_t* wire_lens, uint8_t* status, void* stream) {
  if (!c) return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  if (npk == 0) return UGO_FEC_OK;
  if (!info || !wire || !wire_lens || !status || slot % 16 || slot == 0 || slot > 0xffff ||
      reinterpret_cast<uintptr_t>(wire) % 16 || (pad && reinterpret_cast<uintptr_t>(pad) % 16) ||
      (max_ranges && !ranges) || (max_segments && (!segs || !payload)) || max_ranges > 0xffff ||
      max_segments > 0xffff || (flags & ~UGO_PKT_FEC_FRAMED) || ((flags & UGO_PKT_FEC_FRAMED) && pad))
    return UGO_FEC_ERR_INVALID_ARG;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  if (!device_view(info) || !device_view(ranges) || !device_view(segs) || !device_view(payload) ||
      !device_view(pad) || !device_view(wire) || !device_view(wire_lens) || !device_view(status))
    return UGO_FEC_ERR_INVALID_ARG;
  TimerScope ts(c);
  ugo::kern::PktEncArgs a{};
  a.info = info;
  a.ranges = ranges;
  a.segs = segs;
  a.payload = payload;
  a.pad = pad;
  a.wire = wire;
  a.wire_lens = wire_lens;
  a.status = status;
  a.npk = npk;
  a.slot = slot;
  a.payload_stride = payload_stride;
  a.max_ranges = static_cast<uint32_t>(max_ranges);
  a.max_segments = static_cast<uint32_t>(max_segments);
  a.framed = flags & UGO_PKT_FEC_FRAMED;
  return hip_status(ugo::kern::launch_packet_encode(a, static_cast<hipStream_t>(stream)));
}
}  // extern "C"
