// ugo_sent.cpp -- C ABI of the sent histories (include/ugo_sent.h), and the one
// call of include/ugo_cc.h that is a call on a set of them, ugo_fec_cc_sent_ack.
// Host-side control plane only: the argument rules are host/sent_args.hpp and
// host/cc_args.hpp, the kernels sent_kernels.hip.
#include "host/cc_args.hpp"
#include "host/set_call.hpp"

using namespace ugo::host;

namespace {
// What ugo_fec_sent_set_ack (split and rows null) and ugo_fec_cc_sent_ack do alike, each under its own rule.
template <class Rule>
int sent_ack_call(ugo_sent_tx_set* set, Rule rule, const ugo_pkt_info* info, const uint64_t* ranges,
                  size_t max_ranges, const uint32_t* conn_of, size_t npk, uint64_t now_us, ugo_sent_event* events,
                  const uint64_t* split, ugo_cc_row* rows, void* stream) {
  SetCall call(set, false, rule, stream, info, ranges, conn_of, events, split, rows);
  if (!call.go) return call.status;
  ugo::kern::SentAckArgs a{};
  a.table = set->table;
  a.call = set->call;
  a.chunk_member = set->chunk_member;
  a.chunk_sum = set->chunk_sum;
  a.info = info;
  a.ranges = ranges;
  a.conn_of = conn_of;
  a.events = events;
  a.cc_call = set->cc_call;
  a.split = reinterpret_cast<const unsigned long long*>(split);
  a.rows = rows;
  a.npk = npk;
  a.now_us = now_us;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.max_ranges = static_cast<uint32_t>(max_ranges);
  a.nchunks = static_cast<uint32_t>(set->nchunks);
  return hip_status(ugo::kern::launch_sent_ack(a, call.s));
}
}  // namespace

extern "C" {

int ugo_fec_sent_tx_create(ugo_fec* c, size_t window_packets, size_t seg_cap, ugo_sent_tx** out) {
  static_assert(sizeof(ugo_sent_state) == 160 && sizeof(ugo_sent_slot) == 32 && sizeof(ugo_sent_event) == 64,
                "the layouts ugo_sent.h states");
  static_assert(sizeof(ugo_sent_state) <= ugo::sentargs::kRecordRoom, "the record fits its share of the block");
  static_assert(UGO_FEC_KERNEL_SENT == ugo::kern::kKSent, "kernel class matches sent_kernels.hpp");
  if (out) *out = nullptr;
  if (!c || !out || !ugo::sentargs::window_ok(window_packets) || !ugo::sentargs::seg_cap_ok(seg_cap))
    return UGO_FEC_ERR_INVALID_ARG;
  if (c->poisoned) return UGO_FEC_ERR_HIP;
  DeviceGuard g(c->device);
  if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
  ugo_sent_tx* tx = new (std::nothrow) ugo_sent_tx();
  if (!tx) return UGO_FEC_ERR_HIP;
  tx->ctx = c;
  tx->m.ctx = c;
  tx->m.window_packets = window_packets;
  tx->m.seg_cap = seg_cap;
  const ugo::sentargs::Layout l = ugo::sentargs::layout(window_packets, seg_cap);
  ugo_sent_state init{};
  init.scan_from = 1;
  if (hipMalloc(&tx->m.block, l.bytes) != hipSuccess || hipMemset(tx->m.block, 0, l.bytes) != hipSuccess ||
      hipMemcpy(tx->m.block + l.rec, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {  // the fill ran on the null stream
    (void)hipGetLastError();
    ugo_fec_sent_tx_destroy(tx);
    return UGO_FEC_ERR_HIP;
  }
  *out = tx;
  return UGO_FEC_OK;
}

void ugo_fec_sent_tx_destroy(ugo_sent_tx* tx) {
  if (!tx) return;
  {
    DeviceGuard g(tx->ctx->device);
    (void)sync_sets(tx);
    (void)hipFree(tx->m.block);
  }
  delete tx;
}

int ugo_fec_sent_tx_slots(ugo_sent_tx* tx, ugo_sent_slot** slots_dev, size_t* window_packets) {
  if (!tx || !slots_dev || !window_packets) return UGO_FEC_ERR_INVALID_ARG;
  const ugo::sentargs::Layout l = ugo::sentargs::layout(tx->m.window_packets, tx->m.seg_cap);
  *slots_dev = reinterpret_cast<ugo_sent_slot*>(tx->m.block + l.slots);
  *window_packets = tx->m.window_packets;
  return UGO_FEC_OK;
}

int ugo_fec_sent_tx_segments(ugo_sent_tx* tx, ugo_stream_tx_rq_entry** segs_dev, size_t* window_packets,
                             size_t* seg_cap) {
  if (!tx || !segs_dev || !window_packets || !seg_cap) return UGO_FEC_ERR_INVALID_ARG;
  const ugo::sentargs::Layout l = ugo::sentargs::layout(tx->m.window_packets, tx->m.seg_cap);
  *segs_dev = reinterpret_cast<ugo_stream_tx_rq_entry*>(tx->m.block + l.segs);
  *window_packets = tx->m.window_packets;
  *seg_cap = tx->m.seg_cap;
  return UGO_FEC_OK;
}

int ugo_fec_sent_tx_scratch(ugo_sent_tx* tx, uint32_t** words_dev, size_t* n_words) {
  if (!tx || !words_dev || !n_words) return UGO_FEC_ERR_INVALID_ARG;
  const ugo::sentargs::Layout l = ugo::sentargs::layout(tx->m.window_packets, tx->m.seg_cap);
  *words_dev = reinterpret_cast<uint32_t*>(tx->m.block + l.diff);  // the claim ring follows the difference ring
  *n_words = 2 * tx->m.window_packets;
  return UGO_FEC_OK;
}

int ugo_fec_sent_set_create(ugo_fec* c, ugo_sent_tx* const* txs, size_t nconn, ugo_sent_tx_set** out) {
  if (out) *out = nullptr;
  if (!c || !txs || !out || nconn == 0 || nconn > ugo::kern::kSentSetMaxConn) return UGO_FEC_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::vector<const ugo::sentargs::Member*> ms(nconn);
    for (size_t i = 0; i < nconn; ++i) ms[i] = txs[i] ? &txs[i]->m : nullptr;
    if (!ugo::sentargs::members_ok(c, ms.data(), nconn)) return UGO_FEC_ERR_INVALID_ARG;
    if (c->poisoned) return UGO_FEC_ERR_HIP;
    std::vector<uint32_t> chunk_member;
    size_t min_seg_cap = 0;
    const std::vector<ugo::kern::SentEntry> host =
        ugo::sentargs::build_table(ms.data(), nconn, chunk_member, min_seg_cap);
    DeviceGuard g(c->device);
    if (!g.ok) return UGO_FEC_ERR_NO_DEVICE;
    ugo_sent_tx_set* set = new (std::nothrow) ugo_sent_tx_set();
    if (!set) return UGO_FEC_ERR_HIP;
    set->ctx = c;
    set->nchunks = chunk_member.size();
    set->min_seg_cap = min_seg_cap;
    const size_t nwords = ugo::kern::kSentScanBlock + 1;
    if (hipMalloc(&set->table, nconn * sizeof(host[0])) != hipSuccess ||
        hipMalloc(&set->gathered, nconn * sizeof(ugo_sent_state)) != hipSuccess ||
        hipMalloc(&set->call, nconn * sizeof(ugo::kern::SentCall)) != hipSuccess ||
        hipMalloc(&set->cc_call, nconn * sizeof(ugo::kern::SentCcCall)) != hipSuccess ||
        hipMalloc(&set->chunk_member, set->nchunks * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&set->chunk_sum, set->nchunks * sizeof(int2)) != hipSuccess ||
        hipMalloc(&set->start_local, nconn * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&set->words, nwords * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(set->call, 0, nconn * sizeof(ugo::kern::SentCall)) != hipSuccess ||
        hipMemset(set->cc_call, 0, nconn * sizeof(ugo::kern::SentCcCall)) != hipSuccess ||
        hipMemset(set->chunk_sum, 0, set->nchunks * sizeof(int2)) != hipSuccess ||
        hipMemset(set->start_local, 0, nconn * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(set->words, 0, nwords * sizeof(uint64_t)) != hipSuccess ||
        hipMemcpy(set->table, host.data(), nconn * sizeof(host[0]), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(set->chunk_member, chunk_member.data(), set->nchunks * sizeof(uint32_t), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
      (void)hipGetLastError();
      ugo_fec_sent_set_destroy(set);
      return UGO_FEC_ERR_HIP;
    }
    set_register(set, txs, nconn, ugo_fec_sent_set_destroy);
    *out = set;
    return UGO_FEC_OK;
  });
}

void ugo_fec_sent_set_destroy(ugo_sent_tx_set* set) {
  set_destroy(set, [set] {
    for (ugo_cc_set* cs : set->cc_sets) {  // they read the table: wait for them, then they are closed
      (void)cs->use.wait();
      cs->sent = nullptr;
    }
    (void)hipFree(set->table);
    (void)hipFree(set->gathered);
    (void)hipFree(set->call);
    (void)hipFree(set->cc_call);
    (void)hipFree(set->chunk_member);
    (void)hipFree(set->chunk_sum);
    (void)hipFree(set->start_local);
    (void)hipFree(set->words);
  });
}

int ugo_fec_sent_set_record(ugo_sent_tx_set* set, const ugo_pkt_info* info, const ugo_pkt_segment* segs,
                            size_t max_segments, const uint32_t* conn_of, const uint16_t* wire_lens,
                            const uint8_t* status, size_t npk, uint64_t now_us, void* stream) {
  const auto rule = [&] {
    return ugo::sentargs::record_ok(info, segs, max_segments, set->min_seg_cap, conn_of, wire_lens, status, npk);
  };
  SetCall call(set, npk == 0, rule, stream, info, segs, conn_of, wire_lens, status);
  if (!call.go) return call.status;
  ugo::kern::SentRecordArgs a{};
  a.table = set->table;
  a.call = set->call;
  a.info = info;
  a.segs = segs;
  a.conn_of = conn_of;
  a.wire_lens = wire_lens;
  a.status = status;
  a.npk = npk;
  a.now_us = now_us;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.max_segments = static_cast<uint32_t>(max_segments);
  return hip_status(ugo::kern::launch_sent_record(a, call.s));
}

int ugo_fec_sent_set_ack(ugo_sent_tx_set* set, const ugo_pkt_info* info, const uint64_t* ranges, size_t max_ranges,
                         const uint32_t* conn_of, size_t npk, uint64_t now_us, ugo_sent_event* events, void* stream) {
  const auto rule = [&] { return ugo::sentargs::ack_ok(info, ranges, max_ranges, conn_of, npk, events); };
  return sent_ack_call(set, rule, info, ranges, max_ranges, conn_of, npk, now_us, events, nullptr, nullptr, stream);
}

// include/ugo_cc.h, but a call on the set of sent histories: its handle logic is this family's
int ugo_fec_cc_sent_ack(ugo_sent_tx_set* set, const ugo_pkt_info* info, const uint64_t* ranges, size_t max_ranges,
                        const uint32_t* conn_of, size_t npk, uint64_t now_us, ugo_sent_event* events,
                        const uint64_t* split, ugo_cc_row* rows, void* stream) {
  const auto rule = [&] {
    return ugo::ccargs::sent_ack_ok(info, ranges, max_ranges, conn_of, npk, events, split, rows);
  };
  return sent_ack_call(set, rule, info, ranges, max_ranges, conn_of, npk, now_us, events, split, rows, stream);
}

int ugo_fec_sent_set_rto(ugo_sent_tx_set* set, const uint64_t* delay_us, uint64_t now_us, uint8_t* fired,
                         void* stream) {
  SetCall call(set, false, [&] { return ugo::sentargs::rto_ok(delay_us, fired); }, stream, delay_us, fired);
  if (!call.go) return call.status;
  ugo::kern::SentRtoArgs a{};
  a.table = set->table;
  a.delay_us = reinterpret_cast<const unsigned long long*>(delay_us);
  a.fired = fired;
  a.now_us = now_us;
  a.nconn = static_cast<uint32_t>(set->members.size());
  return hip_status(ugo::kern::launch_sent_rto(a, call.s));
}

int ugo_fec_sent_set_drain(ugo_sent_tx_set* set, size_t max_entries, uint32_t* conn_of, uint64_t* offset,
                           uint32_t* len, uint64_t* n_entries, uint8_t* touch, uint64_t* upto, void* stream) {
  const auto rule = [&] { return ugo::sentargs::drain_ok(max_entries, conn_of, offset, len, n_entries, touch, upto); };
  SetCall call(set, false, rule, stream, conn_of, offset, len, n_entries, touch, upto);
  if (!call.go) return call.status;
  ugo::kern::SentDrainArgs a{};
  a.table = set->table;
  a.call = set->call;
  a.chunk_member = set->chunk_member;
  a.chunk_sum = set->chunk_sum;
  a.start_local = set->start_local;
  a.block_start = set->words;
  a.n_written = reinterpret_cast<unsigned long long*>(set->words + ugo::kern::kSentScanBlock);
  a.conn_of = conn_of;
  a.offset = offset;
  a.len = len;
  a.n_entries = reinterpret_cast<unsigned long long*>(n_entries);
  a.touch = touch;
  a.upto = upto;
  a.max_entries = max_entries;
  a.nconn = static_cast<uint32_t>(set->members.size());
  a.nchunks = static_cast<uint32_t>(set->nchunks);
  return hip_status(ugo::kern::launch_sent_drain(a, call.s));
}

int ugo_fec_sent_set_attach(ugo_sent_tx_set* set, const uint64_t* first_packet, const uint32_t* n_packets,
                            size_t max_packets, ugo_pkt_info* info, uint8_t* attached, void* stream) {
  const auto rule = [&] { return ugo::sentargs::attach_ok(first_packet, n_packets, max_packets, info, attached); };
  SetCall call(set, false, rule, stream, first_packet, n_packets, info, attached);
  if (!call.go) return call.status;
  ugo::kern::SentAttachArgs a{};
  a.table = set->table;
  a.first_packet = reinterpret_cast<const unsigned long long*>(first_packet);
  a.n_packets = n_packets;
  a.info = info;
  a.attached = attached;
  a.max_packets = max_packets;
  a.nconn = static_cast<uint32_t>(set->members.size());
  return hip_status(ugo::kern::launch_sent_attach(a, call.s));
}

int ugo_fec_sent_set_state(ugo_sent_tx_set* set, ugo_sent_state* host_out) {
  return set_state(set, host_out, ugo::kern::launch_sent_gather);  // departs from SetCall: no poisoned test
}

}  // extern "C"
