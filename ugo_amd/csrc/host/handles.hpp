// handles.hpp -- the handle structs of the C ABI that cross family boundaries:
// the loop set reads four neighbours' tables, the controllers read the sent
// set's, and every set closes the loop sets that read it.  One header, so that
// each family's unit (ugo_stream_rx.cpp ... ugo_listen.cpp) sees complete types.
#pragma once
#include <algorithm>
#include <vector>

#include "../ack_kernels.hpp"
#include "../cc_kernels.hpp"
#include "../listen_kernels.hpp"
#include "../loop_kernels.hpp"
#include "../sent_kernels.hpp"
#include "../stream_kernels.hpp"
#include "../stream_set_kernels.hpp"
#include "../stream_tx_kernels.hpp"
#include "ack_args.hpp"
#include "context.hpp"
#include "sent_args.hpp"

namespace ugo {
namespace host __attribute__((visibility("hidden"))) {

// The stream a handle was last used on: what its destroy, its state call and
// the handles that share its device memory wait for.
struct StreamUse {
  hipStream_t last = nullptr;  // the stream of the last call on the handle
  bool used = false;
  hipStream_t record(void* stream) {
    last = static_cast<hipStream_t>(stream);
    used = true;
    return last;
  }
  hipError_t wait() const { return used ? hipStreamSynchronize(last) : hipSuccess; }
};

}  // namespace host
}  // namespace ugo

// ---------------------------------------------------------------- stream delivery (include/ugo_stream.h)
struct ugo_stream_rx {
  ugo_fec* ctx = nullptr;
  size_t cap = 0;
  uint8_t* win = nullptr;
  unsigned long long* bits = nullptr;  // C | S | claim | contested, cap / 64 words each
  ugo::kern::StreamRecord* rec = nullptr;
  ugo::host::StreamUse use;              // the last deliver / read
  std::vector<ugo_stream_rx_set*> sets;  // the live sets it is a member of: their calls are its calls
};

struct ugo_stream_rx_set {
  ugo_fec* ctx = nullptr;
  std::vector<ugo_loop_set*> loop_sets;  // the live loop sets that read its table
  std::vector<ugo_stream_rx*> members;
  ugo::kern::StreamSetEntry* table = nullptr;  // device, [nconn], uploaded once
  ugo_stream_rx_state* gathered = nullptr;     // device, [nconn], for ugo_fec_stream_set_state
  uint32_t wblocks = 1, rblocks = 1;           // per-connection grid sizes, from the largest member window
  ugo::host::StreamUse use;
};

// ---------------------------------------------------------------- send windows (include/ugo_stream.h)
struct ugo_stream_tx {
  ugo_fec* ctx = nullptr;
  size_t cap = 0, rq_cap = 0;
  uint8_t* win = nullptr;
  ugo_stream_tx_rq_entry* rq = nullptr;
  ugo::kern::StreamTxRecord* rec = nullptr;
  std::vector<ugo_stream_tx_set*> sets;  // the live sets it is a member of
};

struct ugo_stream_tx_set {
  ugo_fec* ctx = nullptr;
  std::vector<ugo_loop_set*> loop_sets;  // the live loop sets that read its table
  std::vector<ugo_stream_tx*> members;
  ugo::kern::StreamTxEntry* table = nullptr;         // device, [nconn], uploaded once
  ugo_stream_tx_state* gathered = nullptr;           // device, [nconn], for ugo_fec_stream_tx_set_state
  ugo::kern::StreamTxPlanScratch* scratch = nullptr; // device, [nconn]
  uint64_t* words = nullptr;  // device: block_budget | block_first (kTxScanBlock each) | first_dense [nconn] | unsorted
  uint32_t wblocks = 1;       // write's blocks per connection, from the largest member window
  ugo::host::StreamUse use;
};

// ---------------------------------------------------------------- receive histories (include/ugo_ack.h)
struct ugo_ack_rx {
  ugo::ackargs::Member m{};             // ctx, bitmap, record, window: what a set's table is built from
  ugo_fec* ctx = nullptr;
  std::vector<ugo_ack_rx_set*> sets;    // the live sets it is a member of
};

struct ugo_ack_rx_set {
  ugo_fec* ctx = nullptr;
  std::vector<ugo_loop_set*> loop_sets;  // the live loop sets that read its table
  std::vector<ugo_ack_rx*> members;
  ugo::kern::AckEntry* table = nullptr;  // device, [nconn], uploaded once
  ugo_ack_state* gathered = nullptr;     // device, [nconn], for ugo_fec_ack_set_state
  ugo::kern::AckCall* call = nullptr;    // device, [nconn], zero between receive calls
  uint32_t* slot_local = nullptr;        // device, [nconn]
  uint64_t* words = nullptr;             // device: block_slots [kAckScanBlock] | total_in
  ugo::host::StreamUse use;
};

// ---------------------------------------------------------------- sent histories (include/ugo_sent.h)
struct ugo_sent_tx {
  ugo::sentargs::Member m{};             // ctx, device block, window, seg_cap: what a set's table is built from
  ugo_fec* ctx = nullptr;
  std::vector<ugo_sent_tx_set*> sets;    // the live sets it is a member of
};

struct ugo_sent_tx_set {
  ugo_fec* ctx = nullptr;
  std::vector<ugo_loop_set*> loop_sets;  // the live loop sets that read its table
  std::vector<ugo_sent_tx*> members;
  ugo::kern::SentEntry* table = nullptr;  // device, [nconn], uploaded once
  ugo_sent_state* gathered = nullptr;     // device, [nconn], for ugo_fec_sent_set_state
  ugo::kern::SentCall* call = nullptr;    // device, [nconn], zero between calls
  ugo::kern::SentCcCall* cc_call = nullptr;  // device, [nconn], zero between calls (ugo_fec_cc_sent_ack)
  std::vector<ugo_cc_set*> cc_sets;       // the live controller sets that read its table
  uint32_t* chunk_member = nullptr;       // device, [nchunks], uploaded once
  int2* chunk_sum = nullptr;              // device, [nchunks]
  uint32_t* start_local = nullptr;        // device, [nconn]
  uint64_t* words = nullptr;              // device: block_start [kSentScanBlock] | n_written
  size_t nchunks = 0;
  size_t min_seg_cap = 0;
  ugo::host::StreamUse use;
};

// A set of congestion controllers (include/ugo_cc.h), one per member of a set of sent histories.
struct ugo_cc_set {
  ugo_fec* ctx = nullptr;
  ugo_sent_tx_set* sent = nullptr;        // null once the sent set is gone: every call is then an argument error
  ugo::kern::CcRecord* recs = nullptr;    // device, [nconn]
  unsigned long long* cutback = nullptr;  // device, [nconn]
  ugo_cc_params params{};
  size_t nconn = 0;
  ugo::host::StreamUse use;
};

// The connection loop of a set (include/ugo_loop.h): one record per member of four neighbouring sets.
struct ugo_loop_set {
  ugo_fec* ctx = nullptr;
  ugo_stream_rx_set* stream_rx = nullptr;  // all four null once one of them is gone: every call is then an
  ugo_ack_rx_set* ack_rx = nullptr;        // argument error
  ugo_stream_tx_set* stream_tx = nullptr;
  ugo_sent_tx_set* sent_tx = nullptr;
  ugo::kern::LoopTables t{};   // recs, call, block_a, block_b and words are the set's own
  ugo::host::StreamUse use;
};

// The connection table (include/ugo_listen.h).
struct ugo_listen_table {
  ugo_fec* ctx = nullptr;
  ugo::kern::ListenTable t{};  // every array of it is the table's own
  ugo::host::StreamUse use;
};

namespace ugo {
namespace host __attribute__((visibility("hidden"))) {

// A handle a per-call entry point may use: not NULL and, for the two that read
// a neighbour's tables, not closed by that neighbour's destroy.
template <class H>
bool is_open(const H* h) { return h != nullptr; }
inline bool is_open(const ugo_cc_set* set) { return set && set->sent; }
inline bool is_open(const ugo_loop_set* set) { return set && set->sent_tx; }

// Takes the loop set out of its four neighbours' lists; its calls are argument errors from then on.
inline void loop_set_detach(ugo_loop_set* set) {
  auto forget = [set](std::vector<ugo_loop_set*>& sets) {
    sets.erase(std::remove(sets.begin(), sets.end(), set), sets.end());
  };
  if (set->stream_rx) forget(set->stream_rx->loop_sets);
  if (set->ack_rx) forget(set->ack_rx->loop_sets);
  if (set->stream_tx) forget(set->stream_tx->loop_sets);
  if (set->sent_tx) forget(set->sent_tx->loop_sets);
  set->stream_rx = nullptr;
  set->ack_rx = nullptr;
  set->stream_tx = nullptr;
  set->sent_tx = nullptr;
}

// A neighbouring set goes: wait for the loop sets that read its table, then they are closed.
inline void loop_sets_close(const std::vector<ugo_loop_set*>& sets) {
  const std::vector<ugo_loop_set*> copy = sets;  // detach edits the list
  for (ugo_loop_set* ls : copy) {
    (void)ls->use.wait();
    loop_set_detach(ls);
  }
}

}  // namespace host
}  // namespace ugo
