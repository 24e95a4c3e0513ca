// fec_core.hpp -- what the three units behind include/ugo_fec.h and ugo_pkt.h
// use of each other: ugo_fec.cpp (context and the device-memory calls),
// ugo_fec_host.cpp (the per-call service and the host-memory paths) and
// ugo_pkt.cpp (RX/TX assembly and the packet codec).  Each function's comment is
// at its definition.
#pragma once
#include "context.hpp"

namespace ugo {
namespace host __attribute__((visibility("hidden"))) {

struct Layout {
  uint64_t rstride;  // bytes between rows of one group
  uint64_t gstride;  // bytes between groups
};

// Separate output batch of a reconstruct (ugo_fec_reconstruct_into); none = in place.
struct OutBatch {
  uint8_t* base = nullptr;
  Layout L{0, 0};
};

// ugo_fec.cpp
size_t mask_words(const ugo_fec* c);
Layout interleaved(const ugo_fec* c, size_t pitch);
ugo::kern::Batch base_batch(const ugo_fec* c, uint8_t* shards, size_t S, const Layout& L);
bool layout_disjoint(size_t S, size_t rstride, size_t rows, size_t gstride, size_t groups);
int check_batch(const ugo_fec* c, const void* shards, size_t groups, size_t S, const Layout& L);
int encode_dev(ugo_fec* c, uint8_t* shards, size_t groups, size_t S, const Layout& L, hipStream_t s);
int scratch_alloc(ugo_fec* c, size_t bytes, hipStream_t s, void** out);
int scratch_free(ugo_fec* c, void* ptr, hipStream_t s);
int reconstruct_dev(ugo_fec* c, uint8_t* shards, const uint64_t* present, size_t groups, size_t S,
                    const Layout& L, unsigned flags, int8_t* status, hipStream_t s, const OutBatch& O = {},
                    const uint64_t* host_present = nullptr);
int lossy_list_dev(ugo_fec* c, const uint64_t* present, size_t groups, unsigned flags, uint32_t* list,
                   uint32_t* count, hipStream_t s, uint32_t* rowoff = nullptr, uint32_t* rows = nullptr);
int reconstruct_list_dev(ugo_fec* c, const uint8_t* shards, const uint64_t* present, const uint32_t* list,
                         const uint32_t* count, size_t max_entries, size_t S, const Layout& L, uint8_t* out,
                         size_t out_row_stride, size_t out_entry_stride, unsigned flags, int8_t* status,
                         hipStream_t s, const uint32_t* rowoff = nullptr, uint32_t* rowid = nullptr,
                         uint32_t max_rows = 0xffffffffu);

// ugo_fec_host.cpp
int svc_stop(ugo_fec* c);
bool is_shared_stream(const ugo_fec* c, int i);

// ugo_pkt.cpp
size_t rx_scratch_bytes(const ugo_fec* c, size_t groups);
int rx_assemble_dev(ugo_fec* c, const uint8_t* wire, size_t slot_stride, const uint16_t* lens, size_t npk,
                    const uint8_t* pad, uint64_t first_group, size_t groups, uint8_t* shards, size_t S,
                    size_t row_stride, size_t group_stride, uint64_t* present, uint32_t* stats, hipStream_t s,
                    bool frame = false, void* call_scratch = nullptr, bool own_lines = false);

}  // namespace host
}  // namespace ugo
