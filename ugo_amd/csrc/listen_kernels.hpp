// listen_kernels.hpp -- internal interface of the connection table
// (ugo_fec_listen_*, include/ugo_listen.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/ugo_listen.h"

namespace ugo {
namespace kern {

constexpr uint32_t kKListen = 15;  // UGO_FEC_KERNEL_LISTEN

constexpr uint32_t kListenEmpty = 0xffffffffu;  // a slot's member word and claim word; a member's slot word
constexpr uint32_t kListenDead = 0xfffffffeu;   // a slot's member word, deviation (b)
constexpr uint32_t kListenScanBlocks = 1024;    // the blocks of the numbering scan, whatever npackets

// One slot of the open-addressing table (32 bytes): THE KEY, the member, and
// the batch index of the ACCEPT or REFUSED packet of the call that last
// claimed the slot.
struct ListenSlot {
  uint32_t ip[4];
  uint32_t scope;
  uint32_t port;
  uint32_t member;  // kListenEmpty, kListenDead or the member
  uint32_t first;
};

// What a call hands from one kernel to the next.
struct ListenCall {
  uint32_t base;  // route: nconn before the call
  uint32_t bad;   // remap: the status bits
};

// The device side of a table; every array is allocated by create.
struct ListenTable {
  ListenSlot* slots;      // [n_slots]
  uint32_t* claim;        // [n_slots], kListenEmpty between calls
  uint8_t* names;         // [max_conn] rows of 32 bytes
  uint32_t* member_slot;  // [max_conn], kListenEmpty: no entry
  uint8_t* tmp_names;     // [max_conn] rows, remap
  uint32_t* mark;         // [max_conn], zero between calls, remap
  uint32_t* block_count;  // [kListenScanBlocks]
  ugo_listen_state* st;
  ListenCall* call;
  uint32_t n_slots;
  uint32_t max_conn;
};

struct ListenRouteArgs {
  ListenTable t;
  const uint8_t* names;
  const uint8_t* pkts;
  const uint16_t* lens;
  uint32_t* conn_of;
  uint8_t* cls;
  ugo_listen_accept* accepted;
  uint32_t* n_accepted;
  uint32_t slot;
  uint32_t npackets;
  uint32_t max_accepted;
};
hipError_t launch_listen_route(const ListenRouteArgs& a, hipStream_t s);

struct ListenRemapArgs {
  ListenTable t;
  const uint32_t* new_index;
  uint32_t* status;
  uint32_t n_index;
  uint32_t nconn_new;  // clamped to max_conn + 1 by the caller
};
hipError_t launch_listen_remap(const ListenRemapArgs& a, hipStream_t s);

struct ListenNamesArgs {
  ListenTable t;
  const uint32_t* conn_of;
  uint8_t* names_out;
  uint32_t* name_lens;
  uint32_t npackets;
};
hipError_t launch_listen_names(const ListenNamesArgs& a, hipStream_t s);

hipError_t launch_listen_entries(const ListenTable& t, ugo_listen_entry* out, uint32_t cap, hipStream_t s);

// Empties a new table: slots, claims, member slots, marks and the record.
hipError_t launch_listen_init(const ListenTable& t, hipStream_t s);

}  // namespace kern
}  // namespace ugo
