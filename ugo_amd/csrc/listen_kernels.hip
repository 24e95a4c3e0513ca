// listen_kernels.hip -- the connection table on gfx950 (include/ugo_listen.h):
// listener.handlePacket (ugo/listener.go:64-119) for a whole ring per call.
//
// The table is open addressing with linear probing over 32-byte slots; a
// slot's member word is empty, dead or the member.  Beside the slots lies one
// claim word per slot, empty between calls.
//
// route, one lane per packet, four kernels:
//   claim   the INITs of keys the slots do not hold as a member claim a slot:
//           a compare-and-swap of the claim word from empty to the lane's batch
//           index.  A lane that finds another index there reads that packet's
//           name from the input array (read-only, so visible) and on equality
//           does an atomic min with its own index, otherwise probes on.  After
//           the kernel a claim word holds f of THE RULE.  The lane's slot goes
//           into conn_of[i], the call's scratch.
//   count   a lane whose slot's claim is its own index is its key's f.  The
//           batch is cut into at most 1,024 contiguous pieces, one block each;
//           a block counts the f of its piece.
//   number  the same pieces: the counts before a block's own give its first
//           rank, ballots give the ranks inside it.  f of rank r becomes member
//           base + r: its lane writes the slot, the name row, the accepted row,
//           and empties the claim word.  Past max_conn the slot becomes dead.
//   route   every packet looks its key up and applies THE RULE with the slot's
//           first; classes are counted per block and added to the record.
// Inside claim, table words other lanes may change are touched with agent-scope
// atomics only; in number a lane writes nothing but its own slot and compares a
// claim word with its own index, which no other lane's store can produce.  What
// one phase reads of another's writing lies behind a kernel boundary.  Slot
// placement depends on timing; nothing a caller can read does.
//
// remap validates on the device (marks by atomic exchange), stashes the kept
// name rows under their new numbers, empties the slots and inserts again: four
// kernels, each of which does nothing once the status is not zero.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "listen_kernels.hpp"

namespace ugo {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

static_assert(sizeof(ListenSlot) == 32 && sizeof(ugo_listen_accept) == 48 && sizeof(ugo_listen_entry) == 32 &&
                  sizeof(ugo_listen_state) == 80,
              "layouts");

constexpr uint32_t kAfInet = 2, kAfInet6 = 10;  // Linux
constexpr uint32_t kNoConn = UGO_STREAM_NO_CONN;

#define UGO_ATOMIC_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct Key {
  uint32_t ip[4];
  uint32_t scope;
  uint32_t port;
  bool ok;
};

// THE KEY of a name row given as its two 16-byte halves, and the row as
// accepted[] and the table keep it: sin6_flowinfo and the bytes past the
// address length zeroed.
__device__ __forceinline__ Key key_of_row(u32x4& lo, u32x4& hi) {
  Key k;
  const uint32_t fam = lo.x & 0xffffu, pbe = lo.x >> 16;
  k.port = ((pbe & 0xffu) << 8) | (pbe >> 8);
  k.ok = true;
  if (fam == kAfInet) {
    k.ip[0] = 0;
    k.ip[1] = 0;
    k.ip[2] = 0xffff0000u;  // bytes 00 00 ff ff
    k.ip[3] = lo.y;
    k.scope = 0;
    hi = u32x4{0, 0, 0, 0};
  } else if (fam == kAfInet6) {
    k.ip[0] = lo.z;
    k.ip[1] = lo.w;
    k.ip[2] = hi.x;
    k.ip[3] = hi.y;
    k.scope = hi.z;
    lo.y = 0;
    hi.w = 0;
  } else {
    k.ip[0] = k.ip[1] = k.ip[2] = k.ip[3] = k.scope = 0;
    k.ok = false;
  }
  return k;
}

__device__ __forceinline__ Key key_of(const uint8_t* names, uint32_t i, u32x4& lo, u32x4& hi) {
  const u32x4* row = reinterpret_cast<const u32x4*>(names) + 2 * static_cast<size_t>(i);
  lo = row[0];
  hi = row[1];
  return key_of_row(lo, hi);
}

__device__ __forceinline__ uint32_t hash_key(const Key& k) {
  const uint32_t w[6] = {k.ip[0], k.ip[1], k.ip[2], k.ip[3], k.scope, k.port};
  uint32_t h = 0x9e3779b9u;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    uint32_t x = w[j] * 0xcc9e2d51u;
    x = (x << 15) | (x >> 17);
    h ^= x * 0x1b873593u;
    h = ((h << 13) | (h >> 19)) * 5u + 0xe6546b64u;
  }
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}

__device__ __forceinline__ bool same_key(const u32x4& ip, uint32_t scope, uint32_t port, const Key& k) {
  return ip.x == k.ip[0] && ip.y == k.ip[1] && ip.z == k.ip[2] && ip.w == k.ip[3] && scope == k.scope &&
         port == k.port;
}

__device__ __forceinline__ bool same_key(const Key& a, const Key& b) {
  return a.ip[0] == b.ip[0] && a.ip[1] == b.ip[1] && a.ip[2] == b.ip[2] && a.ip[3] == b.ip[3] &&
         a.scope == b.scope && a.port == b.port;
}

// 0: no INIT, 1: an INIT with byte 1 != 0, 2: a dup-INIT.
__device__ __forceinline__ uint32_t init_kind(const ListenRouteArgs& a, uint32_t i) {
  const uint32_t len = min(static_cast<uint32_t>(a.lens[i]), a.slot);
  if (len != 22u) return 0;
  const uint8_t* p = a.pkts + static_cast<size_t>(i) * a.slot;
  if (p[0] != 0) return 0;
  return p[1] == 0 ? 2u : 1u;
}

// ------------------------------------------------------------------ route: claim
// The slot the INIT i of key k ends at, or kListenEmpty: the key is a member,
// or no slot is free.
__device__ uint32_t claim_slot(const ListenRouteArgs& a, const Key& k, uint32_t i) {
  const ListenTable& t = a.t;
  const uint32_t mask = t.n_slots - 1u;
  uint32_t s = hash_key(k) & mask;
  for (uint32_t n = 0; n < t.n_slots; ++n, s = (s + 1u) & mask) {
    const u32x4* sl = reinterpret_cast<const u32x4*>(t.slots + s);
    const u32x4 tail = sl[1];  // scope, port, member, first: no lane writes them in this kernel
    if (tail.z != kListenEmpty) {
      if (!same_key(sl[0], tail.x, tail.y, k)) continue;
      if (tail.z != kListenDead) return kListenEmpty;
      __hip_atomic_fetch_min(t.claim + s, i, UGO_ATOMIC_RLX);
      return s;
    }
    uint32_t old = kListenEmpty;
    if (__hip_atomic_compare_exchange_strong(t.claim + s, &old, i, __ATOMIC_RELAXED, UGO_ATOMIC_RLX)) return s;
    if (old >= a.npackets) continue;  // never an index of this batch: not followed
    u32x4 lo, hi;
    const Key o = key_of(a.names, old, lo, hi);
    if (o.ok && same_key(o, k)) {
      __hip_atomic_fetch_min(t.claim + s, i, UGO_ATOMIC_RLX);
      return s;
    }
  }
  __hip_atomic_fetch_or(&t.st->err, static_cast<uint32_t>(UGO_LISTEN_FULL), UGO_ATOMIC_RLX);
  return kListenEmpty;
}

__global__ __launch_bounds__(256) void k_listen_claim(ListenRouteArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.npackets) return;
  uint32_t mine = kListenEmpty;
  if (init_kind(a, i) != 0) {
    u32x4 lo, hi;
    const Key k = key_of(a.names, i, lo, hi);
    if (k.ok) mine = claim_slot(a, k, i);
  }
  a.conn_of[i] = mine;
}

// ------------------------------------------------------------------ route: count, number
__device__ __forceinline__ bool is_first(const ListenRouteArgs& a, uint32_t j, uint32_t& s) {
  s = a.conn_of[j];
  return s < a.t.n_slots && __hip_atomic_load(a.t.claim + s, UGO_ATOMIC_RLX) == j;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds /* [4] */) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();  // lds may still be read from the call before
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(256) void k_listen_count(ListenRouteArgs a, uint32_t per) {
  __shared__ uint32_t lds[4];
  const uint32_t start = blockIdx.x * per, end = min(start + per, a.npackets);
  uint32_t n = 0;
  for (uint32_t j = start + threadIdx.x; j < end; j += 256u) {
    uint32_t s;
    n += is_first(a, j, s) ? 1u : 0u;
  }
  n = block_sum(n, lds);
  if (threadIdx.x == 0) {
    a.t.block_count[blockIdx.x] = n;
    if (blockIdx.x == 0) a.t.call->base = a.t.st->nconn;
  }
}

__global__ __launch_bounds__(256) void k_listen_number(ListenRouteArgs a, uint32_t per) {
  __shared__ uint32_t lds[4];
  __shared__ uint32_t wsum[4];
  const ListenTable& t = a.t;
  uint32_t before = 0;
  for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256u) before += t.block_count[b];
  before = block_sum(before, lds);
  const uint32_t base = min(t.call->base, t.max_conn), room = t.max_conn - base;
  if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) {
    const uint32_t total = before + t.block_count[blockIdx.x];
    const uint32_t acc = min(total, room);
    t.st->nconn = base + acc;
    *a.n_accepted = acc;
  }
  const uint32_t start = blockIdx.x * per, end = min(start + per, a.npackets);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t running = before;
  for (uint32_t j0 = start; j0 < end; j0 += 256u) {  // every lane of the block takes every turn
    const uint32_t j = j0 + threadIdx.x;
    uint32_t s = kListenEmpty;
    const bool flag = j < end && is_first(a, j, s);
    const u64 bal = __ballot(flag);
    if (lane == 0) wsum[w] = static_cast<uint32_t>(__popcll(bal));
    __syncthreads();
    uint32_t r = running + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)));
    for (uint32_t x = 0; x < w; ++x) r += wsum[x];
    running += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    if (!flag) continue;
    u32x4 lo, hi;
    const Key k = key_of(a.names, j, lo, hi);  // ok: the lane claimed with it
    u32x4* sl = reinterpret_cast<u32x4*>(t.slots + s);
    const u32x4 ip{k.ip[0], k.ip[1], k.ip[2], k.ip[3]};
    if (r < room) {
      const uint32_t m = base + r;
      sl[0] = ip;
      sl[1] = u32x4{k.scope, k.port, m, j};
      u32x4* row = reinterpret_cast<u32x4*>(t.names) + 2 * static_cast<size_t>(m);
      row[0] = lo;
      row[1] = hi;
      t.member_slot[m] = s;
      if (r < a.max_accepted) {
        const uint8_t* p = a.pkts + static_cast<size_t>(j) * a.slot;
        const uint32_t cid = (uint32_t(p[18]) << 24) | (uint32_t(p[19]) << 16) | (uint32_t(p[20]) << 8) | p[21];
        u32x4* acc = reinterpret_cast<u32x4*>(a.accepted + r);
        acc[0] = u32x4{j, m, cid, 0};
        acc[1] = lo;
        acc[2] = hi;
      }
    } else {  // deviation (b)
      if (t.slots[s].member == kListenEmpty) __hip_atomic_fetch_add(&t.st->n_dead, 1u, UGO_ATOMIC_RLX);
      sl[0] = ip;
      sl[1] = u32x4{k.scope, k.port, kListenDead, j};
    }
    __hip_atomic_store(t.claim + s, kListenEmpty, UGO_ATOMIC_RLX);
  }
}

// ------------------------------------------------------------------ route: THE RULE
// The slot that holds k, or kListenEmpty.
__device__ __forceinline__ uint32_t find_slot(const ListenTable& t, const Key& k, u32x4& tail) {
  const uint32_t mask = t.n_slots - 1u;
  uint32_t s = hash_key(k) & mask;
  for (uint32_t n = 0; n < t.n_slots; ++n, s = (s + 1u) & mask) {
    const u32x4* sl = reinterpret_cast<const u32x4*>(t.slots + s);
    tail = sl[1];
    if (tail.z == kListenEmpty) return kListenEmpty;
    if (same_key(sl[0], tail.x, tail.y, k)) return s;
  }
  return kListenEmpty;
}

__global__ __launch_bounds__(256) void k_listen_route(ListenRouteArgs a) {
  __shared__ uint32_t hist[UGO_LISTEN_NCLASS];
  if (threadIdx.x < UGO_LISTEN_NCLASS) hist[threadIdx.x] = 0;
  __syncthreads();
  const ListenTable& t = a.t;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < a.npackets) {
    const uint32_t base = t.call->base;
    uint32_t cls = UGO_LISTEN_STRANGER, conn = kNoConn;
    u32x4 lo, hi, tail;
    const Key k = key_of(a.names, i, lo, hi);
    if (!k.ok) {
      cls = UGO_LISTEN_BAD_NAME;
    } else if (find_slot(t, k, tail) != kListenEmpty) {
      const uint32_t m = tail.z, f = tail.w, kind = init_kind(a, i);
      if (m == kListenDead) {
        if (kind != 0 && f == i) cls = UGO_LISTEN_REFUSED;
      } else if (m < base || i > f) {
        if (kind == 2u) {
          cls = UGO_LISTEN_DUP_INIT;
        } else {
          cls = m < base ? UGO_LISTEN_FED : UGO_LISTEN_FED_NEW;
          conn = m;
        }
      } else if (i == f) {
        cls = UGO_LISTEN_ACCEPT;
      }
    }
    a.conn_of[i] = conn;
    a.cls[i] = static_cast<uint8_t>(cls);
    atomicAdd(&hist[cls], 1u);
  }
  __syncthreads();
  if (threadIdx.x < UGO_LISTEN_NCLASS && hist[threadIdx.x] != 0)
    __hip_atomic_fetch_add(reinterpret_cast<u64*>(&t.st->counts[threadIdx.x]), static_cast<u64>(hist[threadIdx.x]),
                           UGO_ATOMIC_RLX);
}

// ------------------------------------------------------------------ names, entries
__global__ __launch_bounds__(256) void k_listen_names(ListenNamesArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.npackets) return;
  const uint32_t m = a.conn_of[i], nconn = min(a.t.st->nconn, a.t.max_conn);
  u32x4 lo{0, 0, 0, 0}, hi{0, 0, 0, 0};
  uint32_t len = 0;
  if (m < nconn) {
    const u32x4* row = reinterpret_cast<const u32x4*>(a.t.names) + 2 * static_cast<size_t>(m);
    lo = row[0];
    hi = row[1];
    const uint32_t fam = lo.x & 0xffffu;
    len = fam == kAfInet ? 16u : fam == kAfInet6 ? 28u : 0u;
  }
  u32x4* out = reinterpret_cast<u32x4*>(a.names_out) + 2 * static_cast<size_t>(i);
  out[0] = lo;
  out[1] = hi;
  a.name_lens[i] = len;
}

__global__ __launch_bounds__(256) void k_listen_entries(ListenTable t, ugo_listen_entry* out, uint32_t cap) {
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= cap) return;
  u32x4 ip{0, 0, 0, 0}, tail{0, 0, kNoConn, 0};
  if (m < min(t.st->nconn, t.max_conn)) {
    const uint32_t s = t.member_slot[m];
    if (s < t.n_slots) {
      const u32x4* sl = reinterpret_cast<const u32x4*>(t.slots + s);
      ip = sl[0];
      tail = sl[1];
      if (tail.z != m) tail.z = kListenDead;  // the slot is not the member's: shown, never hidden
      tail.w = 0;
    }
  }
  u32x4* o = reinterpret_cast<u32x4*>(out + m);
  o[0] = ip;
  o[1] = tail;
}

// ------------------------------------------------------------------ init, remap
__device__ __forceinline__ void clear_table(const ListenTable& t, uint32_t idx) {
  if (idx < t.n_slots) {
    u32x4* sl = reinterpret_cast<u32x4*>(t.slots + idx);
    sl[0] = u32x4{0, 0, 0, 0};
    sl[1] = u32x4{0, 0, kListenEmpty, 0};
    t.claim[idx] = kListenEmpty;
  }
  if (idx < t.max_conn) {
    u32x4* row = reinterpret_cast<u32x4*>(t.names) + 2 * static_cast<size_t>(idx);
    row[0] = u32x4{0, 0, 0, 0};
    row[1] = u32x4{0, 0, 0, 0};
    t.member_slot[idx] = kListenEmpty;
  }
}

__global__ __launch_bounds__(256) void k_listen_init(ListenTable t) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  clear_table(t, idx);
  if (idx < t.max_conn) t.mark[idx] = 0;
  if (idx == 0) {
    ugo_listen_state st{};
    st.n_slots = t.n_slots;
    *t.st = st;
    *t.call = ListenCall{0, 0};
  }
}

__global__ __launch_bounds__(256) void k_listen_remap_check(ListenRemapArgs a) {
  const ListenTable& t = a.t;
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  const uint32_t nconn = min(t.st->nconn, t.max_conn);
  uint32_t bad = 0;
  if (m == 0) {
    if (a.n_index != nconn) bad |= UGO_LISTEN_REMAP_LENGTH;
    if (a.nconn_new > t.max_conn) bad |= UGO_LISTEN_REMAP_TOO_MANY;
  }
  if (m < nconn && m < a.n_index) {
    const uint32_t v = a.new_index[m];
    if (v != kNoConn) {
      if (v >= a.nconn_new)
        bad |= UGO_LISTEN_REMAP_OUT_OF_RANGE;
      else if (v < t.max_conn && __hip_atomic_exchange(t.mark + v, 1u, UGO_ATOMIC_RLX) != 0)
        bad |= UGO_LISTEN_REMAP_NOT_INJECTIVE;
    }
  }
  if (bad) __hip_atomic_fetch_or(&t.call->bad, bad, UGO_ATOMIC_RLX);
}

__global__ __launch_bounds__(256) void k_listen_remap_stash(ListenRemapArgs a) {
  const ListenTable& t = a.t;
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (t.call->bad || m >= min(t.st->nconn, t.max_conn)) return;
  const uint32_t v = a.new_index[m];
  if (v == kNoConn) return;  // v < nconn_new <= max_conn: checked
  const u32x4* row = reinterpret_cast<const u32x4*>(t.names) + 2 * static_cast<size_t>(m);
  u32x4* dst = reinterpret_cast<u32x4*>(t.tmp_names) + 2 * static_cast<size_t>(v);
  dst[0] = row[0];
  dst[1] = row[1];
}

__global__ __launch_bounds__(256) void k_listen_remap_clear(ListenRemapArgs a) {
  if (a.t.call->bad) return;
  clear_table(a.t, blockIdx.x * 256u + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_listen_remap_insert(ListenRemapArgs a) {
  const ListenTable& t = a.t;
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  const uint32_t bad = t.call->bad;
  if (v < t.max_conn) {
    const uint32_t marked = t.mark[v];
    t.mark[v] = 0;
    if (!bad && marked) {
      const u32x4* src = reinterpret_cast<const u32x4*>(t.tmp_names) + 2 * static_cast<size_t>(v);
      u32x4 lo = src[0], hi = src[1];
      const Key k = key_of_row(lo, hi);
      if (k.ok) {  // a number without an entry keeps none
        const uint32_t mask = t.n_slots - 1u;
        uint32_t s = hash_key(k) & mask;
        for (uint32_t n = 0; n < t.n_slots; ++n, s = (s + 1u) & mask) {  // the keys of members differ: no compare
          uint32_t old = kListenEmpty;
          if (!__hip_atomic_compare_exchange_strong(&t.slots[s].member, &old, v, __ATOMIC_RELAXED, UGO_ATOMIC_RLX))
            continue;
          ListenSlot* sl = t.slots + s;
          *reinterpret_cast<u32x4*>(sl->ip) = u32x4{k.ip[0], k.ip[1], k.ip[2], k.ip[3]};
          sl->scope = k.scope;
          sl->port = k.port;
          u32x4* row = reinterpret_cast<u32x4*>(t.names) + 2 * static_cast<size_t>(v);
          row[0] = lo;
          row[1] = hi;
          t.member_slot[v] = s;
          break;
        }
      }
    }
  }
  if (v == 0) {
    *a.status = bad;
    if (!bad) {
      t.st->nconn = a.nconn_new;
      t.st->n_dead = 0;
      t.st->err = 0;
    }
  }
}

inline uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace

hipError_t launch_listen_route(const ListenRouteArgs& a, hipStream_t s) {
  const uint32_t tiles = blocks_of(a.npackets);
  uint32_t nb = tiles < kListenScanBlocks ? tiles : kListenScanBlocks;
  const uint32_t per = (tiles + nb - 1u) / nb * 256u;  // a piece is whole tiles
  nb = (tiles + per / 256u - 1u) / (per / 256u);
  launch(kKListen, k_listen_claim, dim3(tiles), dim3(256), 0, s, a);
  launch(kKListen, k_listen_count, dim3(nb), dim3(256), 0, s, a, per);
  launch(kKListen, k_listen_number, dim3(nb), dim3(256), 0, s, a, per);
  launch(kKListen, k_listen_route, dim3(tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_listen_remap(const ListenRemapArgs& a, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(&a.t.call->bad, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint32_t members = blocks_of(a.t.max_conn);
  const uint32_t all = blocks_of(a.t.n_slots > a.t.max_conn ? a.t.n_slots : a.t.max_conn);
  launch(kKListen, k_listen_remap_check, dim3(members), dim3(256), 0, s, a);
  launch(kKListen, k_listen_remap_stash, dim3(members), dim3(256), 0, s, a);
  launch(kKListen, k_listen_remap_clear, dim3(all), dim3(256), 0, s, a);
  launch(kKListen, k_listen_remap_insert, dim3(members), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_listen_names(const ListenNamesArgs& a, hipStream_t s) {
  launch(kKListen, k_listen_names, dim3(blocks_of(a.npackets)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_listen_entries(const ListenTable& t, ugo_listen_entry* out, uint32_t cap, hipStream_t s) {
  launch(kKListen, k_listen_entries, dim3(blocks_of(cap)), dim3(256), 0, s, t, out, cap);
  return hipGetLastError();
}

hipError_t launch_listen_init(const ListenTable& t, hipStream_t s) {
  launch(kKListen, k_listen_init, dim3(blocks_of(t.n_slots > t.max_conn ? t.n_slots : t.max_conn)), dim3(256), 0, s,
         t);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
