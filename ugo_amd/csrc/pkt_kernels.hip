// pkt_kernels.hip -- batch decoder and encoder for ugo's packet wire format on
// gfx950.  The encoder (k_packet_encode) is described
// where it starts, below.  Decoder: one thread per packet restates, for a
// whole batch:
//   Conn.handlePacket  ugo/conn.go:387-419  decrypt, strip the FEC header of
//                                           typeData packets, ugoPacket.decode
//   ugoPacket.decode   ugo/packet.go:138-177
//   parseSack          ugo/packet.go:231-331, validateAckRanges :439-474
//   parseSegment       ugo/packet.go:78-100
//   ReadUfloat16       ugo/utils/float16.go:25-51, binary.ReadUvarint (Go stdlib)
//
// The parse is serial within a packet (varints, data-dependent skips), so the
// parallelism is across packets.  Bytes are read through a 16-byte window
// held in registers (one aligned dwordx4 load, plus the pad chunk when
// decrypting, per 16 bytes touched): a typical data packet touches only its
// first window and the window of its segment header; segment data is never
// read -- segments are reported as (offset, data_off, len, avail) views.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "pkt_kernels.hpp"

namespace ugo {
namespace kern {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct ByteReader {
  const uint8_t* base;  // slot start
  const uint8_t* pad;
  uint32_t pos, end;
  uint32_t wchunk;      // 16-B chunk index held in w (~0u: none)
  u32x4 w;

  __device__ __forceinline__ uint32_t byte_at(uint32_t j) {
    if ((j >> 4) != wchunk) {
      wchunk = j >> 4;
      w = *reinterpret_cast<const u32x4*>(base + (j & ~15u));
      if (pad) w ^= *reinterpret_cast<const u32x4*>(pad + (j & ~15u));
    }
    const uint32_t q = (j >> 2) & 3u;
    const uint32_t d = (q & 2u) ? ((q & 1u) ? w.w : w.z) : ((q & 1u) ? w.y : w.x);
    return (d >> (8u * (j & 3u))) & 0xffu;
  }
  __device__ __forceinline__ uint32_t left() const { return end - pos; }
};

enum : uint32_t {
  kOK = UGO_PKT_OK,
  kEOF = UGO_PKT_EOF,
  kUnexpectedEOF = UGO_PKT_UNEXPECTED_EOF,
  kOverflow = UGO_PKT_VARINT_OVERFLOW,
  kInvalidRanges = UGO_PKT_INVALID_ACK_RANGES,
  kInvalidFirst = UGO_PKT_INVALID_FIRST_ACK_RANGE,
  kCapacity = UGO_PKT_CAPACITY,
};

__device__ __forceinline__ uint32_t read_byte(ByteReader& r, uint32_t& v) {
  if (r.pos >= r.end) return kEOF;
  v = r.byte_at(r.pos++);
  return kOK;
}

// binary.ReadUvarint (at most MaxVarintLen64 = 10 bytes)
__device__ __forceinline__ uint32_t read_uvarint(ByteReader& r, uint64_t& x) {
  x = 0;
  uint32_t s = 0;
  for (int i = 0; i < 10; ++i) {
    if (r.pos >= r.end) return i > 0 ? kUnexpectedEOF : kEOF;
    const uint32_t b = r.byte_at(r.pos++);
    if (b < 0x80u) {
      if (i == 9 && b > 1u) return kOverflow;
      x |= static_cast<uint64_t>(b) << s;
      return kOK;
    }
    x |= static_cast<uint64_t>(b & 0x7fu) << s;
    s += 7;
  }
  return kOverflow;
}

// ReadUfloat16: utils.ReadUint16 (two ReadByte, little endian) + decode
__device__ __forceinline__ uint32_t read_ufloat16(ByteReader& r, uint64_t& v) {
  uint32_t b1, b2;
  uint32_t st = read_byte(r, b1);
  if (st) return st;
  st = read_byte(r, b2);
  if (st) return st;
  const uint32_t val = b1 | (b2 << 8);
  if (val < (1u << 12)) {
    v = val;
    return kOK;
  }
  const uint32_t exponent = (val >> 11) - 1u;
  v = static_cast<uint64_t>(val - (exponent << 11)) << exponent;
  return kOK;
}

// parseSack + validateAckRanges, streaming: a range is final once the next
// one starts (only the last range is ever modified or dropped, ugo/packet.go:
// 285-306), so it is validated against its predecessor and stored then.
// Ranges beyond the caller's cap are validated but not stored (`over`).
// Returns a hard error, or OK with `over` telling whether ranges were dropped.
__device__ uint32_t parse_sack(ByteReader& r, ugo_pkt_info& o, uint64_t* rg, uint32_t cap, bool& over) {
  uint32_t type_byte;
  uint32_t st = read_byte(r, type_byte);
  if (st) return st;
  const bool has_missing = (type_byte & 0x20u) != 0;
  uint64_t largest;
  if ((st = read_uvarint(r, largest))) return st;
  o.largest_acked = largest;
  uint64_t delay;
  if ((st = read_ufloat16(r, delay))) return st;
  o.delay_us = delay;
  uint32_t nblocks = 0;
  if (has_missing && (st = read_byte(r, nblocks))) return st;
  if (has_missing && nblocks == 0) return kInvalidRanges;
  uint64_t blen;
  if ((st = read_uvarint(r, blen))) return st;
  if (blen < 1) return kInvalidFirst;
  if (blen > largest) return kInvalidRanges;
  if (!has_missing) {
    o.largest_in_order = largest + 1 - blen;
    return kOK;
  }
  uint64_t cf = largest - blen + 1, cl = largest;  // current (last) range
  uint64_t pf = 0;                                  // first of the last final range
  uint32_t nfinal = 0;
  bool invalid = false;
  auto finalize = [&](uint64_t f, uint64_t l) {
    if (f > l) invalid = true;
    if (nfinal > 0 && (pf <= f || pf <= l + 1)) invalid = true;
    if (nfinal < cap) {
      rg[2 * nfinal] = f;
      rg[2 * nfinal + 1] = l;
    } else {
      over = true;
    }
    pf = f;
    ++nfinal;
  };
  bool in_long = false, last_complete = false;
  for (uint32_t i = 0; i < nblocks; ++i) {
    uint32_t gap;
    if ((st = read_byte(r, gap))) return st;
    if ((st = read_uvarint(r, blen))) return st;
    if (in_long) {
      cf -= static_cast<uint64_t>(gap) + blen;
      cl -= gap;
    } else {
      last_complete = false;
      finalize(cf, cl);
      cl = cf - gap - 1;
      cf = cl - blen + 1;
    }
    if (blen > 0) last_complete = true;
    in_long = blen == 0;
  }
  if (last_complete) finalize(cf, cl);  // else the last range is dropped
  o.n_ranges = static_cast<uint16_t>(min(nfinal, cap));
  o.largest_in_order = pf;
  // validateAckRanges: >= 2 ranges; range 0 ends at largest (it is never
  // modified after it is final, so this holds by construction)
  if (nfinal == 1 || invalid) return kInvalidRanges;
  return kOK;
}

__device__ uint32_t decode_one(ByteReader& r, ugo_pkt_info& o, uint64_t* rg, uint32_t rcap, ugo_pkt_segment* sg,
                               uint32_t scap) {
  uint32_t flags;
  uint32_t st = read_byte(r, flags);
  if (st) return st;
  o.flags = static_cast<uint8_t>(flags);
  bool over = false;  // more ranges / segments than the caller's arrays hold
  if (flags & 0x80u) {
    st = parse_sack(r, o, rg, rcap, over);
    if (st) return st;
  }
  if (flags != 0x80u && (st = read_uvarint(r, o.packet_number))) return st;
  if ((flags & 0x40u) && (st = read_uvarint(r, o.stop_waiting))) return st;
  uint32_t ns = 0;
  while (r.left() > 0) {
    uint64_t off;
    if ((st = read_uvarint(r, off))) return st;
    // binary.Read(r, BigEndian, &uint16): io.ReadFull of 2 bytes
    if (r.left() == 0) return kEOF;
    if (r.left() == 1) return kUnexpectedEOF;
    const uint32_t len = (r.byte_at(r.pos) << 8) | r.byte_at(r.pos + 1);
    r.pos += 2;
    uint32_t avail = 0;
    const uint32_t data_off = r.pos;
    if (len != 0) {
      if (r.left() == 0) return kEOF;  // bytes.Reader.Read at the end
      avail = min(len, r.left());
      r.pos += avail;
    }
    if (ns < scap) {
      sg[ns] = ugo_pkt_segment{off, data_off, static_cast<uint16_t>(len), static_cast<uint16_t>(avail)};
      o.n_segments = static_cast<uint16_t>(ns + 1);
    } else {
      over = true;
    }
    ++ns;
  }
  return over ? kCapacity : kOK;
}

__global__ __launch_bounds__(256) void k_packet_decode(PktArgs a) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= a.npk) return;
  ByteReader r;
  r.base = a.pkts + i * a.slot;
  r.pad = a.pad;
  r.end = min(static_cast<uint32_t>(a.lens[i]), static_cast<uint32_t>(a.slot));
  r.pos = 0;
  r.wchunk = ~0u;
  r.w = u32x4{0u, 0u, 0u, 0u};
  ugo_pkt_info o{};
  if (a.framed && r.end >= 6u) {
    const uint32_t flag = r.byte_at(4) | (r.byte_at(5) << 8);  // FEC.decode, ugo/fec.go:81
    o.fec_flag_lo = static_cast<uint8_t>(flag);
    if (flag == 0xf1u) r.pos = 6;  // typeData: data = data[fecHeaderSize:] (ugo/conn.go:403-405)
  }
  o.payload_off = r.pos;
  o.status = decode_one(r, o, a.ranges + i * 2ull * a.max_ranges, a.max_ranges, a.segs + i * a.max_segments,
                        a.max_segments);
  a.info[i] = o;
}

// ---------------------------------------------------------------- encoder
// Batch ugoPacket.encode (+ crypt.Encrypt as an XOR with `pad`):
//   ugoPacket.encode       ugo/packet.go:182-228
//   sack.write             ugo/packet.go:338-430
//   numWritableNackRanges  ugo/packet.go:479-505
//   segment.write          ugo/packet.go:101-110
//   WriteUfloat16          ugo/utils/float16.go:54-86, binary.PutUvarint (Go stdlib)
//
// A block of 256 threads encodes kEncPacketsPerBlock packets in two phases.
//   A. One thread per packet (the serial part, as in the decoder): it sizes the
//      packet arithmetically (field sizes, status, total length; no byte is
//      written before the packet is known to be valid and to fit), then writes
//      every 16-B chunk that holds a header byte, a segment boundary or the
//      packet's end through a 16-byte register window -- one aligned store per
//      chunk.  The at most 15 segment bytes on either side of a segment's
//      interior come out of two unaligned 16-B loads (the segment's first and
//      last 16 bytes), not byte loads.  Whole chunks of segment data are
//      skipped.
//   B. kEncLanes lanes per packet copy those skipped interior chunks: one
//      unaligned 16-B load from the payload, the pad XOR, one aligned 16-B
//      store.  A segment's place in the packet follows from the position of
//      the first segment header (left in LDS by phase A) and the sizes of the
//      offset varints, so the lanes re-read only the segment descriptors.
// Every chunk of [0, round_up(len, 16)) is stored exactly once, by one phase.
//
// Measured (tools/pkt_encode_probe.py, 851,968 packets with one 1400-B
// segment, slot 1488; DESIGN.md §4.3, profiles/pkt_encode/): 0.53-0.56 ms
// FEC-framed, 0.55-0.60 ms unframed with the pad, against 0.36 ms for an nt
// copy of the same bytes.  Phase A alone takes 0.11 ms of it.  Nontemporal
// stores in phase B: 0.64 -> 0.56 ms (nontemporal payload loads on top: no
// change).  A wave instead of a half-wave per packet, 32 / 128 / 256 packets
// per block instead of 64, and taking packets two at a time with both
// packets' loads in flight before the stores (88 VGPRs) all measured within
// the run-to-run spread or slower.
#ifndef UGO_PKT_ENC_LANES
#define UGO_PKT_ENC_LANES 32  // lanes per packet in phase B (32 or 64; the A/B is in DESIGN.md)
#endif
constexpr uint32_t kEncLanes = UGO_PKT_ENC_LANES;
constexpr uint32_t kEncPacketsPerBlock = 64;  // phase A fills one wave
static_assert(kEncLanes == 32 || kEncLanes == 64, "a half-wave or a wave per packet");

enum : uint32_t {
  kBadLargest = UGO_PKT_INCONSISTENT_LARGEST_ACKED,
  kBadLowest = UGO_PKT_INCONSISTENT_LOWEST_ACKED,
  kBadRangeCount = UGO_PKT_INCONSISTENT_RANGE_COUNT,
};

typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
__device__ __forceinline__ u32x4 ldu16(const uint8_t* p) {  // 16 bytes at any byte address
  return *reinterpret_cast<const u32x4u*>(p);
}

__device__ __forceinline__ uint32_t byte_of(const u32x4& v, uint32_t j) {
  const uint32_t q = (j >> 2) & 3u;
  const uint32_t d = (q & 2u) ? ((q & 1u) ? v.w : v.z) : ((q & 1u) ? v.y : v.x);
  return (d >> (8u * (j & 3u))) & 0xffu;
}

// len(binary.PutUvarint(v))
__device__ __forceinline__ uint32_t uvarint_len(uint64_t v) {
  const uint32_t bits = 64u - static_cast<uint32_t>(__builtin_clzll(v | 1ull));
  return (bits + 6u) / 7u;
}

// WriteUfloat16's 16-bit result
__device__ __forceinline__ uint32_t ufloat16(uint64_t value) {
  if (value < (1ull << 12)) return static_cast<uint32_t>(value);
  if (value >= 0x3FFC0000000ull) return 0xFFFFu;  // uFloat16MaxValue
  uint32_t exponent = 0;
#pragma unroll
  for (uint32_t offset = 16; offset > 0; offset /= 2) {
    if (value >= (1ull << (11u + offset))) {
      exponent += offset;
      value >>= offset;
    }
  }
  return (static_cast<uint32_t>(value) + (exponent << 11)) & 0xFFFFu;
}

// The packet's bytes in order, through a 16-byte window: a chunk is stored
// (pad applied) when its last byte is put, or by finish() with zeros -- and
// no pad -- past the packet's end.
struct ByteWriter {
  uint8_t* base;  // slot start
  const uint8_t* pad;
  uint32_t pos;
  uint32_t w0, w1, w2, w3;

  __device__ __forceinline__ void flush(uint32_t o, uint32_t keep) {
    u32x4 v = {w0, w1, w2, w3};
    if (pad) {
      u32x4 k = *reinterpret_cast<const u32x4*>(pad + o);
      if (keep < 16u) {
        uint32_t m[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t n = keep >= 4u * j + 4u ? 4u : (keep > 4u * j ? keep - 4u * j : 0u);
          m[j] = n >= 4u ? 0xffffffffu : ((1u << (8u * n)) - 1u);
        }
        k &= u32x4{m[0], m[1], m[2], m[3]};
      }
      v ^= k;
    }
    *reinterpret_cast<u32x4*>(base + o) = v;
    w0 = w1 = w2 = w3 = 0u;
  }
  __device__ __forceinline__ void put(uint32_t b) {
    const uint32_t v = (b & 0xffu) << (8u * (pos & 3u));
    const uint32_t q = (pos >> 2) & 3u;
    w0 |= q == 0u ? v : 0u;
    w1 |= q == 1u ? v : 0u;
    w2 |= q == 2u ? v : 0u;
    w3 |= q == 3u ? v : 0u;
    if ((++pos & 15u) == 0u) flush(pos - 16u, 16u);
  }
  __device__ __forceinline__ void put_uvarint(uint64_t v) {  // at most 10 bytes
    while (v >= 0x80u) {
      put(static_cast<uint32_t>(v) | 0x80u);
      v >>= 7;
    }
    put(static_cast<uint32_t>(v));
  }
  __device__ __forceinline__ void skip_chunks(uint32_t nbytes) { pos += nbytes; }  // window empty, pos % 16 == 0
  __device__ __forceinline__ void finish() {
    if (pos & 15u) flush(pos & ~15u, pos & 15u);
  }
};

// One ACK range after the first, as sack.write sees it (packet.go:385-391):
// its length and the number of blocks the writer emits for the gap before it.
struct GapBlocks {
  uint64_t length, gap, num;
};
__device__ __forceinline__ GapBlocks gap_blocks(uint64_t prev_first, uint64_t first, uint64_t last) {
  GapBlocks g;
  g.length = last - first + 1;
  g.gap = prev_first - last - 1;
  g.num = g.gap / 0xFFu + 1;
  if (g.gap % 0xFFu == 0) --g.num;
  return g;
}

// Where a packet's segment bytes come from: the source policy of
// encode_header and k_packet_encode.  FlatSrc is ugo_fec_packet_encode's
// payload pointer (segment at payload + i*payload_stride + data_off); WinSrc
// is ugo_fec_stream_tx_set_encode's send window of member conn_of[i] (stream
// byte x at win[x & (cap-1)], include/ugo_stream.h), which also refuses a
// packet of no member and a segment outside [base, tail).
struct FlatSrc {
  typedef PktEncArgs Args;
  static constexpr bool kStash = false;  // phase B recomputes the packet's source from the arguments
  struct Seg {
    const uint8_t* s;
    __device__ __forceinline__ u32x4 ld16(uint32_t k) const { return ldu16(s + k); }
    __device__ __forceinline__ uint32_t byte(uint32_t k) const { return s[k]; }
  };
  const uint8_t* p;
  __device__ __forceinline__ FlatSrc(const Args& a, uint64_t i) : p(a.payload + i * a.payload_stride) {}
  __device__ __forceinline__ bool member() const { return true; }
  __device__ __forceinline__ bool holds(const ugo_pkt_segment*, uint32_t) const { return true; }
  __device__ __forceinline__ Seg seg(const ugo_pkt_segment& g) const { return Seg{p + g.data_off}; }
};

struct WinSrc {
  typedef PktEncSetArgs Args;
  // phase A leaves the member's window in LDS: phase B then starts on the bytes
  // without the dependent loads of conn_of[i] and the table entry
  static constexpr bool kStash = true;
  struct Stash {
    const uint8_t* win;
    uint64_t mask;
  };
  struct Seg {
    const uint8_t* win;
    uint64_t mask, o;
    __device__ __forceinline__ uint32_t byte(uint32_t k) const { return win[(o + k) & mask]; }
    __device__ __forceinline__ u32x4 ld16(uint32_t k) const {
      const uint64_t at = (o + k) & mask;
      if (at + 16u <= mask + 1u) return ldu16(win + at);
      uint32_t d[4] = {0u, 0u, 0u, 0u};  // the 16 bytes straddle the wrap point
      for (uint32_t b = 0; b < 16u; ++b) d[b >> 2] |= static_cast<uint32_t>(win[(at + b) & mask]) << (8u * (b & 3u));
      return u32x4{d[0], d[1], d[2], d[3]};
    }
  };
  const uint8_t* win;
  const ugo_stream_tx_state* rec;
  uint64_t mask;
  __device__ __forceinline__ WinSrc(const Args& a, uint64_t i) : win(nullptr), rec(nullptr), mask(0) {
    const uint32_t c = a.conn_of[i];
    if (c < a.nconn) {
      const StreamTxEntry& e = a.table[c];
      win = e.win;
      rec = e.rec;
      mask = e.cap - 1;
    }
  }
  __device__ __forceinline__ explicit WinSrc(const Stash& st) : win(st.win), rec(nullptr), mask(st.mask) {}
  __device__ __forceinline__ Stash stash() const { return Stash{win, mask}; }
  __device__ __forceinline__ bool member() const { return win != nullptr; }
  __device__ __forceinline__ bool holds(const ugo_pkt_segment* sg, uint32_t nseg) const {
    const uint64_t base = rec->base, tail = rec->tail;
    bool ok = true;
    for (uint32_t j = 0; j < nseg; ++j) {
      const uint64_t o = sg[j].offset;
      ok = ok && o >= base && o <= tail && sg[j].len <= tail - o;
    }
    return ok;
  }
  __device__ __forceinline__ Seg seg(const ugo_pkt_segment& g) const { return Seg{win, mask, g.offset}; }
};

// Sizes packet i and, if the reference would encode it and it fits, writes
// its header and boundary chunks.  Returns the status; pos0 = where the first
// segment header starts, ns = segments to place (0 unless the status is OK).
template <class Src>
__device__ uint32_t encode_header(const typename Src::Args& a, const Src& P, uint64_t i, uint32_t& pos0, uint32_t& ns,
                                  uint32_t& total) {
  const ugo_pkt_info& I = a.info[i];
  const uint32_t nr = I.n_ranges, nseg = I.n_segments;
  if (nr > a.max_ranges || nseg > a.max_segments) return kCapacity;
  const uint64_t* rg = a.ranges + i * 2ull * a.max_ranges;
  const ugo_pkt_segment* sg = a.segs + i * a.max_segments;
  if (!P.holds(sg, nseg)) return UGO_PKT_OUT_OF_WINDOW;
  const uint64_t pn = I.packet_number, sw = I.stop_waiting;
  const uint64_t largest = I.largest_acked, in_order = I.largest_in_order;
  const bool has_sack = (I.flags & 0x80u) != 0;  // p.sack != nil
  const uint32_t flags = I.flags | (sw != 0 ? 0x40u : 0u) | (nseg != 0 ? 0x20u : 0u);
  const uint32_t room = a.framed ? 6u : 0u;

  // ---- size and status; every quantity is arithmetic in the field values
  uint64_t len = room + 1u;
  uint64_t num_ranges = 0, first_len = 0;
  if (has_sack) {
    len += 1u + uvarint_len(largest) + 2u;
    if (nr != 0) {
      // numWritableNackRanges: ceil((gap + 1) / 256) blocks per gap while they stay below 255
      uint64_t num = 0;
      for (uint32_t k = 1; k < nr; ++k) {
        const uint64_t g1 = rg[2 * (k - 1)] - rg[2 * k + 1];
        const uint64_t rl = g1 / 256u + (g1 % 256u != 0 ? 1u : 0u);
        if (num + rl < 0xFFu)
          num += rl;
        else
          break;
      }
      num_ranges = num + 1;
      len += 1u;
      if (largest != rg[1]) return kBadLargest;
      if (in_order != rg[2 * (nr - 1)]) return kBadLowest;
      first_len = largest - rg[0] + 1;
    } else {
      first_len = largest - in_order + 1;
    }
    len += uvarint_len(first_len);
    uint64_t written = nr != 0 ? 1u : 0u;
    for (uint32_t k = 1; k < nr; ++k) {
      const GapBlocks g = gap_blocks(rg[2 * (k - 1)], rg[2 * k], rg[2 * k + 1]);
      // written <= num_ranges <= 255 here, and the writer stops at the first
      // range that reaches num_ranges: a range with more blocks than remain
      // ends in "inconsistent number of ACK ranges written" whatever follows
      if (g.num > num_ranges - written) return kBadRangeCount;
      if (g.num != 0) len += 2u * (g.num - 1u) + 1u + uvarint_len(g.length);
      written += g.num;
      if (written >= num_ranges) break;
    }
    if (written != num_ranges) return kBadRangeCount;
  }
  if (flags != 0x80u) len += uvarint_len(pn);
  if (sw != 0) len += uvarint_len(sw);
  const uint64_t seg_start = len;
  for (uint32_t j = 0; j < nseg; ++j) len += uvarint_len(sg[j].offset) + 2u + sg[j].len;
  if (len > a.slot) return kCapacity;

  // ---- write
  ByteWriter w;
  w.base = a.wire + i * a.slot;
  w.pad = a.pad;
  w.pos = room;  // framed: bytes [0, 6) stay zero for markData
  w.w0 = w.w1 = w.w2 = w.w3 = 0u;
  w.put(flags);
  if (has_sack) {
    w.put(nr != 0 ? 0x20u : 0u);
    w.put_uvarint(largest);
    const uint32_t d = ufloat16(I.delay_us);
    w.put(d);  // utils.WriteUint16: little endian
    w.put(d >> 8);
    if (nr != 0) w.put(static_cast<uint32_t>(num_ranges - 1));
    w.put_uvarint(first_len);
    uint64_t written = nr != 0 ? 1u : 0u;
    for (uint32_t k = 1; k < nr; ++k) {
      const GapBlocks g = gap_blocks(rg[2 * (k - 1)], rg[2 * k], rg[2 * k + 1]);
      // g.num <= 254 (checked above): the long-gap blocks are bounded by the
      // block-count byte, not by the gap
      for (uint32_t b = 1; b < static_cast<uint32_t>(g.num); ++b) {
        w.put(0xFFu);
        w.put(0u);
      }
      if (g.num != 0) {
        w.put(g.num == 1 ? static_cast<uint32_t>(g.gap) : static_cast<uint32_t>(g.gap % 0xFFu));
        w.put_uvarint(g.length);
      }
      written += g.num;
      if (written >= num_ranges) break;
    }
  }
  if (flags != 0x80u) w.put_uvarint(pn);
  if (sw != 0) w.put_uvarint(sw);
  for (uint32_t j = 0; j < nseg; ++j) {
    const uint32_t L = sg[j].len;
    w.put_uvarint(sg[j].offset);
    w.put(L >> 8);  // binary.BigEndian uint16
    w.put(L);
    const typename Src::Seg src = P.seg(sg[j]);
    if (L < 16u) {
      for (uint32_t k = 0; k < L; ++k) w.put(src.byte(k));
      continue;
    }
    const uint32_t head = (16u - (w.pos & 15u)) & 15u;  // up to the next chunk boundary (< 16 <= L)
    const uint32_t interior = (L - head) & ~15u;         // whole chunks: phase B
    const uint32_t tail = L - head - interior;
    const u32x4 H = src.ld16(0u), T = src.ld16(L - 16u);
    for (uint32_t k = 0; k < head; ++k) w.put(byte_of(H, k));
    w.skip_chunks(interior);
    for (uint32_t k = 0; k < tail; ++k) w.put(byte_of(T, 16u - tail + k));
  }
  w.finish();
  pos0 = static_cast<uint32_t>(seg_start);
  ns = nseg;
  total = static_cast<uint32_t>(len);
  return kOK;
}

template <class Src>
__device__ __forceinline__ typename Src::Stash* src_stash() {
  __shared__ typename Src::Stash s[kEncPacketsPerBlock];
  return s;
}

template <class Src>
__global__ __launch_bounds__(256) void k_packet_encode(typename Src::Args a) {
  __shared__ uint32_t s_pos0[kEncPacketsPerBlock], s_ns[kEncPacketsPerBlock];
  const uint64_t first = blockIdx.x * static_cast<uint64_t>(kEncPacketsPerBlock);
  if (threadIdx.x < kEncPacketsPerBlock) {
    const uint64_t i = first + threadIdx.x;
    uint32_t pos0 = 0, ns = 0, total = 0;
    if (i < a.npk) {
      const Src P(a, i);
      const uint32_t st = P.member() ? encode_header<Src>(a, P, i, pos0, ns, total) : kOK;
      if constexpr (Src::kStash) src_stash<Src>()[threadIdx.x] = P.stash();
      a.status[i] = static_cast<uint8_t>(st);
      a.wire_lens[i] = static_cast<uint16_t>(st == kOK ? total : 0u);
    }
    s_pos0[threadIdx.x] = pos0;
    s_ns[threadIdx.x] = ns;
  }
  __syncthreads();
  constexpr uint32_t kGroups = 256u / kEncLanes;
  const uint32_t grp = threadIdx.x / kEncLanes, hl = threadIdx.x % kEncLanes;
  for (uint32_t t = grp; t < kEncPacketsPerBlock; t += kGroups) {
    const uint32_t ns = s_ns[t];  // 0: no packet, an error status, or no segment
    if (ns == 0) continue;
    const uint64_t i = first + t;
    const ugo_pkt_segment* sg = a.segs + i * a.max_segments;
    const Src P = [&] {
      if constexpr (Src::kStash)
        return Src(src_stash<Src>()[t]);
      else
        return Src(a, i);
    }();
    uint8_t* out = a.wire + i * a.slot;
    uint32_t pos = s_pos0[t];
    for (uint32_t j = 0; j < ns; ++j) {
      const uint32_t L = sg[j].len;
      pos += uvarint_len(sg[j].offset) + 2u;      // segment data at packet bytes [pos, pos + L)
      const typename Src::Seg src = P.seg(sg[j]);  // packet byte x of it is byte x - pos of the segment
      const uint32_t c0 = (pos + 15u) >> 4, c1 = (pos + L) >> 4;  // interior chunks [c0, c1)
      for (uint32_t c = c0 + hl; c < c1; c += 4u * kEncLanes) {
        u32x4 v[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          const uint32_t cc = c + q * kEncLanes;
          if (cc < c1) {
            v[q] = src.ld16(16u * cc - pos);
            if (a.pad) v[q] ^= *reinterpret_cast<const u32x4*>(a.pad + 16u * cc);
          }
        }
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          const uint32_t cc = c + q * kEncLanes;
          if (cc < c1) __builtin_nontemporal_store(v[q], reinterpret_cast<u32x4*>(out + 16u * cc));
        }
      }
      pos += L;
    }
  }
}

}  // namespace

hipError_t launch_packet_decode(const PktArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const uint64_t blocks = (a.npk + 255) / 256;
  launch(kKPacket, k_packet_decode, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_packet_encode(const PktEncArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const uint64_t blocks = (a.npk + kEncPacketsPerBlock - 1) / kEncPacketsPerBlock;
  launch(kKPacketEncode, k_packet_encode<FlatSrc>, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_packet_encode_set(const PktEncSetArgs& a, hipStream_t s) {
  if (a.npk == 0) return hipSuccess;
  const uint64_t blocks = (a.npk + kEncPacketsPerBlock - 1) / kEncPacketsPerBlock;
  launch(kKPacketEncode, k_packet_encode<WinSrc>, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace ugo
