/*
 * ugo_pkt.h -- C-ABI of the batch codec for ugo's packet wire format
 * (SURVEY.md §8f row 4): the decoder, the step after FEC on the receive path,
 * and the encoder, the step before FEC on the send path.
 *
 * Decoder:
 *
 *   Conn.handlePacket  ugo/conn.go:387-419   decrypt, FEC hook, strip the 6-B
 *                                            FEC header of typeData packets,
 *                                            then ugoPacket.decode
 *   ugoPacket.decode   ugo/packet.go:138-177 flags | SACK | packet number |
 *                                            stop-waiting | segments...
 *   parseSack          ugo/packet.go:231-331 (+ validateAckRanges :439-474)
 *   parseSegment       ugo/packet.go:78-100
 *   ReadUfloat16       ugo/utils/float16.go:25-51
 *
 * One call decodes a whole batch of received packets on the GPU (device
 * memory, stream-ordered).  Segment data is not copied: each segment reports
 * where its bytes sit in the packet (zero-copy view of the caller's buffer).
 *
 * Encoder (ugo_fec_packet_encode, below):
 *
 *   Conn.sendPacket        ugo/conn.go:614,634   ugoPacket.encode, crypt.Encrypt
 *   ugoPacket.encode       ugo/packet.go:182-228
 *   sack.write             ugo/packet.go:338-430 (+ numWritableNackRanges :479-505)
 *   segment.write          ugo/packet.go:101-110
 *   WriteUfloat16          ugo/utils/float16.go:54-86
 *
 * One call serialises a whole batch of packets on the GPU from the decoder's
 * own structs and a payload buffer on the device, with the keystream XOR
 * fused in, either ready for the wire or with 6 B of header room in front,
 * as ugo_fec_tx_assemble expects its input.
 */
#ifndef UGO_PKT_H
#define UGO_PKT_H

#include <stddef.h>
#include <stdint.h>

#include "ugo_fec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-packet status: the error ugoPacket.decode (1-6) or ugoPacket.encode
 * (6-9) would return. */
typedef enum ugo_pkt_status {
  UGO_PKT_OK = 0,
  UGO_PKT_EOF = 1,                     /* io.EOF */
  UGO_PKT_UNEXPECTED_EOF = 2,          /* io.ErrUnexpectedEOF */
  UGO_PKT_VARINT_OVERFLOW = 3,         /* "binary: varint overflows a 64-bit integer" */
  UGO_PKT_INVALID_ACK_RANGES = 4,      /* errInvalidAckRanges (ugo/packet.go:42) */
  UGO_PKT_INVALID_FIRST_ACK_RANGE = 5, /* errInvalidFirstAckRange (ugo/packet.go:44) */
  UGO_PKT_CAPACITY = 6,                /* decoded OK, but more ACK ranges / segments than the caller's arrays hold;
                                          encode: n_ranges / n_segments above the caps, or the packet exceeds its slot */
  UGO_PKT_INCONSISTENT_LARGEST_ACKED = 7, /* encode: errInconsistentAckLargestAcked (ugo/packet.go:367-369) */
  UGO_PKT_INCONSISTENT_LOWEST_ACKED = 8,  /* encode: errInconsistentAckLowestAcked (ugo/packet.go:370-372) */
  UGO_PKT_INCONSISTENT_RANGE_COUNT = 9,   /* encode: "BUG: Inconsistent number of ACK ranges written" (ugo/packet.go:425-427) */
  UGO_PKT_OUT_OF_WINDOW = 10              /* ugo_fec_stream_tx_set_encode (ugo_stream.h): a segment outside its send window */
} ugo_pkt_status;

/* Decoded fixed fields of one packet (64 bytes). */
typedef struct ugo_pkt_info {
  uint64_t packet_number;    /* 0 for a pure ACK (flags == 0x80) */
  uint64_t stop_waiting;
  uint64_t largest_acked;    /* SACK fields: valid when flags & 0x80 */
  uint64_t largest_in_order;
  uint64_t delay_us;         /* ufloat16-decoded delay, microseconds */
  uint32_t status;           /* ugo_pkt_status */
  uint32_t payload_off;      /* where the ugoPacket starts in the slot (0, or 6 after a typeData FEC header) */
  uint16_t n_ranges;         /* ACK ranges stored in ranges[i*max_ranges ...] */
  uint16_t n_segments;       /* segments stored in segs[i*max_segments ...] */
  uint8_t flags;             /* ugoPacket flags byte */
  uint8_t fec_flag_lo;       /* low byte of the FEC header flag (framed mode), else 0 */
  uint8_t reserved[10];
} ugo_pkt_info;

/* One stream segment: offset uvarint, BE16 length, data. */
typedef struct ugo_pkt_segment {
  uint64_t offset;
  uint32_t data_off;  /* byte offset of the data within the slot */
  uint16_t len;       /* declared length = len(segment.data) */
  uint16_t avail;     /* bytes present; < len only for a truncated last segment,
                         whose remaining bytes read as zero (bytes.Reader.Read) */
} ugo_pkt_segment;

/* Framed mode: packets carry ugo's 6-B FEC header (FEC enabled).  As in
 * Conn.handlePacket, the header is stripped only for typeData (0xf1) packets;
 * every other packet is decoded from byte 0. */
#define UGO_PKT_FEC_FRAMED 1u

/* Decode npackets received packets: packet i is at pkts + i*slot (16-B aligned
 * slots), lens[i] bytes.  Buffers: device or pinned host memory (zero-copy,
 * as for ugo_fec_rx_assemble); pageable host memory is rejected.  pad (nullable, >= slot bytes) is XORed over each
 * packet from byte 0 first (the fixed-key RC4 Decrypt, ugo/conn.go:390).
 * info[npackets]; ranges[npackets][max_ranges][2] = {first, last} packet
 * numbers, highest range first; segs[npackets][max_segments].  A packet that
 * decodes without error but has more ranges or segments than the caps gets
 * UGO_PKT_CAPACITY (the first max_* are stored); a packet the reference would
 * reject gets the reference's error whatever its size.  Returns a
 * ugo_fec_status (argument / launch errors); per-packet results are in info.
 *
 * Input: lens[i] is an unsigned 16-bit length (a signed view of the same bits
 * is the same length); a lens[i] above slot reads as slot.  Bytes of a slot
 * past lens[i] are never interpreted: a reused ring slot may hold the tail of
 * an older, longer packet there, and no output byte depends on it.  (The slot
 * is loaded in whole 16-B chunks, so all `slot` bytes must be readable.)
 *
 * Output, per packet i -- the call writes info[i] and nothing outside packet
 * i's own rows ranges[i][0 .. max_ranges) and segs[i][0 .. max_segments):
 *
 *   status OK         the whole 64-byte record: fields the packet does not
 *                     carry (no SACK, no stop-waiting, a pure ACK's packet
 *                     number) and reserved are zero; payload_off is 0, or 6
 *                     behind a stripped typeData header; fec_flag_lo is the
 *                     low byte of the FEC flag in framed mode when
 *                     lens[i] >= 6, else 0.  ranges[i][0 .. n_ranges) and
 *                     segs[i][0 .. n_segments) are written, data_off counted
 *                     from the start of the slot; entries at or past those
 *                     counts keep the caller's bytes.
 *   status CAPACITY   the same, with n_ranges / n_segments clamped to the
 *                     caps and the first max_ranges / max_segments entries
 *                     stored (with a cap of 0 the array may be NULL, the
 *                     count is 0 and nothing is stored).
 *   status 1..5       status, payload_off, fec_flag_lo and reserved as above.
 *                     The record's other fields hold what was parsed before
 *                     the error, and the packet's own ranges / segs rows may
 *                     hold entries parsed before it: both unspecified, as
 *                     Conn.handlePacket drops such a packet (ugo/conn.go:
 *                     416-419).  Nothing outside the packet's own rows is
 *                     written.
 *
 * Arguments: UGO_FEC_ERR_INVALID_ARG, before any launch and with no output
 * written, for a NULL ctx, pkts, lens or info; slot 0, not a multiple of 16
 * or above 0xffff; pkts or pad off a 16-B boundary; flag bits other than
 * UGO_PKT_FEC_FRAMED; max_ranges or max_segments above 0xffff; a NULL ranges
 * (segs) with max_ranges (max_segments) > 0; pageable host memory.
 * npackets == 0 is a no-op that returns UGO_FEC_OK. */
int ugo_fec_packet_decode(ugo_fec* ctx, const uint8_t* pkts, size_t slot, const uint16_t* lens, size_t npackets,
                          const uint8_t* pad, unsigned flags, ugo_pkt_info* info, uint64_t* ranges,
                          size_t max_ranges, ugo_pkt_segment* segs, size_t max_segments, void* stream);

/* Encode npackets packets (batch ugoPacket.encode, then crypt.Encrypt): the
 * decoder's output structs are the input, so what ugo_fec_packet_decode
 * produced can be re-encoded and an encoded packet decodes to what went in.
 *
 * Read of info[i]: flags, packet_number, stop_waiting, largest_acked,
 * largest_in_order, delay_us, n_ranges, n_segments (status, payload_off,
 * fec_flag_lo and reserved are ignored).  flags & 0x80 on input means "this
 * packet carries a SACK" (the reference's p.sack != nil).  The flags byte
 * written is the input byte, | 0x40 if stop_waiting != 0, | 0x20 if
 * n_segments != 0; the packet number is written unless that byte is 0x80,
 * stop-waiting when it is non-zero.
 *
 * SACK: ranges[i*max_ranges + k] = {first, last}, highest range first,
 * n_ranges of them (the decoder's layout); n_ranges == 0 is the
 * no-missing-ranges form (first block length largest_acked -
 * largest_in_order + 1).  Otherwise sack.write exactly: type byte 0x20, the
 * block count of numWritableNackRanges, the first block, then gap / length
 * blocks with long gaps split into (0xFF, 0) blocks -- including what the
 * reference does with a gap that is a multiple of 255, with adjacent ranges,
 * with more ranges than fit 255 blocks and with a single range.  delay_us is
 * the caller's (the reference takes time.Now()) and goes through
 * WriteUfloat16.  All packet-number arithmetic wraps at 2^64 like Go's uint64,
 * and the work per packet does not depend on the size of a gap.
 *
 * Segment j is segs[i*max_segments + j]: uvarint offset, BE16 len, then len
 * bytes read from payload + i*payload_stride + data_off (avail is ignored).
 * payload_stride == 0: one flat stream buffer addressed by data_off;
 * payload_stride == slot of a decoded batch re-encodes the decoder's views.
 * payload needs no alignment, must hold every [data_off, data_off + len) the
 * segments name, and must not overlap wire.
 *
 * flags: UGO_PKT_FEC_FRAMED -- the packet starts at byte 6 of its slot, bytes
 * [0, 6) are written as zero and wire_lens[i] includes them: the input
 * ugo_fec_tx_assemble expects (markData fills the header there).  pad must be
 * null in this mode (tx_assemble encrypts after marking), else
 * UGO_FEC_ERR_INVALID_ARG.  Without framing, pad (nullable, >= slot bytes) is
 * XORed over the packet from byte 0 (crypt.Encrypt of Conn.sendPacket).
 *
 * Output: packet i at wire + i*slot, wire_lens[i] bytes.  Exactly bytes
 * [0, round_up(len, 16)) of a slot are written, each 16-B chunk once; bytes
 * [len, round_up(len, 16)) are zero (no pad).  Nothing else in the slot and
 * nothing past it is written.  status[i] holds a ugo_pkt_status: 0, 7, 8, 9
 * as the reference's encode, or UGO_PKT_CAPACITY for n_ranges > max_ranges,
 * n_segments > max_segments or an encoded length (header room included)
 * above slot.  A packet with a non-zero status gets wire_lens[i] = 0 and its
 * slot is not touched.
 *
 * Arguments as for the decoder: slot a multiple of 16 and <= 0xffff, wire and
 * pad 16-B aligned, buffers in device or pinned host memory, npackets == 0 a
 * no-op.  Returns a ugo_fec_status (argument / launch errors). */
int ugo_fec_packet_encode(ugo_fec* ctx, const ugo_pkt_info* info, const uint64_t* ranges, size_t max_ranges,
                          const ugo_pkt_segment* segs, size_t max_segments, const uint8_t* payload,
                          size_t payload_stride, size_t npackets, const uint8_t* pad, unsigned flags, uint8_t* wire,
                          size_t slot, uint16_t* wire_lens, uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UGO_PKT_H */
