/*
 * ugo_sent.h -- C-ABI of the sent history on the GPU: the sender's half of
 * ARQ, the link between ugo_fec_stream_tx_set_encode / ugo_fec_packet_decode
 * and ugo_fec_stream_tx_set_retransmit / _release.  What ugo does, per packet
 * and on the host, is
 *
 *   packetSender.sentPacket                     ugo/packet_sender.go:135-163
 *   packetSender.receivedAck, ackPacket,
 *     nackPacket, queuePacketForRetransmission  ugo/packet_sender.go:66-133, 165-260
 *   packetSender.checkRTO, getRTO               ugo/packet_sender.go:314-358
 *   packetSender.dequeuePacketForRetransmission ugo/packet_sender.go:262-285
 *   its call site                               ugo/conn.go:554-568
 *   stopWaitingManager                          ugo/stop_waiting.go
 *
 * Added within ABI version 9 (ugo_fec_abi_version() still returns 9): the
 * presence of the ugo_fec_sent_* symbols is the feature test.
 *
 * Here a connection owns a sent history on the device.  What stays on the host
 * is congestion control (ugo/congestion/), the RTT filter and the clocks: they
 * are fed from one 64-byte event row per connection and call, and hand
 * RetransmissionDelay() and now_us in.  No per-packet record is read back.
 *
 * State (device memory, allocated and zeroed by create), Ws = window_packets,
 * S = seg_cap:
 *   slots  a ring of Ws ugo_sent_slot (32 B each): packet number n lives at
 *          n & (Ws-1); packet_number == 0 is an empty slot, and an empty slot
 *          is 32 zero bytes.  The occupant's number makes a collision
 *          detectable.
 *   segs   a ring [Ws][S] of ugo_stream_tx_rq_entry (16 B each): the stored
 *          packet's segments {offset, len, 0}, entries at or past n_segments
 *          zero.  Freeing a slot leaves its segment row as it is.
 *   a record, mirrored by ugo_sent_state (160 B).
 * Invariants: every occupied number is in (last_sent - Ws, last_sent] and
 * >= scan_from; lio + 1 is in flight or lio == last_sent after set_ack / set_rto.
 *
 * THE ORDER a caller keeps per batch, on one stream:
 *   set_plan, ugo_fec_ack_set_attach, ugo_fec_sent_set_attach, set_encode,
 *   ugo_fec_sent_set_record, [the decoded batch of the other direction:]
 *   ugo_fec_sent_set_ack, ugo_fec_sent_set_rto, ugo_fec_sent_set_drain,
 *   ugo_fec_stream_tx_set_retransmit, ugo_fec_ack_set_touch,
 *   ugo_fec_stream_tx_set_release.
 *
 * THE RULE.  All calls are per member and phase-ordered inside a call; a
 * member with err != 0 is inert in every call (its outputs are written as
 * stated, its state never changes).  Nothing a call leaves behind depends on
 * the order of the packets inside it, but for the two lowest-index tie-breaks
 * stated below.
 *
 * set_record (sentPacket), after set_encode.  Packet i takes part if
 * conn_of[i] < nconn, info[i].packet_number != 0, status[i] == 0,
 * wire_lens[i] != 0 and its member has no err.  A member that has stored
 * nothing yet (last_sent == 0 and lio == 0) first adopts the lowest number m of
 * its packets that take part: lio = m - 1, least_unacked = scan_from = m (a
 * connection need not start at 1).  Then, with n a packet's number and lio as
 * it stands now:
 *   n <= lio                           stale++, not stored
 *   n > lio + Ws, or the slot holds    err = UGO_SENT_TOO_MANY_TRACKED (the
 *     another number                   window takes the place of
 *                                      maxTrackedSentPackets); the packets of
 *                                      the call that did fit are stored
 *   the slot holds n                   duplicates++ (errDuplicatePacketNumber),
 *                                      not stored; of several copies of n in
 *                                      one call the lowest index is the one
 *                                      that may be stored, the others are
 *                                      duplicates
 *   otherwise                          the slot and its segment row are stored
 * A stored slot: sent_us = now_us, len = wire_lens[i], n_segments =
 * min(info.n_segments, max_segments), state in flight, missing 0, bits = 0x80
 * if info.flags & 0x80, | 0x40 if info.stop_waiting != 0, min_offset = the
 * lowest offset of its segments (UINT64_MAX with none).  Per member:
 * bytes_in_flight += len, tracked++, last_sent = max(last_sent, n), and
 * last_sent_us = now_us if anything was stored.
 *
 * set_ack (receivedAck) for a decoded batch.  Packet i carries an ACK if
 * info[i].status == UGO_PKT_OK, flags & 0x80, conn_of[i] < nconn and the
 * member has no err.  It uses min(n_ranges, max_ranges) rows (a lying
 * descriptor is clamped, never followed).  la = largest_acked, lio_a =
 * largest_in_order, w = packet_number.
 *   1. Valid: la <= last_sent (else unsent_acks++), and w == 0 or
 *      w > largest_with_ack as it stood before the call.
 *   2. largest_with_ack = max(itself, every valid w).
 *   3. Accepted: valid and la > max(largest_acked, lio) as they stood before
 *      the call; of several with the same la only the lowest batch index.  If
 *      no ACK is accepted nothing else changes.
 *   4. largest_acked = the highest accepted la.
 *   5. RTT sample: if that number's slot is occupied the event row gets
 *      rtt_us = now_us - sent_us (0 if negative) and that ACK's delay_us, and
 *      rto_count = 0.  One sample per member and call.
 *   6. Marks.  What an accepted ACK acknowledges: every n <= la with
 *      n <= lio_a, or (no rows) every n <= la, or n inside one of its rows.
 *      Rows come highest first; row k counts only below the lowest `first` of
 *      the rows before it, and the n <= lio_a part only below the lowest
 *      `first` of all rows -- for the rows ugo_fec_packet_decode and
 *      ugo_fec_ack_set_attach write that changes nothing, a row out of order
 *      is clamped.  For every occupied slot n <= largest_acked:
 *        acked(n)  some accepted ACK acknowledges n
 *        nacks(n)  the number of accepted ACKs with n <= la that do not
 *      acked: the slot is freed, tracked--, acked_packets / acked_bytes rise;
 *      bytes_in_flight -= len only if it was in flight.  Otherwise missing =
 *      min(255, missing + nacks), and if missing > 3 and in flight: state =
 *      queued, bytes_in_flight -= len, sw_pending = 1, lost_packets /
 *      lost_bytes rise.
 *   7. Advance.  lio = the largest n <= last_sent with no in-flight slot in
 *      (lio, n]; least_unacked = lio + 1.
 *   8. Every member's event row is written, whole.
 *
 * set_rto (checkRTO).  rto = delay_us[c] (0: 500 ms; above 60 s: 60 s), at
 * least 200 ms, << min(rto_count, 16), at most 60 s.  If last_sent_us != 0,
 * now_us >= last_sent_us + rto and a slot in (lio, last_sent] is in flight:
 * the lowest such becomes queued as in 6, lio advances as in 7, last_sent_us =
 * now_us, rto_count++ and fired[c] = 1.  With nothing in flight nothing
 * changes (the reference's loop finds no packet).  Every fired[c] is written.
 *
 * set_drain (dequeuePacketForRetransmission, AddSegmentForRetransmission,
 * conn.go:554-568): see the entry point.  set_attach (GetStopWaitingFrame):
 * see the entry point.
 *
 * DEVIATIONS from the reference, all on purpose:
 *   (a) every distinct snapshot counts.  The reference drops an ACK whose
 *       largestAcked an earlier ACK of the batch has passed; the rule equals
 *       the reference run on the call's ACKs sorted by largestAcked.
 *   (b) a queued packet under lio is freed by an ACK that covers it.  In the
 *       reference receivedAck's first loop starts at largestInOrderAcked,
 *       which queuePacketForRetransmission has moved past it: it is sent
 *       again.
 *   (c) the window bound and a slot collision are the error, in place of the
 *       count of 2,000 (CheckForError).
 *   (d) one RTT sample per call; a packet lost and acknowledged in one call
 *       reports as acknowledged only.
 *   (e) missing saturates at 255.
 *   (f) retransmission order is ascending, everything queued at once (the
 *       reference pops its slice as a stack, one packet per sendPacket).
 *   (g) no stop-waiting-only packet: a pending stop-waiting waits for a
 *       planned packet.
 *   (h) lio passes every number no longer in flight (step 7); ackPacket
 *       advances only over a number it is called for.
 *   (i) acked_packets counts every freed slot, as the reference's ackedPackets
 *       vector does; totalAcked there skips retransmitted ones.
 *   (j) which packets are tracked is decided by the number: packet_number 0
 *       takes no part.  An ACK-only record as ugo_fec_ack_set_attach writes it
 *       (flags 0x80) has packet_number 0 and is not stored, as sentPacket skips
 *       flags == ackFlag; a caller that gives such a record a number of its own
 *       has it tracked and, if lost, drained as no entries with touch[c] = 1.
 * Checked on the CPU against a restatement of packetSender (tests/sent_ref.py,
 * tests/test_sent.py) and on the device against one rule per member
 * (tests/sent_harness.py).
 */
#ifndef UGO_SENT_H
#define UGO_SENT_H

#include <stddef.h>
#include <stdint.h>

#include "ugo_pkt.h"
#include "ugo_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel class of every launch of this header (ugo_fec_launch_time.kernel). */
#define UGO_FEC_KERNEL_SENT 13

#define UGO_SENT_MIN_WINDOW 1024u
#define UGO_SENT_MAX_WINDOW (1u << 20)
#define UGO_SENT_MAX_SEG_CAP 16u
#define UGO_SENT_TOO_MANY_TRACKED 1u /* ugo_sent_state.err */
#define UGO_SENT_RETRANSMIT_THRESHOLD 3u

#define UGO_SENT_IN_FLIGHT 0u /* ugo_sent_slot.state */
#define UGO_SENT_QUEUED 1u

#define UGO_SENT_RTO_DEFAULT_US 500000ull
#define UGO_SENT_RTO_MIN_US 200000ull
#define UGO_SENT_RTO_MAX_US 60000000ull

/* One entry of the slot ring (32 bytes). */
typedef struct ugo_sent_slot {
  uint64_t packet_number; /* 0: empty, and then every byte is zero */
  uint64_t sent_us;
  uint64_t min_offset;    /* lowest stream offset of its segments, UINT64_MAX with none */
  uint32_t len;           /* ugoPacket.Length: the wire length */
  uint8_t state;          /* UGO_SENT_IN_FLIGHT / UGO_SENT_QUEUED */
  uint8_t missing;        /* missingCount, saturating */
  uint8_t n_segments;
  uint8_t bits;           /* 0x80 the packet carried an ACK, 0x40 a stop-waiting */
} ugo_sent_slot;

/* Host mirror of a sent history's record (160 bytes). */
typedef struct ugo_sent_state {
  uint64_t last_sent;        /* lastSentPacketNumber (the highest stored) */
  uint64_t lio;              /* largestInOrderAcked */
  uint64_t largest_acked;
  uint64_t largest_with_ack; /* largestReceivedPacketWithAck */
  uint64_t least_unacked;    /* stopWaitingManager.largestLeastUnackedSent */
  uint64_t bytes_in_flight;
  uint64_t last_sent_us;     /* lastSentPacketTime, 0 = never */
  uint64_t scan_from;        /* no occupied slot holds a number below it (1 after create; the lowest
                                occupied number, or last_sent + 1, after an accepting set_ack and set_drain) */
  uint64_t acked_packets;    /* counters, cumulative over calls */
  uint64_t acked_bytes;
  uint64_t lost_packets;
  uint64_t lost_bytes;
  uint64_t duplicates;
  uint64_t unsent_acks;
  uint64_t stale;
  uint32_t tracked;          /* occupied slots */
  uint32_t queued;           /* of them queued for retransmission */
  uint32_t queued_segments;  /* the segments of the queued slots */
  uint32_t rto_count;        /* consecutiveRTOCount */
  uint8_t sw_pending;        /* stopWaitingManager.state */
  uint8_t err;               /* 0 or UGO_SENT_TOO_MANY_TRACKED */
  uint8_t reserved[22];
} ugo_sent_state;

/* What set_ack tells the host of one member (64 bytes): the arguments of
 * OnCongestionEvent and UpdateRTT. */
typedef struct ugo_sent_event {
  uint64_t rtt_us;          /* valid with has_rtt */
  uint64_t delay_us;        /* the sampled ACK's delay_us */
  uint64_t acked_bytes;     /* of this call */
  uint64_t lost_bytes;
  uint64_t bytes_in_flight; /* after the call */
  uint64_t largest_acked;   /* after the call */
  uint32_t acked_packets;
  uint32_t lost_packets;
  uint8_t accepted;         /* an ACK of this call was accepted */
  uint8_t has_rtt;
  uint8_t reserved[6];
} ugo_sent_event;

typedef struct ugo_sent_tx ugo_sent_tx;
typedef struct ugo_sent_tx_set ugo_sent_tx_set;

/* A sent history of window_packets numbers (a power of two in
 * [UGO_SENT_MIN_WINDOW, UGO_SENT_MAX_WINDOW]) and seg_cap segments per packet
 * (1 .. UGO_SENT_MAX_SEG_CAP) on ctx's device, everything zeroed but
 * scan_from = 1.  ctx must outlive it. */
int ugo_fec_sent_tx_create(ugo_fec* ctx, size_t window_packets, size_t seg_cap, ugo_sent_tx** out);
void ugo_fec_sent_tx_destroy(ugo_sent_tx* tx);

/* The rings themselves (device memory), for tests: window_packets slots;
 * window_packets * seg_cap segment entries. */
int ugo_fec_sent_tx_slots(ugo_sent_tx* tx, ugo_sent_slot** slots_dev, size_t* window_packets);
int ugo_fec_sent_tx_segments(ugo_sent_tx* tx, ugo_stream_tx_rq_entry** segs_dev, size_t* window_packets,
                             size_t* seg_cap);

/* The two scratch rings of set_record / set_ack (device memory, 2 * window_packets
 * 32-bit words: the difference ring, then the claim ring), for tests: every
 * word is zero between calls. */
int ugo_fec_sent_tx_scratch(ugo_sent_tx* tx, uint32_t** words_dev, size_t* n_words);

/* An ordered list of existing sent histories (windows and seg_caps may
 * differ).  Rules as for ugo_fec_ack_set_create: the set does not own its
 * members (destroy the set first), no member twice, 1 <= nconn <= 2^20, one
 * table entry per member uploaded once.  There are no single-connection entry
 * points.  Every operand array is in device or pinned host memory; every call
 * is stream-ordered with no host copy and no synchronisation; the caller
 * orders the calls on one set.  Argument errors return UGO_FEC_ERR_INVALID_ARG
 * before any launch with nothing written.  Every launch reports as
 * UGO_FEC_KERNEL_SENT. */
int ugo_fec_sent_set_create(ugo_fec* ctx, ugo_sent_tx* const* txs, size_t nconn, ugo_sent_tx_set** out);
void ugo_fec_sent_set_destroy(ugo_sent_tx_set* set);

/* set_record of THE RULE.  info [npackets], segs [npackets][max_segments] and
 * conn_of [npackets] as set_plan left them, wire_lens (uint16 [npackets]) and
 * status (uint8 [npackets]) as set_encode wrote them.  info and segs 16-B
 * aligned; 1 <= max_segments <= the smallest seg_cap of the set, else an
 * argument error; npackets <= 2^31; npackets == 0 is a no-op. */
int ugo_fec_sent_set_record(ugo_sent_tx_set* set, const ugo_pkt_info* info, const ugo_pkt_segment* segs,
                            size_t max_segments, const uint32_t* conn_of, const uint16_t* wire_lens,
                            const uint8_t* status, size_t npackets, uint64_t now_us, void* stream);

/* set_ack of THE RULE.  info [npackets] and ranges [npackets][max_ranges][2]
 * as ugo_fec_packet_decode wrote them (ranges may be NULL with max_ranges ==
 * 0), conn_of [npackets]; events [nconn] is written whole for every member,
 * also with npackets == 0.  max_ranges <= 0xffff, npackets <= 2^31, info 16-B
 * aligned. */
int ugo_fec_sent_set_ack(ugo_sent_tx_set* set, const ugo_pkt_info* info, const uint64_t* ranges, size_t max_ranges,
                         const uint32_t* conn_of, size_t npackets, uint64_t now_us, ugo_sent_event* events,
                         void* stream);

/* set_rto of THE RULE.  delay_us uint64 [nconn], fired uint8 [nconn]. */
int ugo_fec_sent_set_rto(ugo_sent_tx_set* set, const uint64_t* delay_us, uint64_t now_us, uint8_t* fired,
                         void* stream);

/* Everything queued leaves, in the form ugo_fec_stream_tx_set_retransmit
 * takes: conn_of (uint32), offset (uint64), len (uint32), each [max_entries].
 * count[c] = queued_segments of member c (0 with err), start[c] = the
 * exclusive sum of count over the members before c.  THE CLAMP is by whole
 * members: a member with start[c] + count[c] > max_entries drains nothing and
 * stays queued.  A member that drains writes the segments of its queued slots,
 * in ascending packet number, from entry start[c]; the slots are freed
 * (tracked--, queued = queued_segments = 0); touch[c] = 1 if one of them had
 * the ACK bit (the input of ugo_fec_ack_set_touch), else 0; sw_pending = 1 if
 * one had the stop bit.  *n_entries (uint64) = the entries written, which are
 * compact; conn_of[*n_entries .. max_entries) = UGO_STREAM_NO_CONN, so the
 * list is non-decreasing and m = max_entries may be passed on without reading
 * a count; offset and len keep the caller's bytes there.  upto[c] (uint64) =
 * the lowest min_offset of the slots still occupied after the drain,
 * UINT64_MAX with none (the input of ugo_fec_stream_tx_set_release, which
 * clamps it); scan_from = the lowest number still occupied, or last_sent + 1.
 * A member with err: touch[c] = 0, upto[c] = 0, nothing else.  touch and upto
 * [nconn] are written whole.  max_entries <= 2^31; with max_entries == 0 the
 * three lists may be NULL. */
int ugo_fec_sent_set_drain(ugo_sent_tx_set* set, size_t max_entries, uint32_t* conn_of, uint64_t* offset,
                           uint32_t* len, uint64_t* n_entries, uint8_t* touch, uint64_t* upto, void* stream);

/* GetStopWaitingFrame, after set_plan: for a member with sw_pending, no err,
 * n_packets[c] > 0 and first_packet[c] < max_packets:
 * info[first_packet[c]].stop_waiting = least_unacked, sw_pending = 0,
 * attached[c] = 1 (the encoder sets 0x40 itself).  Every other member gets
 * attached[c] = 0 and stays as it is.  Nothing else in info is written.
 * first_packet uint64 [nconn], n_packets uint32 [nconn], attached uint8
 * [nconn]; info 16-B aligned, max_packets <= 2^31. */
int ugo_fec_sent_set_attach(ugo_sent_tx_set* set, const uint64_t* first_packet, const uint32_t* n_packets,
                            size_t max_packets, ugo_pkt_info* info, uint8_t* attached, void* stream);

/* The nconn records, in set order, after synchronising the stream of the last
 * call on the set. */
int ugo_fec_sent_set_state(ugo_sent_tx_set* set, ugo_sent_state* host_out /* [nconn] */);

#ifdef __cplusplus
}
#endif
#endif /* UGO_SENT_H */
