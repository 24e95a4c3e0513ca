/*
 * ugo_ack.h -- C-ABI of the receive history on the GPU: the receiver's
 * acknowledgement state, the link between ugo_fec_packet_decode on the receive
 * path and ugo_fec_stream_tx_set_encode on the send path.  What ugo does, per
 * packet and on the host, is
 *
 *   packetReceiver.receivedPacket       ugo/packet_receiver.go:39-96
 *   packetReceiver.receivedStopWaiting  ugo/packet_receiver.go:98-130
 *   packetReceiver.buildSack            ugo/packet_receiver.go:132-163
 *   recvHistory                         ugo/recv_history.go:24-117
 *   their call sites                    ugo/conn.go:446-468, 572-601
 *
 * Added within ABI version 9 (ugo_fec_abi_version() still returns 9): the
 * presence of the ugo_fec_ack_* symbols is the feature test.
 *
 * Here a connection owns a receive history on the device.  One call
 * (ugo_fec_ack_set_receive) runs receivedPacket and receivedStopWaiting for
 * every packet of a decoded batch, for all the connections of a set; one more
 * (ugo_fec_ack_set_attach) is buildSack for every connection, written into the
 * info records and range rows ugo_fec_stream_tx_set_plan left on the device,
 * where ugo_fec_stream_tx_set_encode (or ugo_fec_packet_encode) reads them.
 * The host neither reads the decoded records back nor patches a SACK in.
 *
 * State (device memory, allocated and zeroed by create), Wp = window_packets:
 *   B     a ring bitmap of Wp bits: packet number n is bit n & (Wp-1).  A set
 *         bit means "n received, and some number below it not yet".  It is
 *         meaningful for n in (lio, lio+Wp] and zero everywhere else.
 *   a record, mirrored by ugo_ack_state: lio = largest_in_order (every number
 *   <= lio is received or given up by the peer), lo = largest_observed,
 *   ipb = ignore_below.
 *
 * THE RULE of ugo_fec_ack_set_receive.  Packet i takes part if all of
 *   - info[i].status == UGO_PKT_OK,
 *   - conn_of[i] < nconn (anything else is no connection: the clamp policy of
 *     ugo_stream.h, a lying descriptor is clamped, never followed),
 *   - its member has no err,
 *   - seg_status is NULL, or none of the packet's first min(n_segments,
 *     max_segments) entries seg_status[i*max_segments ..] is
 *     UGO_STREAM_OUT_OF_WINDOW.  A packet that passes the first three tests
 *     and fails this one must not be acknowledged (ugo_stream.h, deviation
 *     (a)): it counts in its member's out_of_window and is otherwise ignored,
 *     its stop-waiting included.
 * Per member, with the packets of the call that take part, in three phases:
 *
 *   1. Floor.  m = the largest non-zero stop_waiting.  If m > ipb:
 *      ipb = m-1, changed = 1, lio = max(lio, m-1), and the bits of all
 *      numbers <= lio are cleared.
 *   2. Packets.  For every packet_number n != 0:
 *        n <= lio, or bit n already set      old++ (a second copy of a number
 *                                            within the call is one of these)
 *        n > lio + Wp                        out_of_window++
 *        otherwise                           set bit n, fresh++, changed = 1,
 *                                            lo = max(lo, n)
 *   3. Advance.  While bit lio+1 is set: lio++, clear the bit.  Then
 *      lo = max(lo, lio); outstanding = the number of set bits; if lo rose in
 *      this call lo_time_us = now_us; if outstanding >
 *      UGO_ACK_MAX_OUTSTANDING, err = UGO_ACK_TOO_MANY_OUTSTANDING
 *      (errTooManyOutstandingReceivedPackets): the member is inert for receive
 *      and attach from then on.
 *
 * A member none of whose packets takes part keeps its bitmap and its record
 * bit for bit, but for the out_of_window count of the fourth test.  Nothing
 * a call leaves behind depends on the order of the packets inside it.  Applied
 * packet by packet (every packet a call of its own) the rule gives the same
 * bitmap, lio, lo, ipb, lo_time_us, outstanding and changed as long as neither
 * form meets the window bound or the limit of step 3; at those two it need not
 * (deviation (d): a number within Wp of the call's floor but not of the lio
 * before it is recorded here and out of window packet by packet; a count above
 * the limit that later packets of the call bring down again is no error here).
 * How the packets of a call divide into fresh and old follows the phase order
 * in any case (a number that the call's own floor passes counts as old).
 *
 * DEVIATIONS from the reference, all on purpose:
 *   (a) contiguous advance.  When packet lio+1 arrives, receivedPacket
 *       (:69-75) walks i up to largestObserved and does
 *       largestInOrderObserved++ for every i it finds, without stopping at the
 *       first missing one: after 1, 3, 5, then 2 it stands at 4, and the next
 *       SACK acknowledges packet 4, which never arrived.  (The loop of
 *       receivedStopWaiting, :114-122, stops as it should.)  Step 3 advances
 *       over received numbers only.
 *   (b) lo never falls below lio.  In the reference a stop-waiting past
 *       largestObserved leaves largestObserved below largestInOrderObserved;
 *       gcReceivedTimes then deletes receivedTimes[largestObserved], buildSack
 *       returns errTimeLost and sendPacket fails the connection.
 *   (c) the window bound of step 2: the reference's map has no bound but (d).
 *       A number past lio + Wp is not recorded and must be sent again.
 *   (d) the phase order inside a call (floor, packets, advance), and the
 *       error judged once after the call on the rule's count of set bits; the
 *       reference judges len(receivedTimes) after each packet, a map it
 *       prunes only on a stop-waiting.
 *   (e) ipb is m - 1 and nothing else.  The loop of receivedStopWaiting also
 *       raises ignorePacketsBelow to largestInOrderObserved - 1 as it
 *       advances (the advance of receivedPacket does not), so which later
 *       stop-waitings the reference ignores depends on the order of arrival
 *       inside a batch.  ipb <= ignorePacketsBelow always: a stop-waiting in
 *       between sets changed here and not there, one more ACK of the same
 *       content and never one fewer.
 * Checked on the CPU against a restatement of packetReceiver and recvHistory
 * (tests/ack_ref.py, tests/test_ack.py): largestAcked, largestInOrder and
 * ackRanges equal after every call wherever the reference meets neither (a)
 * nor (b), and up to that event elsewhere, stateChanged equal but for (e); and
 * on the device against one rule per member (tests/ack_harness.py).
 */
#ifndef UGO_ACK_H
#define UGO_ACK_H

#include <stddef.h>
#include <stdint.h>

#include "ugo_pkt.h"
#include "ugo_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel class of every launch of this header (ugo_fec_launch_time.kernel). */
#define UGO_FEC_KERNEL_ACK 12

#define UGO_ACK_MIN_WINDOW 1024u
#define UGO_ACK_MAX_WINDOW (1u << 20)
#define UGO_ACK_MAX_OUTSTANDING 1000u
#define UGO_ACK_TOO_MANY_OUTSTANDING 1u /* ugo_ack_state.err */

/* ugo_fec_ack_set_attach, attached[c] */
#define UGO_ACK_NOT_ATTACHED 0u
#define UGO_ACK_ATTACHED 1u
#define UGO_ACK_TRUNCATED 2u /* more runs than max_ranges holds: the highest are kept */

/* Host mirror of a receive history's record (64 bytes). */
typedef struct ugo_ack_state {
  uint64_t largest_in_order; /* lio: packetReceiver.largestInOrderObserved */
  uint64_t largest_observed; /* lo:  packetReceiver.largestObserved */
  uint64_t ignore_below;     /* ipb: packetReceiver.ignorePacketsBelow */
  uint64_t lo_time_us;       /* now_us of the call in which lo last rose */
  uint64_t fresh;            /* counters, cumulative over calls */
  uint64_t old;
  uint64_t out_of_window;
  uint32_t outstanding;      /* set bits: received above lio */
  uint8_t changed;           /* packetReceiver.stateChanged */
  uint8_t err;               /* 0 or UGO_ACK_TOO_MANY_OUTSTANDING */
  uint8_t reserved[2];
} ugo_ack_state;

typedef struct ugo_ack_rx ugo_ack_rx;
typedef struct ugo_ack_rx_set ugo_ack_rx_set;

/* A receive history of window_packets numbers (a power of two in
 * [UGO_ACK_MIN_WINDOW, UGO_ACK_MAX_WINDOW]) on ctx's device, everything
 * zeroed.  ctx must outlive it. */
int ugo_fec_ack_rx_create(ugo_fec* ctx, size_t window_packets, ugo_ack_rx** out);
void ugo_fec_ack_rx_destroy(ugo_ack_rx* rx);

/* The record, after synchronising the streams of the sets it is a member of. */
int ugo_fec_ack_rx_state(ugo_ack_rx* rx, ugo_ack_state* host_out);

/* The bitmap itself (device memory, window_packets / 64 words; packet number n
 * is bit n & 63 of word (n & (window_packets-1)) >> 6), for tests. */
int ugo_fec_ack_rx_bitmap(ugo_ack_rx* rx, uint64_t** bitmap_dev, size_t* window_packets);

/* An ordered list of existing receive histories (their windows may differ);
 * packet i of a batch belongs to member conn_of[i].  Rules as for
 * ugo_fec_stream_set_create: the set does not own its members (destroy the set
 * first), members cannot be added or removed, create uploads one table entry
 * per member, once, so the per-call entry points make no host-to-device copy
 * and no host synchronisation.  UGO_FEC_ERR_INVALID_ARG for a NULL argument,
 * nconn == 0 or nconn > 2^20, a NULL member, a member of another context, or
 * the same ugo_ack_rx listed twice.  There are no single-connection entry
 * points: a set of one member is that form.
 *
 * Every operand array is in device or pinned host memory (pageable memory is
 * rejected); every call is stream-ordered; the caller orders the calls on one
 * set.  Argument errors return UGO_FEC_ERR_INVALID_ARG before any launch, with
 * nothing written.  Every launch reports as UGO_FEC_KERNEL_ACK. */
int ugo_fec_ack_set_create(ugo_fec* ctx, ugo_ack_rx* const* rxs, size_t nconn, ugo_ack_rx_set** out);
void ugo_fec_ack_set_destroy(ugo_ack_rx_set* set);

/* THE RULE above for a decoded batch: info[npackets] as ugo_fec_packet_decode
 * wrote it (packet_number, stop_waiting, status and n_segments are read),
 * conn_of[npackets] (uint32) the member of each packet, seg_status (nullable,
 * uint8 [npackets][max_segments], any alignment) as ugo_fec_stream_set_deliver
 * wrote it.  info is 16-B aligned (the records are read in 16-B pieces);
 * max_segments <= 0xffff, and >= 1 with a seg_status; npackets <= 2^31;
 * npackets == 0 is a no-op.  Only the members' bitmaps and records are
 * written. */
int ugo_fec_ack_set_receive(ugo_ack_rx_set* set, const ugo_pkt_info* info, const uint32_t* conn_of, size_t npackets,
                            const uint8_t* seg_status, size_t max_segments, uint64_t now_us, void* stream);

/* changed = 1 for every member c with flags[c] != 0 (uint8 [nconn]): a
 * retransmitted packet carried an ACK (ugo/conn.go:558-560). */
int ugo_fec_ack_set_touch(ugo_ack_rx_set* set, const uint8_t* flags, void* stream);

/* buildSack for every member, written where ugo_fec_stream_tx_set_encode reads
 * it.  first_packet (uint64 [nconn]), n_packets (uint32 [nconn]) and total
 * (uint64 [1]) are ugo_fec_stream_tx_set_plan's outputs, still on the device;
 * info [max_packets], ranges [max_packets][max_ranges][2] and conn_of
 * [max_packets] are the arrays the encoder will be given.  may_ack_only
 * (nullable, uint8 [nconn]) is the host's delayed-ACK decision
 * (ugo/conn.go:587-593).
 *
 * Every member with changed != 0 and no err gets a target t:
 *   n_packets[c] > 0     t = first_packet[c]: the SACK rides on the member's
 *                        first planned packet
 *   else, with may_ack_only non-NULL and may_ack_only[c] != 0
 *                        t = *total + k, k = the number of such members before
 *                        c: an ACK-only packet is appended, and its whole
 *                        64-byte record is written -- zeros, flags = 0x80 --
 *                        and conn_of[t] = c
 *   otherwise            none: the member stays changed.
 * THE CLAMP: a target t >= max_packets is no target.
 *
 * At info[t]: flags |= 0x80, largest_acked = lo, largest_in_order = lio,
 * delay_us = now_us - lo_time_us (0 if that is negative), n_ranges, and the
 * row ranges[t*max_ranges ..]: the maximal runs of set bits as {first, last},
 * highest first, then {lio, lio}; with no run n_ranges = 0 and no row is
 * written (the reference's len(ackRanges) > 1).  When runs + 1 > max_ranges
 * the highest max_ranges - 1 runs and {lio, lio} are kept and attached[c] =
 * UGO_ACK_TRUNCATED: a received packet may be sent again, a missing one is
 * never acknowledged; with max_ranges < 2 that leaves largest_acked = lio and
 * n_ranges = 0 (ranges may then be NULL if max_ranges == 0).  Otherwise
 * attached[c] = UGO_ACK_ATTACHED; a member without a target gets
 * UGO_ACK_NOT_ATTACHED (uint8 [nconn], every entry is written).  changed is
 * cleared for exactly the attached members.  *total_out (uint64, may be total
 * itself) = *total + the number of ACK-only records appended.  Nothing else in
 * info, ranges or conn_of is written; the SACK passes the encoder's checks
 * 7-9 by construction.  max_ranges <= 0xffff, max_packets <= 2^31, info 16-B
 * aligned. */
int ugo_fec_ack_set_attach(ugo_ack_rx_set* set, uint64_t now_us, const uint64_t* first_packet,
                           const uint32_t* n_packets, const uint64_t* total, const uint8_t* may_ack_only,
                           size_t max_packets, ugo_pkt_info* info, uint64_t* ranges, size_t max_ranges,
                           uint32_t* conn_of, uint64_t* total_out, uint8_t* attached, void* stream);

/* The nconn records, in set order, after synchronising the stream of the last
 * call on the set. */
int ugo_fec_ack_set_state(ugo_ack_rx_set* set, ugo_ack_state* host_out /* [nconn] */);

#ifdef __cplusplus
}
#endif
#endif /* UGO_ACK_H */
