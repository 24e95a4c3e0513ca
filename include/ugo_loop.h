/*
 * ugo_loop.h -- C-ABI of the connection loop on the GPU: the timers, FIN / RST
 * and the exits of a set of connections.  What ugo does, per connection and on
 * the host, is
 *
 *   Conn.run, exitLoop           ugo/conn.go
 *   Close, SetLinger,
 *   SetACKNoDelay                ugo/conn.go:283-353
 *   resetTimer                   ugo/conn.go:358-385
 *   the top of handlePacket      ugo/conn.go:388-444
 *   resetConn                    ugo/conn.go:500-512
 *   the top of sendPacket        ugo/conn.go:521-552, 582-593, 632
 *   sendFin, sendRst             ugo/conn.go
 *
 * Added within ABI version 9 (ugo_fec_abi_version() still returns 9): the
 * presence of the ugo_fec_loop_* symbols is the feature test.
 *
 * Conventions as in ugo_cc.h: operands in device or pinned host memory; every
 * call stream-ordered with no host copy and no synchronisation; argument errors
 * return UGO_FEC_ERR_INVALID_ARG before any launch with nothing written; output
 * arrays are written whole; descriptors that lie are clamped, never followed;
 * the per-call scratch lives in the set and is idle after every call.  With
 * these calls the host hands in now_us and reads back two sizes (*total_out,
 * *n_exits) and one deadline.
 *
 * THE ORDER a caller keeps per batch, on one stream:
 *   ugo_fec_listen_route, ugo_fec_packet_decode, ugo_fec_loop_set_receive, the
 *   RX stages as before, ugo_fec_cc_* / ugo_fec_sent_* as before,
 *   ugo_fec_loop_set_check, ugo_fec_stream_tx_set_plan,
 *   ugo_fec_loop_set_append, ugo_fec_ack_set_attach, ugo_fec_sent_set_attach,
 *   ugo_fec_stream_tx_set_encode, ugo_fec_sent_set_record,
 *   ugo_fec_loop_set_sent.
 * ugo_fec_loop_set_close goes anywhere between two batches' calls.
 *
 * THE RULE, per member.  A member is live until exited = 1; an exited member is
 * inert in every call: its record never changes again but for dropped,
 * reported and what ugo_fec_loop_set_append does to a member whose FIN or RST is
 * still pending (pending, fin_sent, linger_deadline_us).
 *
 * ugo_fec_loop_set_receive (the top of handlePacket; the only per-packet call).
 * For a member c live at the start of the call, over its packets in batch
 * order: a packet ends the loop if its status is 1..5 (decode failed,
 * conn.go:416-419), or its status is OK or CAPACITY and its flags are 0x90
 * (ACK|FIN, conn.go:434) or 0x08 (RST, conn.go:441).  E is the lowest index of
 * such a packet; packets of c below E (all of them without E) are handled.
 *   last_activity_us = now_us if c has a handled packet or an E (conn.go:388);
 *   origin_ack_us = now_us if it is 0 and a handled packet has packet_number
 *   != 0 (conn.go:421-425);
 *   fin_rcvd = 1 if a handled packet has flags & 0x10, or E is an ACK|FIN
 *   (conn.go:429-432);
 *   E exits the member, exit_us = now_us: ACK|FIN with reason PEER_ACK_FIN, RST
 *   with PEER_RST, a decode error with BAD_PACKET and pending = RST.
 * conn_of[i] = UGO_STREAM_NO_CONN for every packet of c at or past E, and for
 * every packet of a member that had exited before the call; both count in
 * dropped.  Entries of conn_of that are >= nconn stay as they are.  Nothing
 * else is written.  Every later stage skips a packet marked so, so a connection
 * stops where the reference's loop returns.
 *
 * ugo_fec_loop_set_close (Close, SetLinger, SetACKNoDelay of many members).
 * Bits of how[c]: 1 close -- a member not yet closed gets closed = 1 and, with
 * linger_us[c] > 0, linger_deadline_us = now_us + linger_us[c].  2 abort --
 * the linger == 0 branch: exit with reason ABORT, pending = RST.  Neither
 * changes a closed member: Close on a closed connection returns before it
 * looks at linger.  4 sets ack_no_delay, 8 clears it.  Abort wins over close; 8
 * is applied after 4.
 *
 * ugo_fec_loop_set_check (the top of sendPacket, the tail of run).  The first
 * that matches exits the member with pending = RST, exit_us = now_us:
 *   1. the receive window's err            STREAM_ERR
 *   2. the receive history's err           ACK_ERR
 *   3. the sent history's err              SENT_ERR
 *   4. rto_count > max_retries             FAILURES
 *   5. closed, linger_deadline_us != 0 and now_us >= linger_deadline_us  LINGER
 *   6. now_us - last_activity_us >= idle_us (now_us >= last_activity_us)  IDLE
 * Then, for a member still live: closed && !fin_sent with the send window's
 * tail == write_pos, its rq_len == 0 and the sent history's tracked == 0 sets
 * pending = FIN; closed && fin_rcvd && (fin_sent || pending == FIN) exits with
 * reason CLOSED, and the FIN still goes out (conn.go:523-539).
 * Outputs for every member: budget[c] = 0 if the member is exited, fin_sent or
 * pending != 0, else unchanged; may_ack_only[c] = 0 if the member is exited,
 * else ack_no_delay || origin_ack_us == 0 || now_us - origin_ack_us >
 * ack_delay_us (an unset originAckTime reads as long ago, conn.go:587).
 *
 * ugo_fec_loop_set_append (sendFin / sendRst where set_encode reads).  The
 * members with pending != 0 in set order; the k-th gets t = *total + k.  THE
 * CLAMP of ugo_ack.h: t >= max_packets is no target and the member stays
 * pending.  At t the whole 64-byte record is zeros but flags = 0x10, n_segments
 * = 1 (FIN) or flags = 0x08, n_segments = 0 (RST); conn_of[t] = c; for a FIN
 * segs[t * max_segments] = {offset = write_pos, data_off = offset & (cap - 1),
 * len 0, avail 0}.  Then fin_sent = 1 and linger_deadline_us = 0 for a FIN,
 * pending = 0, appended[c] = 0, 1 (FIN) or 2 (RST), and *total_out = *total +
 * the number appended (total_out may be total).
 *
 * ugo_fec_loop_set_sent.  origin_ack_us = 0 where n_packets[c] > 0 ||
 * attached[c] != 0 (conn.go:632), for live members.  *deadline_us is
 * resetTimer: the minimum over live members of last_activity_us + idle_us;
 * origin_ack_us + ack_delay_us if set; linger_deadline_us if set; last_sent_us
 * + RTO if last_sent_us != 0 and that time is > now_us -- RTO as
 * ugo_fec_sent_set_rto computes it from delay_us[c] (NULL: 0) and rto_count.
 * UINT64_MAX with no live member.  Members exited and not yet
 * reported go in set order into exits[] / reasons[]; the first max_exits are
 * stored and marked reported, *n_exits counts them all.  With new_index: live
 * members get 0, 1, 2, ... in set order, exited ones UGO_STREAM_NO_CONN, and
 * *nconn_new is the count -- the operand of ugo_fec_listen_remap.
 *
 * DEVIATIONS from the reference, all on purpose:
 *   (a) one clock and one send loop per call: every packet of a batch and
 *       every member of a call sees the same now_us, and the send stages run
 *       once behind the batch, where run calls sendPacket behind every packet.
 *   (b) the idle test runs before the send loop (in check), not after it in
 *       run's select.
 *   (c) an exit found by check takes the member's budget from this batch on;
 *       what cc / sent did to its records earlier in the batch stands.
 *   (d) FIN waits for the segment retransmission queue (rq_len == 0) as well:
 *       after dequeuePacketForRetransmission the reference has an empty history
 *       with segments still queued, and would send FIN in front of them.
 *   (e) the linger timer is a deadline judged at check, not a timer that fires
 *       between calls.
 *   (f) Read / Write deadlines, the close callback itself and crand ids stay
 *       the host's.
 *   (g) sendAckFin has no caller in ugo: ACK|FIN is received, never sent.
 *   (h) a member that exits with a pending RST that never fits max_packets
 *       stays pending; it is reported as exited all the same.
 *   (i) a packet whose flags are 0x90 or 0x08 ends the loop also when its
 *       status is CAPACITY: the reference has no such status, and the packet
 *       decoded.
 *   (j) the reference's Close on a closed connection returns an error, whatever
 *       linger says; here close and abort change nothing then and report
 *       nothing.
 *   (k) a clock behind a stored time reads as no time elapsed (idle, the
 *       delayed ACK); sums of times saturate at UINT64_MAX.
 *   (l) run calls sendPacket once more behind the packet that ended the loop,
 *       and looks at closeChan only then; here a member that has exited sends
 *       nothing but the RST it owes.
 *   (m) an error of the receive history or the receive window ends the
 *       reference's loop at the packet that raised it (conn.go:446-463); here
 *       the member's later packets of the batch pass receive -- the stage in err
 *       is inert for them -- and check finds the error behind the batch.
 *   (n) check looks at the sent history's err and the failure count before the
 *       FIN test; sendPacket sends FIN and may exit with finSent && finRcvd
 *       before CheckForError (conn.go:523-544).  A closed member with nothing
 *       left to send and such an error ends SENT_ERR / FAILURES with an RST
 *       here, CLOSED with a FIN there.
 * Checked on the CPU against a restatement of conn.go (tests/loop_ref.py,
 * tests/test_loop.py) and on the device against one rule per member
 * (tests/loop_harness.py).
 */
#ifndef UGO_LOOP_H
#define UGO_LOOP_H

#include <stddef.h>
#include <stdint.h>

#include "ugo_ack.h"
#include "ugo_cc.h"
#include "ugo_sent.h"
#include "ugo_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel class of every launch of this header (ugo_fec_launch_time.kernel). */
#define UGO_FEC_KERNEL_LOOP 16

/* ugo_loop_state.reason */
#define UGO_LOOP_PEER_ACK_FIN 1
#define UGO_LOOP_PEER_RST 2
#define UGO_LOOP_BAD_PACKET 3
#define UGO_LOOP_CLOSED 4
#define UGO_LOOP_FAILURES 5
#define UGO_LOOP_SENT_ERR 6
#define UGO_LOOP_ACK_ERR 7
#define UGO_LOOP_STREAM_ERR 8
#define UGO_LOOP_IDLE 9
#define UGO_LOOP_LINGER 10
#define UGO_LOOP_ABORT 11

/* ugo_loop_state.pending, appended[] */
#define UGO_LOOP_PENDING_NONE 0
#define UGO_LOOP_PENDING_FIN 1
#define UGO_LOOP_PENDING_RST 2

/* how[] of ugo_fec_loop_set_close */
#define UGO_LOOP_HOW_CLOSE 1u
#define UGO_LOOP_HOW_ABORT 2u
#define UGO_LOOP_HOW_NODELAY_ON 4u
#define UGO_LOOP_HOW_NODELAY_OFF 8u

/* The reference's constants; NULL params means these. */
typedef struct ugo_loop_params {
  uint64_t ack_delay_us; /* 5,000: ackSendDelay */
  uint64_t idle_us;      /* 300,000,000: initialIdleConnectionStateLifetime */
  uint32_t max_retries;  /* 10: maxRetriesAttempted */
  uint32_t reserved;
} ugo_loop_params;
/* idle_us >= 1. */

/* Host mirror of a member's record (64 bytes).  Times in us. */
typedef struct ugo_loop_state {
  uint64_t last_activity_us;   /* lastNetworkActivityTime; now_us of create */
  uint64_t origin_ack_us;      /* originAckTime, 0 = unset */
  uint64_t linger_deadline_us; /* lingerTimer, 0 = none */
  uint64_t exit_us;            /* now_us of the call that exited the member */
  uint64_t dropped;            /* packets receive took from the member */
  uint8_t closed;
  uint8_t fin_sent;
  uint8_t fin_rcvd;
  uint8_t ack_no_delay;
  uint8_t exited;
  uint8_t reason;              /* UGO_LOOP_* reason, 0 while live */
  uint8_t pending;             /* UGO_LOOP_PENDING_* */
  uint8_t reported;            /* ugo_fec_loop_set_sent has listed the exit */
  uint8_t reserved[16];
} ugo_loop_state;

typedef struct ugo_loop_set ugo_loop_set;

/* One record per member, in set order: last_activity_us = now_us, everything
 * else zero.  The four sets must belong to ctx and have the same number of
 * members, else INVALID_ARG.  The loop set reads their records on the device:
 * destroy it before them. */
int ugo_fec_loop_set_create(ugo_fec* ctx, ugo_stream_rx_set* stream_rx, ugo_ack_rx_set* ack_rx,
                            ugo_stream_tx_set* stream_tx, ugo_sent_tx_set* sent_tx, const ugo_loop_params* params,
                            uint64_t now_us, ugo_loop_set** out);
void ugo_fec_loop_set_destroy(ugo_loop_set* set);

/* ugo_fec_loop_set_receive of THE RULE.  info [npackets] as
 * ugo_fec_packet_decode wrote it, 16-B aligned; conn_of uint32 [npackets], in
 * and out.  npackets == 0 is a no-op; npackets <= 2^31. */
int ugo_fec_loop_set_receive(ugo_loop_set* set, const ugo_pkt_info* info, uint32_t* conn_of, size_t npackets,
                             uint64_t now_us, void* stream);

/* ugo_fec_loop_set_close of THE RULE.  how uint8 [nconn]; linger_us uint64
 * [nconn], nullable (NULL: no linger deadline). */
int ugo_fec_loop_set_close(ugo_loop_set* set, const uint8_t* how, const uint64_t* linger_us, uint64_t now_us,
                           void* stream);

/* ugo_fec_loop_set_check of THE RULE.  budget uint32 [nconn], in and out;
 * may_ack_only uint8 [nconn], out. */
int ugo_fec_loop_set_check(ugo_loop_set* set, uint64_t now_us, uint32_t* budget, uint8_t* may_ack_only,
                           void* stream);

/* ugo_fec_loop_set_append of THE RULE.  total uint64 [1]; info [max_packets],
 * 16-B aligned; segs [max_packets][max_segments], max_segments >= 1; conn_of
 * uint32 [max_packets]; total_out uint64 [1], may be total; appended uint8
 * [nconn].  max_packets <= 2^31. */
int ugo_fec_loop_set_append(ugo_loop_set* set, const uint64_t* total, size_t max_packets, ugo_pkt_info* info,
                            ugo_pkt_segment* segs, size_t max_segments, uint32_t* conn_of, uint64_t* total_out,
                            uint8_t* appended, void* stream);

/* ugo_fec_loop_set_sent of THE RULE.  n_packets uint32 [nconn] as
 * ugo_fec_stream_tx_set_plan wrote it; attached uint8 [nconn] as
 * ugo_fec_ack_set_attach wrote it; delay_us uint64 [nconn] as
 * ugo_fec_cc_set_ack wrote it, nullable; deadline_us uint64 [1]; exits uint32
 * [max_exits] and reasons uint8 [max_exits], both nullable with max_exits == 0;
 * n_exits uint64 [1]; new_index uint32 [nconn] and nconn_new uint64 [1], both
 * or neither. */
int ugo_fec_loop_set_sent(ugo_loop_set* set, const uint32_t* n_packets, const uint8_t* attached,
                          const uint64_t* delay_us, uint64_t now_us, uint64_t* deadline_us, uint32_t* exits,
                          uint8_t* reasons, size_t max_exits, uint64_t* n_exits, uint32_t* new_index,
                          uint64_t* nconn_new, void* stream);

/* The nconn records, in set order, after synchronising the stream of the last
 * call on the set. */
int ugo_fec_loop_set_state(ugo_loop_set* set, ugo_loop_state* host_out /* [nconn] */);

#ifdef __cplusplus
}
#endif
#endif /* UGO_LOOP_H */
