/*
 * ugo_cc.h -- C-ABI of congestion control on the GPU: the RTT filter, hybrid
 * slow start and CUBIC of a set of connections, fed by the sent histories
 * (ugo_sent.h) and feeding ugo_fec_sent_set_rto and
 * ugo_fec_stream_tx_set_plan.  What ugo does, per packet and on the host, is
 *
 *   cubicSender                  ugo/congestion/cubic_sender.go
 *   Cubic                        ugo/congestion/cubic.go
 *   RTTStats.UpdateRTT           ugo/congestion/rtt_stats.go:83-114
 *   HybridSlowStart              ugo/congestion/hybrid_slow_start.go
 *   their call sites             ugo/packet_sender.go:193-257, 314-340,
 *                                ugo/conn.go:546-551
 *
 * Added within ABI version 9 (ugo_fec_abi_version() still returns 9): the
 * presence of the ugo_fec_cc_* symbols is the feature test.
 *
 * Conventions as in ugo_sent.h: operands in device or pinned host memory;
 * every call stream-ordered with no host copy and no synchronisation; argument
 * errors return UGO_FEC_ERR_INVALID_ARG before any launch with nothing
 * written; output arrays are written whole; a member whose sent history has
 * err != 0 is inert (its outputs are written as stated, its state never
 * changes).  With these calls the host hands in clocks and sizes only.
 *
 * THE ORDER a caller keeps per batch, on one stream:
 *   ... ugo_fec_sent_set_record, ugo_fec_cc_sent_ack (in place of
 *   ugo_fec_sent_set_ack, split = ugo_fec_cc_set_cutback), ugo_fec_cc_set_ack,
 *   ugo_fec_sent_set_rto (with the delay_us just written), ugo_fec_cc_set_rto,
 *   ugo_fec_sent_set_drain, ugo_fec_stream_tx_set_retransmit,
 *   ugo_fec_ack_set_touch, ugo_fec_stream_tx_set_release, and the next
 *   ugo_fec_stream_tx_set_plan (with the budget just written).
 *
 * THE RULE, per member.  InSlowStart is cwnd < ssthresh; W = cwnd * mss.
 *
 * ugo_fec_cc_sent_ack is ugo_fec_sent_set_ack (THE RULE of ugo_sent.h, the
 * same records, events and scratch rings) and writes one ugo_cc_row per member:
 * max_lost the highest number the call declared lost (0: none), max_acked the
 * highest number whose slot the call freed (0: none), acked_le how many of the
 * freed slots have n <= split[c].  A member with no accepted ACK gets a row of
 * zeros.
 *
 * ugo_fec_cc_set_ack (UpdateRTT, then OnCongestionEvent, as receivedAck calls
 * them).  A member whose event has accepted == 0 changes nothing but what step
 * 5 writes.  Otherwise, in this order:
 *   1. RTT sample.  If has_rtt and rtt_us > 0: min_rtt = rtt_us if it is 0 or
 *      larger; sample = rtt_us, less the event's delay_us if sample > delay_us;
 *      latest_rtt = sample.  The first sample (srtt == 0) sets srtt = sample,
 *      mean_dev = sample / 2.  Later ones, in float32, every product and sum
 *      rounded to float32, nothing fused, the result truncated to whole us:
 *        mean_dev = 0.75 * mean_dev + 0.25 * |srtt - sample|
 *        srtt     = srtt * 0.875 + sample * 0.125
 *   2. Slow-start exit.  If has_rtt (also with rtt_us == 0) and InSlowStart:
 *      ShouldExitSlowStart(latest_rtt, min_rtt, cwnd), lastSentPacketNumber
 *      being the sent record's last_sent; true sets ssthresh = cwnd.
 *   3. Loss.  If lost_packets > 0 and the row's max_lost > cutback:
 *      last_cutback_exited_slowstart = InSlowStart; cwnd =
 *      CongestionWindowAfterPacketLoss(cwnd) (float32, beta() and betaLastMax
 *      as written, epoch_us = 0), at least min_cwnd; ssthresh = cwnd; cutback =
 *      last_sent; cutbacks++.
 *   4. Acks.  A = acked_packets, prior = largest_acked, largest_acked =
 *      max(prior, max_acked).  Acknowledged in recovery (they change nothing
 *      else): A if step 3 cut in this call, else 0 if prior > cutback, else
 *      acked_le.  Each of the other G = A - that does maybeIncreaseCwnd with
 *      the event's bytes_in_flight and clock now_us: not cwnd-limited ->
 *      app_limited_us = now_us if unset, and every later step is the same;
 *      cwnd >= max_cwnd -> nothing; InSlowStart -> cwnd++; else cwnd =
 *      min(max_cwnd, CongestionWindowAfterAck(cwnd, min_rtt)) in Go's 64-bit
 *      wrapping arithmetic, cubeFactor = 2^40 / 410, time_to_origin the integer
 *      cube root.  cwnd-limited is isCwndLimited with maxBurstBytes = 3 * mss.
 *      After the G steps: if G > 0, InSlowStart and max_acked >
 *      end_packet_number, started = 0.
 *   5. Outputs, for every member: delay_us[c] = srtt == 0 ? 0 : srtt + 4 *
 *      mean_dev; rto_candidate = the sent record's lio + 1, or 0 if lio ==
 *      last_sent; cutback[c] of the dense array.  An inert member gets
 *      delay_us[c] = 0 and keeps its rto_candidate.
 * The work per member does not grow with G.
 *
 * ugo_fec_cc_set_rto, after ugo_fec_sent_set_rto.  Where fired[c] (checkRTO's
 * two calls): if rto_candidate != 0 and rto_candidate > cutback, the loss
 * reaction of step 3; then OnRetransmissionTimeout(true): cutback = 0, started
 * = found = 0, the CUBIC fields zero, ssthresh = cwnd / 2, cwnd = min_cwnd,
 * rtos++.  Then for every member, bif being the sent record's bytes_in_flight
 * as it stands: budget[c] = bif > W ? 0 : min(max_budget, (W - bif) /
 * packet_bytes + 1) -- the loop of conn.go:546-551 with
 * CongestionAllowsSending before every packet of packet_bytes.  An inert
 * member gets budget 0.
 *
 * DEVIATIONS from the reference, all on purpose:
 *   (a) one congestion event per member and call, over the union of what the
 *       call's accepted ACKs acknowledged and lost; with one accepted ACK per
 *       member and call it equals the reference.
 *   (b) the clock of every step of a call is now_us.
 *   (c) whole microseconds: mean_dev = sample / 2 truncated.
 *   (d) not kept, because ugo never reads it: PRR (TimeUntilSend has no caller
 *       outside congestion/), the recent-min / half / quarter RTT samples,
 *       connectionStats, Reno, slow-start large reduction, connection
 *       migration, ExpireSmoothedMetrics.
 *   (e) started is cleared by the call's highest acknowledged number, judged
 *       after the call's increments; the reference clears it per packet while
 *       still in slow start.  The value is read only in slow start.
 *   (f) the cube root is the integer root (the largest t with t^3 <= x).  For
 *       every difference last_max_cwnd - cwnd of 1 .. 2^20, the whole range
 *       UGO_CC_MAX_CWND_LIMIT permits, it equals the restatement's
 *       uint32(cbrt(float64(x))), which is numpy's cbrt; Go's own math.Cbrt has
 *       not been run against it.
 *   (g) a budget counts packets of packet_bytes; a shorter packet still counts
 *       as one.
 *   (h) byte counts are 64-bit (the reference's are uint32).
 *   (i) the packet an RTO takes is lio + 1 as ugo_fec_cc_set_ack saw it (the
 *       sent histories' invariant).
 *   (j) consecutiveRTOCount > maxRetriesAttempted (the connection failure)
 *       stays the host's: it reads rto_count from the sent state.
 * Checked on the CPU against a restatement of congestion/ (tests/cc_ref.py,
 * tests/test_cc.py) and on the device against one rule per member
 * (tests/cc_harness.py).
 */
#ifndef UGO_CC_H
#define UGO_CC_H

#include <stddef.h>
#include <stdint.h>

#include "ugo_sent.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel class of every launch of this header (ugo_fec_launch_time.kernel),
 * those of ugo_fec_cc_sent_ack included. */
#define UGO_FEC_KERNEL_CC 14

#define UGO_CC_MAX_CWND_LIMIT (1u << 20)

/* The reference's constants; NULL params means these. */
typedef struct ugo_cc_params {
  uint32_t initial_cwnd;    /* 32, initialCongestionWindow (constants.go) */
  uint32_t max_cwnd;        /* 200, defaultMaxCongestionWindow (constants.go) */
  uint32_t min_cwnd;        /* 2 */
  uint32_t num_connections; /* 2 */
  uint32_t mss;             /* 1460 */
} ugo_cc_params;
/* 1 <= min_cwnd <= initial_cwnd <= max_cwnd <= UGO_CC_MAX_CWND_LIMIT,
 * num_connections >= 1, mss >= 1. */

/* What ugo_fec_cc_sent_ack tells of one member beside its event row (32 bytes). */
typedef struct ugo_cc_row {
  uint64_t max_lost;
  uint64_t max_acked;
  uint32_t acked_le;
  uint8_t reserved[12];
} ugo_cc_row;

/* Host mirror of a controller's record (192 bytes).  Times in us; 0 = unset
 * for epoch_us, app_limited_us and last_update_us, as last_sent_us in
 * ugo_sent.h.  Windows in packets. */
typedef struct ugo_cc_state {
  uint64_t cwnd;               /* congestionWindow */
  uint64_t ssthresh;           /* slowstartThreshold */
  uint64_t largest_acked;      /* largestAckedPacketNumber */
  uint64_t cutback;            /* largestSentAtLastCutback */
  uint64_t min_rtt_us;         /* RTTStats */
  uint64_t latest_rtt_us;
  uint64_t srtt_us;
  uint64_t mean_dev_us;
  uint64_t end_packet_number;  /* HybridSlowStart */
  uint64_t current_min_rtt_us;
  uint64_t epoch_us;           /* Cubic */
  uint64_t app_limited_us;
  uint64_t last_update_us;
  uint64_t last_cwnd;
  uint64_t last_max_cwnd;
  uint64_t est_tcp_cwnd;
  uint64_t origin_cwnd;
  uint64_t last_target_cwnd;
  uint64_t rto_candidate;      /* lio + 1 as ugo_fec_cc_set_ack saw it, 0 = nothing outstanding */
  uint64_t cutbacks;           /* counters */
  uint64_t rtos;
  uint32_t sample_count;       /* HybridSlowStart.rttSampleCount */
  uint32_t acked_count;        /* Cubic.ackedPacketsCount */
  uint32_t time_to_origin;     /* Cubic.timeToOriginPoint */
  uint8_t last_cutback_exited_slowstart;
  uint8_t started;             /* HybridSlowStart */
  uint8_t found;               /* hystartFound */
  uint8_t reserved[9];
} ugo_cc_state;

typedef struct ugo_cc_set ugo_cc_set;

/* One controller per member of sent, in set order: cwnd = initial_cwnd,
 * ssthresh = max_cwnd, everything else zero.  The set reads the members' sent
 * records on the device; destroy it before sent. */
int ugo_fec_cc_set_create(ugo_fec* ctx, ugo_sent_tx_set* sent, const ugo_cc_params* params, ugo_cc_set** out);
void ugo_fec_cc_set_destroy(ugo_cc_set* set);

/* The dense device array cutback[nconn]: what ugo_fec_cc_sent_ack takes as
 * split.  ugo_fec_cc_set_ack and ugo_fec_cc_set_rto keep it current. */
int ugo_fec_cc_set_cutback(ugo_cc_set* set, const uint64_t** dev);

/* ugo_fec_sent_set_ack, and rows [nconn] written whole beside events.  split
 * uint64 [nconn].  Arguments otherwise as ugo_fec_sent_set_ack; rows 16-B
 * aligned. */
int ugo_fec_cc_sent_ack(ugo_sent_tx_set* set, const ugo_pkt_info* info, const uint64_t* ranges, size_t max_ranges,
                        const uint32_t* conn_of, size_t npackets, uint64_t now_us, ugo_sent_event* events,
                        const uint64_t* split, ugo_cc_row* rows, void* stream);

/* ugo_fec_cc_set_ack of THE RULE.  events and rows [nconn] as
 * ugo_fec_cc_sent_ack wrote them, both 16-B aligned; delay_us uint64 [nconn]. */
int ugo_fec_cc_set_ack(ugo_cc_set* set, const ugo_sent_event* events, const ugo_cc_row* rows, uint64_t now_us,
                       uint64_t* delay_us, void* stream);

/* ugo_fec_cc_set_rto of THE RULE.  fired uint8 [nconn] as ugo_fec_sent_set_rto
 * wrote it; packet_bytes >= 1, max_budget <= 2^31; budget uint32 [nconn]. */
int ugo_fec_cc_set_rto(ugo_cc_set* set, const uint8_t* fired, size_t packet_bytes, size_t max_budget,
                       uint32_t* budget, void* stream);

/* The nconn records, in set order, after synchronising the stream of the last
 * call on the set. */
int ugo_fec_cc_set_state(ugo_cc_set* set, ugo_cc_state* host_out /* [nconn] */);

#ifdef __cplusplus
}
#endif
#endif /* UGO_CC_H */
