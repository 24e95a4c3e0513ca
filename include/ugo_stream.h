/*
 * ugo_stream.h -- C-ABI of stream delivery on the GPU: the step after
 * ugo_fec_packet_decode on the receive path.  The decoder ends with views
 * (ugo_pkt_segment: stream offset, data_off, len, avail) into the still
 * encrypted ring; what ugo does next, per segment and on the host, is
 *
 *   Conn.handleSegment   ugo/conn.go:473-490           segmentSorter.push, wake Read
 *   segmentSorter.push   ugo/segment_sorter.go:31-98   duplicate / overlap / gap list
 *   segmentSorter.pop    ugo/segment_sorter.go:100-107
 *   segmentSorter.head   ugo/segment_sorter.go:109-115
 *   Conn.Read            ugo/conn.go:149-245           drain queued segments in order
 *   Conn.run             ugo/conn.go:130-134           a handlePacket error resets the conn
 *
 * Here a connection owns a receive window on the device.  One call
 * (ugo_fec_stream_deliver) runs handleSegment for every segment of a decoded
 * batch and moves the accepted bytes, RC4 pad fused, into the window; one more
 * (ugo_fec_stream_read) is Conn.Read.  With ugo_fec_rx_assemble, recovery and
 * ugo_fec_packet_decode in front, the receive chain is device-resident from
 * the wire to ordered stream bytes.
 *
 * State (device memory, allocated and zeroed by create):
 *   W     the window, cap = window_bytes; stream byte x lives at W[x & (cap-1)]
 *   C     coverage bitmap, one bit per window byte: byte x received
 *   S     start bitmap, one bit per window byte: a queued segment starts at x
 *         (the reference's queuedFrames keys)
 *   two scratch bitmaps of the same size (claims of a call, contested bytes),
 *   all zero between calls
 *   a record, mirrored by ugo_stream_rx_state
 *
 * THE RULE.  Arrival order is packet index, then segment index.  A packet with
 * info[i].status != UGO_PKT_OK is skipped whole: its seg_status entries are 0
 * and it counts in skipped_packets (the reference drops a packet whose decode
 * fails; a UGO_PKT_CAPACITY packet cannot be delivered faithfully, so the
 * caller sizes the decoder's caps).  Segment (o, len, avail) is the bytes
 * [o, o+len): avail bytes from the packet, then len-avail zeros (what
 * bytes.Reader.Read leaves of a truncated last segment).  "covered(x)" means
 * x < read_pos or C[x] set.  For each segment in arrival order:
 *
 *   1. err already set: nothing is processed, seg_status 0 -- the connection
 *      was reset (ugo/conn.go:130-134).
 *   2. S[o] set (o in [read_pos, read_pos+cap)), or o == head_off while
 *      head_off is valid: UGO_STREAM_DUPLICATE (push's map lookup, :32-35).
 *   3. len == 0 (fin, :40-44): o in [read_pos, read_pos+cap) sets S[o],
 *      UGO_STREAM_ACCEPTED, no byte moves; else UGO_STREAM_OUT_OF_WINDOW.
 *   4. o+len > read_pos+cap: UGO_STREAM_OUT_OF_WINDOW, not applied.
 *   5. no byte of the range covered: UGO_STREAM_ACCEPTED -- C set over the
 *      range, S[o] set, hi raised to o+len, the bytes copied.
 *   6. every byte covered: UGO_STREAM_DUPLICATE (!foundInGap, :88-90).
 *   7. otherwise UGO_STREAM_OVERLAP (errOverlappingStreamData, :54-60), fatal:
 *      err, err_packet and err_segment are set, nothing after it in this call
 *      or in later calls is processed (seg_status 0), and the window's
 *      content is unspecified from then on.
 *
 * After the call: ngaps = the uncovered runs of [read_pos, hi) plus one (the
 * reference's gap list always ends in an open gap); if the call accepted a
 * non-empty segment and ngaps > 50 (MaxStreamFrameSorterGaps, :92-94) err =
 * UGO_STREAM_TOO_MANY_GAPS.  readable = u - read_pos for the first uncovered
 * u >= read_pos (at most cap); eof = S[u] set (u < read_pos+cap): a start bit
 * on an uncovered byte can only be a queued empty segment.
 *
 * ugo_fec_stream_read(n) is Conn.Read(p[:n]) that never waits: m = min(n,
 * readable) bytes are copied (two pieces at the wrap), *n_read = m, *eof =
 * (m == readable && eof) -- io.EOF is reported with the last byte in front of
 * the empty segment, where the reference returns it from the same call only
 * if p had room left and else from the next one.  C and S are cleared over
 * [read_pos, read_pos+m) and read_pos advances.  If m > 0: when the new
 * read_pos is covered and has no start bit the head segment is partly read
 * (:184-195) and head_off becomes the highest start bit below the new
 * read_pos (unchanged if the bytes read held none); otherwise head_off is
 * invalid.  read works after an error too (on whatever is readable).
 *
 * DEVIATIONS from the reference, all on purpose:
 *   (a) the window bound of step 4 (and of step 3): the reference buffers
 *       without bound.  The caller must treat a packet with an out-of-window
 *       segment as not received (no ACK), as for ugo_fec_rx_assemble's batch
 *       window.
 *   (b) the gap limit is applied to the state after the call; the reference
 *       applies it after each push, so it also trips on a transient the batch
 *       does not see (a 51st gap that a later segment of the batch closes).
 *   (c) a queued empty segment that Read passes over -- a later data segment
 *       spanned its offset -- is forgotten; the reference keeps its map entry
 *       for ever (and answers "duplicate" for that offset for ever).
 * Checked on the CPU against a literal restatement of push / pop / head and
 * the Read loop (tests/stream_ref.py, tests/test_stream_deliver.py), and on
 * the device at the sizes, offsets and descriptors where kernels go wrong
 * (tests/test_stream_deliver_sizes.py).
 */
#ifndef UGO_STREAM_H
#define UGO_STREAM_H

#include <stddef.h>
#include <stdint.h>

#include "ugo_pkt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-segment result (seg_status) and, for the last two, the connection
 * error (ugo_stream_rx_state.err). */
typedef enum ugo_stream_status {
  UGO_STREAM_NONE = 0,          /* not processed: unused entry, skipped packet, after an error */
  UGO_STREAM_ACCEPTED = 1,
  UGO_STREAM_DUPLICATE = 2,     /* errDuplicateStreamData: dropped, the connection goes on */
  UGO_STREAM_OUT_OF_WINDOW = 3, /* deviation (a): not applied */
  UGO_STREAM_OVERLAP = 4,       /* errOverlappingStreamData: fatal */
  UGO_STREAM_TOO_MANY_GAPS = 5  /* errTooManyGapsInReceivedStreamData: fatal, err only */
} ugo_stream_status;

#define UGO_STREAM_MAX_GAPS 50u        /* MaxStreamFrameSorterGaps */
#define UGO_STREAM_MIN_WINDOW 4096u

/* Host mirror of the connection's record (96 bytes). */
typedef struct ugo_stream_rx_state {
  uint64_t read_pos;         /* Conn.readOffset */
  uint64_t head_off;         /* offset of the segment Read has partly consumed (head_valid) */
  uint64_t hi;               /* highest accepted end */
  uint64_t readable;         /* contiguous covered bytes at read_pos */
  uint64_t accepted;         /* counters, cumulative over calls */
  uint64_t duplicate;
  uint64_t out_of_window;
  uint64_t skipped_packets;
  uint64_t ordered_segments; /* segments that went through the ordered pass */
  uint64_t err_packet;       /* packet index (within its call) of the fatal segment */
  uint32_t err_segment;      /* its segment index */
  uint32_t err;              /* 0, UGO_STREAM_OVERLAP, UGO_STREAM_TOO_MANY_GAPS */
  uint32_t ngaps;
  uint8_t head_valid;
  uint8_t eof;               /* an empty segment is queued at read_pos + readable */
  uint8_t reserved[2];
} ugo_stream_rx_state;

typedef struct ugo_stream_rx ugo_stream_rx;

/* A receive window of window_bytes (a power of two, >= UGO_STREAM_MIN_WINDOW)
 * on ctx's device, everything zeroed, read_pos = 0.  ctx must outlive it. */
int ugo_fec_stream_rx_create(ugo_fec* ctx, size_t window_bytes, ugo_stream_rx** out);
void ugo_fec_stream_rx_destroy(ugo_stream_rx* rx);

/* handleSegment for every segment of a decoded batch: pkts, slot, pad, info,
 * segs, max_segments and npackets as given to / written by
 * ugo_fec_packet_decode (packet i at pkts + i*slot, still encrypted; its
 * segments at segs[i*max_segments ..], info[i].n_segments of them).  pad
 * (nullable, >= slot bytes) is XORed over segment bytes by their position in
 * the slot, exactly as the decoder applied it (the decoder never wrote the
 * plaintext back).  THE CLAMP: whatever the descriptors hold, the call uses
 *   avail      = min(avail, len, max(0, slot - data_off))
 *   n_segments = min(n_segments, max_segments)
 * so the bytes of a segment are read from [data_off, data_off + avail) of its
 * own slot (and of pad) and from nowhere else, what the clamp cuts off reads
 * as zeros like the tail of a truncated segment, and no seg_status entry or
 * descriptor beyond a packet's max_segments is touched.  len == 0 with avail
 * > 0 is an empty segment.  seg_status[npackets][max_segments]
 * (uint8, device) receives a ugo_stream_status per segment entry.
 *
 * Buffers: device or pinned host memory, pageable memory is rejected;
 * slot % 16 == 0, slot <= 0xffff, pkts and pad 16-B aligned; npackets == 0 is
 * a no-op.  Stream-ordered, no host synchronisation; calls on one rx must be
 * ordered by the caller (one stream, or events).  Window bytes outside the
 * accepted segments' ranges are neither written nor read-modify-written.
 * Returns a ugo_fec_status (argument / launch errors); stream results are in
 * seg_status and the record. */
int ugo_fec_stream_deliver(ugo_stream_rx* rx, const uint8_t* pkts, size_t slot, const uint8_t* pad,
                           const ugo_pkt_info* info, const ugo_pkt_segment* segs, size_t max_segments,
                           size_t npackets, uint8_t* seg_status, void* stream);

/* Conn.Read(p[:n]): m = min(n, readable) bytes to dst (device or pinned host
 * memory, any alignment; NULL discards them), *n_read = m (uint64, device or
 * pinned), *eof (uint8, nullable) as described above.  Stream-ordered. */
int ugo_fec_stream_read(ugo_stream_rx* rx, uint8_t* dst, size_t n, uint64_t* n_read, uint8_t* eof, void* stream);

/* The record, after synchronising the stream of the last deliver / read. */
int ugo_fec_stream_rx_state(ugo_stream_rx* rx, ugo_stream_rx_state* host_out);

/* The window itself, for consumers that read in place (stream byte x at
 * window_dev[x & (window_bytes-1)], valid for x in [read_pos, read_pos +
 * readable)). */
int ugo_fec_stream_rx_window(ugo_stream_rx* rx, uint8_t** window_dev, size_t* window_bytes);

/* ---- Receive-window sets: many connections per call ----------------------
 *
 * Added within ABI version 9 (ugo_fec_abi_version() still returns 9): the
 * presence of the ugo_fec_stream_set_* symbols is the feature test.
 *
 * ugo uses one fixed RC4 key, so a decoded batch holds packets of any number
 * of connections, interleaved as the listener received them.  A set is an
 * ordered list of existing receive windows (their sizes may differ); packet i
 * of a batch belongs to member conn_of[i].  The set does not own its members:
 * destroy the set first, then the members.  Members cannot be added to or
 * removed from a live set; destroy it and create another.  create uploads one
 * table entry per member (window, four bitmaps, record, cap), once, so the
 * per-call entry points make no host-to-device copy and no host
 * synchronisation.  create returns UGO_FEC_ERR_INVALID_ARG for a NULL
 * argument, nconn == 0 or nconn > 2^20, a NULL member, a member of another
 * context, or the same ugo_stream_rx listed twice.
 *
 * Calls on a member through the single entry points and through a set may be
 * mixed; the caller orders them, as it orders the calls on one rx.
 * ugo_fec_stream_rx_state and ugo_fec_stream_rx_window on a member reflect
 * the set's calls.  The launches report as kernel classes
 * UGO_FEC_KERNEL_STREAM_DELIVER and UGO_FEC_KERNEL_STREAM_READ.  Checked on
 * the device against one rule per member, where blocks mix connections
 * (tests/stream_set_harness.py, tests/test_stream_set.py), and at the launch
 * shapes of large and unequal sets (tests/test_stream_set_sizes.py): reads,
 * bitmap passes and gap counts with up to 256 blocks per connection over
 * windows of 4 KiB to 4 MiB in one set, wrapped windows, a status array that
 * is not 16-B aligned with three segment slots per packet, a member across
 * 2^32 beside one at 0, lying descriptors between another member's packets,
 * and a set of 32,769 members. */
#define UGO_STREAM_NO_CONN 0xffffffffu

typedef struct ugo_stream_rx_set ugo_stream_rx_set;

int ugo_fec_stream_set_create(ugo_fec* ctx, ugo_stream_rx* const* rxs, size_t nconn, ugo_stream_rx_set** out);
void ugo_fec_stream_set_destroy(ugo_stream_rx_set* set);

/* ugo_fec_stream_deliver with one more operand: conn_of[npackets] (uint32,
 * device or pinned host memory), the index into the set of the connection
 * packet i belongs to.  For every member c the call has exactly the effect of
 * ugo_fec_stream_deliver on member c with the subsequence of packets
 * {i : conn_of[i] == c}, in batch order -- statuses, record, window, bitmaps --
 * except that err_packet is the packet's index in this call's batch and
 * seg_status rows are indexed by batch packet index.  A member with no packet
 * in the call keeps its record bit for bit.  A packet whose conn_of[i] is
 * UGO_STREAM_NO_CONN or any other value >= nconn belongs to no connection (the
 * clamp policy: a lying descriptor is clamped, never followed): its seg_status
 * row is all zero over max_segments and it is counted in no record.  Errors
 * stay per connection: a fatal overlap stops its own connection only, and a
 * member that is already in error gets status 0 for all its packets and
 * nothing of it is touched.  Argument checks, alignment rules, npackets == 0
 * and stream ordering as for ugo_fec_stream_deliver. */
int ugo_fec_stream_set_deliver(ugo_stream_rx_set* set, const uint8_t* pkts, size_t slot, const uint8_t* pad,
                               const ugo_pkt_info* info, const ugo_pkt_segment* segs, size_t max_segments,
                               size_t npackets, const uint32_t* conn_of, uint8_t* seg_status, void* stream);

/* Conn.Read for every member in one launch; n, dst_off, n_read and eof are
 * arrays of nconn elements in device or pinned host memory.  Per member c the
 * effect is ugo_fec_stream_read(member c, dst + dst_off[c], n[c], &n_read[c],
 * &eof[c]), except that n[c] == 0 skips the member: its record is untouched,
 * n_read[c] = 0, eof[c] = 0.  dst NULL discards for all members (dst_off may
 * then be NULL); eof may be NULL.  The caller keeps the destination ranges
 * disjoint; the call does not check them. */
int ugo_fec_stream_set_read(ugo_stream_rx_set* set, uint8_t* dst, const uint64_t* dst_off, const uint64_t* n,
                            uint64_t* n_read, uint8_t* eof, void* stream);

/* The nconn records, in set order, after synchronising the stream of the last
 * call on the set: gathered on the device and copied out in one transfer. */
int ugo_fec_stream_set_state(ugo_stream_rx_set* set, ugo_stream_rx_state* host_out /* [nconn] */);

/* ---- Send windows: Conn.Write, PopSegments and encode per set -------------
 *
 * Added within ABI version 9: the presence of the ugo_fec_stream_tx_* symbols
 * is the feature test.  The transmit mirror of the receive-window sets:
 *
 *   Conn.Write            ugo/conn.go:247-275
 *   lenOfDataForWriting,
 *   getDataForWriting     ugo/conn.go:753-779   (advances writeOffset)
 *   PopSegments,
 *   popSegmentsForRetransmission, popNormalSegments,
 *   maybeSplitOffFrame    ugo/segment_sender.go:18-99
 *   Conn.sendPacket       ugo/conn.go:521-640   PopSegments(maxPacketSize - 40),
 *                                               lastPacketNumber++, encode, encrypt
 *   retransmitted segments go to the back of retransmissionQueue
 *                         ugo/conn.go:565-568, ugo/packet_sender.go:262-285
 *
 * A send window (ugo_stream_tx) holds a connection's unsent and
 * unacknowledged stream bytes on the device:
 *   W     the window, cap = window_bytes, a power of two in [4096, 2^31];
 *         stream byte x lives at W[x & (cap-1)]
 *   Q     the retransmission queue, a FIFO ring of rq_cap entries
 *         (ugo_stream_tx_rq_entry); the queue is Q[(rq_head + k) % rq_cap],
 *         k < rq_len
 *   a record, mirrored by ugo_stream_tx_state; base <= write_pos <= tail <=
 *   base + cap
 * Three hot calls per batch -- write, plan, encode -- keep the send chain on
 * the device from Conn.Write to the slots ugo_fec_tx_assemble consumes.  ARQ,
 * ACK processing and congestion control stay on the host and hand these calls
 * a packet budget (plan), the segments to retransmit (retransmit) and how far
 * the peer has acknowledged (release).
 *
 * THE RULE of plan, with M = max_payload (the reference's maxPacketSize - 40 =
 * 1436) and H = 4.  Member c, at most budget_eff[c] times:
 *
 *   cur = 0, segs = []
 *   while queue not empty and len(segs) < max_segments:
 *       if cur + H >= M: break                                   (a)
 *       cur += H; s = queue front; room = M - cur
 *       if s.len > room: emit (s.offset, room); s.offset += room;
 *                        s.len -= room; cur += room; break
 *       pop; emit (s.offset, s.len); cur += s.len
 *   rem = M - cur; pending = tail - write_pos
 *   if rem > H and pending > 0 and len(segs) < max_segments:     (a)
 *       n = min(pending, rem - H); emit (write_pos, n); write_pos += n
 *   if segs is empty: stop
 *   packet_number = ++last_packet_number
 *
 * budget_eff[c] = min(budget[c], max(0, max_packets - sum of budget[c'] for
 * c' < c)): a budget array that asks for more than the caller's arrays hold is
 * clamped, never followed.
 *
 * DEVIATIONS from the reference, all on purpose:
 *   (a) no empty segment from plan.  popSegmentsForRetransmission tests
 *       currentLen + 4 > maxLen and popNormalSegments tests 4 > maxBytes, so
 *       with exactly 4 bytes of room left the reference emits a segment with
 *       no data -- which the receiver reads as a FIN.  Here a piece is emitted
 *       only if at least one byte of it fits; FIN is the caller's packet.  The
 *       reference's packets with their empty segments removed are the rule's
 *       packets, and the final state (queue, write_pos) is identical.
 *   (b) the window bound: Go's Write hands over a slice of any size and blocks
 *       until it is sent; write here is partial and never waits.
 *   (c) the segment cap: a packet closes when it holds max_segments segments.
 *       The reference has no cap (a packet of 1-byte retransmissions could
 *       hold 287).
 *   (d) the empty write: a zero-length write is a no-op.  In the reference
 *       Write([]byte{}) makes getDataForWriting return an empty non-nil slice,
 *       which is sent as an empty segment.
 * Checked on the CPU against a literal restatement of the Go loop
 * (tests/stream_tx_ref.py) and on the device against one rule per member
 * (tests/stream_tx_harness.py, tests/test_stream_tx.py).
 *
 * Every operand array is in device or pinned host memory (pageable memory is
 * rejected); every call is stream-ordered with no host synchronisation and no
 * host-to-device copy of its own; the caller orders the calls on one set.
 * Argument errors return UGO_FEC_ERR_INVALID_ARG before any launch, with
 * nothing written.  There are no single-connection entry points: a set of one
 * member is the single-connection form.  write, release, retransmit, plan and
 * the state gather report as kernel class UGO_FEC_KERNEL_STREAM_TX, encode as
 * UGO_FEC_KERNEL_PACKET_ENCODE. */
#define UGO_STREAM_TX_MAX_WINDOW 0x80000000u

/* Per-entry result of ugo_fec_stream_tx_set_retransmit. */
typedef enum ugo_stream_tx_rq_status {
  UGO_STREAM_TX_RQ_QUEUED = 1,
  UGO_STREAM_TX_RQ_REJECTED = 2, /* len 0 or > 0xffff, not inside [base, write_pos), conn_of >= nconn */
  UGO_STREAM_TX_RQ_FULL = 3,     /* the queue is full: this entry and the connection's later ones */
  UGO_STREAM_TX_RQ_UNSORTED = 4  /* conn_of decreases somewhere: nothing of the call was applied */
} ugo_stream_tx_rq_status;

/* One retransmission-queue entry (16 bytes). */
typedef struct ugo_stream_tx_rq_entry {
  uint64_t offset;
  uint32_t len;
  uint32_t reserved;
} ugo_stream_tx_rq_entry;

/* Host mirror of a send window's record (80 bytes). */
typedef struct ugo_stream_tx_state {
  uint64_t base;                /* lowest retained stream offset */
  uint64_t write_pos;           /* Conn.writeOffset: the next byte not yet packetised */
  uint64_t tail;                /* end of the bytes written */
  uint64_t last_packet_number;  /* Conn.lastPacketNumber */
  uint64_t packets;             /* counters, cumulative over calls */
  uint64_t segments;
  uint64_t bytes_new;
  uint64_t bytes_retransmitted;
  uint64_t rq_rejected;         /* retransmit entries answered REJECTED or FULL */
  uint32_t rq_len;              /* entries queued */
  uint32_t rq_head;             /* ring index of the queue's front */
} ugo_stream_tx_state;

typedef struct ugo_stream_tx ugo_stream_tx;
typedef struct ugo_stream_tx_set ugo_stream_tx_set;

/* A send window on ctx's device, everything zeroed, base = write_pos = tail =
 * start_offset and last_packet_number = start_packet_number (the reference
 * starts both at 0; other values adopt a connection mid-life).  window_bytes
 * a power of two in [UGO_STREAM_MIN_WINDOW, UGO_STREAM_TX_MAX_WINDOW],
 * 1 <= rq_cap <= 2^24.  ctx must outlive it. */
int ugo_fec_stream_tx_create(ugo_fec* ctx, size_t window_bytes, size_t rq_cap, uint64_t start_offset,
                             uint64_t start_packet_number, ugo_stream_tx** out);
void ugo_fec_stream_tx_destroy(ugo_stream_tx* tx);

/* The window and the queue ring themselves (device memory), for consumers and
 * tests that look at them in place, after synchronising the set's stream. */
int ugo_fec_stream_tx_window(ugo_stream_tx* tx, uint8_t** window_dev, size_t* window_bytes);
int ugo_fec_stream_tx_queue(ugo_stream_tx* tx, ugo_stream_tx_rq_entry** rq_dev, size_t* rq_cap);

/* An ordered list of existing send windows (sizes may differ).  Ownership,
 * lifetime, duplicate-member and nconn <= 2^20 rules as for
 * ugo_fec_stream_set_create: the set does not own its members, destroy the
 * set first; INVALID_ARG for a NULL argument, nconn == 0 or > 2^20, a NULL
 * member, a member of another context or one listed twice.  The member table
 * and the plan's scratch are made here, once. */
int ugo_fec_stream_tx_set_create(ugo_fec* ctx, ugo_stream_tx* const* txs, size_t nconn, ugo_stream_tx_set** out);
void ugo_fec_stream_tx_set_destroy(ugo_stream_tx_set* set);

/* Conn.Write that never waits (deviation (b)), for every member: m = min(n[c],
 * cap - (tail - base)) bytes go from src + src_off[c] to W[(tail + k) &
 * (cap-1)] (two pieces at the wrap), tail += m, n_written[c] = m.  n[c] == 0
 * leaves the member untouched (deviation (d)) and gives n_written[c] = 0.  src
 * may have any alignment; src_off, n and n_written are uint64[nconn].  Window
 * bytes outside [tail, tail + m) are neither written nor read-modify-written.
 * The caller keeps the source ranges readable; the call does not check them. */
int ugo_fec_stream_tx_set_write(ugo_stream_tx_set* set, const uint8_t* src, const uint64_t* src_off,
                                const uint64_t* n, uint64_t* n_written, void* stream);

/* Per member: base = max(base, min(upto[c], write_pos, the lowest offset still
 * held in the member's retransmission queue)).  upto is uint64[nconn]. */
int ugo_fec_stream_tx_set_release(ugo_stream_tx_set* set, const uint64_t* upto, void* stream);

/* Append m entries (conn_of uint32, offset uint64, len uint32) to the
 * members' queues, in index order within a connection.  conn_of must be
 * non-decreasing over the list; if any conn_of[j] < conn_of[j-1] nothing is
 * applied and every status is UGO_STREAM_TX_RQ_UNSORTED.  Otherwise status[j]
 * (uint8[m]) is a ugo_stream_tx_rq_status; REJECTED and FULL entries count in
 * the member's rq_rejected (an entry with conn_of >= nconn in no record).
 * A cold path: the list is the loss rate's share of a batch.  m == 0 is a
 * no-op. */
int ugo_fec_stream_tx_set_retransmit(ugo_stream_tx_set* set, const uint32_t* conn_of, const uint64_t* offset,
                                     const uint32_t* len, size_t m, uint8_t* status, void* stream);

/* The loop of Conn.sendPacket for every member: THE RULE above.  budget is
 * uint32[nconn]; 16 <= max_payload <= 0xffff; 1 <= max_segments <= 0xffff;
 * max_packets <= 2^31.  The packets are compact and connection-major: member
 * c's packets are batch indices [first_packet[c], first_packet[c] +
 * n_packets[c]) (uint64[nconn], uint32[nconn]), members in set order; *total
 * (uint64) is the number of packets planned.  For i < total the whole 64-byte
 * info[i] is written (flags 0, packet_number, n_segments, everything else
 * zero), segs[i][0 .. n_segments) get offset, len, avail = len and data_off =
 * offset & (cap-1), and conn_of[i] = c.  For total <= i < max_packets,
 * conn_of[i] = UGO_STREAM_NO_CONN and nothing else of packet i is written;
 * segment entries at or past n_segments keep the caller's bytes.  A member
 * with budget_eff == 0 or nothing to send keeps its record bit for bit, gets
 * n_packets = 0 and first_packet = where its packets would have started.
 * first_packet tells the caller where to patch a SACK or a stop-waiting into a
 * connection's first packet before encode; ACK-only, stop-waiting-only, FIN
 * and RST packets are the caller's, appended by it. */
int ugo_fec_stream_tx_set_plan(ugo_stream_tx_set* set, const uint32_t* budget, size_t max_payload,
                               size_t max_segments, size_t max_packets, ugo_pkt_info* info, ugo_pkt_segment* segs,
                               uint32_t* conn_of, uint64_t* first_packet, uint32_t* n_packets, uint64_t* total,
                               void* stream);

/* ugo_fec_packet_encode (ugo_pkt.h) with two differences.  The bytes of
 * segment j of packet i are stream bytes [offset, offset + len) of member
 * conn_of[i], read at W[x & (cap-1)] -- data_off and avail are ignored, a
 * segment may straddle the wrap point.  And validation: a packet one of whose
 * segments is not inside its member's [base, tail) (an empty segment:
 * base <= offset <= tail) gets status UGO_PKT_OUT_OF_WINDOW, wire_lens[i] = 0
 * and an untouched slot (checked after the n_ranges / n_segments caps, before
 * everything else); a packet with conn_of[i] >= nconn gets status 0,
 * wire_lens[i] = 0 and an untouched slot.  Header bytes, SACK, framing, the
 * pad, statuses 6-9, the argument rules and the write extent -- exactly
 * [0, round_up(len, 16)) of a slot, each 16-B chunk once, zeros past the
 * packet's end -- are those of ugo_fec_packet_encode. */
int ugo_fec_stream_tx_set_encode(ugo_stream_tx_set* set, const ugo_pkt_info* info, const uint64_t* ranges,
                                 size_t max_ranges, const ugo_pkt_segment* segs, size_t max_segments,
                                 const uint32_t* conn_of, size_t npackets, const uint8_t* pad, unsigned flags,
                                 uint8_t* wire, size_t slot, uint16_t* wire_lens, uint8_t* status, void* stream);

/* The nconn records, in set order, after synchronising the stream of the last
 * call on the set. */
int ugo_fec_stream_tx_set_state(ugo_stream_tx_set* set, ugo_stream_tx_state* host_out /* [nconn] */);

#ifdef __cplusplus
}
#endif
#endif /* UGO_STREAM_H */
