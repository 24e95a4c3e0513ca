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

#ifdef __cplusplus
}
#endif
#endif /* UGO_STREAM_H */
