/*
 * ugo_listen.h -- C-ABI of the connection table on the GPU: the demultiplexer
 * of a listening socket.  What ugo does per datagram, on the host and under
 * the listener's mutex, is
 *
 *   listener.handlePacket        ugo/listener.go:64-119
 *
 * a map lookup of remoteAddr.String() and, for an unknown address, the INIT
 * test that creates a connection.  Here one call routes a whole recvmmsg ring:
 * it writes the conn_of[npackets] array that ugo_fec_stream_set_deliver,
 * ugo_fec_ack_set_receive and ugo_fec_cc_sent_ack take, and the opposite call
 * turns the conn_of[] of ugo_fec_stream_tx_set_plan into sendmmsg names.
 *
 * Added within ABI version 9 (ugo_fec_abi_version() still returns 9): the
 * presence of the ugo_fec_listen_* symbols is the feature test.
 *
 * Conventions as in ugo_sent.h and ugo_cc.h: operands in device or pinned host
 * memory; every call stream-ordered with no host copy and no synchronisation;
 * argument errors return UGO_FEC_ERR_INVALID_ARG before any launch with
 * nothing written; output arrays are written whole; a lying descriptor (a
 * lens[i] beyond the slot, a conn_of[i] beyond the members) is clamped, never
 * followed.
 *
 * INPUTS as recvmmsg leaves them.  names[npackets] are rows of 32 bytes, the
 * array 16-B aligned; row i starts with the msg_name of datagram i, a Linux
 * sockaddr_in (16 bytes) or sockaddr_in6 (28 bytes); the rest of the row is
 * ignored.  pkts / slot / lens are the ring of ugo_fec_packet_decode: raw
 * bytes, before decryption (the reference demultiplexes before Decrypt).  The
 * length of packet i is min(lens[i], slot).
 *
 * THE KEY is what remoteAddr.String() distinguishes for a *net.UDPAddr: the
 * 16-byte IP (an AF_INET address and the v4-mapped AF_INET6 address are the
 * same key), the port, and the scope id (0 for AF_INET).  sin6_flowinfo is not
 * part of the key.  Any other family is no address: the packet gets class
 * UGO_LISTEN_BAD_NAME and UGO_STREAM_NO_CONN.
 *
 * THE RULE (ugo_fec_listen_route): handlePacket, per key, over the packets of
 * a call in batch order.  An INIT is a packet of length 22 whose byte 0 is 0
 * (packetInit); a dup-INIT is an INIT whose byte 1 is 0 (aesEncrypt).  For a
 * known key the reference tests both bytes, for an unknown key byte 0 only;
 * that asymmetry is kept.
 *
 *   Key known before the call, as member m:
 *     a dup-INIT          class DUP_INIT, conn_of[i] = NO_CONN
 *     anything else       class FED,      conn_of[i] = m
 *   Key unknown before the call; f = the lowest i of the call that is an INIT
 *   of this key:
 *     no f, or i < f      class STRANGER, NO_CONN
 *     i == f              class ACCEPT,   NO_CONN (the reference does not feed
 *                         the INIT to the new connection); the key becomes a
 *                         member
 *     i > f               as for a known key, FED reported as FED_NEW: the
 *                         connection was served in the batch that created it
 *
 *   New members are numbered nconn, nconn + 1, ... in the batch order of their
 *   ACCEPT packets, the order in which the reference appends to l.pending.
 *   Each gets one row of accepted[], in the same order: the packet index, the
 *   member, the client connection id BE32(pkts[i][18:22]) and the 32-byte name
 *   row of the accepting datagram with sin6_flowinfo and the bytes past the
 *   address length zeroed.  *n_accepted is how many the call accepted; it is
 *   the one word the host reads back per batch.  A max_accepted below it
 *   truncates the list only: the members exist and the full count is reported.
 *   The host then does what stays the host's: the crand connection id, the
 *   4-byte reply, the windows and the rebuild of its sets.
 *
 * THE ORDER a caller keeps per batch, on one stream: ugo_fec_listen_route
 * first (it needs only the raw ring), then ugo_fec_packet_decode and the
 * stages that take conn_of.  The caller reads *n_accepted with the other sizes
 * of the batch; if it is not zero it creates the new connections' windows and
 * rebuilds its sets before ugo_fec_stream_set_deliver, so
 * that the FED_NEW packets of the batch find their member.  After
 * ugo_fec_stream_tx_set_plan, ugo_fec_listen_names gives the sendmmsg names.
 * When connections close, ugo_fec_listen_remap goes with the set rebuild.
 *
 * DEVIATIONS from the reference, all on purpose:
 *   (a) there is no receivedPackets queue of 1024: every fed packet is fed.
 *   (b) new keys past max_conn, in the batch order of their first INIT, are
 *       refused: that INIT gets class REFUSED, the key's other packets
 *       STRANGER, and the key's slot is dead (counted in n_dead) until the
 *       next remap.  A dead key stays unknown: in a later call its first INIT
 *       is REFUSED again, without another dead slot.
 *   (c) a call in which an INIT of an unknown key finds no free slot sets
 *       err = UGO_LISTEN_FULL.  Known keys still route exactly; which unknown
 *       keys of that call were accepted is unspecified (those that found no
 *       slot are STRANGER); the table stays consistent: no key twice, no
 *       member twice.  remap clears the error.
 *   (d) a data packet whose ciphertext happens to look like an INIT is judged
 *       as the reference judges it.
 * Checked on the CPU against a per-packet replay of listener.go
 * (tests/listen_ref.py, tests/test_listen.py) and on the device against the
 * rule (tests/listen_harness.py).
 */
#ifndef UGO_LISTEN_H
#define UGO_LISTEN_H

#include <stddef.h>
#include <stdint.h>

#include "ugo_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel class of every launch of this header (ugo_fec_launch_time.kernel). */
#define UGO_FEC_KERNEL_LISTEN 15

#define UGO_LISTEN_MAX_CONN (1u << 20)
#define UGO_LISTEN_NAME_BYTES 32

/* cls[i] */
#define UGO_LISTEN_FED 0
#define UGO_LISTEN_FED_NEW 1
#define UGO_LISTEN_DUP_INIT 2
#define UGO_LISTEN_ACCEPT 3
#define UGO_LISTEN_STRANGER 4
#define UGO_LISTEN_REFUSED 5
#define UGO_LISTEN_BAD_NAME 6
#define UGO_LISTEN_NCLASS 8 /* counts[] of the state; class 7 is not used */

/* ugo_listen_state.err */
#define UGO_LISTEN_FULL 1

/* *status of ugo_fec_listen_remap: 0, or these bits. */
#define UGO_LISTEN_REMAP_NOT_INJECTIVE 1
#define UGO_LISTEN_REMAP_OUT_OF_RANGE 2
#define UGO_LISTEN_REMAP_TOO_MANY 4 /* nconn_new > max_conn */
#define UGO_LISTEN_REMAP_LENGTH 8   /* n_index is not the table's nconn */

/* One new member of a call (48 bytes). */
typedef struct ugo_listen_accept {
  uint32_t packet;    /* i of the ACCEPT packet */
  uint32_t member;
  uint32_t client_id; /* BE32(pkts[i][18:22]) */
  uint32_t reserved;
  uint8_t name[UGO_LISTEN_NAME_BYTES];
} ugo_listen_accept;

/* The table's record (80 bytes).  counts[] are cumulative over the calls. */
typedef struct ugo_listen_state {
  uint32_t nconn;   /* members 0 .. nconn-1 */
  uint32_t n_dead;  /* dead slots, deviation (b) */
  uint32_t n_slots; /* a power of two chosen by create */
  uint32_t err;     /* 0 or UGO_LISTEN_FULL */
  uint64_t counts[UGO_LISTEN_NCLASS];
} ugo_listen_state;

/* One live entry (32 bytes): THE KEY and its member. */
typedef struct ugo_listen_entry {
  uint8_t ip[16];
  uint32_t scope;
  uint32_t port;
  uint32_t member; /* UGO_STREAM_NO_CONN: no entry in this row */
  uint32_t reserved;
} ugo_listen_entry;

typedef struct ugo_listen_table ugo_listen_table;

/* An empty table for up to max_conn members, 1 <= max_conn <=
 * UGO_LISTEN_MAX_CONN, with max(16, the power of two >= 2 * max_conn) slots. */
int ugo_fec_listen_create(ugo_fec* ctx, size_t max_conn, ugo_listen_table** out);
void ugo_fec_listen_destroy(ugo_listen_table* table);

/* The record, after synchronising the stream of the last call on the table. */
int ugo_fec_listen_state(ugo_listen_table* table, ugo_listen_state* host_out);

/* THE RULE.  names 16-B aligned; pkts, slot and lens under the rules of
 * ugo_fec_packet_decode (pkts 16-B aligned, slot a multiple of 16, 0 < slot <=
 * 65535); npackets <= 2^31, 0 is a no-op.  conn_of uint32 [npackets], cls uint8
 * [npackets] and *n_accepted are written whole, accepted[] (16-B aligned, may
 * be NULL with max_accepted 0) up to min(*n_accepted, max_accepted) rows.
 * conn_of serves as the call's scratch before it gets its values. */
int ugo_fec_listen_route(ugo_listen_table* table, const uint8_t* names, const uint8_t* pkts, size_t slot,
                         const uint16_t* lens, size_t npackets, uint32_t* conn_of, uint8_t* cls,
                         ugo_listen_accept* accepted, size_t max_accepted, uint32_t* n_accepted, void* stream);

/* Member m becomes new_index[m]; UGO_STREAM_NO_CONN closes it (the delete of
 * the close callback); the table has nconn_new members afterwards (numbers no
 * member maps to have no entry) and is rebuilt without dead slots; err is
 * cleared.  new_index uint32 [n_index], n_index the table's nconn.  If
 * new_index is not injective, names a member >= nconn_new, nconn_new >
 * max_conn or n_index is not nconn, nothing is applied and *status says so. */
int ugo_fec_listen_remap(ugo_listen_table* table, const uint32_t* new_index, size_t n_index, size_t nconn_new,
                         uint32_t* status, void* stream);

/* The sendmmsg side: for packet i the stored name row of member conn_of[i]
 * into names_out (rows of 32 bytes, 16-B aligned) and its length (16 or 28)
 * into name_lens uint32 [npackets]; zeros and length 0 for conn_of[i] >= nconn
 * or a number without an entry. */
int ugo_fec_listen_names(ugo_listen_table* table, const uint32_t* conn_of, size_t npackets, uint8_t* names_out,
                         uint32_t* name_lens, void* stream);

/* For tests and the shim: row m of out[cap] (16-B aligned) gets the entry of
 * member m as the slots hold it, member UGO_STREAM_NO_CONN and zeros for m >=
 * nconn or a number without an entry. */
int ugo_fec_listen_entries(ugo_listen_table* table, ugo_listen_entry* out, size_t cap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UGO_LISTEN_H */
