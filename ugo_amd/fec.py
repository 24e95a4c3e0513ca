"""Python host mirror of the reedsolomon.Encoder subset used by jflyup/ugo.

ugo/fec.go drives klauspost/reedsolomon through three calls:
  reedsolomon.New(dataShards, parityShards)   ugo/fec.go:59
  enc.Reconstruct(shards)                     ugo/fec.go:202
  enc.Encode(shards)                          ugo/fec.go:238
This module exposes the same names and argument meaning over the C-ABI in
include/ugo_fec.h (libugofec.so, gfx950 kernels):

* ``New(d, p, device=0)`` -> ``Encoder`` (raises ``ErrInvShardNum`` /
  ``ErrMaxShardNum`` like upstream ``New``).
* ``Encoder.Encode(shards)`` / ``Encoder.Reconstruct(shards)`` /
  ``Encoder.ReconstructData(shards)``: Go-shaped, one group per call, shards
  are a list of ``bytearray`` (``None`` or empty = missing), same error
  behaviour (``ErrTooFewShards``, ``ErrShardNoData``, ``ErrShardSize``).
* ``Encoder.encode_batch`` / ``reconstruct_batch``: the device-resident batch
  form (torch uint8 tensors on the GPU, shape [groups, d+p, pitch]).
* ``Encoder.encode_host`` / ``reconstruct_host``: host numpy batches, staged
  through the engine's pipelined H2D -> kernel -> D2H path.

There is no CPU fallback: if libugofec.so is missing the import fails, and
every compute call needs a gfx950 device.
"""
from __future__ import annotations

import ctypes
import os
import re
import weakref
from typing import List, Optional, Sequence

import numpy as np

try:  # load torch first so libugofec.so binds torch's libamdhip64.so.7 (same soname)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the host-only paths
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# UGO_FEC_LIB: another build of the same library (interleaved A/B runs in tools/)
LIB_PATH = os.environ.get("UGO_FEC_LIB") or os.path.join(_HERE, "libugofec.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_fec.h")
CONN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_fec_conn.h")
PKT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_pkt.h")
STREAM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_stream.h")
ACK_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_ack.h")
SENT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_sent.h")
CC_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_cc.h")
LISTEN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_listen.h")
LOOP_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ugo_loop.h")

OK = 0
RECONSTRUCT_DATA_ONLY = 1


class FecError(Exception):
    code = -1


class ErrInvShardNum(FecError):
    code = 1


class ErrMaxShardNum(FecError):
    code = 2


class ErrTooFewShards(FecError):
    code = 3


class ErrShardNoData(FecError):
    code = 4


class ErrShardSize(FecError):
    code = 5


class ErrInvalidArg(FecError):
    code = 6


class ErrSingular(FecError):
    code = 7


class ErrHip(FecError):
    code = 8


class ErrNoDevice(FecError):
    code = 9


_ERRORS = {c.code: c for c in (ErrInvShardNum, ErrMaxShardNum, ErrTooFewShards, ErrShardNoData,
                                ErrShardSize, ErrInvalidArg, ErrSingular, ErrHip, ErrNoDevice)}

_lib = None

# include/ugo_pkt.h
PKT_FEC_FRAMED = 1
PKT_CAPACITY = 6
PKT_INCONSISTENT_LARGEST_ACKED = 7  # packet_encode's per-packet statuses
PKT_INCONSISTENT_LOWEST_ACKED = 8
PKT_INCONSISTENT_RANGE_COUNT = 9
PKT_OUT_OF_WINDOW = 10  # stream_tx set_encode: a segment outside its send window
PKT_INFO_DTYPE = np.dtype([("packet_number", "<u8"), ("stop_waiting", "<u8"), ("largest_acked", "<u8"),
                           ("largest_in_order", "<u8"), ("delay_us", "<u8"), ("status", "<u4"),
                           ("payload_off", "<u4"), ("n_ranges", "<u2"), ("n_segments", "<u2"), ("flags", "u1"),
                           ("fec_flag_lo", "u1"), ("reserved", "u1", (10,))])
# include/ugo_fec.h launch timing
KERNEL_NAMES = {1: "encode", 2: "reconstruct", 3: "prepare", 4: "bytes", 5: "rx_assemble", 6: "tx_assemble",
                7: "packet_decode", 8: "packet_encode", 9: "stream_deliver", 10: "stream_read", 11: "stream_tx",
                12: "ack", 13: "sent", 14: "cc", 15: "listen", 16: "loop"}
KERNEL_IDS = {v: k for k, v in KERNEL_NAMES.items()}
LAUNCH_TIME_DTYPE = np.dtype([("kernel", "<u4"), ("ms", "<f4")])
PKT_SEGMENT_DTYPE = np.dtype([("offset", "<u8"), ("data_off", "<u4"), ("len", "<u2"), ("avail", "<u2")])
assert PKT_INFO_DTYPE.itemsize == 64 and PKT_SEGMENT_DTYPE.itemsize == 16
# include/ugo_stream.h: ugo_stream_status (per segment; the last two are the connection's err) and the record
STREAM_NONE = 0
STREAM_ACCEPTED = 1
STREAM_DUPLICATE = 2
STREAM_OUT_OF_WINDOW = 3
STREAM_OVERLAP = 4
STREAM_TOO_MANY_GAPS = 5
STREAM_MAX_GAPS = 50
STREAM_MIN_WINDOW = 4096
STREAM_NO_CONN = 0xffffffff   # conn_of: the packet belongs to no member of the set
STREAM_SET_MAX_CONN = 1 << 20
STREAM_STATE_DTYPE = np.dtype([("read_pos", "<u8"), ("head_off", "<u8"), ("hi", "<u8"), ("readable", "<u8"),
                               ("accepted", "<u8"), ("duplicate", "<u8"), ("out_of_window", "<u8"),
                               ("skipped_packets", "<u8"), ("ordered_segments", "<u8"), ("err_packet", "<u8"),
                               ("err_segment", "<u4"), ("err", "<u4"), ("ngaps", "<u4"), ("head_valid", "u1"),
                               ("eof", "u1"), ("reserved", "u1", (2,))])
assert STREAM_STATE_DTYPE.itemsize == 96
# include/ugo_stream.h, send windows
STREAM_TX_MAX_WINDOW = 1 << 31
STREAM_TX_HEADER = 4  # frameHeaderLen of segment_sender.go: H of THE RULE
STREAM_TX_RQ_QUEUED = 1
STREAM_TX_RQ_REJECTED = 2
STREAM_TX_RQ_FULL = 3
STREAM_TX_RQ_UNSORTED = 4
STREAM_TX_RQ_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("reserved", "<u4")])
STREAM_TX_STATE_DTYPE = np.dtype([("base", "<u8"), ("write_pos", "<u8"), ("tail", "<u8"),
                                  ("last_packet_number", "<u8"), ("packets", "<u8"), ("segments", "<u8"),
                                  ("bytes_new", "<u8"), ("bytes_retransmitted", "<u8"), ("rq_rejected", "<u8"),
                                  ("rq_len", "<u4"), ("rq_head", "<u4")])
assert STREAM_TX_STATE_DTYPE.itemsize == 80 and STREAM_TX_RQ_DTYPE.itemsize == 16
# include/ugo_ack.h, receive histories
ACK_MIN_WINDOW = 1024
ACK_MAX_WINDOW = 1 << 20
ACK_MAX_OUTSTANDING = 1000
ACK_TOO_MANY_OUTSTANDING = 1  # ugo_ack_state.err
ACK_NOT_ATTACHED, ACK_ATTACHED, ACK_TRUNCATED = 0, 1, 2  # attach's attached[c]
ACK_STATE_DTYPE = np.dtype([("largest_in_order", "<u8"), ("largest_observed", "<u8"), ("ignore_below", "<u8"),
                            ("lo_time_us", "<u8"), ("fresh", "<u8"), ("old", "<u8"), ("out_of_window", "<u8"),
                            ("outstanding", "<u4"), ("changed", "u1"), ("err", "u1"), ("reserved", "u1", (2,))])
assert ACK_STATE_DTYPE.itemsize == 64

# include/ugo_sent.h, sent histories
SENT_MIN_WINDOW = 1024
SENT_MAX_WINDOW = 1 << 20
SENT_MAX_SEG_CAP = 16
SENT_TOO_MANY_TRACKED = 1  # ugo_sent_state.err
SENT_IN_FLIGHT, SENT_QUEUED = 0, 1  # ugo_sent_slot.state
SENT_RTO_DEFAULT_US, SENT_RTO_MIN_US, SENT_RTO_MAX_US = 500_000, 200_000, 60_000_000
SENT_SLOT_DTYPE = np.dtype([("packet_number", "<u8"), ("sent_us", "<u8"), ("min_offset", "<u8"), ("len", "<u4"),
                            ("state", "u1"), ("missing", "u1"), ("n_segments", "u1"), ("bits", "u1")])
SENT_SEG_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("reserved", "<u4")])  # ugo_stream_tx_rq_entry
SENT_STATE_DTYPE = np.dtype([("last_sent", "<u8"), ("lio", "<u8"), ("largest_acked", "<u8"),
                             ("largest_with_ack", "<u8"), ("least_unacked", "<u8"), ("bytes_in_flight", "<u8"),
                             ("last_sent_us", "<u8"), ("scan_from", "<u8"), ("acked_packets", "<u8"),
                             ("acked_bytes", "<u8"), ("lost_packets", "<u8"), ("lost_bytes", "<u8"),
                             ("duplicates", "<u8"), ("unsent_acks", "<u8"), ("stale", "<u8"), ("tracked", "<u4"),
                             ("queued", "<u4"), ("queued_segments", "<u4"), ("rto_count", "<u4"),
                             ("sw_pending", "u1"), ("err", "u1"), ("reserved", "u1", (22,))])
SENT_EVENT_DTYPE = np.dtype([("rtt_us", "<u8"), ("delay_us", "<u8"), ("acked_bytes", "<u8"), ("lost_bytes", "<u8"),
                             ("bytes_in_flight", "<u8"), ("largest_acked", "<u8"), ("acked_packets", "<u4"),
                             ("lost_packets", "<u4"), ("accepted", "u1"), ("has_rtt", "u1"),
                             ("reserved", "u1", (6,))])
assert SENT_SLOT_DTYPE.itemsize == 32 and SENT_SEG_DTYPE.itemsize == 16
assert SENT_STATE_DTYPE.itemsize == 160 and SENT_EVENT_DTYPE.itemsize == 64

# include/ugo_cc.h, congestion control
CC_MAX_CWND_LIMIT = 1 << 20
CC_DEFAULTS = dict(initial_cwnd=32, max_cwnd=200, min_cwnd=2, num_connections=2, mss=1460)
CC_PARAMS_DTYPE = np.dtype([("initial_cwnd", "<u4"), ("max_cwnd", "<u4"), ("min_cwnd", "<u4"),
                            ("num_connections", "<u4"), ("mss", "<u4")])
CC_ROW_DTYPE = np.dtype([("max_lost", "<u8"), ("max_acked", "<u8"), ("acked_le", "<u4"), ("reserved", "u1", (12,))])
CC_STATE_DTYPE = np.dtype([("cwnd", "<u8"), ("ssthresh", "<u8"), ("largest_acked", "<u8"), ("cutback", "<u8"),
                           ("min_rtt_us", "<u8"), ("latest_rtt_us", "<u8"), ("srtt_us", "<u8"),
                           ("mean_dev_us", "<u8"), ("end_packet_number", "<u8"), ("current_min_rtt_us", "<u8"),
                           ("epoch_us", "<u8"), ("app_limited_us", "<u8"), ("last_update_us", "<u8"),
                           ("last_cwnd", "<u8"), ("last_max_cwnd", "<u8"), ("est_tcp_cwnd", "<u8"),
                           ("origin_cwnd", "<u8"), ("last_target_cwnd", "<u8"), ("rto_candidate", "<u8"),
                           ("cutbacks", "<u8"), ("rtos", "<u8"), ("sample_count", "<u4"), ("acked_count", "<u4"),
                           ("time_to_origin", "<u4"), ("last_cutback_exited_slowstart", "u1"), ("started", "u1"),
                           ("found", "u1"), ("reserved", "u1", (9,))])
assert CC_PARAMS_DTYPE.itemsize == 20 and CC_ROW_DTYPE.itemsize == 32 and CC_STATE_DTYPE.itemsize == 192
# ugo_listen.h
LISTEN_MAX_CONN = 1 << 20
LISTEN_NAME_BYTES = 32
LISTEN_FED, LISTEN_FED_NEW, LISTEN_DUP_INIT, LISTEN_ACCEPT = 0, 1, 2, 3
LISTEN_STRANGER, LISTEN_REFUSED, LISTEN_BAD_NAME = 4, 5, 6
LISTEN_NCLASS = 8
LISTEN_FULL = 1  # ugo_listen_state.err
LISTEN_REMAP_NOT_INJECTIVE, LISTEN_REMAP_OUT_OF_RANGE, LISTEN_REMAP_TOO_MANY, LISTEN_REMAP_LENGTH = 1, 2, 4, 8
LISTEN_ACCEPT_DTYPE = np.dtype([("packet", "<u4"), ("member", "<u4"), ("client_id", "<u4"), ("reserved", "<u4"),
                                ("name", "u1", (32,))])
LISTEN_STATE_DTYPE = np.dtype([("nconn", "<u4"), ("n_dead", "<u4"), ("n_slots", "<u4"), ("err", "<u4"),
                               ("counts", "<u8", (8,))])
LISTEN_ENTRY_DTYPE = np.dtype([("ip", "u1", (16,)), ("scope", "<u4"), ("port", "<u4"), ("member", "<u4"),
                               ("reserved", "<u4")])
assert (LISTEN_ACCEPT_DTYPE.itemsize == 48 and LISTEN_STATE_DTYPE.itemsize == 80 and
        LISTEN_ENTRY_DTYPE.itemsize == 32)
# include/ugo_loop.h, the connection loop
LOOP_DEFAULTS = dict(ack_delay_us=5000, idle_us=300000000, max_retries=10)
LOOP_PEER_ACK_FIN, LOOP_PEER_RST, LOOP_BAD_PACKET, LOOP_CLOSED, LOOP_FAILURES, LOOP_SENT_ERR = 1, 2, 3, 4, 5, 6
LOOP_ACK_ERR, LOOP_STREAM_ERR, LOOP_IDLE, LOOP_LINGER, LOOP_ABORT = 7, 8, 9, 10, 11
LOOP_PENDING_NONE, LOOP_PENDING_FIN, LOOP_PENDING_RST = 0, 1, 2
LOOP_HOW_CLOSE, LOOP_HOW_ABORT, LOOP_HOW_NODELAY_ON, LOOP_HOW_NODELAY_OFF = 1, 2, 4, 8
LOOP_PARAMS_DTYPE = np.dtype([("ack_delay_us", "<u8"), ("idle_us", "<u8"), ("max_retries", "<u4"),
                              ("reserved", "<u4")])
LOOP_STATE_DTYPE = np.dtype([("last_activity_us", "<u8"), ("origin_ack_us", "<u8"), ("linger_deadline_us", "<u8"),
                             ("exit_us", "<u8"), ("dropped", "<u8"), ("closed", "u1"), ("fin_sent", "u1"),
                             ("fin_rcvd", "u1"), ("ack_no_delay", "u1"), ("exited", "u1"), ("reason", "u1"),
                             ("pending", "u1"), ("reported", "u1"), ("reserved", "u1", (16,))])
assert LOOP_PARAMS_DTYPE.itemsize == 24 and LOOP_STATE_DTYPE.itemsize == 64


def load_library(path: str = LIB_PATH):
    """Load libugofec.so.  Raises loudly if it was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run `make -C ugo_amd/csrc` (or __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    sz, vp, i, u = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    lib.ugo_fec_create.argtypes = [i, i, i, ctypes.POINTER(vp)]
    lib.ugo_fec_destroy.argtypes = [vp]
    lib.ugo_fec_destroy.restype = None
    lib.ugo_fec_geometry.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(i)]
    lib.ugo_fec_matrix.argtypes = [vp, vp]
    lib.ugo_fec_encode.argtypes = [vp, vp, sz, sz, sz, vp]
    lib.ugo_fec_reconstruct.argtypes = [vp, vp, vp, sz, sz, sz, u, vp, vp]
    lib.ugo_fec_encode_strided.argtypes = [vp, vp, sz, sz, sz, sz, vp]
    lib.ugo_fec_reconstruct_strided.argtypes = [vp, vp, vp, sz, sz, sz, sz, u, vp, vp]
    lib.ugo_fec_reconstruct_into.argtypes = [vp, vp, vp, sz, sz, sz, sz, vp, sz, sz, u, vp, vp]
    lib.ugo_fec_encode_host.argtypes = [vp, vp, sz, sz, sz]
    lib.ugo_fec_reconstruct_host.argtypes = [vp, vp, vp, sz, sz, sz, u, vp]
    lib.ugo_fec_service_start.argtypes = [vp, u]
    lib.ugo_fec_service_stop.argtypes = [vp]
    lib.ugo_fec_service_config.argtypes = [vp, u, u, u]
    lib.ugo_fec_poisoned.argtypes = [vp]
    lib.ugo_fec_check_shards.argtypes = [i, vp, i, ctypes.POINTER(sz)]
    lib.ugo_fec_host_alloc.argtypes = [sz, ctypes.POINTER(vp)]
    lib.ugo_fec_host_free.argtypes = [vp]
    lib.ugo_fec_strerror.argtypes = [i]
    lib.ugo_fec_strerror.restype = ctypes.c_char_p
    lib.ugo_fec_abi_version.argtypes = []
    lib.ugo_fec_rx_assemble.argtypes = [vp, vp, sz, vp, sz, vp, ctypes.c_uint64, sz, vp, sz, sz, sz, vp, vp, vp]
    lib.ugo_fec_rx_assemble_frames.argtypes = lib.ugo_fec_rx_assemble.argtypes
    lib.ugo_fec_rc4_keystream.argtypes = [vp, sz, vp, sz]
    lib.ugo_fec_tx_assemble.argtypes = [vp, vp, sz, vp, sz, ctypes.c_uint32, vp, sz, vp, sz, vp, vp, vp]
    lib.ugo_fec_packet_decode.argtypes = [vp, vp, sz, vp, sz, vp, u, vp, vp, sz, vp, sz, vp]
    lib.ugo_fec_packet_encode.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, sz, vp, u, vp, sz, vp, vp, vp]
    lib.ugo_fec_stream_rx_create.argtypes = [vp, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_stream_rx_destroy.argtypes = [vp]
    lib.ugo_fec_stream_rx_destroy.restype = None
    lib.ugo_fec_stream_deliver.argtypes = [vp, vp, sz, vp, vp, vp, sz, sz, vp, vp]
    lib.ugo_fec_stream_read.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ugo_fec_stream_rx_state.argtypes = [vp, vp]
    lib.ugo_fec_stream_rx_window.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.ugo_fec_stream_set_create.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_stream_set_destroy.argtypes = [vp]
    lib.ugo_fec_stream_set_destroy.restype = None
    lib.ugo_fec_stream_set_deliver.argtypes = [vp, vp, sz, vp, vp, vp, sz, sz, vp, vp, vp]
    lib.ugo_fec_stream_set_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.ugo_fec_stream_set_state.argtypes = [vp, vp]
    u64 = ctypes.c_uint64
    lib.ugo_fec_stream_tx_create.argtypes = [vp, sz, sz, u64, u64, ctypes.POINTER(vp)]
    lib.ugo_fec_stream_tx_destroy.argtypes = [vp]
    lib.ugo_fec_stream_tx_destroy.restype = None
    lib.ugo_fec_stream_tx_window.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.ugo_fec_stream_tx_queue.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.ugo_fec_stream_tx_set_create.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_stream_tx_set_destroy.argtypes = [vp]
    lib.ugo_fec_stream_tx_set_destroy.restype = None
    lib.ugo_fec_stream_tx_set_write.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.ugo_fec_stream_tx_set_release.argtypes = [vp, vp, vp]
    lib.ugo_fec_stream_tx_set_retransmit.argtypes = [vp, vp, vp, vp, sz, vp, vp]
    lib.ugo_fec_stream_tx_set_plan.argtypes = [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.ugo_fec_stream_tx_set_encode.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, vp, u, vp, sz, vp, vp, vp]
    lib.ugo_fec_stream_tx_set_state.argtypes = [vp, vp]
    lib.ugo_fec_ack_rx_create.argtypes = [vp, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_ack_rx_destroy.argtypes = [vp]
    lib.ugo_fec_ack_rx_destroy.restype = None
    lib.ugo_fec_ack_rx_state.argtypes = [vp, vp]
    lib.ugo_fec_ack_rx_bitmap.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.ugo_fec_ack_set_create.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_ack_set_destroy.argtypes = [vp]
    lib.ugo_fec_ack_set_destroy.restype = None
    lib.ugo_fec_ack_set_receive.argtypes = [vp, vp, vp, sz, vp, sz, u64, vp]
    lib.ugo_fec_ack_set_touch.argtypes = [vp, vp, vp]
    lib.ugo_fec_ack_set_attach.argtypes = [vp, u64, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp]
    lib.ugo_fec_ack_set_state.argtypes = [vp, vp]
    lib.ugo_fec_sent_tx_create.argtypes = [vp, sz, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_sent_tx_destroy.argtypes = [vp]
    lib.ugo_fec_sent_tx_destroy.restype = None
    lib.ugo_fec_sent_tx_slots.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.ugo_fec_sent_tx_segments.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.ugo_fec_sent_tx_scratch.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.ugo_fec_sent_set_create.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_sent_set_destroy.argtypes = [vp]
    lib.ugo_fec_sent_set_destroy.restype = None
    lib.ugo_fec_sent_set_record.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, u64, vp]
    lib.ugo_fec_sent_set_ack.argtypes = [vp, vp, vp, sz, vp, sz, u64, vp, vp]
    lib.ugo_fec_sent_set_rto.argtypes = [vp, vp, u64, vp, vp]
    lib.ugo_fec_sent_set_drain.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.ugo_fec_sent_set_attach.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    lib.ugo_fec_sent_set_state.argtypes = [vp, vp]
    lib.ugo_fec_cc_set_create.argtypes = [vp, vp, vp, ctypes.POINTER(vp)]
    lib.ugo_fec_cc_set_destroy.argtypes = [vp]
    lib.ugo_fec_cc_set_destroy.restype = None
    lib.ugo_fec_cc_set_cutback.argtypes = [vp, ctypes.POINTER(vp)]
    lib.ugo_fec_cc_sent_ack.argtypes = [vp, vp, vp, sz, vp, sz, u64, vp, vp, vp, vp]
    lib.ugo_fec_cc_set_ack.argtypes = [vp, vp, vp, u64, vp, vp]
    lib.ugo_fec_cc_set_rto.argtypes = [vp, vp, sz, sz, vp, vp]
    lib.ugo_fec_cc_set_state.argtypes = [vp, vp]
    lib.ugo_fec_listen_create.argtypes = [vp, sz, ctypes.POINTER(vp)]
    lib.ugo_fec_listen_destroy.argtypes = [vp]
    lib.ugo_fec_listen_destroy.restype = None
    lib.ugo_fec_listen_state.argtypes = [vp, vp]
    lib.ugo_fec_listen_route.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp]
    lib.ugo_fec_listen_remap.argtypes = [vp, vp, sz, sz, vp, vp]
    lib.ugo_fec_listen_names.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ugo_fec_listen_entries.argtypes = [vp, vp, sz, vp]
    lib.ugo_fec_loop_set_create.argtypes = [vp, vp, vp, vp, vp, vp, u64, ctypes.POINTER(vp)]
    lib.ugo_fec_loop_set_destroy.argtypes = [vp]
    lib.ugo_fec_loop_set_destroy.restype = None
    lib.ugo_fec_loop_set_receive.argtypes = [vp, vp, vp, sz, u64, vp]
    lib.ugo_fec_loop_set_close.argtypes = [vp, vp, vp, u64, vp]
    lib.ugo_fec_loop_set_check.argtypes = [vp, u64, vp, vp, vp]
    lib.ugo_fec_loop_set_append.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp, vp, vp]
    lib.ugo_fec_loop_set_sent.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.ugo_fec_loop_set_state.argtypes = [vp, vp]
    lib.ugo_fec_reconstruct_rows.argtypes = [vp, vp, vp, sz, sz, vp, sz, sz, u, vp, vp]
    lib.ugo_fec_lossy_groups.argtypes = [vp, vp, sz, u, vp, vp, vp]
    lib.ugo_fec_rx_recover_host.argtypes = [vp, vp, sz, vp, sz, vp, ctypes.c_uint64, sz, sz, vp, vp, vp, sz, sz, vp,
                                            ctypes.POINTER(sz)]
    lib.ugo_fec_tx_assemble_host.argtypes = [vp, vp, sz, vp, sz, ctypes.c_uint32, vp, sz, vp, sz, vp, vp]
    lib.ugo_fec_set_tx_host_route.argtypes = [vp, ctypes.c_int]
    lib.ugo_fec_set_host_copy_queue.argtypes = [vp, ctypes.c_int]
    lib.ugo_fec_reconstruct_list.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, sz, sz, vp, sz, sz, u, vp, vp]
    lib.ugo_fec_recover_data.argtypes = [vp, vp, vp, sz, sz, sz, sz, vp, sz, sz, vp, vp, vp]
    lib.ugo_fec_device_address.argtypes = [vp, vp, ctypes.POINTER(vp)]
    lib.ugo_fec_timing_begin.argtypes = [vp, sz]
    lib.ugo_fec_timing_end.argtypes = [vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    _lib = lib
    return lib


HEADER_PATHS = (HEADER_PATH, CONN_HEADER_PATH, PKT_HEADER_PATH, STREAM_HEADER_PATH, ACK_HEADER_PATH,
                SENT_HEADER_PATH, CC_HEADER_PATH, LISTEN_HEADER_PATH, LOOP_HEADER_PATH)


def header_symbols(paths=HEADER_PATHS) -> List[str]:
    """Every entry point declared in include/ugo_fec.h, ugo_fec_conn.h, ugo_pkt.h, ugo_stream.h, ugo_ack.h,
    ugo_sent.h, ugo_cc.h, ugo_listen.h and ugo_loop.h."""
    out = set()
    for path in paths:
        src = open(path).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        out |= set(re.findall(r"\b(ugo_fec(?:conn)?_[a-z0-9_]+)\s*\(", src))
    return sorted(out)


def header_stream_symbols(paths=HEADER_PATHS) -> List[str]:
    """The entry points of header_symbols() whose prototype ends in `void* stream`: the stream-ordered calls."""
    out = set()
    for path in paths:
        src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        for name, params in re.findall(r"\b(ugo_fec(?:conn)?_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
            if re.search(r"\bvoid\s*\*\s*stream\s*$", params):
                out.add(name)
    return sorted(out)


def strerror(code: int) -> str:
    return load_library().ugo_fec_strerror(code).decode()


def _require(cond, msg: str = "argument does not match the batch layout the entry point expects"):
    """Argument checks that guard device memory (sizes the kernels index by):
    explicit, so they hold under `python -O` too."""
    if not cond:
        raise ValueError(msg)


def _raise(code: int):
    if code != OK:
        raise _ERRORS.get(code, FecError)(f"{strerror(code)} (status {code})")


def check_shards(lens: Sequence[int], nil_ok: bool) -> int:
    """klauspost checkShards over shard lengths; returns the shard size."""
    lib = load_library()
    arr = (ctypes.c_size_t * len(lens))(*lens)
    out = ctypes.c_size_t(0)
    _raise(lib.ugo_fec_check_shards(len(lens), ctypes.cast(arr, ctypes.c_void_p), int(nil_ok),
                                    ctypes.byref(out)))
    return out.value


def _stream_handle(stream) -> Optional[int]:
    if stream is None and torch is not None and torch.cuda.is_available():
        stream = torch.cuda.current_stream()
    if stream is None:
        return None
    return int(getattr(stream, "cuda_stream", stream))


class Encoder:
    """A (d, p) code bound to one GPU (reedsolomon.Encoder equivalent)."""

    def __init__(self, data_shards: int, parity_shards: int, device: int = 0):
        lib = load_library()
        h = ctypes.c_void_p()
        _raise(lib.ugo_fec_create(device, data_shards, parity_shards, ctypes.byref(h)))
        self._h = h
        self.DataShards = data_shards
        self.ParityShards = parity_shards
        self.Shards = data_shards + parity_shards
        self.mask_words = (self.Shards + 63) // 64  # presence words per group (include/ugo_fec.h)
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_destroy(self._h)
            self._h = None
        if getattr(self, "_stage_buf", None) is not None:
            host_free(self._stage_buf)
            self._stage_buf = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def matrix(self) -> np.ndarray:
        out = np.zeros((self.Shards, self.DataShards), np.uint8)
        _raise(load_library().ugo_fec_matrix(self._h, out.ctypes.data))
        return out

    # -------------------------------------------------- device-resident batch
    def _geom(self, shards, shard_major: bool):
        """(groups, pitch, row_stride, group_stride) of a uint8 tensor whose
        last dimension is contiguous: group-major [G, d+p, pitch] or
        shard-major [d+p, G, pitch] (planar); the row and group strides are the
        tensor's own (a padded row stride is a strided view)."""
        _require(shards.dim() == 3 and shards.element_size() == 1 and shards.stride(2) == 1)
        if shard_major:
            n, G, pitch = shards.shape
            rs, gs = shards.stride(0), shards.stride(1)
        else:
            G, n, pitch = shards.shape
            gs, rs = shards.stride(0), shards.stride(1)
        _require(n == self.Shards, f"expected {self.Shards} rows per group, got {n}")
        return G, pitch, rs, gs

    def encode_batch(self, shards, shard_size: Optional[int] = None, stream=None, shard_major: bool = False):
        """Encode every group of a device tensor: [G, d+p, pitch] (default) or,
        with shard_major=True, the planar [d+p, G, pitch] layout."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        S = pitch if shard_size is None else shard_size
        _raise(load_library().ugo_fec_encode_strided(self._h, shards.data_ptr(), G, S, rs, gs,
                                                     _stream_handle(stream)))

    def reconstruct_batch(self, shards, present, shard_size: Optional[int] = None, data_only=False,
                          status=None, stream=None, shard_major: bool = False):
        """present: int64/uint64 CUDA tensor [G] of presence bitmasks (bit r = shard r
        non-empty), [G][W] words for d+p > 64 (W = mask_words); status: optional int8
        CUDA tensor [G]."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G * self.mask_words and present.element_size() == 8)
        S = pitch if shard_size is None else shard_size
        st = None if status is None else status.data_ptr()
        _raise(load_library().ugo_fec_reconstruct_strided(self._h, shards.data_ptr(), present.data_ptr(), G, S, rs,
                                                          gs, RECONSTRUCT_DATA_ONLY if data_only else 0, st,
                                                          _stream_handle(stream)))

    def reconstruct_into(self, shards, present, out, shard_size: Optional[int] = None, data_only=False,
                         status=None, stream=None, shard_major: bool = False, out_shard_major: bool = True):
        """Reconstruct with a separate output batch (include/ugo_fec.h
        ugo_fec_reconstruct_into): `shards` is only read; output i of group g (the
        i-th erased row, ascending) goes to `out`, a contiguous uint8 CUDA tensor
        [p][G][opitch] (out_shard_major) or [G][p][opitch]."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G * self.mask_words and present.element_size() == 8)
        _require(out.is_contiguous() and out.element_size() == 1 and out.dim() == 3)
        p = self.ParityShards
        if out_shard_major:
            _require(out.shape[0] == p and out.shape[1] == G)
            opitch = out.shape[2]
            ors, ogs = G * opitch, opitch
        else:
            _require(out.shape[0] == G and out.shape[1] == p)
            opitch = out.shape[2]
            ors, ogs = opitch, p * opitch
        S = pitch if shard_size is None else shard_size
        _require(opitch >= S)
        st = None if status is None else status.data_ptr()
        _raise(load_library().ugo_fec_reconstruct_into(self._h, shards.data_ptr(), present.data_ptr(), G, S, rs, gs,
                                                       out.data_ptr(), ors, ogs,
                                                       RECONSTRUCT_DATA_ONLY if data_only else 0, st,
                                                       _stream_handle(stream)))

    def lossy_groups(self, present, data_only: bool = True, out=None, count=None, stream=None):
        """ugo_fec_lossy_groups: the groups of `present` (int64 CUDA [G]) with an
        erased row to rebuild (data rows only with data_only), ascending.  Returns
        (list, count): an int32 CUDA tensor [G] whose first *count entries are the
        groups, and an int32 CUDA tensor [1]; nothing is synchronised."""
        import torch

        G = present.numel()
        _require(present.is_contiguous() and present.element_size() == 8 and self.mask_words == 1)
        lst = torch.empty(max(G, 1), dtype=torch.int32, device=present.device) if out is None else out
        cnt = torch.empty(1, dtype=torch.int32, device=present.device) if count is None else count
        _require(lst.numel() >= G and lst.element_size() == 4 and cnt.element_size() == 4)
        _raise(load_library().ugo_fec_lossy_groups(self._h, present.data_ptr(), G,
                                                   RECONSTRUCT_DATA_ONLY if data_only else 0, lst.data_ptr(),
                                                   cnt.data_ptr(), _stream_handle(stream)))
        return lst, cnt

    def reconstruct_list(self, shards, present, lst, count, out, shard_size: Optional[int] = None,
                         data_only: bool = True, status=None, stream=None, shard_major: bool = True,
                         max_entries: Optional[int] = None):
        """ugo_fec_reconstruct_list: Reconstruct the groups lst[0 .. *count) of the
        batch; output i of list entry j goes to out[j, i] (out: contiguous uint8
        CUDA tensor [max_entries][slots][opitch], compact in list order) or, out =
        None, in place.  status: int8 CUDA [max_entries] (entry j's status)."""
        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G and present.element_size() == 8)
        m = G if max_entries is None else max_entries
        S = pitch if shard_size is None else shard_size
        ors = oes = 0
        if out is not None:
            _require(out.is_contiguous() and out.element_size() == 1 and out.dim() == 3 and out.shape[0] >= m)
            ors, oes = out.shape[2], out.shape[1] * out.shape[2]
            _require(out.shape[2] >= S)
        _raise(load_library().ugo_fec_reconstruct_list(
            self._h, shards.data_ptr(), present.data_ptr(), G, lst.data_ptr(), count.data_ptr(), m, S, rs, gs,
            None if out is None else out.data_ptr(), ors, oes, RECONSTRUCT_DATA_ONLY if data_only else 0,
            None if status is None else status.data_ptr(), _stream_handle(stream)))

    def recover_data(self, shards, present, out, index, count=None, shard_size: Optional[int] = None,
                     stream=None, shard_major: bool = True):
        """ugo_fec_recover_data: `input`'s recovered data shards of a device batch,
        row-compact in `recovered` order: out[r, :shard_size] (out: contiguous
        uint8 CUDA [max_rows, row]), index[r] = group*(d+p) + row (int32 CUDA
        [max_rows]); returns count (int32 CUDA [1], the number recovered,
        written on the stream)."""
        import torch

        G, pitch, rs, gs = self._geom(shards, shard_major)
        _require(present.is_contiguous() and present.numel() == G and present.element_size() == 8)
        S = pitch if shard_size is None else shard_size
        _require(out.is_contiguous() and out.element_size() == 1 and out.dim() == 2 and out.shape[1] >= S)
        _require(index.is_contiguous() and index.element_size() == 4 and index.numel() >= out.shape[0])
        cnt = torch.empty(1, dtype=torch.int32, device=present.device) if count is None else count
        _raise(load_library().ugo_fec_recover_data(
            self._h, shards.data_ptr(), present.data_ptr(), G, S, rs, gs, out.data_ptr(), out.shape[1], out.shape[0],
            index.data_ptr(), cnt.data_ptr(), _stream_handle(stream)))
        return cnt

    def rx_recover_host(self, wire: np.ndarray, lens: np.ndarray, shard_size: int, groups: int,
                        first_group: int = 0, pad: Optional[bytes] = None, out: Optional[np.ndarray] = None,
                        max_out: Optional[int] = None, present_out: Optional[np.ndarray] = None,
                        out_index: Optional[np.ndarray] = None):
        """ugo_fec_rx_recover_host: the RX path host memory to host memory.  wire =
        uint8 [npk, slot] (pinned for DMA rates), lens = uint16 [npk].  Returns
        (n, index, out, stats): n recovered data shards, the first
        min(n, max_out) of them row-compact in out[r, :shard_size] (out: uint8
        [max_out, row] with row >= shard_size, allocated if None) in ugo's
        `recovered` order, index[r] = window group * (d+p) + row (index: out_index,
        uint32 [>= max_out], or allocated if None).  out's row stride is its second
        dimension; only out[r, :shard_size] and index[r] for r < min(n, max_out)
        are written."""
        npk, slot = wire.shape
        _require(wire.flags.c_contiguous and wire.itemsize == 1)
        _require(lens.flags.c_contiguous and lens.size == npk and lens.itemsize == 2)
        _require(pad is None or len(pad) >= slot, "pad must hold at least slot_stride keystream bytes")
        if present_out is not None:  # C writes groups * 8 bytes there
            _require(isinstance(present_out, np.ndarray) and present_out.flags.c_contiguous
                     and present_out.itemsize == 8 and present_out.size >= groups)
        m = groups * min(self.DataShards, self.ParityShards) if max_out is None else max_out
        if out is None:
            out = np.zeros((max(m, 1), (shard_size + 15) // 16 * 16), np.uint8)
        _require(out.ndim == 2 and out.flags.c_contiguous and out.shape[0] >= m and out.shape[1] >= shard_size)
        index = np.zeros(max(m, 1), np.uint32) if out_index is None else out_index
        _require(isinstance(index, np.ndarray) and index.flags.c_contiguous and index.itemsize == 4
                 and index.size >= m)
        stats = np.zeros(5, np.uint32)
        padb = None if pad is None else np.frombuffer(bytes(pad), np.uint8)
        n_out = ctypes.c_size_t(0)
        _raise(load_library().ugo_fec_rx_recover_host(
            self._h, wire.ctypes.data, slot, lens.ctypes.data, npk, None if padb is None else padb.ctypes.data,
            first_group, groups, shard_size, None if present_out is None else present_out.ctypes.data,
            stats.ctypes.data, out.ctypes.data, out.shape[1], m, index.ctypes.data, ctypes.byref(n_out)))
        return n_out.value, index, out, stats

    def tx_assemble_host(self, pkts: np.ndarray, lens: np.ndarray, wire: np.ndarray, wire_lens: np.ndarray,
                         first_seq: int = 0, pad: Optional[bytes] = None, max_len: int = 1476,
                         status: Optional[np.ndarray] = None):
        """ugo_fec_tx_assemble_host: tx_assemble with host numpy buffers (pinned for
        DMA rates): pkts uint8 [G*d, slot_in], lens uint16 [G*d], wire uint8
        [G*(d+p), slot_out], wire_lens uint16 [G*(d+p)], status int8 [G] or None."""
        d, n = self.DataShards, self.Shards
        _require(pkts.ndim == 2 and wire.ndim == 2 and pkts.shape[0] % d == 0)
        G = pkts.shape[0] // d
        _require(lens.size == G * d and wire.shape[0] == G * n and wire_lens.size == G * n)
        # the C side copies G*d*2, G*n*2 and G bytes and reads round_up(max_len, 16) pad bytes
        for a in (pkts, wire, lens, wire_lens):
            _require(isinstance(a, np.ndarray) and a.flags.c_contiguous)
        _require(pkts.itemsize == 1 and wire.itemsize == 1 and lens.itemsize == 2 and wire_lens.itemsize == 2)
        if status is not None:
            _require(isinstance(status, np.ndarray) and status.flags.c_contiguous and status.size == G
                     and status.itemsize == 1)
        _require(pad is None or len(pad) >= (max_len + 15) // 16 * 16,
                 "pad must hold at least round_up(max_len, 16) keystream bytes")
        padb = None if pad is None else np.frombuffer(bytes(pad), np.uint8)
        _raise(load_library().ugo_fec_tx_assemble_host(
            self._h, pkts.ctypes.data, pkts.shape[1], lens.ctypes.data, G, first_seq,
            None if padb is None else padb.ctypes.data, max_len, wire.ctypes.data, wire.shape[1],
            wire_lens.ctypes.data, None if status is None else status.ctypes.data))

    def set_host_copy_queue(self, on: bool):
        """ugo_fec_set_host_copy_queue: the host paths' H2D copies on a
        low-priority stream (a hardware-queue pool of its own)."""
        _raise(load_library().ugo_fec_set_host_copy_queue(self._h, 1 if on else 0))

    def set_tx_host_route(self, route: str):
        """ugo_fec_set_tx_host_route: tx_assemble_host's wire packets by D2H
        copy ("copy", the default) or written through the pinned buffer's
        mapping ("mapped")."""
        _require(route in ("copy", "mapped"))
        _raise(load_library().ugo_fec_set_tx_host_route(self._h, {"copy": 0, "mapped": 1}[route]))

    def reconstruct_rows(self, rows, present, out, shard_size: int, data_only=False, status=None, stream=None,
                         out_shard_major: bool = True):
        """Reconstruct from a row-pointer table (include/ugo_fec.h
        ugo_fec_reconstruct_rows): rows = int64 tensor [G, d+p] of device
        addresses (device tensor, or pinned host memory as a numpy array /
        CPU tensor viewed through ugo_fec_device_address), present = [G] masks
        (device tensor or pinned numpy array), out = contiguous uint8 CUDA
        tensor [p][G][opitch] (out_shard_major) or [G][p][opitch]."""
        G = present.shape[0]
        _require(rows.shape[0] == G and rows.shape[1] == self.Shards and self.Shards <= 64)
        p = self.ParityShards
        _require(out.dim() == 3 and out.is_contiguous() and out.element_size() == 1)
        if out_shard_major:
            _require(out.shape[0] == p and out.shape[1] == G)
            ors, ogs = G * out.shape[2], out.shape[2]
        else:
            _require(out.shape[0] == G and out.shape[1] == p)
            ors, ogs = out.shape[2], p * out.shape[2]
        _require(out.shape[2] >= shard_size)

        def ptr(x):
            return None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())

        _raise(load_library().ugo_fec_reconstruct_rows(self._h, ptr(rows), ptr(present), G, shard_size, ptr(out),
                                                       ors, ogs, RECONSTRUCT_DATA_ONLY if data_only else 0,
                                                       ptr(status), _stream_handle(stream)))

    def device_address(self, addr: int) -> int:
        """ugo_fec_device_address: the device address of host/device pointer addr."""
        out = ctypes.c_void_p()
        _raise(load_library().ugo_fec_device_address(self._h, ctypes.c_void_p(addr), ctypes.byref(out)))
        return out.value or 0

    def rx_assemble(self, wire, lens, shards, present, first_group: int = 0, shard_size: Optional[int] = None,
                    pad=None, stats=None, stream=None, shard_major: bool = True, frames: bool = False):
        """RX group assembly (include/ugo_fec.h ugo_fec_rx_assemble): wire = uint8 CUDA
        tensor [npk, slot] of received packets, lens = int16/uint16 CUDA tensor [npk];
        pad = uint8 CUDA keystream (>= slot bytes) or None; present = int64 CUDA [G]
        (zeroed by the caller); stats = int32 CUDA [5] (accepted, bad flag, out of
        window, too short, duplicate) or None.  A repeated seqid keeps its first
        copy in ring order (ugo/fec.go:123-129).  frames=True:
        ugo_fec_rx_assemble_frames -- a row holds the decrypted packet (payload at
        column 6, shard_size + 6 bytes); reconstruct it with shard_size + 6."""
        if stats is not None:
            _require(stats.numel() >= 5 and stats.element_size() == 4)
        G, pitch, rs, gs = self._geom(shards, shard_major)
        npk, slot = wire.shape
        _require(wire.is_contiguous() and lens.is_contiguous() and lens.element_size() == 2 and lens.numel() == npk)
        S = (pitch - 6 if frames else pitch) if shard_size is None else shard_size
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        entry = load_library().ugo_fec_rx_assemble_frames if frames else load_library().ugo_fec_rx_assemble
        _raise(entry(
            self._h, wire.data_ptr(), slot, lens.data_ptr(), npk, None if pad is None else pad.data_ptr(),
            first_group, G, shards.data_ptr(), S, rs, gs, present.data_ptr(),
            None if stats is None else stats.data_ptr(), _stream_handle(stream)))

    def tx_assemble(self, pkts, lens, wire, wire_lens, first_seq: int = 0, pad=None, max_len: int = 1476,
                    status=None, stream=None):
        """TX group assembly (include/ugo_fec.h ugo_fec_tx_assemble): pkts = uint8 CUDA
        tensor [G*d, slot_in] of outgoing data packets (6-B header space first),
        lens = int16/uint16 CUDA [G*d]; wire = uint8 CUDA [G*(d+p), slot_out],
        wire_lens = int16/uint16 CUDA [G*(d+p)]; pad = uint8 CUDA keystream or None;
        status = int8 CUDA [G] or None."""
        d, n = self.DataShards, self.Shards
        npk, slot_in = pkts.shape
        _require(npk % d == 0, "pkts must hold whole groups of d data packets")
        G = npk // d
        _require(wire.shape[0] == G * n and wire_lens.numel() == G * n and lens.numel() == npk)
        _require(pkts.is_contiguous() and wire.is_contiguous() and lens.is_contiguous() and wire_lens.is_contiguous())
        _require(lens.element_size() == 2 and wire_lens.element_size() == 2)
        if status is not None:
            _require(status.numel() == G and status.element_size() == 1)
        _raise(load_library().ugo_fec_tx_assemble(
            self._h, pkts.data_ptr(), slot_in, lens.data_ptr(), G, first_seq,
            None if pad is None else pad.data_ptr(), max_len, wire.data_ptr(), wire.shape[1],
            wire_lens.data_ptr(), None if status is None else status.data_ptr(), _stream_handle(stream)))

    def packet_decode(self, pkts, lens, pad=None, framed: bool = False, max_ranges: int = 32,
                      max_segments: int = 8, stream=None, out=None):
        """Batch ugoPacket.decode (include/ugo_pkt.h): pkts = uint8 CUDA [npk, slot],
        lens = int16/uint16 CUDA [npk].  Returns CUDA tensors (info [npk, 64] bytes --
        view on the host with PKT_INFO_DTYPE --, ranges int64 [npk, max_ranges, 2],
        segs [npk, max_segments, 16] bytes -- PKT_SEGMENT_DTYPE)."""
        npk, slot = pkts.shape
        _require(pkts.is_contiguous() and lens.is_contiguous() and lens.element_size() == 2 and lens.numel() == npk)
        dev = pkts.device
        if out is not None:  # reuse (info, ranges, segs) from an earlier call
            info, ranges, segs = out
            _require(info.shape == (npk, 64) and ranges.shape[0] == npk and segs.shape[0] == npk)
            _require(ranges.shape[1] >= max(max_ranges, 1) and segs.shape[1] >= max(max_segments, 1))
        else:
            info = torch.empty((npk, 64), dtype=torch.uint8, device=dev)
            ranges = torch.zeros((npk, max(max_ranges, 1), 2), dtype=torch.int64, device=dev)
            segs = torch.zeros((npk, max(max_segments, 1), 16), dtype=torch.uint8, device=dev)
        _raise(load_library().ugo_fec_packet_decode(
            self._h, pkts.data_ptr(), slot, lens.data_ptr(), npk, None if pad is None else pad.data_ptr(),
            PKT_FEC_FRAMED if framed else 0, info.data_ptr(), ranges.data_ptr(), max_ranges, segs.data_ptr(),
            max_segments, _stream_handle(stream)))
        return info, ranges, segs

    def packet_encode(self, info, ranges, segs, payload, slot: int, payload_stride: int = 0, pad=None,
                      framed: bool = False, stream=None, out=None):
        """Batch ugoPacket.encode (include/ugo_pkt.h ugo_fec_packet_encode), the
        reverse of packet_decode: info = uint8 CUDA [npk, 64] (PKT_INFO_DTYPE),
        ranges = int64 CUDA [npk, max_ranges, 2], segs = uint8 CUDA [npk,
        max_segments, 16] (PKT_SEGMENT_DTYPE); segment data is read from payload
        (uint8 CUDA, any alignment) at i*payload_stride + data_off.  framed: 6 B
        of zeroed header room in front (tx_assemble's input; pad must be None);
        else pad = uint8 CUDA keystream (>= slot bytes) or None.  Returns CUDA
        tensors (wire uint8 [npk, slot], wire_lens int16 [npk], status uint8
        [npk]); out = such a triple to reuse.  Only bytes [0, round_up(len, 16))
        of a slot are written."""
        npk = info.shape[0]
        _require(info.is_contiguous() and info.element_size() == 1 and tuple(info.shape) == (npk, 64))
        _require(ranges.is_contiguous() and ranges.element_size() == 8 and ranges.dim() == 3 and
                 ranges.shape[0] == npk and ranges.shape[2] == 2)
        _require(segs.is_contiguous() and segs.element_size() == 1 and segs.dim() == 3 and segs.shape[0] == npk and
                 segs.shape[2] == 16)
        _require(payload.is_contiguous() and payload.element_size() == 1)
        _require(not (framed and pad is not None), "framed packets are encrypted by tx_assemble: pad must be None")
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        if out is not None:
            wire, wire_lens, status = out
            _require(tuple(wire.shape) == (npk, slot) and wire.is_contiguous() and wire.element_size() == 1)
            _require(wire_lens.numel() == npk and wire_lens.element_size() == 2 and wire_lens.is_contiguous())
            _require(status.numel() == npk and status.element_size() == 1 and status.is_contiguous())
        else:
            dev = info.device
            wire = torch.zeros((npk, slot), dtype=torch.uint8, device=dev)
            wire_lens = torch.zeros(npk, dtype=torch.int16, device=dev)
            status = torch.zeros(npk, dtype=torch.uint8, device=dev)
        _raise(load_library().ugo_fec_packet_encode(
            self._h, info.data_ptr(), ranges.data_ptr(), ranges.shape[1], segs.data_ptr(), segs.shape[1],
            payload.data_ptr(), payload_stride, npk, None if pad is None else pad.data_ptr(),
            PKT_FEC_FRAMED if framed else 0, wire.data_ptr(), slot, wire_lens.data_ptr(), status.data_ptr(),
            _stream_handle(stream)))
        return wire, wire_lens, status

    # ---------------------------------------------------------- launch timing
    def timing_begin(self, max_launches: int):
        """Time the next max_launches kernel launches of this context with
        hipExtLaunchKernel start/stop events (kernel durations, nothing inserted
        between kernels).  Read them with timing_end()."""
        _raise(load_library().ugo_fec_timing_begin(self._h, max_launches))
        self._timing_cap = max_launches

    def timing_end(self):
        """Waits for the timed launches; returns (records, untimed): records is a
        LAUNCH_TIME_DTYPE array (kernel id, ms) in launch order, untimed the
        number of launches past max_launches."""
        cap = getattr(self, "_timing_cap", 0)
        out = np.zeros(cap, LAUNCH_TIME_DTYPE)
        n, untimed = ctypes.c_size_t(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_timing_end(self._h, out.ctypes.data if cap else None, cap, ctypes.byref(n),
                                                 ctypes.byref(untimed)))
        return out[:n.value], untimed.value

    # ------------------------------------------------------ host-buffer batch
    def service_start(self, idle_us: int = 0):
        """Per-call latency service (ugo_fec_service_start): small pinned host
        batches are served by a resident workgroup, no launch per call."""
        _raise(load_library().ugo_fec_service_start(self._h, idle_us))

    def service_stop(self):
        _raise(load_library().ugo_fec_service_stop(self._h))

    def service_config(self, timeout_ms: int = 0, grace_ms: int = 0, test_stall_us: int = 0):
        """The service's watchdog (ugo_fec_service_config): a call's wait for an
        answer and the wait for the workgroup to leave after a timeout (0 = 5000
        ms each); test_stall_us (tests only) delays every request it serves."""
        _raise(load_library().ugo_fec_service_config(self._h, timeout_ms, grace_ms, test_stall_us))

    @property
    def poisoned(self) -> bool:
        """True if a service workgroup never left after a failed call (every call
        on this context now fails; include/ugo_fec.h)."""
        return bool(load_library().ugo_fec_poisoned(self._h))

    def encode_host(self, shards: np.ndarray, shard_size: Optional[int] = None):
        _require(shards.dtype == np.uint8 and shards.flags["C_CONTIGUOUS"] and shards.ndim == 3)
        G, n, pitch = shards.shape
        _require(n == self.Shards)
        S = pitch if shard_size is None else shard_size
        _raise(load_library().ugo_fec_encode_host(self._h, shards.ctypes.data, G, S, pitch))

    def reconstruct_host(self, shards: np.ndarray, present: np.ndarray, shard_size: Optional[int] = None,
                         data_only=False, status: Optional[np.ndarray] = None) -> int:
        """Returns the aggregate status (0 or the first failing group's code);
        per-group codes go to `status` when given.  Does not raise for
        ErrTooFewShards groups (they are reported and left untouched)."""
        _require(shards.dtype == np.uint8 and shards.flags["C_CONTIGUOUS"] and shards.ndim == 3)
        G, n, pitch = shards.shape
        _require(n == self.Shards)
        present = np.ascontiguousarray(present, dtype=np.uint64)
        _require(present.size == G * self.mask_words)
        S = pitch if shard_size is None else shard_size
        st = None if status is None else status.ctypes.data
        if status is not None:
            _require(status.dtype == np.int8 and status.size == G)
        rc = load_library().ugo_fec_reconstruct_host(self._h, shards.ctypes.data, present.ctypes.data, G, S, pitch,
                                                     RECONSTRUCT_DATA_ONLY if data_only else 0, st)
        if rc not in (OK, ErrTooFewShards.code, ErrSingular.code):
            _raise(rc)
        return rc

    # ------------------------------------------- Go-shaped, one group per call
    def _stage(self, S: int) -> np.ndarray:
        """One pinned group [d+p][P] at the 16-B pitch P, reused across calls
        (the cgo shim's staging): the vector kernels, and the
        per-call service when it is on, serve it."""
        P = (S + 15) // 16 * 16
        need = self.Shards * P
        st = getattr(self, "_stage_buf", None)
        if st is None or st.size < need:
            if st is not None:
                host_free(st)
            st = self._stage_buf = host_alloc(max(need, self.Shards * 1488))
        return st[:need].reshape(1, self.Shards, P)

    def Encode(self, shards: List[bytearray]) -> None:
        """reedsolomon Encode: parity shards written in place (ugo/fec.go:238)."""
        if len(shards) != self.Shards:
            raise ErrTooFewShards(strerror(ErrTooFewShards.code))
        S = check_shards([len(s) for s in shards], nil_ok=False)
        buf = self._stage(S)
        for k in range(self.DataShards):
            buf[0, k, :S] = np.frombuffer(bytes(shards[k]), np.uint8)
        self.encode_host(buf, S)
        for k in range(self.DataShards, self.Shards):
            shards[k][:] = buf[0, k, :S].tobytes()

    def _reconstruct(self, shards: list, data_only: bool) -> None:
        if len(shards) != self.Shards:
            raise ErrTooFewShards(strerror(ErrTooFewShards.code))
        lens = [0 if s is None else len(s) for s in shards]
        S = check_shards(lens, nil_ok=True)
        mask = np.zeros(self.mask_words, np.uint64)
        buf = self._stage(S)
        for r, s in enumerate(shards):
            if lens[r]:
                mask[r >> 6] |= np.uint64(1 << (r & 63))
                buf[0, r, :S] = np.frombuffer(bytes(s), np.uint8)
        status = np.zeros(1, np.int8)
        rc = self.reconstruct_host(buf, mask, S, data_only, status)
        _raise(rc)
        limit = self.DataShards if data_only else self.Shards
        for r in range(limit):
            if not lens[r]:
                shards[r] = bytearray(buf[0, r, :S].tobytes())

    def Reconstruct(self, shards: list) -> None:
        """reedsolomon Reconstruct (ugo/fec.go:202): fills every missing shard."""
        self._reconstruct(shards, data_only=False)

    def ReconstructData(self, shards: list) -> None:
        self._reconstruct(shards, data_only=True)


class _DeviceBytes:
    """A span of device memory for torch.as_tensor (__cuda_array_interface__)."""

    def __init__(self, ptr: int, nbytes: int, owner):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        self._owner = owner


class StreamRx:
    """A connection's receive window on the GPU (include/ugo_stream.h): batch
    Conn.handleSegment (deliver) and Conn.Read (read) behind packet_decode."""

    def __init__(self, enc: Encoder, window_bytes: int):
        self.check_window(window_bytes)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_stream_rx_create(enc._h, window_bytes, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the window
        self.window_bytes = window_bytes
        self.device = enc.device

    @staticmethod
    def check_window(window_bytes: int):
        _require(window_bytes >= STREAM_MIN_WINDOW and window_bytes & (window_bytes - 1) == 0,
                 f"window_bytes must be a power of two >= {STREAM_MIN_WINDOW}")

    @staticmethod
    def check_batch(slot: int, pkts_ptr: int, pad_ptr: Optional[int]):
        _require(slot % 16 == 0 and 0 < slot <= 0xffff, "slot must be a multiple of 16, at most 0xffff")
        _require(pkts_ptr % 16 == 0 and (pad_ptr is None or pad_ptr % 16 == 0), "pkts and pad must be 16-B aligned")

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_stream_rx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def deliver(self, pkts, info, segs, pad=None, stream=None, out=None):
        """ugo_fec_stream_deliver: pkts = uint8 CUDA [npk, slot] (still encrypted),
        info / segs as packet_decode returned them, pad = the decoder's keystream
        or None.  Returns seg_status, uint8 CUDA [npk, max_segments] of STREAM_*
        (out = such a tensor to reuse).  Nothing is synchronised."""
        npk, slot = pkts.shape
        _require(pkts.is_contiguous() and pkts.element_size() == 1)
        _require(info.is_contiguous() and info.element_size() == 1 and tuple(info.shape) == (npk, 64))
        _require(segs.is_contiguous() and segs.element_size() == 1 and segs.dim() == 3 and segs.shape[0] == npk and
                 segs.shape[2] == 16)
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        self.check_batch(slot, pkts.data_ptr(), None if pad is None else pad.data_ptr())
        max_segments = segs.shape[1]
        if out is None:
            out = torch.empty((npk, max_segments), dtype=torch.uint8, device=pkts.device)
        _require(tuple(out.shape) == (npk, max_segments) and out.is_contiguous() and out.element_size() == 1)
        _raise(load_library().ugo_fec_stream_deliver(
            self._h, pkts.data_ptr(), slot, None if pad is None else pad.data_ptr(), info.data_ptr(),
            segs.data_ptr(), max_segments, npk, out.data_ptr(), _stream_handle(stream)))
        return out

    def read(self, n: int, out=None, discard: bool = False, stream=None, n_read=None, eof=None):
        """ugo_fec_stream_read, Conn.Read(p[:n]) that never waits.  Returns CUDA
        tensors (buf uint8 [n] -- None with discard --, n_read int64 [1], eof uint8
        [1]): buf[:n_read] holds the bytes.  out (any alignment), n_read and eof
        may be given, in device or pinned host memory.  Nothing is synchronised."""
        _require(n >= 0)
        dev = torch.device("cuda", self.device)
        if discard:
            out = None
        elif out is None:
            out = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        if out is not None:
            _require(out.is_contiguous() and out.element_size() == 1 and out.numel() >= n)
        if n_read is None:
            n_read = torch.zeros(1, dtype=torch.int64, device=dev)
        if eof is None:
            eof = torch.zeros(1, dtype=torch.uint8, device=dev)
        _require(n_read.numel() == 1 and n_read.element_size() == 8 and eof.numel() == 1 and eof.element_size() == 1)
        _raise(load_library().ugo_fec_stream_read(self._h, None if out is None else out.data_ptr(), n,
                                                  n_read.data_ptr(), eof.data_ptr(), _stream_handle(stream)))
        return out, n_read, eof

    def state(self) -> np.ndarray:
        """The connection's record (STREAM_STATE_DTYPE scalar); waits for the last deliver / read."""
        out = np.zeros(1, STREAM_STATE_DTYPE)
        _raise(load_library().ugo_fec_stream_rx_state(self._h, out.ctypes.data))
        return out[0]

    def window(self):
        """The window as a uint8 CUDA tensor [window_bytes] over the device memory
        itself (stream byte x at index x & (window_bytes - 1)); valid while this
        object lives."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_stream_rx_window(self._h, ctypes.byref(p), ctypes.byref(n)))
        return torch.as_tensor(_DeviceBytes(p.value, n.value, self), device=torch.device("cuda", self.device))


class StreamRxSet:
    """An ordered set of receive windows (ugo_fec_stream_set_*, include/ugo_stream.h):
    one deliver for a batch that holds the packets of many connections, one read
    for all of them.  The set does not own its members; close it before them."""

    def __init__(self, enc: Encoder, rxs):
        rxs = list(rxs)
        self.check_members(enc, rxs)
        arr = (ctypes.c_void_p * len(rxs))(*[rx._h.value for rx in rxs])
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_stream_set_create(enc._h, ctypes.addressof(arr), len(rxs), ctypes.byref(h)))
        self._h, self._enc, self.rxs = h, enc, rxs  # context and members must outlive the set
        self.nconn = len(rxs)
        self.device = enc.device

    @staticmethod
    def check_members(enc, rxs):
        _require(0 < len(rxs) <= STREAM_SET_MAX_CONN, f"a set holds 1 to {STREAM_SET_MAX_CONN} windows")
        _require(all(isinstance(rx, StreamRx) and getattr(rx, "_h", None) for rx in rxs), "members must be open StreamRx")
        _require(all(rx._enc is enc for rx in rxs), "every member must belong to the set's context")
        _require(len({id(rx) for rx in rxs}) == len(rxs), "a window may be listed once")

    @staticmethod
    def check_conn_of(conn_of, npk: int):
        _require(conn_of.is_contiguous() and conn_of.element_size() == 4 and conn_of.numel() == npk and
                 not conn_of.dtype.is_floating_point, "conn_of must be npackets contiguous 32-bit integers")

    def check_per_conn(self, t, element_size: int, name: str):
        _require(t.is_contiguous() and t.element_size() == element_size and t.numel() == self.nconn and
                 not t.dtype.is_floating_point, f"{name} must be nconn contiguous {8 * element_size}-bit integers")

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_stream_set_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def deliver(self, pkts, info, segs, conn_of, pad=None, stream=None, out=None):
        """ugo_fec_stream_set_deliver: StreamRx.deliver with conn_of, int32 [npk]
        in device or pinned host memory -- the member index of each packet
        (STREAM_NO_CONN as -1, or any index >= nconn: no connection).  Returns
        seg_status, uint8 [npk, max_segments].  Nothing is synchronised."""
        npk, slot = pkts.shape
        _require(pkts.is_contiguous() and pkts.element_size() == 1)
        _require(info.is_contiguous() and info.element_size() == 1 and tuple(info.shape) == (npk, 64))
        _require(segs.is_contiguous() and segs.element_size() == 1 and segs.dim() == 3 and segs.shape[0] == npk and
                 segs.shape[2] == 16)
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        StreamRx.check_batch(slot, pkts.data_ptr(), None if pad is None else pad.data_ptr())
        self.check_conn_of(conn_of, npk)
        max_segments = segs.shape[1]
        if out is None:
            out = torch.empty((npk, max_segments), dtype=torch.uint8, device=pkts.device)
        _require(tuple(out.shape) == (npk, max_segments) and out.is_contiguous() and out.element_size() == 1)
        _raise(load_library().ugo_fec_stream_set_deliver(
            self._h, pkts.data_ptr(), slot, None if pad is None else pad.data_ptr(), info.data_ptr(),
            segs.data_ptr(), max_segments, npk, conn_of.data_ptr(), out.data_ptr(), _stream_handle(stream)))
        return out

    def read(self, n, dst=None, dst_off=None, stream=None, n_read=None, eof=None):
        """ugo_fec_stream_set_read: n = int64 [nconn] bytes wanted per member (0
        skips it), dst = uint8 buffer or None to discard, dst_off = int64 [nconn]
        offsets into dst (the caller keeps the ranges disjoint and inside dst).
        Returns (n_read int64 [nconn], eof uint8 [nconn]); both may be given.
        Operands in device or pinned host memory.  Nothing is synchronised."""
        dev = torch.device("cuda", self.device)
        self.check_per_conn(n, 8, "n")
        if dst is not None:
            _require(dst.is_contiguous() and dst.element_size() == 1)
            _require(dst_off is not None, "dst needs dst_off")
            self.check_per_conn(dst_off, 8, "dst_off")
        if n_read is None:
            n_read = torch.zeros(self.nconn, dtype=torch.int64, device=dev)
        if eof is None:
            eof = torch.zeros(self.nconn, dtype=torch.uint8, device=dev)
        self.check_per_conn(n_read, 8, "n_read")
        self.check_per_conn(eof, 1, "eof")
        _raise(load_library().ugo_fec_stream_set_read(
            self._h, None if dst is None else dst.data_ptr(), None if dst is None else dst_off.data_ptr(),
            n.data_ptr(), n_read.data_ptr(), eof.data_ptr(), _stream_handle(stream)))
        return n_read, eof

    def states(self) -> np.ndarray:
        """The members' records (STREAM_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, STREAM_STATE_DTYPE)
        _raise(load_library().ugo_fec_stream_set_state(self._h, out.ctypes.data))
        return out


class StreamTx:
    """A connection's send window on the GPU (include/ugo_stream.h, send
    windows): its unsent and unacknowledged stream bytes and its retransmission
    queue.  Every call goes through a StreamTxSet; a set of one is the
    single-connection form."""

    def __init__(self, enc: Encoder, window_bytes: int, rq_cap: int = 64, start_offset: int = 0,
                 start_packet_number: int = 0):
        self.check_create(window_bytes, rq_cap)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_stream_tx_create(enc._h, window_bytes, rq_cap, start_offset,
                                                       start_packet_number, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the window
        self.window_bytes, self.rq_cap = window_bytes, rq_cap
        self.device = enc.device

    @staticmethod
    def check_create(window_bytes: int, rq_cap: int):
        _require(STREAM_MIN_WINDOW <= window_bytes <= STREAM_TX_MAX_WINDOW and window_bytes & (window_bytes - 1) == 0,
                 f"window_bytes must be a power of two in [{STREAM_MIN_WINDOW}, 2^31]")
        _require(1 <= rq_cap <= 1 << 24, "rq_cap must be in [1, 2^24]")

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_stream_tx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def window(self):
        """The window as a uint8 CUDA tensor [window_bytes] over the device memory
        itself (stream byte x at index x & (window_bytes - 1))."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_stream_tx_window(self._h, ctypes.byref(p), ctypes.byref(n)))
        return torch.as_tensor(_DeviceBytes(p.value, n.value, self), device=torch.device("cuda", self.device))

    def queue(self):
        """The retransmission ring as a uint8 CUDA tensor [rq_cap, 16] over the
        device memory itself (view on the host with STREAM_TX_RQ_DTYPE)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_stream_tx_queue(self._h, ctypes.byref(p), ctypes.byref(n)))
        t = torch.as_tensor(_DeviceBytes(p.value, n.value * 16, self), device=torch.device("cuda", self.device))
        return t.view(n.value, 16)


class StreamTxSet:
    """An ordered set of send windows (ugo_fec_stream_tx_set_*): write, plan and
    encode for all of them per call, release and retransmit for what ARQ on the
    host decides.  Per-connection operands are tensors of nconn elements in
    device or pinned host memory.  Nothing is synchronised but states().  The
    set does not own its members; close it before them."""

    def __init__(self, enc: Encoder, txs):
        txs = list(txs)
        self.check_members(enc, txs)
        arr = (ctypes.c_void_p * len(txs))(*[tx._h.value for tx in txs])
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_stream_tx_set_create(enc._h, ctypes.addressof(arr), len(txs), ctypes.byref(h)))
        self._h, self._enc, self.txs = h, enc, txs
        self.nconn = len(txs)
        self.device = enc.device

    @staticmethod
    def check_members(enc, txs):
        _require(0 < len(txs) <= STREAM_SET_MAX_CONN, f"a set holds 1 to {STREAM_SET_MAX_CONN} windows")
        _require(all(isinstance(tx, StreamTx) and getattr(tx, "_h", None) for tx in txs), "members must be open StreamTx")
        _require(all(tx._enc is enc for tx in txs), "every member must belong to the set's context")
        _require(len({id(tx) for tx in txs}) == len(txs), "a window may be listed once")

    @staticmethod
    def check_plan(max_payload: int, max_segments: int, max_packets: int):
        _require(16 <= max_payload <= 0xffff, "max_payload must be in [16, 0xffff]")
        _require(1 <= max_segments <= 0xffff, "max_segments must be in [1, 0xffff]")
        _require(0 <= max_packets <= 1 << 31, "max_packets must be at most 2^31")

    def check_per_conn(self, t, element_size: int, name: str):
        _require(t.is_contiguous() and t.element_size() == element_size and t.numel() == self.nconn and
                 not t.dtype.is_floating_point, f"{name} must be nconn contiguous {8 * element_size}-bit integers")

    @staticmethod
    def _check_list(t, m: int, element_size: int, name: str):
        _require(t.is_contiguous() and t.element_size() == element_size and t.numel() == m and
                 not t.dtype.is_floating_point, f"{name} must be {m} contiguous {8 * element_size}-bit integers")

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_stream_tx_set_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def write(self, src, src_off, n, n_written=None, stream=None):
        """Conn.Write that never waits: n[c] bytes from src[src_off[c]:] (uint8,
        any alignment; int64 [nconn] both) to member c, as many as its window
        has room for.  Returns n_written int64 [nconn]."""
        _require(src.is_contiguous() and src.element_size() == 1)
        self.check_per_conn(src_off, 8, "src_off")
        self.check_per_conn(n, 8, "n")
        if n_written is None:
            n_written = torch.zeros(self.nconn, dtype=torch.int64, device=torch.device("cuda", self.device))
        self.check_per_conn(n_written, 8, "n_written")
        _raise(load_library().ugo_fec_stream_tx_set_write(self._h, src.data_ptr(), src_off.data_ptr(), n.data_ptr(),
                                                          n_written.data_ptr(), _stream_handle(stream)))
        return n_written

    def release(self, upto, stream=None):
        """The peer acknowledged everything below upto[c] (int64 [nconn])."""
        self.check_per_conn(upto, 8, "upto")
        _raise(load_library().ugo_fec_stream_tx_set_release(self._h, upto.data_ptr(), _stream_handle(stream)))

    def retransmit(self, conn_of, offset, length, status=None, stream=None):
        """Queue segments for retransmission: conn_of int32 [m] (non-decreasing),
        offset int64 [m], length int32 [m].  Returns status uint8 [m] of
        STREAM_TX_RQ_*."""
        m = conn_of.numel()
        self._check_list(conn_of, m, 4, "conn_of")
        self._check_list(offset, m, 8, "offset")
        self._check_list(length, m, 4, "length")
        if status is None:
            status = torch.zeros(m, dtype=torch.uint8, device=torch.device("cuda", self.device))
        self._check_list(status, m, 1, "status")
        _raise(load_library().ugo_fec_stream_tx_set_retransmit(
            self._h, conn_of.data_ptr(), offset.data_ptr(), length.data_ptr(), m, status.data_ptr(),
            _stream_handle(stream)))
        return status

    def plan(self, budget, max_packets: int, max_payload: int = 1436, max_segments: int = 8, out=None, stream=None):
        """The loop of Conn.sendPacket for every member (THE RULE of
        include/ugo_stream.h): budget int32 [nconn] packets at the most per
        member.  Returns (info uint8 [max_packets, 64], segs uint8 [max_packets,
        max_segments, 16], conn_of int32 [max_packets], first_packet int64
        [nconn], n_packets int32 [nconn], total int64 [1]); out = such a tuple
        to reuse."""
        self.check_plan(max_payload, max_segments, max_packets)
        self.check_per_conn(budget, 4, "budget")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = (torch.zeros((max_packets, 64), dtype=torch.uint8, device=dev),
                   torch.zeros((max_packets, max_segments, 16), dtype=torch.uint8, device=dev),
                   torch.zeros(max_packets, dtype=torch.int32, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int64, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int32, device=dev),
                   torch.zeros(1, dtype=torch.int64, device=dev))
        info, segs, conn_of, first_packet, n_packets, total = out
        _require(info.is_contiguous() and info.element_size() == 1 and tuple(info.shape) == (max_packets, 64))
        _require(segs.is_contiguous() and segs.element_size() == 1 and
                 tuple(segs.shape) == (max_packets, max_segments, 16))
        self._check_list(conn_of, max_packets, 4, "conn_of")
        self.check_per_conn(first_packet, 8, "first_packet")
        self.check_per_conn(n_packets, 4, "n_packets")
        self._check_list(total, 1, 8, "total")
        _raise(load_library().ugo_fec_stream_tx_set_plan(
            self._h, budget.data_ptr(), max_payload, max_segments, max_packets, info.data_ptr(), segs.data_ptr(),
            conn_of.data_ptr(), first_packet.data_ptr(), n_packets.data_ptr(), total.data_ptr(),
            _stream_handle(stream)))
        return out

    def encode(self, info, ranges, segs, conn_of, slot: int, npackets: Optional[int] = None, pad=None,
               framed: bool = False, stream=None, out=None):
        """Encoder.packet_encode with the segment bytes read from the members'
        windows: conn_of int32 [>= npackets] names packet i's member.  npackets
        defaults to info.shape[0]; the arrays may be longer (plan's
        max_packets).  Returns (wire uint8 [npackets, slot], wire_lens int16,
        status uint8)."""
        npk = info.shape[0] if npackets is None else npackets
        _require(0 <= npk <= info.shape[0])
        _require(info.is_contiguous() and info.element_size() == 1 and info.dim() == 2 and info.shape[1] == 64)
        _require(ranges.is_contiguous() and ranges.element_size() == 8 and ranges.dim() == 3 and
                 ranges.shape[0] >= npk and ranges.shape[2] == 2)
        _require(segs.is_contiguous() and segs.element_size() == 1 and segs.dim() == 3 and segs.shape[0] >= npk and
                 segs.shape[2] == 16)
        _require(conn_of.is_contiguous() and conn_of.element_size() == 4 and conn_of.numel() >= npk and
                 not conn_of.dtype.is_floating_point)
        _require(not (framed and pad is not None), "framed packets are encrypted by tx_assemble: pad must be None")
        _require(slot % 16 == 0 and 0 < slot <= 0xffff, "slot must be a multiple of 16, at most 0xffff")
        if pad is not None:
            _require(pad.is_contiguous() and pad.element_size() == 1 and pad.numel() >= slot)
        if out is not None:
            wire, wire_lens, status = out
            _require(wire.dim() == 2 and wire.shape[0] >= npk and wire.shape[1] == slot and wire.is_contiguous() and
                     wire.element_size() == 1)
            _require(wire_lens.numel() >= npk and wire_lens.element_size() == 2 and wire_lens.is_contiguous())
            _require(status.numel() >= npk and status.element_size() == 1 and status.is_contiguous())
        else:
            dev = info.device
            wire = torch.zeros((npk, slot), dtype=torch.uint8, device=dev)
            wire_lens = torch.zeros(npk, dtype=torch.int16, device=dev)
            status = torch.zeros(npk, dtype=torch.uint8, device=dev)
        _raise(load_library().ugo_fec_stream_tx_set_encode(
            self._h, info.data_ptr(), ranges.data_ptr(), ranges.shape[1], segs.data_ptr(), segs.shape[1],
            conn_of.data_ptr(), npk, None if pad is None else pad.data_ptr(), PKT_FEC_FRAMED if framed else 0,
            wire.data_ptr(), slot, wire_lens.data_ptr(), status.data_ptr(), _stream_handle(stream)))
        return wire, wire_lens, status

    def states(self) -> np.ndarray:
        """The members' records (STREAM_TX_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, STREAM_TX_STATE_DTYPE)
        _raise(load_library().ugo_fec_stream_tx_set_state(self._h, out.ctypes.data))
        return out


class AckRx:
    """A connection's receive history on the GPU (include/ugo_ack.h): the
    packetReceiver's state, a ring bitmap of window_packets numbers and a
    record.  Every call goes through an AckRxSet; a set of one is the
    single-connection form."""

    def __init__(self, enc: Encoder, window_packets: int = 4096):
        self.check_window(window_packets)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_ack_rx_create(enc._h, window_packets, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the history
        self.window_packets = window_packets
        self.device = enc.device

    @staticmethod
    def check_window(window_packets: int):
        _require(ACK_MIN_WINDOW <= window_packets <= ACK_MAX_WINDOW and window_packets & (window_packets - 1) == 0,
                 f"window_packets must be a power of two in [{ACK_MIN_WINDOW}, 2^20]")

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_ack_rx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def state(self) -> np.ndarray:
        """The record (ACK_STATE_DTYPE scalar); waits for the last call of the sets it is in."""
        out = np.zeros(1, ACK_STATE_DTYPE)
        _raise(load_library().ugo_fec_ack_rx_state(self._h, out.ctypes.data))
        return out[0]

    def bitmap(self):
        """The ring bitmap as an int64 CUDA tensor [window_packets / 64] over the
        device memory itself (packet number n is bit n & 63 of word
        (n & (window_packets - 1)) >> 6); valid while this object lives."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_ack_rx_bitmap(self._h, ctypes.byref(p), ctypes.byref(n)))
        t = torch.as_tensor(_DeviceBytes(p.value, n.value // 8, self), device=torch.device("cuda", self.device))
        return t.view(torch.int64)


class AckRxSet:
    """An ordered set of receive histories (ugo_fec_ack_set_*): receive for a
    decoded batch that holds the packets of many connections, attach to write
    every member's SACK into the arrays StreamTxSet.plan left for
    StreamTxSet.encode.  Operands are tensors in device or pinned host memory.
    Nothing is synchronised but states().  The set does not own its members;
    close it before them."""

    def __init__(self, enc: Encoder, rxs):
        rxs = list(rxs)
        self.check_members(enc, rxs)
        arr = (ctypes.c_void_p * len(rxs))(*[rx._h.value for rx in rxs])
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_ack_set_create(enc._h, ctypes.addressof(arr), len(rxs), ctypes.byref(h)))
        self._h, self._enc, self.rxs = h, enc, rxs  # context and members must outlive the set
        self.nconn = len(rxs)
        self.device = enc.device

    @staticmethod
    def check_members(enc, rxs):
        _require(0 < len(rxs) <= STREAM_SET_MAX_CONN, f"a set holds 1 to {STREAM_SET_MAX_CONN} histories")
        _require(all(isinstance(rx, AckRx) and getattr(rx, "_h", None) for rx in rxs), "members must be open AckRx")
        _require(all(rx._enc is enc for rx in rxs), "every member must belong to the set's context")
        _require(len({id(rx) for rx in rxs}) == len(rxs), "a history may be listed once")

    def check_per_conn(self, t, element_size: int, name: str):
        _require(t.is_contiguous() and t.element_size() == element_size and t.numel() == self.nconn and
                 not t.dtype.is_floating_point, f"{name} must be nconn contiguous {8 * element_size}-bit integers")

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_ack_set_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def receive(self, info, conn_of, now_us: int, seg_status=None, npackets: Optional[int] = None, stream=None):
        """ugo_fec_ack_set_receive: info uint8 [>= npackets, 64] as packet_decode
        returned it, conn_of int32 [>= npackets] the member of each packet,
        seg_status uint8 [>= npackets, max_segments] as StreamRxSet.deliver
        returned it, or None.  npackets defaults to info.shape[0]."""
        npk = info.shape[0] if npackets is None else npackets
        _require(0 <= npk <= info.shape[0] and 0 <= now_us < 1 << 64)
        _require(info.is_contiguous() and info.element_size() == 1 and info.dim() == 2 and info.shape[1] == 64)
        _require(conn_of.is_contiguous() and conn_of.element_size() == 4 and conn_of.numel() >= npk and
                 not conn_of.dtype.is_floating_point, "conn_of must be npackets contiguous 32-bit integers")
        max_segments = 0
        if seg_status is not None:
            _require(seg_status.is_contiguous() and seg_status.element_size() == 1 and seg_status.dim() == 2 and
                     seg_status.shape[0] >= npk and 1 <= seg_status.shape[1] <= 0xffff)
            max_segments = seg_status.shape[1]
        _raise(load_library().ugo_fec_ack_set_receive(
            self._h, info.data_ptr(), conn_of.data_ptr(), npk, None if seg_status is None else seg_status.data_ptr(),
            max_segments, now_us, _stream_handle(stream)))

    def touch(self, flags, stream=None):
        """changed = 1 for the members with flags[c] != 0 (uint8 [nconn])."""
        self.check_per_conn(flags, 1, "flags")
        _raise(load_library().ugo_fec_ack_set_touch(self._h, flags.data_ptr(), _stream_handle(stream)))

    def attach(self, now_us: int, first_packet, n_packets, total, info, ranges, conn_of, may_ack_only=None,
               total_out=None, attached=None, stream=None):
        """ugo_fec_ack_set_attach: first_packet int64 [nconn], n_packets int32
        [nconn] and total int64 [1] as StreamTxSet.plan returned them; info uint8
        [max_packets, 64], ranges int64 [max_packets, max_ranges, 2] and conn_of
        int32 [max_packets] the arrays StreamTxSet.encode will be given;
        may_ack_only uint8 [nconn] or None.  Returns (total_out int64 [1],
        attached uint8 [nconn] of ACK_*); both may be given, and total_out may
        be total itself."""
        max_packets = info.shape[0]
        _require(0 <= now_us < 1 << 64 and max_packets <= 1 << 31)
        _require(info.is_contiguous() and info.element_size() == 1 and info.dim() == 2 and info.shape[1] == 64)
        _require(ranges.is_contiguous() and ranges.element_size() == 8 and ranges.dim() == 3 and
                 ranges.shape[0] == max_packets and ranges.shape[1] <= 0xffff and ranges.shape[2] == 2)
        _require(conn_of.is_contiguous() and conn_of.element_size() == 4 and conn_of.numel() == max_packets and
                 not conn_of.dtype.is_floating_point)
        self.check_per_conn(first_packet, 8, "first_packet")
        self.check_per_conn(n_packets, 4, "n_packets")
        _require(total.numel() == 1 and total.element_size() == 8)
        if may_ack_only is not None:
            self.check_per_conn(may_ack_only, 1, "may_ack_only")
        dev = torch.device("cuda", self.device)
        if total_out is None:
            total_out = torch.zeros(1, dtype=torch.int64, device=dev)
        if attached is None:
            attached = torch.zeros(self.nconn, dtype=torch.uint8, device=dev)
        _require(total_out.numel() == 1 and total_out.element_size() == 8)
        self.check_per_conn(attached, 1, "attached")
        _raise(load_library().ugo_fec_ack_set_attach(
            self._h, now_us, first_packet.data_ptr(), n_packets.data_ptr(), total.data_ptr(),
            None if may_ack_only is None else may_ack_only.data_ptr(), max_packets, info.data_ptr(),
            ranges.data_ptr() if ranges.numel() else None, ranges.shape[1], conn_of.data_ptr(), total_out.data_ptr(),
            attached.data_ptr(), _stream_handle(stream)))
        return total_out, attached

    def states(self) -> np.ndarray:
        """The members' records (ACK_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, ACK_STATE_DTYPE)
        _raise(load_library().ugo_fec_ack_set_state(self._h, out.ctypes.data))
        return out


class SentTx:
    """A connection's sent history on the GPU (include/ugo_sent.h): the
    packetSender's state, a slot ring of window_packets numbers, their segment
    rows and a record.  Every call goes through a SentTxSet; a set of one is
    the single-connection form."""

    def __init__(self, enc: Encoder, window_packets: int = 4096, seg_cap: int = 8):
        self.check_create(window_packets, seg_cap)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_sent_tx_create(enc._h, window_packets, seg_cap, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the history
        self.window_packets, self.seg_cap = window_packets, seg_cap
        self.device = enc.device
        self._sets = weakref.WeakSet()  # the open sets it is a member of: closed before it

    @staticmethod
    def check_create(window_packets: int, seg_cap: int):
        _require(SENT_MIN_WINDOW <= window_packets <= SENT_MAX_WINDOW and
                 window_packets & (window_packets - 1) == 0,
                 f"window_packets must be a power of two in [{SENT_MIN_WINDOW}, 2^20]")
        _require(1 <= seg_cap <= SENT_MAX_SEG_CAP, f"seg_cap must be 1 to {SENT_MAX_SEG_CAP}")

    def close(self):
        if getattr(self, "_h", None):
            for s in list(self._sets):
                s.close()
            load_library().ugo_fec_sent_tx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def slots(self):
        """The slot ring as a uint8 CUDA tensor [window_packets, 32] over the
        device memory itself (SENT_SLOT_DTYPE rows); valid while this object lives."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_sent_tx_slots(self._h, ctypes.byref(p), ctypes.byref(n)))
        t = torch.as_tensor(_DeviceBytes(p.value, n.value * 32, self), device=torch.device("cuda", self.device))
        return t.view(n.value, 32)

    def segments(self):
        """The segment ring as a uint8 CUDA tensor [window_packets, seg_cap, 16]
        (SENT_SEG_DTYPE entries) over the device memory itself."""
        p, n, s = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_sent_tx_segments(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(s)))
        t = torch.as_tensor(_DeviceBytes(p.value, n.value * s.value * 16, self),
                            device=torch.device("cuda", self.device))
        return t.view(n.value, s.value, 16)


    def scratch(self):
        """The difference ring and the claim ring as an int32 CUDA tensor
        [2 * window_packets] over the device memory itself: zero between calls."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _raise(load_library().ugo_fec_sent_tx_scratch(self._h, ctypes.byref(p), ctypes.byref(n)))
        t = torch.as_tensor(_DeviceBytes(p.value, n.value * 4, self), device=torch.device("cuda", self.device))
        return t.view(torch.int32)


class SentTxSet:
    """An ordered set of sent histories (ugo_fec_sent_set_*): record what
    StreamTxSet.encode sent, ack for a decoded batch, rto, drain into the form
    StreamTxSet.retransmit takes, attach a pending stop-waiting to the plan.
    Operands are tensors in device or pinned host memory.  Nothing is
    synchronised but states().  The set does not own its members; close it
    before them."""

    def __init__(self, enc: Encoder, txs):
        txs = list(txs)
        self.check_members(enc, txs)
        arr = (ctypes.c_void_p * len(txs))(*[tx._h.value for tx in txs])
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_sent_set_create(enc._h, ctypes.addressof(arr), len(txs), ctypes.byref(h)))
        self._h, self._enc, self.txs = h, enc, txs  # context and members must outlive the set
        self.nconn = len(txs)
        self.min_seg_cap = min(tx.seg_cap for tx in txs)
        for tx in txs:
            tx._sets.add(self)
        self.device = enc.device
        self._cc_sets = weakref.WeakSet()  # the open controller sets that read it: closed before it

    @staticmethod
    def check_members(enc, txs):
        _require(0 < len(txs) <= STREAM_SET_MAX_CONN, f"a set holds 1 to {STREAM_SET_MAX_CONN} histories")
        _require(all(isinstance(tx, SentTx) and getattr(tx, "_h", None) for tx in txs), "members must be open SentTx")
        _require(all(tx._enc is enc for tx in txs), "every member must belong to the set's context")
        _require(len({id(tx) for tx in txs}) == len(txs), "a history may be listed once")

    def check_per_conn(self, t, element_size: int, name: str):
        _require(t.is_contiguous() and t.element_size() == element_size and t.numel() == self.nconn and
                 not t.dtype.is_floating_point, f"{name} must be nconn contiguous {8 * element_size}-bit integers")

    @staticmethod
    def _check_info(info, npk):
        _require(info.is_contiguous() and info.element_size() == 1 and info.dim() == 2 and info.shape[1] == 64 and
                 0 <= npk <= info.shape[0] and npk <= 1 << 31)

    @staticmethod
    def _check_list(t, n, element_size: int, name: str):
        _require(t.is_contiguous() and t.element_size() == element_size and t.numel() >= n and
                 not t.dtype.is_floating_point, f"{name} must be contiguous {8 * element_size}-bit integers")

    def close(self):
        if getattr(self, "_h", None):
            for s in list(getattr(self, "_cc_sets", ())):
                s.close()
            load_library().ugo_fec_sent_set_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _dev(self):
        return torch.device("cuda", self.device)

    def record(self, info, segs, conn_of, wire_lens, status, now_us: int, npackets: Optional[int] = None,
               stream=None):
        """ugo_fec_sent_set_record: info uint8 [>= npackets, 64], segs uint8
        [>= npackets, max_segments, 16] and conn_of int32 as StreamTxSet.plan left
        them, wire_lens int16 and status uint8 as StreamTxSet.encode returned them."""
        npk = info.shape[0] if npackets is None else npackets
        self._check_info(info, npk)
        _require(0 <= now_us < 1 << 64)
        _require(segs.is_contiguous() and segs.element_size() == 1 and segs.dim() == 3 and segs.shape[2] == 16 and
                 segs.shape[0] >= npk and 1 <= segs.shape[1] <= self.min_seg_cap,
                 "segs must be [npackets, max_segments, 16] with max_segments at most the smallest seg_cap")
        self._check_list(conn_of, npk, 4, "conn_of")
        self._check_list(wire_lens, npk, 2, "wire_lens")
        self._check_list(status, npk, 1, "status")
        _raise(load_library().ugo_fec_sent_set_record(
            self._h, info.data_ptr(), segs.data_ptr(), segs.shape[1], conn_of.data_ptr(), wire_lens.data_ptr(),
            status.data_ptr(), npk, now_us, _stream_handle(stream)))

    def ack(self, info, ranges, conn_of, now_us: int, npackets: Optional[int] = None, events=None, stream=None):
        """ugo_fec_sent_set_ack: info uint8 [>= npackets, 64] and ranges int64
        [>= npackets, max_ranges, 2] as packet_decode returned them, conn_of int32.
        Returns events uint8 [nconn, 64] (SENT_EVENT_DTYPE rows); may be given."""
        npk = info.shape[0] if npackets is None else npackets
        self._check_info(info, npk)
        _require(0 <= now_us < 1 << 64)
        _require(ranges.is_contiguous() and ranges.element_size() == 8 and ranges.dim() == 3 and
                 ranges.shape[0] >= npk and ranges.shape[1] <= 0xffff and ranges.shape[2] == 2)
        self._check_list(conn_of, npk, 4, "conn_of")
        if events is None:
            events = torch.zeros((self.nconn, 64), dtype=torch.uint8, device=self._dev())
        _require(events.is_contiguous() and events.element_size() == 1 and tuple(events.shape) == (self.nconn, 64))
        _raise(load_library().ugo_fec_sent_set_ack(
            self._h, info.data_ptr(), ranges.data_ptr() if ranges.numel() else None, ranges.shape[1],
            conn_of.data_ptr(), npk, now_us, events.data_ptr(), _stream_handle(stream)))
        return events

    def rto(self, delay_us, now_us: int, fired=None, stream=None):
        """ugo_fec_sent_set_rto: delay_us int64 [nconn].  Returns fired uint8 [nconn]."""
        self.check_per_conn(delay_us, 8, "delay_us")
        _require(0 <= now_us < 1 << 64)
        if fired is None:
            fired = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        self.check_per_conn(fired, 1, "fired")
        _raise(load_library().ugo_fec_sent_set_rto(self._h, delay_us.data_ptr(), now_us, fired.data_ptr(),
                                                   _stream_handle(stream)))
        return fired

    def drain(self, max_entries: int, out=None, stream=None):
        """ugo_fec_sent_set_drain.  Returns (conn_of int32 [max_entries], offset
        int64 [max_entries], len int32 [max_entries], n_entries int64 [1], touch
        uint8 [nconn], upto int64 [nconn]); out = such a tuple to write into."""
        _require(0 <= max_entries <= 1 << 31)
        dev = self._dev()
        if out is None:
            out = (torch.zeros(max_entries, dtype=torch.int32, device=dev),
                   torch.zeros(max_entries, dtype=torch.int64, device=dev),
                   torch.zeros(max_entries, dtype=torch.int32, device=dev),
                   torch.zeros(1, dtype=torch.int64, device=dev),
                   torch.zeros(self.nconn, dtype=torch.uint8, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int64, device=dev))
        conn_of, offset, length, n_entries, touch, upto = out
        self._check_list(conn_of, max_entries, 4, "conn_of")
        self._check_list(offset, max_entries, 8, "offset")
        self._check_list(length, max_entries, 4, "len")
        _require(n_entries.numel() == 1 and n_entries.element_size() == 8)
        self.check_per_conn(touch, 1, "touch")
        self.check_per_conn(upto, 8, "upto")
        _raise(load_library().ugo_fec_sent_set_drain(
            self._h, max_entries, conn_of.data_ptr() if max_entries else None,
            offset.data_ptr() if max_entries else None, length.data_ptr() if max_entries else None,
            n_entries.data_ptr(), touch.data_ptr(), upto.data_ptr(), _stream_handle(stream)))
        return out

    def attach(self, first_packet, n_packets, info, attached=None, stream=None):
        """ugo_fec_sent_set_attach: first_packet int64 [nconn] and n_packets int32
        [nconn] as StreamTxSet.plan returned them, info uint8 [max_packets, 64].
        Returns attached uint8 [nconn]."""
        self._check_info(info, info.shape[0])
        self.check_per_conn(first_packet, 8, "first_packet")
        self.check_per_conn(n_packets, 4, "n_packets")
        if attached is None:
            attached = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        self.check_per_conn(attached, 1, "attached")
        _raise(load_library().ugo_fec_sent_set_attach(
            self._h, first_packet.data_ptr(), n_packets.data_ptr(), info.shape[0],
            info.data_ptr() if info.shape[0] else None, attached.data_ptr(), _stream_handle(stream)))
        return attached

    def states(self) -> np.ndarray:
        """The members' records (SENT_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, SENT_STATE_DTYPE)
        _raise(load_library().ugo_fec_sent_set_state(self._h, out.ctypes.data))
        return out


class CcSet:
    """The congestion controllers of a SentTxSet's members (include/ugo_cc.h):
    RTT filter, hybrid slow start and CUBIC, one record per member.  Per batch:
    sent_ack in place of SentTxSet.ack, ack, SentTxSet.rto with the delays ack
    returned, rto, and the next StreamTxSet.plan with the budget rto returned.
    Operands are tensors in device or pinned host memory; nothing is
    synchronised but states().  Close it before the SentTxSet."""

    def __init__(self, enc: Encoder, sent: "SentTxSet", **params):
        p = self.check_params(**params)
        _require(isinstance(sent, SentTxSet) and getattr(sent, "_h", None) and sent._enc is enc,
                 "sent must be an open SentTxSet of the same context")
        arr = np.array([tuple(p[k] for k in CC_PARAMS_DTYPE.names)], CC_PARAMS_DTYPE)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_cc_set_create(enc._h, sent._h, arr.ctypes.data if params else None,
                                                    ctypes.byref(h)))
        self._h, self._enc, self.sent = h, enc, sent  # context and sent set must outlive the set
        self.nconn, self.params, self.device = sent.nconn, p, enc.device
        sent._cc_sets.add(self)

    @staticmethod
    def check_params(**params):
        _require(set(params) <= set(CC_DEFAULTS), f"parameters are {sorted(CC_DEFAULTS)}")
        p = dict(CC_DEFAULTS, **params)
        _require(all(isinstance(v, int) and 0 <= v < 1 << 32 for v in p.values()))
        _require(1 <= p["min_cwnd"] <= p["initial_cwnd"] <= p["max_cwnd"] <= CC_MAX_CWND_LIMIT,
                 "1 <= min_cwnd <= initial_cwnd <= max_cwnd <= 2^20")
        _require(p["num_connections"] >= 1 and p["mss"] >= 1, "num_connections and mss must be at least 1")
        return p

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_cc_set_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _dev(self):
        return torch.device("cuda", self.device)

    def cutback(self):
        """ugo_fec_cc_set_cutback: the dense cutback array as an int64 CUDA tensor
        [nconn] over the device memory itself: what sent_ack takes as split."""
        p = ctypes.c_void_p()
        _raise(load_library().ugo_fec_cc_set_cutback(self._h, ctypes.byref(p)))
        t = torch.as_tensor(_DeviceBytes(p.value, self.nconn * 8, self), device=self._dev())
        return t.view(torch.int64)

    def sent_ack(self, info, ranges, conn_of, now_us: int, npackets: Optional[int] = None, events=None, split=None,
                 rows=None, stream=None):
        """ugo_fec_cc_sent_ack: SentTxSet.ack, and rows uint8 [nconn, 32]
        (CC_ROW_DTYPE) beside events.  split int64 [nconn]; None: the set's own
        cutback array.  Returns (events, rows)."""
        sent = self.sent
        npk = info.shape[0] if npackets is None else npackets
        sent._check_info(info, npk)
        _require(0 <= now_us < 1 << 64)
        _require(ranges.is_contiguous() and ranges.element_size() == 8 and ranges.dim() == 3 and
                 ranges.shape[0] >= npk and ranges.shape[1] <= 0xffff and ranges.shape[2] == 2)
        sent._check_list(conn_of, npk, 4, "conn_of")
        if events is None:
            events = torch.zeros((self.nconn, 64), dtype=torch.uint8, device=self._dev())
        if rows is None:
            rows = torch.zeros((self.nconn, 32), dtype=torch.uint8, device=self._dev())
        if split is None:
            split = self.cutback()
        _require(events.is_contiguous() and events.element_size() == 1 and tuple(events.shape) == (self.nconn, 64))
        _require(rows.is_contiguous() and rows.element_size() == 1 and tuple(rows.shape) == (self.nconn, 32))
        sent.check_per_conn(split, 8, "split")
        _raise(load_library().ugo_fec_cc_sent_ack(
            sent._h, info.data_ptr(), ranges.data_ptr() if ranges.numel() else None, ranges.shape[1],
            conn_of.data_ptr(), npk, now_us, events.data_ptr(), split.data_ptr(), rows.data_ptr(),
            _stream_handle(stream)))
        return events, rows

    def ack(self, events, rows, now_us: int, delay_us=None, stream=None):
        """ugo_fec_cc_set_ack: events uint8 [nconn, 64] and rows uint8 [nconn, 32]
        as sent_ack returned them.  Returns delay_us int64 [nconn]: the input of
        SentTxSet.rto."""
        _require(0 <= now_us < 1 << 64)
        _require(events.is_contiguous() and events.element_size() == 1 and tuple(events.shape) == (self.nconn, 64))
        _require(rows.is_contiguous() and rows.element_size() == 1 and tuple(rows.shape) == (self.nconn, 32))
        if delay_us is None:
            delay_us = torch.zeros(self.nconn, dtype=torch.int64, device=self._dev())
        self.sent.check_per_conn(delay_us, 8, "delay_us")
        _raise(load_library().ugo_fec_cc_set_ack(self._h, events.data_ptr(), rows.data_ptr(), now_us,
                                                 delay_us.data_ptr(), _stream_handle(stream)))
        return delay_us

    def rto(self, fired, packet_bytes: int, max_budget: int, budget=None, stream=None):
        """ugo_fec_cc_set_rto: fired uint8 [nconn] as SentTxSet.rto returned it.
        Returns budget int32 [nconn]: the input of StreamTxSet.plan."""
        _require(packet_bytes >= 1 and 0 <= max_budget <= 1 << 31)
        self.sent.check_per_conn(fired, 1, "fired")
        if budget is None:
            budget = torch.zeros(self.nconn, dtype=torch.int32, device=self._dev())
        self.sent.check_per_conn(budget, 4, "budget")
        _raise(load_library().ugo_fec_cc_set_rto(self._h, fired.data_ptr(), packet_bytes, max_budget,
                                                 budget.data_ptr(), _stream_handle(stream)))
        return budget

    def states(self) -> np.ndarray:
        """The members' records (CC_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, CC_STATE_DTYPE)
        _raise(load_library().ugo_fec_cc_set_state(self._h, out.ctypes.data))
        return out


class ListenTable:
    """The connection table of a listening socket (include/ugo_listen.h):
    listener.handlePacket for a whole ring per call.  route writes conn_of for
    the stages that take it and the list of accepted connections; names turns
    the conn_of of StreamTxSet.plan into sendmmsg names; remap goes with a set
    rebuild.  Operands are tensors in device or pinned host memory; nothing is
    synchronised but state() and entries()."""

    def __init__(self, enc: "Encoder", max_conn: int):
        _require(isinstance(max_conn, int) and 1 <= max_conn <= LISTEN_MAX_CONN, "1 <= max_conn <= 2^20")
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_listen_create(enc._h, max_conn, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the table
        self.max_conn, self.device = max_conn, enc.device

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_listen_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _dev(self):
        return torch.device("cuda", self.device)

    @staticmethod
    def _check(t, n, item, what, row=None):
        shape = (n,) if row is None else (n, row)
        _require(t.is_contiguous() and t.element_size() == item and t.dim() == len(shape) and t.shape[0] >= n and
                 tuple(t.shape[1:]) == shape[1:], f"{what} must be contiguous, {item}-byte, at least {shape}")

    def route(self, names, pkts, lens, npackets: Optional[int] = None, conn_of=None, cls=None, accepted=None,
              n_accepted=None, stream=None):
        """ugo_fec_listen_route.  names uint8 [npackets, 32], pkts uint8
        [npackets, slot], lens int16 [npackets].  Returns (conn_of int32
        [npackets], cls uint8 [npackets], accepted uint8 [max_accepted, 48]
        (LISTEN_ACCEPT_DTYPE), n_accepted int32 [1]); accepted defaults to
        min(npackets, max_conn) rows."""
        npk = pkts.shape[0] if npackets is None else npackets
        _require(0 <= npk <= 1 << 31)
        _require(pkts.is_contiguous() and pkts.element_size() == 1 and pkts.dim() == 2 and pkts.shape[0] >= npk)
        self._check(names, npk, 1, "names", LISTEN_NAME_BYTES)
        self._check(lens, npk, 2, "lens")
        dev = self._dev()
        if conn_of is None:
            conn_of = torch.zeros(npk, dtype=torch.int32, device=dev)
        if cls is None:
            cls = torch.zeros(npk, dtype=torch.uint8, device=dev)
        if accepted is None:
            accepted = torch.zeros((min(npk, self.max_conn), 48), dtype=torch.uint8, device=dev)
        if n_accepted is None:
            n_accepted = torch.zeros(1, dtype=torch.int32, device=dev)
        self._check(conn_of, npk, 4, "conn_of")
        self._check(cls, npk, 1, "cls")
        self._check(accepted, accepted.shape[0], 1, "accepted", 48)
        self._check(n_accepted, 1, 4, "n_accepted")
        _raise(load_library().ugo_fec_listen_route(
            self._h, names.data_ptr(), pkts.data_ptr(), pkts.shape[1], lens.data_ptr(), npk, conn_of.data_ptr(),
            cls.data_ptr(), accepted.data_ptr() if accepted.shape[0] else None, accepted.shape[0],
            n_accepted.data_ptr(), _stream_handle(stream)))
        return conn_of, cls, accepted, n_accepted

    def remap(self, new_index, nconn_new: int, status=None, stream=None):
        """ugo_fec_listen_remap.  new_index int32 [nconn] (STREAM_NO_CONN as -1
        closes a member).  Returns status int32 [1]: 0 or LISTEN_REMAP_* bits."""
        _require(isinstance(nconn_new, int) and nconn_new >= 0)
        self._check(new_index, new_index.shape[0], 4, "new_index")
        _require(new_index.shape[0] <= LISTEN_MAX_CONN)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=self._dev())
        self._check(status, 1, 4, "status")
        _raise(load_library().ugo_fec_listen_remap(
            self._h, new_index.data_ptr() if new_index.shape[0] else None, new_index.shape[0], nconn_new,
            status.data_ptr(), _stream_handle(stream)))
        return status

    def names(self, conn_of, npackets: Optional[int] = None, names_out=None, name_lens=None, stream=None):
        """ugo_fec_listen_names.  conn_of int32 [npackets] as StreamTxSet.plan
        wrote it.  Returns (names_out uint8 [npackets, 32], name_lens int32
        [npackets])."""
        npk = conn_of.shape[0] if npackets is None else npackets
        _require(0 <= npk <= 1 << 31)
        self._check(conn_of, npk, 4, "conn_of")
        if names_out is None:
            names_out = torch.zeros((npk, LISTEN_NAME_BYTES), dtype=torch.uint8, device=self._dev())
        if name_lens is None:
            name_lens = torch.zeros(npk, dtype=torch.int32, device=self._dev())
        self._check(names_out, npk, 1, "names_out", LISTEN_NAME_BYTES)
        self._check(name_lens, npk, 4, "name_lens")
        _raise(load_library().ugo_fec_listen_names(self._h, conn_of.data_ptr(), npk, names_out.data_ptr(),
                                                   name_lens.data_ptr(), _stream_handle(stream)))
        return names_out, name_lens

    def state(self) -> np.ndarray:
        """The table's record (LISTEN_STATE_DTYPE scalar); waits for the last call on the table."""
        out = np.zeros(1, LISTEN_STATE_DTYPE)
        _raise(load_library().ugo_fec_listen_state(self._h, out.ctypes.data))
        return out[0]

    def entries(self, out=None, stream=None) -> np.ndarray:
        """ugo_fec_listen_entries, then the rows that hold an entry
        (LISTEN_ENTRY_DTYPE), in member order; synchronises."""
        if out is None:
            out = torch.zeros((self.max_conn, 32), dtype=torch.uint8, device=self._dev())
        self._check(out, out.shape[0], 1, "out", 32)
        _raise(load_library().ugo_fec_listen_entries(self._h, out.data_ptr(), out.shape[0], _stream_handle(stream)))
        rows = out.cpu().numpy().view(LISTEN_ENTRY_DTYPE).reshape(-1)
        return rows[rows["member"] != STREAM_NO_CONN]


class LoopSet:
    """The connection loop of a set of connections (include/ugo_loop.h): the
    timers, FIN / RST and the exits, one record per member of a StreamRxSet, an
    AckRxSet, a StreamTxSet and a SentTxSet of the same size.  Per batch:
    receive after packet_decode, check before StreamTxSet.plan, append after it,
    sent after StreamTxSet.encode; close between batches.  Operands are tensors
    in device or pinned host memory; nothing is synchronised but states().
    Close it before the four sets."""

    def __init__(self, enc: Encoder, stream_rx: "StreamRxSet", ack_rx: "AckRxSet", stream_tx: "StreamTxSet",
                 sent_tx: "SentTxSet", now_us: int = 0, **params):
        p = self.check_params(**params)
        sets = (stream_rx, ack_rx, stream_tx, sent_tx)
        kinds = (StreamRxSet, AckRxSet, StreamTxSet, SentTxSet)
        _require(all(isinstance(s, k) and getattr(s, "_h", None) and s._enc is enc for s, k in zip(sets, kinds)),
                 "the four sets must be open sets of the same context")
        _require(len({s.nconn for s in sets}) == 1, "the four sets must have the same number of members")
        _require(0 <= now_us < 1 << 64)
        arr = np.array([(p["ack_delay_us"], p["idle_us"], p["max_retries"], 0)], LOOP_PARAMS_DTYPE)
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_loop_set_create(enc._h, stream_rx._h, ack_rx._h, stream_tx._h, sent_tx._h,
                                                      arr.ctypes.data if params else None, now_us, ctypes.byref(h)))
        self._h, self._enc, self.sets = h, enc, sets  # the context and the four sets must outlive the set
        self.nconn, self.params, self.device = sent_tx.nconn, p, enc.device

    @staticmethod
    def check_params(**params):
        _require(set(params) <= set(LOOP_DEFAULTS), f"parameters are {sorted(LOOP_DEFAULTS)}")
        p = dict(LOOP_DEFAULTS, **params)
        _require(all(isinstance(v, int) for v in p.values()))
        _require(0 <= p["ack_delay_us"] < 1 << 64 and 1 <= p["idle_us"] < 1 << 64 and
                 0 <= p["max_retries"] < 1 << 32, "idle_us must be at least 1")
        return p

    def close(self):
        if getattr(self, "_h", None):
            load_library().ugo_fec_loop_set_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _dev(self):
        return torch.device("cuda", self.device)

    def _per_conn(self, t, item: int, name: str):
        _require(t.is_contiguous() and t.element_size() == item and tuple(t.shape) == (self.nconn,),
                 f"{name} must be contiguous, {item}-byte, [nconn]")

    @staticmethod
    def _list(t, n: int, item: int, name: str, row=None):
        shape = (n,) if row is None else (n, row)
        _require(t.is_contiguous() and t.element_size() == item and t.dim() == len(shape) and t.shape[0] >= n and
                 tuple(t.shape[1:]) == shape[1:], f"{name} must be contiguous, {item}-byte, at least {shape}")

    def receive(self, info, conn_of, now_us: int, npackets: Optional[int] = None, stream=None):
        """ugo_fec_loop_set_receive: info uint8 [npackets, 64] as packet_decode
        wrote it, conn_of int32 [npackets], masked in place.  Returns conn_of."""
        npk = info.shape[0] if npackets is None else npackets
        _require(0 <= npk <= 1 << 31 and 0 <= now_us < 1 << 64)
        self._list(info, npk, 1, "info", 64)
        self._list(conn_of, npk, 4, "conn_of")
        _raise(load_library().ugo_fec_loop_set_receive(self._h, info.data_ptr() if npk else None,
                                                       conn_of.data_ptr() if npk else None, npk, now_us,
                                                       _stream_handle(stream)))
        return conn_of

    def close_members(self, how, now_us: int, linger_us=None, stream=None):
        """ugo_fec_loop_set_close: how uint8 [nconn] of LOOP_HOW_* bits,
        linger_us int64 [nconn] or None."""
        _require(0 <= now_us < 1 << 64)
        self._per_conn(how, 1, "how")
        if linger_us is not None:
            self._per_conn(linger_us, 8, "linger_us")
        _raise(load_library().ugo_fec_loop_set_close(self._h, how.data_ptr(),
                                                     None if linger_us is None else linger_us.data_ptr(), now_us,
                                                     _stream_handle(stream)))

    def check(self, now_us: int, budget, may_ack_only=None, stream=None):
        """ugo_fec_loop_set_check: budget int32 [nconn], zeroed in place where a
        member may send no data.  Returns may_ack_only uint8 [nconn]: the input
        of AckRxSet.attach."""
        _require(0 <= now_us < 1 << 64)
        self._per_conn(budget, 4, "budget")
        if may_ack_only is None:
            may_ack_only = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        self._per_conn(may_ack_only, 1, "may_ack_only")
        _raise(load_library().ugo_fec_loop_set_check(self._h, now_us, budget.data_ptr(), may_ack_only.data_ptr(),
                                                     _stream_handle(stream)))
        return may_ack_only

    def append(self, total, info, segs, conn_of, total_out=None, appended=None, max_packets: Optional[int] = None,
               stream=None):
        """ugo_fec_loop_set_append: total int64 [1], info uint8 [max_packets, 64],
        segs uint8 [max_packets, max_segments, 16], conn_of int32 [max_packets] as
        StreamTxSet.plan wrote them.  Returns (total_out int64 [1], appended uint8
        [nconn]); total_out defaults to total itself."""
        cap = info.shape[0] if max_packets is None else max_packets
        _require(0 <= cap <= 1 << 31)
        self._list(total, 1, 8, "total")
        self._list(info, cap, 1, "info", 64)
        _require(segs.is_contiguous() and segs.element_size() == 1 and segs.dim() == 3 and segs.shape[0] >= cap and
                 1 <= segs.shape[1] <= 0xffff and segs.shape[2] == 16, "segs must be uint8 [max_packets, S, 16]")
        self._list(conn_of, cap, 4, "conn_of")
        if total_out is None:
            total_out = total
        if appended is None:
            appended = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        self._list(total_out, 1, 8, "total_out")
        self._per_conn(appended, 1, "appended")
        _raise(load_library().ugo_fec_loop_set_append(self._h, total.data_ptr(), cap, info.data_ptr(),
                                                      segs.data_ptr(), segs.shape[1], conn_of.data_ptr(),
                                                      total_out.data_ptr(), appended.data_ptr(),
                                                      _stream_handle(stream)))
        return total_out, appended

    def sent(self, n_packets, attached, now_us: int, delay_us=None, max_exits: Optional[int] = None, remap=False,
             out=None, stream=None):
        """ugo_fec_loop_set_sent: n_packets int32 [nconn] as StreamTxSet.plan
        wrote it, attached uint8 [nconn] as AckRxSet.attach wrote it, delay_us
        int64 [nconn] as CcSet.ack wrote it or None.  Returns (deadline_us int64
        [1], exits int32 [max_exits], reasons uint8 [max_exits], n_exits int64 [1],
        new_index int32 [nconn] or None, nconn_new int64 [1] or None); out: the
        same tuple, preallocated.  max_exits defaults to nconn."""
        _require(0 <= now_us < 1 << 64)
        self._per_conn(n_packets, 4, "n_packets")
        self._per_conn(attached, 1, "attached")
        if delay_us is not None:
            self._per_conn(delay_us, 8, "delay_us")
        dev = self._dev()
        if out is None:
            cap = self.nconn if max_exits is None else max_exits
            out = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev),
                   torch.zeros(cap, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int32, device=dev) if remap else None,
                   torch.zeros(1, dtype=torch.int64, device=dev) if remap else None)
        deadline, exits, reasons, n_exits, new_index, nconn_new = out
        cap = exits.shape[0] if max_exits is None else max_exits
        self._list(deadline, 1, 8, "deadline_us")
        self._list(exits, cap, 4, "exits")
        self._list(reasons, cap, 1, "reasons")
        self._list(n_exits, 1, 8, "n_exits")
        _require((new_index is None) == (nconn_new is None), "new_index and nconn_new go together")
        if new_index is not None:
            self._per_conn(new_index, 4, "new_index")
            self._list(nconn_new, 1, 8, "nconn_new")
        _raise(load_library().ugo_fec_loop_set_sent(
            self._h, n_packets.data_ptr(), attached.data_ptr(), None if delay_us is None else delay_us.data_ptr(),
            now_us, deadline.data_ptr(), exits.data_ptr() if cap else None, reasons.data_ptr() if cap else None, cap,
            n_exits.data_ptr(), None if new_index is None else new_index.data_ptr(),
            None if nconn_new is None else nconn_new.data_ptr(), _stream_handle(stream)))
        return out

    def states(self) -> np.ndarray:
        """The members' records (LOOP_STATE_DTYPE [nconn]); waits for the last call on the set."""
        out = np.zeros(self.nconn, LOOP_STATE_DTYPE)
        _raise(load_library().ugo_fec_loop_set_state(self._h, out.ctypes.data))
        return out


def rc4_keystream(key: bytes, n: int) -> bytes:
    """RC4 keystream prefix (ugo/crypto.go's fixed-key per-packet cipher)."""
    out = (ctypes.c_uint8 * n)()
    k = (ctypes.c_uint8 * len(key)).from_buffer_copy(key)
    _raise(load_library().ugo_fec_rc4_keystream(ctypes.addressof(k), len(key), ctypes.addressof(out), n))
    return bytes(out)


def New(data_shards: int, parity_shards: int, device: int = 0) -> Encoder:
    """reedsolomon.New as called at ugo/fec.go:59."""
    return Encoder(data_shards, parity_shards, device)


def host_alloc(nbytes: int) -> np.ndarray:
    """Pinned host buffer (uint8 numpy view); free with host_free(arr)."""
    lib = load_library()
    p = ctypes.c_void_p()
    _raise(lib.ugo_fec_host_alloc(nbytes, ctypes.byref(p)))
    arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    return arr


def host_free(arr: np.ndarray) -> None:
    _raise(load_library().ugo_fec_host_free(ctypes.c_void_p(arr.ctypes.data)))


# ---------------------------------------------------------------- FEC object
UGO_FEC_MAX_PACKET = 1476
_CLOCK_T = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_void_p)


def _bind_conn(lib):
    if getattr(lib, "_conn_bound", False):
        return lib
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.ugo_fecconn_new.argtypes = [i, i, i, i, ctypes.POINTER(vp)]
    lib.ugo_fecconn_free.argtypes = [vp]
    lib.ugo_fecconn_free.restype = None
    lib.ugo_fecconn_set_clock.argtypes = [vp, _CLOCK_T, vp]
    lib.ugo_fecconn_mark_data.argtypes = [vp, vp]
    lib.ugo_fecconn_mark_fec.argtypes = [vp, vp]
    lib.ugo_fecconn_get_next.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    lib.ugo_fecconn_set_next.argtypes = [vp, ctypes.c_uint32]
    lib.ugo_fecconn_input.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint16),
                                      vp, sz, ctypes.POINTER(i), ctypes.POINTER(sz)]
    lib.ugo_fecconn_calc_ecc.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), i, i, i]
    lib.ugo_fecconn_rx_len.argtypes = [vp, ctypes.POINTER(sz)]
    lib.ugo_fecconn_set_batch.argtypes = [vp, i, vp, sz, ctypes.POINTER(i), ctypes.POINTER(sz)]
    lib.ugo_fecconn_set_batch_ex.argtypes = [vp, i, ctypes.c_uint, vp, sz, ctypes.POINTER(i), ctypes.POINTER(sz)]
    lib.ugo_fecconn_flush.argtypes = [vp, vp, sz, ctypes.POINTER(i), ctypes.POINTER(sz)]
    lib.ugo_fecconn_pending.argtypes = [vp, ctypes.POINTER(sz)]
    lib.ugo_fecconn_service.argtypes = [vp, ctypes.c_int]
    lib._conn_bound = True
    return lib


class FecConn:
    """ugo's per-connection FEC object (ugo/fec.go:14-27) as implemented by the
    C++ host mirror (ugo_amd/csrc/host/fec.cpp) behind include/ugo_fec_conn.h."""

    def __init__(self, rxlimit: int, data_shards: int, parity_shards: int, device: int = 0):
        lib = _bind_conn(load_library())
        h = ctypes.c_void_p()
        _raise(lib.ugo_fecconn_new(rxlimit, data_shards, parity_shards, device, ctypes.byref(h)))
        self._h, self._lib = h, lib
        self.dataShards, self.parityShards = data_shards, parity_shards
        self._clock_cb = None
        self._out = (ctypes.c_uint8 * (data_shards * UGO_FEC_MAX_PACKET))()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ugo_fecconn_free(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_clock(self, fn):
        """fn() -> uint32 milliseconds (replaces currentMs, ugo/fec.go:73)."""
        self._clock_cb = _CLOCK_T(lambda _u: fn() & 0xFFFFFFFF)
        _raise(self._lib.ugo_fecconn_set_clock(self._h, self._clock_cb, None))

    def markData(self, buf: bytearray):
        c = (ctypes.c_uint8 * len(buf)).from_buffer(buf)
        _raise(self._lib.ugo_fecconn_mark_data(self._h, ctypes.addressof(c)))

    def markFEC(self, buf: bytearray):
        c = (ctypes.c_uint8 * len(buf)).from_buffer(buf)
        _raise(self._lib.ugo_fecconn_mark_fec(self._h, ctypes.addressof(c)))

    @property
    def next(self) -> int:
        v = ctypes.c_uint32()
        _raise(self._lib.ugo_fecconn_get_next(self._h, ctypes.byref(v)))
        return v.value

    @next.setter
    def next(self, v: int):
        _raise(self._lib.ugo_fecconn_set_next(self._h, v))

    def _recovered(self, nrec, rlen):
        if not nrec.value:
            return None
        raw = bytes(self._out)
        return [bytearray(raw[i * UGO_FEC_MAX_PACKET: i * UGO_FEC_MAX_PACKET + rlen.value])
                for i in range(nrec.value)]

    def input(self, wire: bytes):
        """decode + input (ugo/conn.go:394-396): returns (seqid, flag, recovered list | None)."""
        seq, flag = ctypes.c_uint32(), ctypes.c_uint16()
        nrec, rlen = ctypes.c_int(), ctypes.c_size_t()
        w = (ctypes.c_uint8 * len(wire)).from_buffer_copy(wire)
        _raise(self._lib.ugo_fecconn_input(self._h, ctypes.addressof(w), len(wire), ctypes.byref(seq),
                                           ctypes.byref(flag), ctypes.addressof(self._out), len(self._out),
                                           ctypes.byref(nrec), ctypes.byref(rlen)))
        return seq.value, flag.value, self._recovered(nrec, rlen)

    def set_batch(self, groups: int, overlap: bool = False):
        """Batched recovery (include/ugo_fec_conn.h): recoverable lossy groups are
        recovered `groups` at a time in one launch; 0 = per call.  overlap: the
        launch runs while input goes on, its shards come back one batch later
        (UGO_FECCONN_BATCH_OVERLAP).  Returns the recovered shards of groups that
        were pending (list | None)."""
        nrec, rlen = ctypes.c_int(), ctypes.c_size_t()
        need = max(groups, 1) * (2 if overlap else 1) * self.dataShards * UGO_FEC_MAX_PACKET
        new_out = (ctypes.c_uint8 * max(need, len(self._out)))()
        old_out, self._out = self._out, new_out
        try:
            _raise(self._lib.ugo_fecconn_set_batch_ex(self._h, groups, 1 if overlap else 0,
                                                      ctypes.addressof(self._out), len(self._out),
                                                      ctypes.byref(nrec), ctypes.byref(rlen)))
        except Exception:
            self._out = old_out
            raise
        rec = self._recovered(nrec, rlen)
        self._out = (ctypes.c_uint8 * need)()
        return rec

    def flush(self):
        """Recover every pending group now (list | None)."""
        nrec, rlen = ctypes.c_int(), ctypes.c_size_t()
        _raise(self._lib.ugo_fecconn_flush(self._h, ctypes.addressof(self._out), len(self._out),
                                           ctypes.byref(nrec), ctypes.byref(rlen)))
        return self._recovered(nrec, rlen)

    def service(self, idle_us: int = 0):
        """Per-call latency service on this object's encoder (ugo_fecconn_service);
        idle_us < 0 stops it."""
        _raise(self._lib.ugo_fecconn_service(self._h, idle_us))

    def pending(self) -> int:
        v = ctypes.c_size_t()
        _raise(self._lib.ugo_fecconn_pending(self._h, ctypes.byref(v)))
        return v.value

    def calcECC(self, data: List[bytearray], offset: int, maxlen: int):
        n = len(data)
        arrs = [(ctypes.c_uint8 * len(b)).from_buffer(b) for b in data]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(a) for a in arrs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in data])
        _raise(self._lib.ugo_fecconn_calc_ecc(self._h, ptrs, lens, n, offset, maxlen))
        return data[self.dataShards:]

    def rx_len(self) -> int:
        v = ctypes.c_size_t()
        _raise(self._lib.ugo_fecconn_rx_len(self._h, ctypes.byref(v)))
        return v.value
