"""The Python binding's surface, pinned: the names ugo_amd.fec exports, the
argument types it gives every entry point, its dtypes and constants, which
operands every method of the set and table classes refuses before the library
is called, and the life cycle of the handle owners.  The literals are the
binding's behaviour before it was split into one module per header; the split
must not move any of them."""
import ctypes
import re

import numpy as np
import pytest
import torch

from ugo_amd import fec

# ------------------------------------------------------------------ CPU part
# Every non-dunder name of ugo_amd.fec.
NAMES = """
ACK_ATTACHED ACK_HEADER_PATH ACK_MAX_OUTSTANDING ACK_MAX_WINDOW ACK_MIN_WINDOW ACK_NOT_ATTACHED ACK_STATE_DTYPE
ACK_TOO_MANY_OUTSTANDING ACK_TRUNCATED AckRx AckRxSet CC_DEFAULTS CC_HEADER_PATH CC_MAX_CWND_LIMIT CC_PARAMS_DTYPE
CC_ROW_DTYPE CC_STATE_DTYPE CONN_HEADER_PATH CcSet Encoder ErrHip ErrInvShardNum ErrInvalidArg ErrMaxShardNum
ErrNoDevice ErrShardNoData ErrShardSize ErrSingular ErrTooFewShards FecConn FecError HEADER_PATH HEADER_PATHS
KERNEL_IDS KERNEL_NAMES LAUNCH_TIME_DTYPE LIB_PATH LISTEN_ACCEPT LISTEN_ACCEPT_DTYPE LISTEN_BAD_NAME LISTEN_DUP_INIT
LISTEN_ENTRY_DTYPE LISTEN_FED LISTEN_FED_NEW LISTEN_FULL LISTEN_HEADER_PATH LISTEN_MAX_CONN LISTEN_NAME_BYTES
LISTEN_NCLASS LISTEN_REFUSED LISTEN_REMAP_LENGTH LISTEN_REMAP_NOT_INJECTIVE LISTEN_REMAP_OUT_OF_RANGE
LISTEN_REMAP_TOO_MANY LISTEN_STATE_DTYPE LISTEN_STRANGER LOOP_ABORT LOOP_ACK_ERR LOOP_BAD_PACKET LOOP_CLOSED
LOOP_DEFAULTS LOOP_FAILURES LOOP_HEADER_PATH LOOP_HOW_ABORT LOOP_HOW_CLOSE LOOP_HOW_NODELAY_OFF LOOP_HOW_NODELAY_ON
LOOP_IDLE LOOP_LINGER LOOP_PARAMS_DTYPE LOOP_PEER_ACK_FIN LOOP_PEER_RST LOOP_PENDING_FIN LOOP_PENDING_NONE
LOOP_PENDING_RST LOOP_SENT_ERR LOOP_STATE_DTYPE LOOP_STREAM_ERR List ListenTable LoopSet New OK Optional PKT_CAPACITY
PKT_FEC_FRAMED PKT_HEADER_PATH PKT_INCONSISTENT_LARGEST_ACKED PKT_INCONSISTENT_LOWEST_ACKED
PKT_INCONSISTENT_RANGE_COUNT PKT_INFO_DTYPE PKT_OUT_OF_WINDOW PKT_SEGMENT_DTYPE RECONSTRUCT_DATA_ONLY SENT_EVENT_DTYPE
SENT_HEADER_PATH SENT_IN_FLIGHT SENT_MAX_SEG_CAP SENT_MAX_WINDOW SENT_MIN_WINDOW SENT_QUEUED SENT_RTO_DEFAULT_US
SENT_RTO_MAX_US SENT_RTO_MIN_US SENT_SEG_DTYPE SENT_SLOT_DTYPE SENT_STATE_DTYPE SENT_TOO_MANY_TRACKED STREAM_ACCEPTED
STREAM_DUPLICATE STREAM_HEADER_PATH STREAM_MAX_GAPS STREAM_MIN_WINDOW STREAM_NONE STREAM_NO_CONN STREAM_OUT_OF_WINDOW
STREAM_OVERLAP STREAM_SET_MAX_CONN STREAM_STATE_DTYPE STREAM_TOO_MANY_GAPS STREAM_TX_HEADER STREAM_TX_MAX_WINDOW
STREAM_TX_RQ_DTYPE STREAM_TX_RQ_FULL STREAM_TX_RQ_QUEUED STREAM_TX_RQ_REJECTED STREAM_TX_RQ_UNSORTED
STREAM_TX_STATE_DTYPE SentTx SentTxSet Sequence StreamRx StreamRxSet StreamTx StreamTxSet UGO_FEC_MAX_PACKET _CLOCK_T
_DeviceBytes _ERRORS _HERE _bind_conn _lib _raise _require _stream_handle annotations check_shards ctypes
header_stream_symbols header_symbols host_alloc host_free load_library np os rc4_keystream re strerror torch weakref
""".split()

# argtypes -> restype as ctypes type names: vp c_void_p, sz c_ulong (size_t and uint64_t), i c_int, u c_uint,
# h c_ushort, s c_char_p, *x POINTER(x), fn the clock callback; "-" = no argtypes set.
_SHORT = {"c_void_p": "vp", "c_ulong": "sz", "c_int": "i", "c_uint": "u", "c_ushort": "h", "c_char_p": "s",
          "LP_c_void_p": "*vp", "LP_c_ulong": "*sz", "LP_c_int": "*i", "LP_c_uint": "*u", "LP_c_ushort": "*h",
          "CFunctionType": "fn", "NoneType": "None"}
PROTOTYPES = {
    # ugo_fec.h
    "ugo_fec_create": "i i i *vp -> i",
    "ugo_fec_destroy": "vp -> None",
    "ugo_fec_geometry": "vp *i *i *i -> i",
    "ugo_fec_matrix": "vp vp -> i",
    "ugo_fec_encode": "vp vp sz sz sz vp -> i",
    "ugo_fec_encode_strided": "vp vp sz sz sz sz vp -> i",
    "ugo_fec_reconstruct": "vp vp vp sz sz sz u vp vp -> i",
    "ugo_fec_reconstruct_strided": "vp vp vp sz sz sz sz u vp vp -> i",
    "ugo_fec_reconstruct_into": "vp vp vp sz sz sz sz vp sz sz u vp vp -> i",
    "ugo_fec_reconstruct_rows": "vp vp vp sz sz vp sz sz u vp vp -> i",
    "ugo_fec_lossy_groups": "vp vp sz u vp vp vp -> i",
    "ugo_fec_reconstruct_list": "vp vp vp sz vp vp sz sz sz sz vp sz sz u vp vp -> i",
    "ugo_fec_recover_data": "vp vp vp sz sz sz sz vp sz sz vp vp vp -> i",
    "ugo_fec_device_address": "vp vp *vp -> i",
    "ugo_fec_encode_host": "vp vp sz sz sz -> i",
    "ugo_fec_reconstruct_host": "vp vp vp sz sz sz u vp -> i",
    "ugo_fec_service_start": "vp u -> i",
    "ugo_fec_service_stop": "vp -> i",
    "ugo_fec_service_config": "vp u u u -> i",
    "ugo_fec_poisoned": "vp -> i",
    "ugo_fec_check_shards": "i vp i *sz -> i",
    "ugo_fec_rx_assemble": "vp vp sz vp sz vp sz sz vp sz sz sz vp vp vp -> i",
    "ugo_fec_rx_assemble_frames": "vp vp sz vp sz vp sz sz vp sz sz sz vp vp vp -> i",
    "ugo_fec_tx_assemble": "vp vp sz vp sz u vp sz vp sz vp vp vp -> i",
    "ugo_fec_rx_recover_host": "vp vp sz vp sz vp sz sz sz vp vp vp sz sz vp *sz -> i",
    "ugo_fec_tx_assemble_host": "vp vp sz vp sz u vp sz vp sz vp vp -> i",
    "ugo_fec_set_tx_host_route": "vp i -> i",
    "ugo_fec_set_host_copy_queue": "vp i -> i",
    "ugo_fec_rc4_keystream": "vp sz vp sz -> i",
    "ugo_fec_timing_begin": "vp sz -> i",
    "ugo_fec_timing_end": "vp vp sz *sz *sz -> i",
    "ugo_fec_host_alloc": "sz *vp -> i",
    "ugo_fec_set_host_alloc_limit": "- -> i",
    "ugo_fec_host_free": "vp -> i",
    "ugo_fec_strerror": "i -> s",
    "ugo_fec_abi_version": " -> i",
    # ugo_fec_conn.h
    "ugo_fecconn_new": "i i i i *vp -> i",
    "ugo_fecconn_free": "vp -> None",
    "ugo_fecconn_set_clock": "vp fn vp -> i",
    "ugo_fecconn_mark_data": "vp vp -> i",
    "ugo_fecconn_mark_fec": "vp vp -> i",
    "ugo_fecconn_get_next": "vp *u -> i",
    "ugo_fecconn_set_next": "vp u -> i",
    "ugo_fecconn_input": "vp vp sz *u *h vp sz *i *sz -> i",
    "ugo_fecconn_calc_ecc": "vp *vp *sz i i i -> i",
    "ugo_fecconn_set_batch": "vp i vp sz *i *sz -> i",
    "ugo_fecconn_set_batch_ex": "vp i u vp sz *i *sz -> i",
    "ugo_fecconn_flush": "vp vp sz *i *sz -> i",
    "ugo_fecconn_pending": "vp *sz -> i",
    "ugo_fecconn_service": "vp i -> i",
    "ugo_fecconn_rx_len": "vp *sz -> i",
    # ugo_pkt.h
    "ugo_fec_packet_decode": "vp vp sz vp sz vp u vp vp sz vp sz vp -> i",
    "ugo_fec_packet_encode": "vp vp vp sz vp sz vp sz sz vp u vp sz vp vp vp -> i",
    # ugo_stream.h
    "ugo_fec_stream_rx_create": "vp sz *vp -> i",
    "ugo_fec_stream_rx_destroy": "vp -> None",
    "ugo_fec_stream_deliver": "vp vp sz vp vp vp sz sz vp vp -> i",
    "ugo_fec_stream_read": "vp vp sz vp vp vp -> i",
    "ugo_fec_stream_rx_state": "vp vp -> i",
    "ugo_fec_stream_rx_window": "vp *vp *sz -> i",
    "ugo_fec_stream_set_create": "vp vp sz *vp -> i",
    "ugo_fec_stream_set_destroy": "vp -> None",
    "ugo_fec_stream_set_deliver": "vp vp sz vp vp vp sz sz vp vp vp -> i",
    "ugo_fec_stream_set_read": "vp vp vp vp vp vp vp -> i",
    "ugo_fec_stream_set_state": "vp vp -> i",
    "ugo_fec_stream_tx_create": "vp sz sz sz sz *vp -> i",
    "ugo_fec_stream_tx_destroy": "vp -> None",
    "ugo_fec_stream_tx_window": "vp *vp *sz -> i",
    "ugo_fec_stream_tx_queue": "vp *vp *sz -> i",
    "ugo_fec_stream_tx_set_create": "vp vp sz *vp -> i",
    "ugo_fec_stream_tx_set_destroy": "vp -> None",
    "ugo_fec_stream_tx_set_write": "vp vp vp vp vp vp -> i",
    "ugo_fec_stream_tx_set_release": "vp vp vp -> i",
    "ugo_fec_stream_tx_set_retransmit": "vp vp vp vp sz vp vp -> i",
    "ugo_fec_stream_tx_set_plan": "vp vp sz sz sz vp vp vp vp vp vp vp -> i",
    "ugo_fec_stream_tx_set_encode": "vp vp vp sz vp sz vp sz vp u vp sz vp vp vp -> i",
    "ugo_fec_stream_tx_set_state": "vp vp -> i",
    # ugo_ack.h
    "ugo_fec_ack_rx_create": "vp sz *vp -> i",
    "ugo_fec_ack_rx_destroy": "vp -> None",
    "ugo_fec_ack_rx_state": "vp vp -> i",
    "ugo_fec_ack_rx_bitmap": "vp *vp *sz -> i",
    "ugo_fec_ack_set_create": "vp vp sz *vp -> i",
    "ugo_fec_ack_set_destroy": "vp -> None",
    "ugo_fec_ack_set_receive": "vp vp vp sz vp sz sz vp -> i",
    "ugo_fec_ack_set_touch": "vp vp vp -> i",
    "ugo_fec_ack_set_attach": "vp sz vp vp vp vp sz vp vp sz vp vp vp vp -> i",
    "ugo_fec_ack_set_state": "vp vp -> i",
    # ugo_sent.h
    "ugo_fec_sent_tx_create": "vp sz sz *vp -> i",
    "ugo_fec_sent_tx_destroy": "vp -> None",
    "ugo_fec_sent_tx_slots": "vp *vp *sz -> i",
    "ugo_fec_sent_tx_segments": "vp *vp *sz *sz -> i",
    "ugo_fec_sent_tx_scratch": "vp *vp *sz -> i",
    "ugo_fec_sent_set_create": "vp vp sz *vp -> i",
    "ugo_fec_sent_set_destroy": "vp -> None",
    "ugo_fec_sent_set_record": "vp vp vp sz vp vp vp sz sz vp -> i",
    "ugo_fec_sent_set_ack": "vp vp vp sz vp sz sz vp vp -> i",
    "ugo_fec_sent_set_rto": "vp vp sz vp vp -> i",
    "ugo_fec_sent_set_drain": "vp sz vp vp vp vp vp vp vp -> i",
    "ugo_fec_sent_set_attach": "vp vp vp sz vp vp vp -> i",
    "ugo_fec_sent_set_state": "vp vp -> i",
    # ugo_cc.h
    "ugo_fec_cc_set_create": "vp vp vp *vp -> i",
    "ugo_fec_cc_set_destroy": "vp -> None",
    "ugo_fec_cc_set_cutback": "vp *vp -> i",
    "ugo_fec_cc_sent_ack": "vp vp vp sz vp sz sz vp vp vp vp -> i",
    "ugo_fec_cc_set_ack": "vp vp vp sz vp vp -> i",
    "ugo_fec_cc_set_rto": "vp vp sz sz vp vp -> i",
    "ugo_fec_cc_set_state": "vp vp -> i",
    # ugo_listen.h
    "ugo_fec_listen_create": "vp sz *vp -> i",
    "ugo_fec_listen_destroy": "vp -> None",
    "ugo_fec_listen_state": "vp vp -> i",
    "ugo_fec_listen_route": "vp vp vp sz vp sz vp vp vp sz vp vp -> i",
    "ugo_fec_listen_remap": "vp vp sz sz vp vp -> i",
    "ugo_fec_listen_names": "vp vp sz vp vp vp -> i",
    "ugo_fec_listen_entries": "vp vp sz vp -> i",
    # ugo_loop.h
    "ugo_fec_loop_set_create": "vp vp vp vp vp vp sz *vp -> i",
    "ugo_fec_loop_set_destroy": "vp -> None",
    "ugo_fec_loop_set_receive": "vp vp vp sz sz vp -> i",
    "ugo_fec_loop_set_close": "vp vp vp sz vp -> i",
    "ugo_fec_loop_set_check": "vp sz vp vp vp -> i",
    "ugo_fec_loop_set_append": "vp vp sz vp vp sz vp vp vp vp -> i",
    "ugo_fec_loop_set_sent": "vp vp vp vp sz vp vp vp sz vp vp vp vp -> i",
    "ugo_fec_loop_set_state": "vp vp -> i",
}

# name -> (item size, [(field, format[, shape]) ...]) with u1 for |u1 and the little-endian mark left out
DTYPES = {
    "ACK_STATE_DTYPE": (64, "largest_in_order:u8 largest_observed:u8 ignore_below:u8 lo_time_us:u8 fresh:u8 old:u8 "
                            "out_of_window:u8 outstanding:u4 changed:u1 err:u1 reserved:u1*2"),
    "CC_PARAMS_DTYPE": (20, "initial_cwnd:u4 max_cwnd:u4 min_cwnd:u4 num_connections:u4 mss:u4"),
    "CC_ROW_DTYPE": (32, "max_lost:u8 max_acked:u8 acked_le:u4 reserved:u1*12"),
    "CC_STATE_DTYPE": (192, "cwnd:u8 ssthresh:u8 largest_acked:u8 cutback:u8 min_rtt_us:u8 latest_rtt_us:u8 srtt_us:u8 "
                            "mean_dev_us:u8 end_packet_number:u8 current_min_rtt_us:u8 epoch_us:u8 app_limited_us:u8 "
                            "last_update_us:u8 last_cwnd:u8 last_max_cwnd:u8 est_tcp_cwnd:u8 origin_cwnd:u8 "
                            "last_target_cwnd:u8 rto_candidate:u8 cutbacks:u8 rtos:u8 sample_count:u4 acked_count:u4 "
                            "time_to_origin:u4 last_cutback_exited_slowstart:u1 started:u1 found:u1 reserved:u1*9"),
    "LAUNCH_TIME_DTYPE": (8, "kernel:u4 ms:f4"),
    "LISTEN_ACCEPT_DTYPE": (48, "packet:u4 member:u4 client_id:u4 reserved:u4 name:u1*32"),
    "LISTEN_ENTRY_DTYPE": (32, "ip:u1*16 scope:u4 port:u4 member:u4 reserved:u4"),
    "LISTEN_STATE_DTYPE": (80, "nconn:u4 n_dead:u4 n_slots:u4 err:u4 counts:u8*8"),
    "LOOP_PARAMS_DTYPE": (24, "ack_delay_us:u8 idle_us:u8 max_retries:u4 reserved:u4"),
    "LOOP_STATE_DTYPE": (64, "last_activity_us:u8 origin_ack_us:u8 linger_deadline_us:u8 exit_us:u8 dropped:u8 "
                             "closed:u1 fin_sent:u1 fin_rcvd:u1 ack_no_delay:u1 exited:u1 reason:u1 pending:u1 "
                             "reported:u1 reserved:u1*16"),
    "PKT_INFO_DTYPE": (64, "packet_number:u8 stop_waiting:u8 largest_acked:u8 largest_in_order:u8 delay_us:u8 "
                           "status:u4 payload_off:u4 n_ranges:u2 n_segments:u2 flags:u1 fec_flag_lo:u1 reserved:u1*10"),
    "PKT_SEGMENT_DTYPE": (16, "offset:u8 data_off:u4 len:u2 avail:u2"),
    "SENT_EVENT_DTYPE": (64, "rtt_us:u8 delay_us:u8 acked_bytes:u8 lost_bytes:u8 bytes_in_flight:u8 largest_acked:u8 "
                             "acked_packets:u4 lost_packets:u4 accepted:u1 has_rtt:u1 reserved:u1*6"),
    "SENT_SEG_DTYPE": (16, "offset:u8 len:u4 reserved:u4"),
    "SENT_SLOT_DTYPE": (32, "packet_number:u8 sent_us:u8 min_offset:u8 len:u4 state:u1 missing:u1 n_segments:u1 "
                            "bits:u1"),
    "SENT_STATE_DTYPE": (160, "last_sent:u8 lio:u8 largest_acked:u8 largest_with_ack:u8 least_unacked:u8 "
                              "bytes_in_flight:u8 last_sent_us:u8 scan_from:u8 acked_packets:u8 acked_bytes:u8 "
                              "lost_packets:u8 lost_bytes:u8 duplicates:u8 unsent_acks:u8 stale:u8 tracked:u4 "
                              "queued:u4 queued_segments:u4 rto_count:u4 sw_pending:u1 err:u1 reserved:u1*22"),
    "STREAM_STATE_DTYPE": (96, "read_pos:u8 head_off:u8 hi:u8 readable:u8 accepted:u8 duplicate:u8 out_of_window:u8 "
                               "skipped_packets:u8 ordered_segments:u8 err_packet:u8 err_segment:u4 err:u4 ngaps:u4 "
                               "head_valid:u1 eof:u1 reserved:u1*2"),
    "STREAM_TX_RQ_DTYPE": (16, "offset:u8 len:u4 reserved:u4"),
    "STREAM_TX_STATE_DTYPE": (80, "base:u8 write_pos:u8 tail:u8 last_packet_number:u8 packets:u8 segments:u8 "
                                  "bytes_new:u8 bytes_retransmitted:u8 rq_rejected:u8 rq_len:u4 rq_head:u4"),
}

CONSTANTS = dict(
    ACK_ATTACHED=1, ACK_MAX_OUTSTANDING=1000, ACK_MAX_WINDOW=1048576, ACK_MIN_WINDOW=1024, ACK_NOT_ATTACHED=0,
    ACK_TOO_MANY_OUTSTANDING=1, ACK_TRUNCATED=2, CC_MAX_CWND_LIMIT=1048576, LISTEN_ACCEPT=3, LISTEN_BAD_NAME=6,
    LISTEN_DUP_INIT=2, LISTEN_FED=0, LISTEN_FED_NEW=1, LISTEN_FULL=1, LISTEN_MAX_CONN=1048576, LISTEN_NAME_BYTES=32,
    LISTEN_NCLASS=8, LISTEN_REFUSED=5, LISTEN_REMAP_LENGTH=8, LISTEN_REMAP_NOT_INJECTIVE=1,
    LISTEN_REMAP_OUT_OF_RANGE=2, LISTEN_REMAP_TOO_MANY=4, LISTEN_STRANGER=4, LOOP_ABORT=11, LOOP_ACK_ERR=7,
    LOOP_BAD_PACKET=3, LOOP_CLOSED=4, LOOP_FAILURES=5, LOOP_HOW_ABORT=2, LOOP_HOW_CLOSE=1, LOOP_HOW_NODELAY_OFF=8,
    LOOP_HOW_NODELAY_ON=4, LOOP_IDLE=9, LOOP_LINGER=10, LOOP_PEER_ACK_FIN=1, LOOP_PEER_RST=2, LOOP_PENDING_FIN=1,
    LOOP_PENDING_NONE=0, LOOP_PENDING_RST=2, LOOP_SENT_ERR=6, LOOP_STREAM_ERR=8, OK=0, PKT_CAPACITY=6,
    PKT_FEC_FRAMED=1, PKT_INCONSISTENT_LARGEST_ACKED=7, PKT_INCONSISTENT_LOWEST_ACKED=8,
    PKT_INCONSISTENT_RANGE_COUNT=9, PKT_OUT_OF_WINDOW=10, RECONSTRUCT_DATA_ONLY=1, SENT_IN_FLIGHT=0,
    SENT_MAX_SEG_CAP=16, SENT_MAX_WINDOW=1048576, SENT_MIN_WINDOW=1024, SENT_QUEUED=1, SENT_RTO_DEFAULT_US=500000,
    SENT_RTO_MAX_US=60000000, SENT_RTO_MIN_US=200000, SENT_TOO_MANY_TRACKED=1, STREAM_ACCEPTED=1, STREAM_DUPLICATE=2,
    STREAM_MAX_GAPS=50, STREAM_MIN_WINDOW=4096, STREAM_NONE=0, STREAM_NO_CONN=4294967295, STREAM_OUT_OF_WINDOW=3,
    STREAM_OVERLAP=4, STREAM_SET_MAX_CONN=1048576, STREAM_TOO_MANY_GAPS=5, STREAM_TX_HEADER=4,
    STREAM_TX_MAX_WINDOW=2147483648, STREAM_TX_RQ_FULL=3, STREAM_TX_RQ_QUEUED=1, STREAM_TX_RQ_REJECTED=2,
    STREAM_TX_RQ_UNSORTED=4, UGO_FEC_MAX_PACKET=1476)


def test_every_name_is_still_there():
    missing = [n for n in NAMES if not hasattr(fec, n)]
    assert not missing, missing


def test_a_replaced_load_library_reaches_the_binding(monkeypatch):
    """What tests/test_stream_order.py's census and tests/test_abi.py rely on: fec is one namespace."""
    lib, seen = fec.load_library(), []
    assert fec._lib is lib

    class Proxy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(fec, "load_library", lambda path=None: Proxy())
    assert fec.strerror(3) == "too few shards given" and len(fec.rc4_keystream(b"key", 4)) == 4
    monkeypatch.undo()
    assert seen == ["ugo_fec_strerror", "ugo_fec_rc4_keystream"]
    assert fec.strerror(3) == "too few shards given" and len(seen) == 2 and fec.load_library() is lib


def _type_name(t):
    return _SHORT[type(None).__name__ if t is None else t.__name__]


def test_argument_types_of_every_header_symbol():
    lib = fec._bind_conn(fec.load_library())
    assert sorted(PROTOTYPES) == fec.header_symbols()
    got = {}
    for s in PROTOTYPES:
        fn = getattr(lib, s)
        args = "-" if fn.argtypes is None else " ".join(_type_name(t) for t in fn.argtypes)
        got[s] = f"{args} -> {_type_name(fn.restype)}"
    assert got == PROTOTYPES


def _fields(dt):
    out = []
    for f in dt.descr:
        name, fmt = f[0], f[1].lstrip("<|")
        out.append(f"{name}:{fmt}" + (f"*{f[2][0]}" if len(f) == 3 else ""))
    return " ".join(out)


def test_dtypes_and_constants():
    names = [n for n in NAMES if n.endswith("_DTYPE")]
    assert sorted(names) == sorted(DTYPES)
    assert {n: (getattr(fec, n).itemsize, _fields(getattr(fec, n))) for n in names} == DTYPES
    ints = {n: getattr(fec, n) for n in NAMES if n.isupper() and type(getattr(fec, n)) is int}
    assert ints == CONSTANTS
    assert fec.CC_DEFAULTS == dict(initial_cwnd=32, max_cwnd=200, min_cwnd=2, num_connections=2, mss=1460)
    assert fec.LOOP_DEFAULTS == dict(ack_delay_us=5000, idle_us=300000000, max_retries=10)
    assert fec.KERNEL_IDS == {v: k for k, v in fec.KERNEL_NAMES.items()} and len(fec.KERNEL_NAMES) == 16
    assert fec._ERRORS == {c.code: c for c in (fec.ErrInvShardNum, fec.ErrMaxShardNum, fec.ErrTooFewShards,
                                               fec.ErrShardNoData, fec.ErrShardSize, fec.ErrInvalidArg,
                                               fec.ErrSingular, fec.ErrHip, fec.ErrNoDevice)}
    assert fec.np is np and fec.torch is torch and fec.ctypes is ctypes


def test_static_checks_on_the_class():
    fec.StreamRx.check_window(4096)
    fec.StreamRx.check_batch(1488, 4096, 256)
    fec.StreamTx.check_create(1 << 31, 1)
    fec.StreamTxSet.check_plan(1436, 8, 0)
    fec.AckRx.check_window(1024)
    fec.SentTx.check_create(1024, 16)
    fec.StreamRxSet.check_conn_of(torch.zeros(5, dtype=torch.int32), 5)
    assert fec.CcSet.check_params() == fec.CC_DEFAULTS and fec.CcSet.check_params(mss=9)["mss"] == 9
    assert fec.LoopSet.check_params() == fec.LOOP_DEFAULTS and fec.LoopSet.check_params(idle_us=1)["idle_us"] == 1
    for bad in (lambda: fec.StreamRx.check_window(4097), lambda: fec.StreamRx.check_batch(1480, 4096, None),
                lambda: fec.StreamRx.check_batch(1488, 4096, 8), lambda: fec.StreamTx.check_create(4096, 0),
                lambda: fec.StreamTxSet.check_plan(15, 8, 0), lambda: fec.AckRx.check_window(512),
                lambda: fec.SentTx.check_create(1024, 17), lambda: fec.CcSet.check_params(mss=0),
                lambda: fec.CcSet.check_params(pace=1), lambda: fec.LoopSet.check_params(idle_us=0),
                lambda: fec.StreamRxSet.check_conn_of(torch.zeros(5, dtype=torch.float32), 5),
                lambda: fec.StreamRxSet.check_conn_of(torch.zeros(4, dtype=torch.int32), 5)):
        with pytest.raises(ValueError):
            bad()
    for kind, noun in ((fec.StreamRxSet, "windows"), (fec.StreamTxSet, "windows"), (fec.AckRxSet, "histories"),
                       (fec.SentTxSet, "histories")):
        with pytest.raises(ValueError, match=f"a set holds 1 to {fec.STREAM_SET_MAX_CONN} {noun}"):
            kind.check_members(None, [])
        with pytest.raises(ValueError, match=f"members must be open {kind.__name__[:-3]}"):
            kind.check_members(None, [object()])


# ------------------------------------------------------------------ GPU part
# The smallest configuration in which every check has something to refuse: C members per family, N packets,
# S segments and R ranges a packet, SLOT bytes a slot, M retransmissions.
C, N, S, R, SLOT, M = 2, 4, 1, 2, 64, 2
U8, I16, I32, I64 = torch.uint8, torch.int16, torch.int32, torch.int64
WIDER = {U8: I16, I16: I32, I32: I64, I64: I32}     # the element width off by a factor of two
FLOAT = {U8: torch.float8_e5m2, I16: torch.float16, I32: torch.float32, I64: torch.float64}
WAYS = ("width", "short", "strided", "row", "float")

INFO, SEGS, RANGES, CONN = (U8, N, 64), (U8, N, S, 16), (I64, N, R, 2), (I32, N)
EVENTS, ROWS = (U8, C, 64), (U8, C, 32)


def per(dtype):
    return (dtype, C)


# (object, method, operands): an operand is (dtype, *shape), a tuple of them under `out`, or a plain value.
CALLS = (
    ("StreamRxSet", "deliver", dict(pkts=(U8, N, SLOT), info=INFO, segs=SEGS, conn_of=CONN, pad=(U8, SLOT),
                                    out=(U8, N, S))),
    ("StreamRxSet", "read", dict(n=per(I64), dst=(U8, 256), dst_off=per(I64), n_read=per(I64), eof=per(U8))),
    ("StreamTxSet", "write", dict(src=(U8, 256), src_off=per(I64), n=per(I64), n_written=per(I64))),
    ("StreamTxSet", "release", dict(upto=per(I64))),
    ("StreamTxSet", "retransmit", dict(conn_of=(I32, M), offset=(I64, M), length=(I32, M), status=(U8, M))),
    ("StreamTxSet", "plan", dict(budget=per(I32), max_packets=N, max_payload=1436, max_segments=S,
                                 out=dict(info=INFO, segs=SEGS, conn_of=CONN, first_packet=per(I64),
                                          n_packets=per(I32), total=(I64, 1)))),
    ("StreamTxSet", "encode", dict(info=INFO, ranges=RANGES, segs=SEGS, conn_of=CONN, slot=SLOT, npackets=N,
                                   pad=(U8, SLOT), out=dict(wire=(U8, N, SLOT), wire_lens=(I16, N), status=(U8, N)))),
    ("AckRxSet", "receive", dict(info=INFO, conn_of=CONN, now_us=1, seg_status=(U8, N, S), npackets=N)),
    ("AckRxSet", "touch", dict(flags=per(U8))),
    ("AckRxSet", "attach", dict(now_us=1, first_packet=per(I64), n_packets=per(I32), total=(I64, 1), info=INFO,
                                ranges=RANGES, conn_of=CONN, may_ack_only=per(U8), total_out=(I64, 1),
                                attached=per(U8))),
    ("SentTxSet", "record", dict(info=INFO, segs=SEGS, conn_of=CONN, wire_lens=(I16, N), status=(U8, N), now_us=1,
                                 npackets=N)),
    ("SentTxSet", "ack", dict(info=INFO, ranges=RANGES, conn_of=CONN, now_us=1, npackets=N, events=EVENTS)),
    ("SentTxSet", "rto", dict(delay_us=per(I64), now_us=1, fired=per(U8))),
    ("SentTxSet", "drain", dict(max_entries=N, out=dict(conn_of=CONN, offset=(I64, N), len=(I32, N),
                                                        n_entries=(I64, 1), touch=per(U8), upto=per(I64)))),
    ("SentTxSet", "attach", dict(first_packet=per(I64), n_packets=per(I32), info=INFO, attached=per(U8))),
    ("CcSet", "sent_ack", dict(info=INFO, ranges=RANGES, conn_of=CONN, now_us=1, npackets=N, events=EVENTS,
                               split=per(I64), rows=ROWS)),
    ("CcSet", "ack", dict(events=EVENTS, rows=ROWS, now_us=1, delay_us=per(I64))),
    ("CcSet", "rto", dict(fired=per(U8), packet_bytes=1460, max_budget=8, budget=per(I32))),
    ("ListenTable", "route", dict(names=(U8, N, 32), pkts=(U8, N, SLOT), lens=(I16, N), npackets=N, conn_of=CONN,
                                  cls=(U8, N), accepted=(U8, C, 48), n_accepted=(I32, 1))),
    ("ListenTable", "remap", dict(new_index=per(I32), nconn_new=C, status=(I32, 1))),
    ("ListenTable", "names", dict(conn_of=CONN, npackets=N, names_out=(U8, N, 32), name_lens=(I32, N))),
    ("ListenTable", "entries", dict(out=(U8, C, 32))),
    ("LoopSet", "receive", dict(info=INFO, conn_of=CONN, now_us=1, npackets=N)),
    ("LoopSet", "close_members", dict(how=per(U8), now_us=1, linger_us=per(I64))),
    ("LoopSet", "check", dict(now_us=1, budget=per(I32), may_ack_only=per(U8))),
    ("LoopSet", "append", dict(total=(I64, 1), info=INFO, segs=SEGS, conn_of=CONN, total_out=(I64, 1),
                               appended=per(U8), max_packets=N)),
    ("LoopSet", "sent", dict(n_packets=per(I32), attached=per(U8), now_us=1, delay_us=per(I64), max_exits=C,
                             out=dict(deadline_us=(I64, 1), exits=(I32, C), reasons=(U8, C), n_exits=(I64, 1),
                                      new_index=per(I32), nconn_new=(I64, 1)))),
)

# The rows the binding accepts: the call goes through to the library with the operand as described and
# everything else valid.  Every other row of rows() is refused with ValueError before the library is called.
# Among them the asymmetries between the families: the loop and the listen table take a floating-point tensor
# of the right width where the stream, ack and sent families refuse it; the list that is too long is a test
# of its own below.
ACCEPTED = frozenset("""
StreamRxSet.deliver:pkts:float StreamRxSet.deliver:info:float StreamRxSet.deliver:segs:float
StreamRxSet.deliver:pad:float StreamRxSet.deliver:out:float StreamRxSet.read:dst:short StreamRxSet.read:dst:float
StreamTxSet.write:src:short StreamTxSet.write:src:float StreamTxSet.plan:out.info:float
StreamTxSet.plan:out.segs:float StreamTxSet.encode:info:float StreamTxSet.encode:ranges:float
StreamTxSet.encode:segs:float StreamTxSet.encode:pad:float StreamTxSet.encode:out.wire:float
StreamTxSet.encode:out.wire_lens:float StreamTxSet.encode:out.status:float
AckRxSet.receive:info:float AckRxSet.receive:seg_status:float AckRxSet.attach:total:float AckRxSet.attach:info:float
AckRxSet.attach:ranges:float AckRxSet.attach:total_out:float
SentTxSet.record:info:float SentTxSet.record:segs:float SentTxSet.ack:info:float SentTxSet.ack:ranges:float
SentTxSet.ack:events:float SentTxSet.drain:out.n_entries:float SentTxSet.attach:info:short SentTxSet.attach:info:float
CcSet.sent_ack:info:float CcSet.sent_ack:ranges:float CcSet.sent_ack:events:float CcSet.sent_ack:rows:float
CcSet.ack:events:float CcSet.ack:rows:float
ListenTable.route:names:float ListenTable.route:pkts:float ListenTable.route:lens:float
ListenTable.route:conn_of:float ListenTable.route:cls:float ListenTable.route:accepted:short
ListenTable.route:accepted:float ListenTable.route:n_accepted:float ListenTable.remap:new_index:short
ListenTable.remap:new_index:float ListenTable.remap:status:float ListenTable.names:conn_of:float
ListenTable.names:names_out:float ListenTable.names:name_lens:float ListenTable.entries:out:short
LoopSet.receive:info:float LoopSet.receive:conn_of:float LoopSet.close_members:how:float
LoopSet.close_members:linger_us:float LoopSet.check:budget:float LoopSet.check:may_ack_only:float
LoopSet.append:total:float LoopSet.append:info:float LoopSet.append:segs:float LoopSet.append:conn_of:float
LoopSet.append:total_out:float LoopSet.append:appended:float LoopSet.sent:n_packets:float
LoopSet.sent:attached:float LoopSet.sent:delay_us:float LoopSet.sent:out.deadline_us:float
LoopSet.sent:out.exits:float LoopSet.sent:out.reasons:float LoopSet.sent:out.n_exits:float
LoopSet.sent:out.new_index:float LoopSet.sent:out.nconn_new:float
""".split())
N_ROWS = 477
# Left out, both accepted: route takes packet rows of any width, and 63-byte rows are not clearly safe to hand
# to the kernel; the table takes a one-byte floating-point `out`, and entries() then fails turning it into numpy
# rows, after the library call.
OMITTED = frozenset(["ListenTable.route:pkts:row", "ListenTable.entries:out:float"])
# What a refusal says, one row for every form of message the checks have.
LAYOUT = "argument does not match the batch layout the entry point expects"
MESSAGES = {
    "StreamRxSet.read:n:width": "n must be nconn contiguous 64-bit integers",
    "StreamRxSet.deliver:conn_of:short": "conn_of must be npackets contiguous 32-bit integers",
    "StreamRxSet.deliver:info:row": LAYOUT,
    "StreamTxSet.retransmit:offset:short": "offset must be 2 contiguous 64-bit integers",
    "StreamTxSet.plan:out.total:float": "total must be 1 contiguous 64-bit integers",
    "StreamTxSet.plan:out.segs:row": LAYOUT,
    "StreamTxSet.encode:conn_of:float": LAYOUT,
    "AckRxSet.receive:conn_of:short": "conn_of must be npackets contiguous 32-bit integers",
    "AckRxSet.attach:ranges:row": LAYOUT,
    "SentTxSet.record:wire_lens:short": "wire_lens must be contiguous 16-bit integers",
    "SentTxSet.record:segs:row": "segs must be [npackets, max_segments, 16] with max_segments at most the smallest "
                                 "seg_cap",
    "SentTxSet.drain:out.len:width": "len must be contiguous 32-bit integers",
    "CcSet.rto:budget:float": "budget must be nconn contiguous 32-bit integers",
    "CcSet.ack:rows:row": LAYOUT,
    "ListenTable.names:name_lens:short": "name_lens must be contiguous, 4-byte, at least (4,)",
    "ListenTable.route:names:row": "names must be contiguous, 1-byte, at least (4, 32)",
    "LoopSet.check:budget:short": "budget must be contiguous, 4-byte, [nconn]",
    "LoopSet.receive:info:row": "info must be contiguous, 1-byte, at least (4, 64)",
    "LoopSet.append:segs:row": "segs must be uint8 [max_packets, S, 16]",
    "LoopSet.sent:out.exits:strided": "exits must be contiguous, 4-byte, at least (2,)",
}


def _is_spec(v):
    return isinstance(v, tuple) and isinstance(v[0], torch.dtype)


def wrong(spec, way, device):
    """The operand wrong in one way, or None where that way does not apply to it."""
    dtype, shape = spec[0], tuple(spec[1:])
    if way == "width":
        return torch.zeros(shape, dtype=WIDER[dtype], device=device)
    if way == "short":
        return torch.zeros((shape[0] - 1,) + shape[1:], dtype=dtype, device=device)
    if way == "strided":  # a tensor of one element is contiguous however it is cut
        big = torch.zeros((2 * shape[0],) + shape[1:], dtype=dtype, device=device)
        return big[::2] if int(np.prod(shape)) > 1 else None
    if way == "row":
        if len(shape) < 2:
            return None
        last = 3 if shape[-1] == 2 else shape[-1] - 1  # 63 for 64, 15 for 16, 3 for the pairs of ranges
        return torch.zeros(shape[:-1] + (last,), dtype=dtype, device=device)
    return torch.zeros(shape, dtype=FLOAT[dtype], device=device)


def rows():
    """(id, object, method, operand path, way) for every operand of CALLS and every way it can be wrong."""
    out = []
    for obj, method, operands in CALLS:
        for name, v in operands.items():
            paths = [(name,)] if _is_spec(v) else [(name, k) for k in v] if isinstance(v, dict) else []
            for path in paths:
                spec = v if len(path) == 1 else v[path[1]]
                for way in WAYS:
                    rid = f"{obj}.{method}:{'.'.join(path)}:{way}"
                    if wrong(spec, way, "cpu") is not None and rid not in OMITTED:
                        out.append((rid, obj, method, path, way))
    return out


def call(objs, obj, method, path, way, device):
    """Run one row: every operand valid and zero but the one at `path`."""
    operands = dict(next(o for k, m, o in CALLS if (k, m) == (obj, method)))
    kw = {}
    for name, v in operands.items():
        if _is_spec(v):
            kw[name] = wrong(v, way, device) if path == (name,) else torch.zeros(v[1:], dtype=v[0], device=device)
        elif isinstance(v, dict):
            kw[name] = tuple(wrong(s, way, device) if path == (name, k) else
                             torch.zeros(s[1:], dtype=s[0], device=device) for k, s in v.items())
        else:
            kw[name] = v
    return getattr(objs[obj], method)(**kw)


ROWS_ = rows()


def test_the_refusal_table_is_whole():
    """The table has a row for every operand and way, and the recorded asymmetries are in it."""
    ids = {r[0] for r in ROWS_}
    assert len(ROWS_) == len(ids) == N_ROWS and ACCEPTED <= ids
    assert {"LoopSet.check:budget:float", "ListenTable.names:conn_of:float"} <= ACCEPTED
    assert "StreamTxSet.plan:budget:float" in ids - ACCEPTED and "SentTxSet.rto:delay_us:float" in ids - ACCEPTED
    assert "AckRxSet.touch:flags:float" in ids - ACCEPTED and set(MESSAGES) <= ids - ACCEPTED


@pytest.fixture(scope="module")
def objs(gpu):
    enc = fec.New(10, 3)
    members = dict(srx=[fec.StreamRx(enc, 4096) for _ in range(C)],
                   stx=[fec.StreamTx(enc, 4096, rq_cap=1) for _ in range(C)],
                   arx=[fec.AckRx(enc, 1024) for _ in range(C)],
                   sent=[fec.SentTx(enc, 1024, seg_cap=1) for _ in range(C)])
    o = dict(StreamRxSet=fec.StreamRxSet(enc, members["srx"]), StreamTxSet=fec.StreamTxSet(enc, members["stx"]),
             AckRxSet=fec.AckRxSet(enc, members["arx"]), SentTxSet=fec.SentTxSet(enc, members["sent"]))
    o["CcSet"] = fec.CcSet(enc, o["SentTxSet"])
    o["LoopSet"] = fec.LoopSet(enc, o["StreamRxSet"], o["AckRxSet"], o["StreamTxSet"], o["SentTxSet"])
    o["ListenTable"] = fec.ListenTable(enc, C)
    yield o
    torch.cuda.synchronize()
    for k in ("LoopSet", "CcSet", "ListenTable", "SentTxSet", "AckRxSet", "StreamTxSet", "StreamRxSet"):
        o[k].close()
    for m in sum(members.values(), []):
        m.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS_, ids=[r[0] for r in ROWS_])
def test_refusal(objs, row):
    rid, obj, method, path, way = row
    if rid in ACCEPTED:
        call(objs, obj, method, path, way, "cuda")
    else:
        with pytest.raises(ValueError, match=re.escape(MESSAGES[rid]) if rid in MESSAGES else None):
            call(objs, obj, method, path, way, "cuda")


@pytest.mark.gpu
def test_a_longer_list_is_refused_by_retransmit_and_taken_by_record(objs):
    """Exactly m against at least n: the one list length on which two families differ."""
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match="offset must be 2 contiguous 64-bit integers"):
        objs["StreamTxSet"].retransmit(z(M, I32), z(M + 1, I64), z(M, I32), z(M, U8))
    objs["SentTxSet"].record(z((N, 64), U8), z((N, S, 16), U8), z(N + 1, I32), z(N + 1, I16), z(N + 1, U8), 1,
                             npackets=N)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_every_valid_call_goes_through(objs):
    """The rows' common ground: with no operand wrong every call of CALLS is accepted, and the views are tensors
    over the library's memory."""
    for obj, method, _ in CALLS:
        call(objs, obj, method, (), None, "cuda")
    torch.cuda.synchronize()
    assert objs["CcSet"].cutback().shape == (C,) and objs["CcSet"].cutback().dtype == I64
    for k in ("StreamRxSet", "StreamTxSet", "AckRxSet", "SentTxSet", "CcSet", "LoopSet"):
        assert objs[k].states().shape == (C,)
    assert int(objs["ListenTable"].state()["nconn"]) == 0


@pytest.mark.gpu
def test_life_cycle(gpu):
    """close() twice is a no-op on the thirteen classes; a SentTx closes the sets it is in and a SentTxSet its
    CcSets; a closed member is refused by check_members."""
    enc = fec.New(10, 3)
    srx, stx, arx = fec.StreamRx(enc, 4096), fec.StreamTx(enc, 4096, rq_cap=1), fec.AckRx(enc, 1024)
    sent = [fec.SentTx(enc, 1024, seg_cap=1) for _ in range(3)]
    sets = [fec.StreamRxSet(enc, [srx]), fec.StreamTxSet(enc, [stx]), fec.AckRxSet(enc, [arx]),
            fec.SentTxSet(enc, sent[:1])]
    assert [s.nconn for s in sets] == [1, 1, 1, 1] and sets[3].min_seg_cap == 1 and sets[0].rxs == [srx]
    assert sets[1].txs == [stx] and sets[2].rxs == [arx] and sets[3].txs == sent[:1]
    assert all(s._enc is enc and s.device == enc.device for s in sets)
    four = (sets[0], sets[2], sets[1], sets[3])
    cc, loop, table = fec.CcSet(enc, sets[3]), fec.LoopSet(enc, *four), fec.ListenTable(enc, C)
    assert cc.sent is sets[3] and loop.sets == four and table.max_conn == C
    assert cc.nconn == loop.nconn == 1 and cc.params == fec.CC_DEFAULTS and loop.params == fec.LOOP_DEFAULTS
    conn = fec.FecConn(128, 10, 3)
    for o in [loop, cc, table] + sets + [srx, stx, arx, sent[0], conn]:
        assert o._h
        o.close()
        assert o._h is None
        o.close()
        assert o._h is None
    for kind, member in ((fec.StreamRxSet, srx), (fec.StreamTxSet, stx), (fec.AckRxSet, arx), (fec.SentTxSet, sent[0])):
        with pytest.raises(ValueError, match="members must be open"):
            kind.check_members(enc, [member])
    # the dependants of the sent family go first
    both, one = fec.SentTxSet(enc, sent[1:]), fec.SentTxSet(enc, sent[2:])
    cc_both, cc_one = fec.CcSet(enc, both), fec.CcSet(enc, one)
    sent[1].close()
    assert both._h is None and cc_both._h is None and sent[1]._h is None
    assert one._h and cc_one._h and sent[2]._h
    one.close()
    assert one._h is None and cc_one._h is None and sent[2]._h
    sent[2].close()
    enc.close()
    assert enc._h is None
    enc.close()
    assert enc._h is None
