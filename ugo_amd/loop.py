"""include/ugo_loop.h: the connection loop of a set of connections."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from .abi import _check_segs, _check_tensor, _Handle, _raise, _require, _stream_handle, load_library, torch
from .ack import AckRxSet
from .encoder import Encoder
from .sent import SentTxSet
from .stream import StreamRxSet, StreamTxSet

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


class LoopSet(_Handle):
    """The connection loop of a set of connections (include/ugo_loop.h): the
    timers, FIN / RST and the exits, one record per member of a StreamRxSet, an
    AckRxSet, a StreamTxSet and a SentTxSet of the same size.  Per batch:
    receive after packet_decode, check before StreamTxSet.plan, append after it,
    sent after StreamTxSet.encode; close between batches.  Operands are tensors
    in device or pinned host memory; nothing is synchronised but states().
    Close it before the four sets.

    Kept: operands are checked by shape, a list may be longer than its count, and a
    float tensor of the right width is taken; the four sets count elements and refuse it."""

    _destroy = "ugo_fec_loop_set_destroy"

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

    def receive(self, info, conn_of, now_us: int, npackets: Optional[int] = None, stream=None):
        """ugo_fec_loop_set_receive: info uint8 [npackets, 64] as packet_decode
        wrote it, conn_of int32 [npackets], masked in place.  Returns conn_of."""
        npk = info.shape[0] if npackets is None else npackets
        _require(0 <= npk <= 1 << 31 and 0 <= now_us < 1 << 64)
        _check_tensor(info, npk, 1, "info", at_least=True, row=(64,))
        _check_tensor(conn_of, npk, 4, "conn_of", at_least=True, row=())
        _raise(load_library().ugo_fec_loop_set_receive(self._h, info.data_ptr() if npk else None,
                                                       conn_of.data_ptr() if npk else None, npk, now_us,
                                                       _stream_handle(stream)))
        return conn_of

    def close_members(self, how, now_us: int, linger_us=None, stream=None):
        """ugo_fec_loop_set_close: how uint8 [nconn] of LOOP_HOW_* bits,
        linger_us int64 [nconn] or None."""
        _require(0 <= now_us < 1 << 64)
        _check_tensor(how, self.nconn, 1, "how", "nconn", row=())
        if linger_us is not None:
            _check_tensor(linger_us, self.nconn, 8, "linger_us", "nconn", row=())
        _raise(load_library().ugo_fec_loop_set_close(self._h, how.data_ptr(),
                                                     None if linger_us is None else linger_us.data_ptr(), now_us,
                                                     _stream_handle(stream)))

    def check(self, now_us: int, budget, may_ack_only=None, stream=None):
        """ugo_fec_loop_set_check: budget int32 [nconn], zeroed in place where a
        member may send no data.  Returns may_ack_only uint8 [nconn]: the input
        of AckRxSet.attach."""
        _require(0 <= now_us < 1 << 64)
        _check_tensor(budget, self.nconn, 4, "budget", "nconn", row=())
        if may_ack_only is None:
            may_ack_only = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        _check_tensor(may_ack_only, self.nconn, 1, "may_ack_only", "nconn", row=())
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
        _check_tensor(total, 1, 8, "total", at_least=True, row=())
        _check_tensor(info, cap, 1, "info", at_least=True, row=(64,))
        _check_segs(segs, cap, at_least=True, max_segments=0xffff, msg="segs must be uint8 [max_packets, S, 16]")
        _check_tensor(conn_of, cap, 4, "conn_of", at_least=True, row=())
        if total_out is None:
            total_out = total
        if appended is None:
            appended = torch.zeros(self.nconn, dtype=torch.uint8, device=self._dev())
        _check_tensor(total_out, 1, 8, "total_out", at_least=True, row=())
        _check_tensor(appended, self.nconn, 1, "appended", "nconn", row=())
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
        _check_tensor(n_packets, self.nconn, 4, "n_packets", "nconn", row=())
        _check_tensor(attached, self.nconn, 1, "attached", "nconn", row=())
        if delay_us is not None:
            _check_tensor(delay_us, self.nconn, 8, "delay_us", "nconn", row=())
        dev = self._dev()
        if out is None:
            cap = self.nconn if max_exits is None else max_exits
            out = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev),
                   torch.zeros(cap, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                   torch.zeros(self.nconn, dtype=torch.int32, device=dev) if remap else None,
                   torch.zeros(1, dtype=torch.int64, device=dev) if remap else None)
        deadline, exits, reasons, n_exits, new_index, nconn_new = out
        cap = exits.shape[0] if max_exits is None else max_exits
        _check_tensor(deadline, 1, 8, "deadline_us", at_least=True, row=())
        _check_tensor(exits, cap, 4, "exits", at_least=True, row=())
        _check_tensor(reasons, cap, 1, "reasons", at_least=True, row=())
        _check_tensor(n_exits, 1, 8, "n_exits", at_least=True, row=())
        _require((new_index is None) == (nconn_new is None), "new_index and nconn_new go together")
        if new_index is not None:
            _check_tensor(new_index, self.nconn, 4, "new_index", "nconn", row=())
            _check_tensor(nconn_new, 1, 8, "nconn_new", at_least=True, row=())
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
