"""include/ugo_cc.h: congestion control, the RTT filter, hybrid slow start and
CUBIC of a SentTxSet's members."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from .abi import (_check_info, _check_ranges, _check_tensor, _Handle, _raise, _require, _stream_handle,
                  load_library, torch)
from .encoder import Encoder
from .sent import SentTxSet

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


class CcSet(_Handle):
    """The congestion controllers of a SentTxSet's members (include/ugo_cc.h):
    RTT filter, hybrid slow start and CUBIC, one record per member.  Per batch:
    sent_ack in place of SentTxSet.ack, ack, SentTxSet.rto with the delays ack
    returned, rto, and the next StreamTxSet.plan with the budget rto returned.
    Operands are tensors in device or pinned host memory; nothing is
    synchronised but states().  Close it before the SentTxSet."""

    _destroy = "ugo_fec_cc_set_destroy"

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

    def cutback(self):
        """ugo_fec_cc_set_cutback: the dense cutback array as an int64 CUDA tensor
        [nconn] over the device memory itself: what sent_ack takes as split."""
        p = ctypes.c_void_p()
        _raise(load_library().ugo_fec_cc_set_cutback(self._h, ctypes.byref(p)))
        return self._view(p.value, self.nconn * 8).view(torch.int64)

    def sent_ack(self, info, ranges, conn_of, now_us: int, npackets: Optional[int] = None, events=None, split=None,
                 rows=None, stream=None):
        """ugo_fec_cc_sent_ack: SentTxSet.ack, and rows uint8 [nconn, 32]
        (CC_ROW_DTYPE) beside events.  split int64 [nconn]; None: the set's own
        cutback array.  Returns (events, rows)."""
        sent = self.sent
        npk = info.shape[0] if npackets is None else npackets
        _check_info(info, npk, at_least=True)
        _require(0 <= npk <= 1 << 31 and 0 <= now_us < 1 << 64)
        _check_ranges(ranges, npk, at_least=True, max_ranges=0xffff)
        _check_tensor(conn_of, npk, 4, "conn_of", at_least=True, integer=True)
        if events is None:
            events = torch.zeros((self.nconn, 64), dtype=torch.uint8, device=self._dev())
        if rows is None:
            rows = torch.zeros((self.nconn, 32), dtype=torch.uint8, device=self._dev())
        if split is None:
            split = self.cutback()
        _check_tensor(events, self.nconn, 1, row=(64,))
        _check_tensor(rows, self.nconn, 1, row=(32,))
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
        _check_tensor(events, self.nconn, 1, row=(64,))
        _check_tensor(rows, self.nconn, 1, row=(32,))
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
