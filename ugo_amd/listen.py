"""include/ugo_listen.h: the connection table of a listening socket."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from .abi import _check_tensor, _Handle, _raise, _require, _stream_handle, load_library, torch
from .encoder import Encoder
from .stream import STREAM_NO_CONN

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


class ListenTable(_Handle):
    """The connection table of a listening socket (include/ugo_listen.h):
    listener.handlePacket for a whole ring per call.  route writes conn_of for
    the stages that take it and the list of accepted connections; names turns
    the conn_of of StreamTxSet.plan into sendmmsg names; remap goes with a set
    rebuild.  Operands are tensors in device or pinned host memory; nothing is
    synchronised but state() and entries().

    Kept: operands are checked by shape and may be longer than their count, and a float
    tensor of the right width is taken; the stream, ack and sent sets refuse it."""

    _destroy = "ugo_fec_listen_destroy"

    def __init__(self, enc: "Encoder", max_conn: int):
        _require(isinstance(max_conn, int) and 1 <= max_conn <= LISTEN_MAX_CONN, "1 <= max_conn <= 2^20")
        h = ctypes.c_void_p()
        _raise(load_library().ugo_fec_listen_create(enc._h, max_conn, ctypes.byref(h)))
        self._h, self._enc = h, enc  # the context must outlive the table
        self.max_conn, self.device = max_conn, enc.device

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
        _check_tensor(names, npk, 1, "names", at_least=True, row=(LISTEN_NAME_BYTES,))
        _check_tensor(lens, npk, 2, "lens", at_least=True, row=())
        dev = self._dev()
        if conn_of is None:
            conn_of = torch.zeros(npk, dtype=torch.int32, device=dev)
        if cls is None:
            cls = torch.zeros(npk, dtype=torch.uint8, device=dev)
        if accepted is None:
            accepted = torch.zeros((min(npk, self.max_conn), 48), dtype=torch.uint8, device=dev)
        if n_accepted is None:
            n_accepted = torch.zeros(1, dtype=torch.int32, device=dev)
        _check_tensor(conn_of, npk, 4, "conn_of", at_least=True, row=())
        _check_tensor(cls, npk, 1, "cls", at_least=True, row=())
        _check_tensor(accepted, accepted.shape[0], 1, "accepted", at_least=True, row=(48,))
        _check_tensor(n_accepted, 1, 4, "n_accepted", at_least=True, row=())
        _raise(load_library().ugo_fec_listen_route(
            self._h, names.data_ptr(), pkts.data_ptr(), pkts.shape[1], lens.data_ptr(), npk, conn_of.data_ptr(),
            cls.data_ptr(), accepted.data_ptr() if accepted.shape[0] else None, accepted.shape[0],
            n_accepted.data_ptr(), _stream_handle(stream)))
        return conn_of, cls, accepted, n_accepted

    def remap(self, new_index, nconn_new: int, status=None, stream=None):
        """ugo_fec_listen_remap.  new_index int32 [nconn] (STREAM_NO_CONN as -1
        closes a member).  Returns status int32 [1]: 0 or LISTEN_REMAP_* bits."""
        _require(isinstance(nconn_new, int) and nconn_new >= 0)
        _check_tensor(new_index, new_index.shape[0], 4, "new_index", at_least=True, row=())
        _require(new_index.shape[0] <= LISTEN_MAX_CONN)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=self._dev())
        _check_tensor(status, 1, 4, "status", at_least=True, row=())
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
        _check_tensor(conn_of, npk, 4, "conn_of", at_least=True, row=())
        if names_out is None:
            names_out = torch.zeros((npk, LISTEN_NAME_BYTES), dtype=torch.uint8, device=self._dev())
        if name_lens is None:
            name_lens = torch.zeros(npk, dtype=torch.int32, device=self._dev())
        _check_tensor(names_out, npk, 1, "names_out", at_least=True, row=(LISTEN_NAME_BYTES,))
        _check_tensor(name_lens, npk, 4, "name_lens", at_least=True, row=())
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
        _check_tensor(out, out.shape[0], 1, "out", at_least=True, row=(32,))
        _raise(load_library().ugo_fec_listen_entries(self._h, out.data_ptr(), out.shape[0], _stream_handle(stream)))
        rows = out.cpu().numpy().view(LISTEN_ENTRY_DTYPE).reshape(-1)
        return rows[rows["member"] != STREAM_NO_CONN]
