"""The base of the ctypes binding over libugofec.so: what the modules of the
public headers (ugo_amd/encoder.py ... ugo_amd/loop.py, one per header of
include/) share.  The library and its prototypes, the errors, and the pieces
every handle-owning class is made of: one handle owner, one member-set base
and one check per kind of operand."""
from __future__ import annotations

import ctypes
import os
import re
from typing import List, Optional, Sequence

try:  # load torch first so libugofec.so binds torch's libamdhip64.so.7 (same soname)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the host-only paths
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# UGO_FEC_LIB: another build of the same library (interleaved A/B runs in tools/)
LIB_PATH = os.environ.get("UGO_FEC_LIB") or os.path.join(_HERE, "libugofec.so")
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
HEADER_PATHS = tuple(os.path.join(_INCLUDE, h) for h in (
    "ugo_fec.h", "ugo_fec_conn.h", "ugo_pkt.h", "ugo_stream.h", "ugo_ack.h", "ugo_sent.h", "ugo_cc.h", "ugo_listen.h",
    "ugo_loop.h"))
(HEADER_PATH, CONN_HEADER_PATH, PKT_HEADER_PATH, STREAM_HEADER_PATH, ACK_HEADER_PATH, SENT_HEADER_PATH, CC_HEADER_PATH,
 LISTEN_HEADER_PATH, LOOP_HEADER_PATH) = HEADER_PATHS

OK = 0
STREAM_SET_MAX_CONN = 1 << 20  # include/ugo_stream.h: the most members of a set, of every family


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

# ------------------------------------------------------------ the prototypes
_CLOCK_T = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_void_p)
sz, vp, i, u, u32, u64, P = (ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint32,
                             ctypes.c_uint64, ctypes.POINTER)
_VOID = ([vp], None)                            # void f(handle): the destroys
_VIEW = [vp, P(vp), P(sz)]                      # f(handle, &pointer, &count): the views of device memory
_SET_CREATE = [vp, vp, sz, P(vp)]               # f(context, members, n, &set)
_STATE = [vp, vp]                               # f(handle, records out)
# header -> {entry point: argtypes, or (argtypes, restype) where it does not return a status}
_PROTOTYPES = {
    "ugo_fec.h": {
        "ugo_fec_create": [i, i, i, P(vp)],
        "ugo_fec_destroy": _VOID,
        "ugo_fec_geometry": [vp, P(i), P(i), P(i)],
        "ugo_fec_matrix": [vp, vp],
        "ugo_fec_encode": [vp, vp, sz, sz, sz, vp],
        "ugo_fec_encode_strided": [vp, vp, sz, sz, sz, sz, vp],
        "ugo_fec_reconstruct": [vp, vp, vp, sz, sz, sz, u, vp, vp],
        "ugo_fec_reconstruct_strided": [vp, vp, vp, sz, sz, sz, sz, u, vp, vp],
        "ugo_fec_reconstruct_into": [vp, vp, vp, sz, sz, sz, sz, vp, sz, sz, u, vp, vp],
        "ugo_fec_reconstruct_rows": [vp, vp, vp, sz, sz, vp, sz, sz, u, vp, vp],
        "ugo_fec_lossy_groups": [vp, vp, sz, u, vp, vp, vp],
        "ugo_fec_reconstruct_list": [vp, vp, vp, sz, vp, vp, sz, sz, sz, sz, vp, sz, sz, u, vp, vp],
        "ugo_fec_recover_data": [vp, vp, vp, sz, sz, sz, sz, vp, sz, sz, vp, vp, vp],
        "ugo_fec_device_address": [vp, vp, P(vp)],
        "ugo_fec_encode_host": [vp, vp, sz, sz, sz],
        "ugo_fec_reconstruct_host": [vp, vp, vp, sz, sz, sz, u, vp],
        "ugo_fec_service_start": [vp, u],
        "ugo_fec_service_stop": [vp],
        "ugo_fec_service_config": [vp, u, u, u],
        "ugo_fec_poisoned": [vp],
        "ugo_fec_check_shards": [i, vp, i, P(sz)],
        "ugo_fec_rx_assemble": [vp, vp, sz, vp, sz, vp, u64, sz, vp, sz, sz, sz, vp, vp, vp],
        "ugo_fec_rx_assemble_frames": [vp, vp, sz, vp, sz, vp, u64, sz, vp, sz, sz, sz, vp, vp, vp],
        "ugo_fec_tx_assemble": [vp, vp, sz, vp, sz, u32, vp, sz, vp, sz, vp, vp, vp],
        "ugo_fec_rx_recover_host": [vp, vp, sz, vp, sz, vp, u64, sz, sz, vp, vp, vp, sz, sz, vp, P(sz)],
        "ugo_fec_tx_assemble_host": [vp, vp, sz, vp, sz, u32, vp, sz, vp, sz, vp, vp],
        "ugo_fec_set_tx_host_route": [vp, i],
        "ugo_fec_set_host_copy_queue": [vp, i],
        "ugo_fec_rc4_keystream": [vp, sz, vp, sz],
        "ugo_fec_timing_begin": [vp, sz],
        "ugo_fec_timing_end": [vp, vp, sz, P(sz), P(sz)],
        "ugo_fec_host_alloc": [sz, P(vp)],
        "ugo_fec_host_free": [vp],
        "ugo_fec_strerror": ([i], ctypes.c_char_p),
        "ugo_fec_abi_version": [],
    },
    "ugo_fec_conn.h": {
        "ugo_fecconn_new": [i, i, i, i, P(vp)],
        "ugo_fecconn_free": _VOID,
        "ugo_fecconn_set_clock": [vp, _CLOCK_T, vp],
        "ugo_fecconn_mark_data": [vp, vp],
        "ugo_fecconn_mark_fec": [vp, vp],
        "ugo_fecconn_get_next": [vp, P(u32)],
        "ugo_fecconn_set_next": [vp, u32],
        "ugo_fecconn_input": [vp, vp, sz, P(u32), P(ctypes.c_uint16), vp, sz, P(i), P(sz)],
        "ugo_fecconn_calc_ecc": [vp, P(vp), P(sz), i, i, i],
        "ugo_fecconn_set_batch": [vp, i, vp, sz, P(i), P(sz)],
        "ugo_fecconn_set_batch_ex": [vp, i, u, vp, sz, P(i), P(sz)],
        "ugo_fecconn_flush": [vp, vp, sz, P(i), P(sz)],
        "ugo_fecconn_pending": [vp, P(sz)],
        "ugo_fecconn_service": [vp, i],
        "ugo_fecconn_rx_len": [vp, P(sz)],
    },
    "ugo_pkt.h": {
        "ugo_fec_packet_decode": [vp, vp, sz, vp, sz, vp, u, vp, vp, sz, vp, sz, vp],
        "ugo_fec_packet_encode": [vp, vp, vp, sz, vp, sz, vp, sz, sz, vp, u, vp, sz, vp, vp, vp],
    },
    "ugo_stream.h": {
        "ugo_fec_stream_rx_create": [vp, sz, P(vp)],
        "ugo_fec_stream_rx_destroy": _VOID,
        "ugo_fec_stream_deliver": [vp, vp, sz, vp, vp, vp, sz, sz, vp, vp],
        "ugo_fec_stream_read": [vp, vp, sz, vp, vp, vp],
        "ugo_fec_stream_rx_state": _STATE,
        "ugo_fec_stream_rx_window": _VIEW,
        "ugo_fec_stream_set_create": _SET_CREATE,
        "ugo_fec_stream_set_destroy": _VOID,
        "ugo_fec_stream_set_deliver": [vp, vp, sz, vp, vp, vp, sz, sz, vp, vp, vp],
        "ugo_fec_stream_set_read": [vp, vp, vp, vp, vp, vp, vp],
        "ugo_fec_stream_set_state": _STATE,
        "ugo_fec_stream_tx_create": [vp, sz, sz, u64, u64, P(vp)],
        "ugo_fec_stream_tx_destroy": _VOID,
        "ugo_fec_stream_tx_window": _VIEW,
        "ugo_fec_stream_tx_queue": _VIEW,
        "ugo_fec_stream_tx_set_create": _SET_CREATE,
        "ugo_fec_stream_tx_set_destroy": _VOID,
        "ugo_fec_stream_tx_set_write": [vp, vp, vp, vp, vp, vp],
        "ugo_fec_stream_tx_set_release": [vp, vp, vp],
        "ugo_fec_stream_tx_set_retransmit": [vp, vp, vp, vp, sz, vp, vp],
        "ugo_fec_stream_tx_set_plan": [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp],
        "ugo_fec_stream_tx_set_encode": [vp, vp, vp, sz, vp, sz, vp, sz, vp, u, vp, sz, vp, vp, vp],
        "ugo_fec_stream_tx_set_state": _STATE,
    },
    "ugo_ack.h": {
        "ugo_fec_ack_rx_create": [vp, sz, P(vp)],
        "ugo_fec_ack_rx_destroy": _VOID,
        "ugo_fec_ack_rx_state": _STATE,
        "ugo_fec_ack_rx_bitmap": _VIEW,
        "ugo_fec_ack_set_create": _SET_CREATE,
        "ugo_fec_ack_set_destroy": _VOID,
        "ugo_fec_ack_set_receive": [vp, vp, vp, sz, vp, sz, u64, vp],
        "ugo_fec_ack_set_touch": [vp, vp, vp],
        "ugo_fec_ack_set_attach": [vp, u64, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp],
        "ugo_fec_ack_set_state": _STATE,
    },
    "ugo_sent.h": {
        "ugo_fec_sent_tx_create": [vp, sz, sz, P(vp)],
        "ugo_fec_sent_tx_destroy": _VOID,
        "ugo_fec_sent_tx_slots": _VIEW,
        "ugo_fec_sent_tx_segments": [vp, P(vp), P(sz), P(sz)],
        "ugo_fec_sent_tx_scratch": _VIEW,
        "ugo_fec_sent_set_create": _SET_CREATE,
        "ugo_fec_sent_set_destroy": _VOID,
        "ugo_fec_sent_set_record": [vp, vp, vp, sz, vp, vp, vp, sz, u64, vp],
        "ugo_fec_sent_set_ack": [vp, vp, vp, sz, vp, sz, u64, vp, vp],
        "ugo_fec_sent_set_rto": [vp, vp, u64, vp, vp],
        "ugo_fec_sent_set_drain": [vp, sz, vp, vp, vp, vp, vp, vp, vp],
        "ugo_fec_sent_set_attach": [vp, vp, vp, sz, vp, vp, vp],
        "ugo_fec_sent_set_state": _STATE,
    },
    "ugo_cc.h": {
        "ugo_fec_cc_set_create": [vp, vp, vp, P(vp)],
        "ugo_fec_cc_set_destroy": _VOID,
        "ugo_fec_cc_set_cutback": [vp, P(vp)],
        "ugo_fec_cc_sent_ack": [vp, vp, vp, sz, vp, sz, u64, vp, vp, vp, vp],
        "ugo_fec_cc_set_ack": [vp, vp, vp, u64, vp, vp],
        "ugo_fec_cc_set_rto": [vp, vp, sz, sz, vp, vp],
        "ugo_fec_cc_set_state": _STATE,
    },
    "ugo_listen.h": {
        "ugo_fec_listen_create": [vp, sz, P(vp)],
        "ugo_fec_listen_destroy": _VOID,
        "ugo_fec_listen_state": _STATE,
        "ugo_fec_listen_route": [vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp],
        "ugo_fec_listen_remap": [vp, vp, sz, sz, vp, vp],
        "ugo_fec_listen_names": [vp, vp, sz, vp, vp, vp],
        "ugo_fec_listen_entries": [vp, vp, sz, vp],
    },
    "ugo_loop.h": {
        "ugo_fec_loop_set_create": [vp, vp, vp, vp, vp, vp, u64, P(vp)],
        "ugo_fec_loop_set_destroy": _VOID,
        "ugo_fec_loop_set_receive": [vp, vp, vp, sz, u64, vp],
        "ugo_fec_loop_set_close": [vp, vp, vp, u64, vp],
        "ugo_fec_loop_set_check": [vp, u64, vp, vp, vp],
        "ugo_fec_loop_set_append": [vp, vp, sz, vp, vp, sz, vp, vp, vp, vp],
        "ugo_fec_loop_set_sent": [vp, vp, vp, vp, u64, vp, vp, vp, sz, vp, vp, vp, vp],
        "ugo_fec_loop_set_state": _STATE,
    },
}
del sz, vp, i, u, u32, u64, P

_lib = None


def load_library(path: str = LIB_PATH):
    """Load libugofec.so.  Raises loudly if it was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run `make -C ugo_amd/csrc` (or __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for protos in _PROTOTYPES.values():
        for name, proto in protos.items():
            fn = getattr(lib, name)
            if isinstance(proto, tuple):
                proto, fn.restype = proto
            fn.argtypes = proto
    _lib = lib
    return lib


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


_LAYOUT = "argument does not match the batch layout the entry point expects"


def _require(cond, msg: str = _LAYOUT):
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


# ------------------------------------------------------------ operand checks
def _check_tensor(t, n: int, item: int, name: Optional[str] = None, count: Optional[str] = None,
                  at_least: bool = False, row: Optional[tuple] = None, integer: bool = False):
    """The one check of a flat or row operand: contiguous, `item` bytes an element, and n elements whatever the
    shape (row=None) or n rows of shape `row` (() = one dimension); at_least: n or more; integer: no
    floating-point dtype.  name and count (how the message calls n) give the ValueError its text."""
    ok = t.is_contiguous() and t.element_size() == item
    if row is None:
        ok = ok and (t.numel() >= n if at_least else t.numel() == n)
    else:
        ok = (ok and t.dim() == 1 + len(row) and (t.shape[0] >= n if at_least else t.shape[0] == n) and
              tuple(t.shape[1:]) == row)
    if ok and not (integer and t.dtype.is_floating_point):
        return
    if name is None:
        _require(False)
    if row is not None:
        raise ValueError(f"{name} must be contiguous, {item}-byte, " +
                         (f"at least {(n,) + row}" if at_least else f"[{count}]"))
    count = ("" if at_least else f"{n} ") if count is None else count + " "
    raise ValueError(f"{name} must be {count}contiguous {8 * item}-bit integers")


def _check_info(info, n: int, at_least: bool = False):
    """info: uint8 [n, 64], PKT_INFO_DTYPE rows."""
    _require(info.is_contiguous() and info.element_size() == 1 and info.dim() == 2 and
             (info.shape[0] >= n if at_least else info.shape[0] == n) and info.shape[1] == 64)


def _check_ranges(ranges, n: int, at_least: bool = False, max_ranges: Optional[int] = None):
    """ranges: 64-bit [n, max_ranges, 2]; max_ranges: the most rows a packet the callee takes."""
    _require(ranges.is_contiguous() and ranges.element_size() == 8 and ranges.dim() == 3 and
             (ranges.shape[0] >= n if at_least else ranges.shape[0] == n) and ranges.shape[2] == 2 and
             (max_ranges is None or ranges.shape[1] <= max_ranges))


def _check_segs(segs, n: int, at_least: bool = False, max_segments: Optional[int] = None, msg: str = _LAYOUT):
    """segs: uint8 [n, max_segments, 16], PKT_SEGMENT_DTYPE entries; max_segments: 1 to that many a packet."""
    _require(segs.is_contiguous() and segs.element_size() == 1 and segs.dim() == 3 and
             (segs.shape[0] >= n if at_least else segs.shape[0] == n) and segs.shape[2] == 16 and
             (max_segments is None or 1 <= segs.shape[1] <= max_segments), msg)


# ------------------------------------------------------------- handle owners
class _DeviceBytes:
    """A span of device memory for torch.as_tensor (__cuda_array_interface__)."""

    def __init__(self, ptr: int, nbytes: int, owner):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        self._owner = owner


class _Handle:
    """The owner of one handle of the library, `_h`: closed once, by close() or with the object."""

    _destroy = ""  # the entry point that frees _h
    _dependants = ()  # the open objects over this one: closed before it

    def close(self):
        if getattr(self, "_h", None):
            for d in list(self._dependants):
                d.close()
            getattr(load_library(), self._destroy)(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _dev(self):
        return torch.device("cuda", self.device)

    def _view(self, ptr: int, nbytes: int):
        """A uint8 CUDA tensor over nbytes of the library's device memory at ptr; it keeps this object alive."""
        return torch.as_tensor(_DeviceBytes(ptr, nbytes, self), device=self._dev())


class _MemberSet(_Handle):
    """An ordered set of members of one class over one context; it does not own them."""

    _member, _nouns, _attr, _create = None, ("", ""), "", ""  # member class, its nouns, attribute and create symbol

    def __init__(self, enc, members):
        members = list(members)
        self.check_members(enc, members)
        arr = (ctypes.c_void_p * len(members))(*[m._h.value for m in members])
        h = ctypes.c_void_p()
        _raise(getattr(load_library(), self._create)(enc._h, ctypes.addressof(arr), len(members), ctypes.byref(h)))
        self._h, self._enc = h, enc  # context and members must outlive the set
        setattr(self, self._attr, members)
        self.nconn = len(members)
        self.device = enc.device

    @classmethod
    def check_members(cls, enc, members):
        one, many = cls._nouns
        _require(0 < len(members) <= STREAM_SET_MAX_CONN, f"a set holds 1 to {STREAM_SET_MAX_CONN} {many}")
        _require(all(isinstance(m, cls._member) and getattr(m, "_h", None) for m in members),
                 f"members must be open {cls._member.__name__}")
        _require(all(m._enc is enc for m in members), "every member must belong to the set's context")
        _require(len({id(m) for m in members}) == len(members), f"a {one} may be listed once")

    def check_per_conn(self, t, element_size: int, name: str):
        _check_tensor(t, self.nconn, element_size, name, "nconn", integer=True)
