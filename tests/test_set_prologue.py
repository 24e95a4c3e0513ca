"""The prologue every per-call entry point of a set shares (include/ugo_stream.h,
ugo_ack.h, ugo_sent.h, ugo_cc.h, ugo_loop.h, ugo_listen.h), held as a whole:
handle, empty batch, argument rule, device view -- in that order -- and the
member rules of the four set creates.  Every case is one the ABI rejects (or
answers) before a launch; the entry points come from the table below."""
import ctypes

import numpy as np
import pytest
import torch

from stream_harness import enc  # noqa: F401  (fixture)
from ugo_amd import fec

OK, BAD = 0, fec.ErrInvalidArg.code
SENTINEL = 0x5C
ROOM = 256  # bytes of device memory behind every pointer argument

# One row per entry point: the family whose handle it takes, then its arguments after the handle.
#   "p"  a pointer: 256 sentinel bytes of device memory of its own, 256-B aligned
#   "n"  the batch size whose zero is the empty batch (2 otherwise)
#   int  a value the argument rule accepts
# The stream (NULL) follows the last argument.
CALLS = [
    ("ugo_fec_stream_set_deliver", "stream_rx", ("p", 16, "p", "p", "p", 1, "n", "p", "p")),
    ("ugo_fec_stream_set_read", "stream_rx", ("p", "p", "p", "p", "p")),
    ("ugo_fec_stream_tx_set_write", "stream_tx", ("p", "p", "p", "p")),
    ("ugo_fec_stream_tx_set_release", "stream_tx", ("p",)),
    ("ugo_fec_stream_tx_set_retransmit", "stream_tx", ("p", "p", "p", "n", "p")),
    ("ugo_fec_stream_tx_set_plan", "stream_tx", ("p", 16, 1, 2, "p", "p", "p", "p", "p", "p")),
    ("ugo_fec_stream_tx_set_encode", "stream_tx", ("p", "p", 1, "p", 1, "p", "n", "p", 0, "p", 16, "p", "p")),
    ("ugo_fec_ack_set_receive", "ack", ("p", "p", "n", "p", 1, 5)),
    ("ugo_fec_ack_set_touch", "ack", ("p",)),
    ("ugo_fec_ack_set_attach", "ack", (5, "p", "p", "p", "p", 2, "p", "p", 1, "p", "p", "p")),
    ("ugo_fec_sent_set_record", "sent", ("p", "p", 1, "p", "p", "p", "n", 5)),
    ("ugo_fec_sent_set_ack", "sent", ("p", "p", 1, "p", 2, 5, "p")),
    ("ugo_fec_sent_set_rto", "sent", ("p", 5, "p")),
    ("ugo_fec_sent_set_drain", "sent", (2, "p", "p", "p", "p", "p", "p")),
    ("ugo_fec_sent_set_attach", "sent", ("p", "p", 2, "p", "p")),
    ("ugo_fec_cc_sent_ack", "sent", ("p", "p", 1, "p", 2, 5, "p", "p", "p")),
    ("ugo_fec_cc_set_ack", "cc", ("p", "p", 5, "p")),
    ("ugo_fec_cc_set_rto", "cc", ("p", 1, 1, "p")),
    ("ugo_fec_loop_set_receive", "loop", ("p", "p", "n", 5)),
    ("ugo_fec_loop_set_close", "loop", ("p", "p", 5)),
    ("ugo_fec_loop_set_check", "loop", (5, "p", "p")),
    ("ugo_fec_loop_set_append", "loop", ("p", 2, "p", "p", 1, "p", "p", "p")),
    ("ugo_fec_loop_set_sent", "loop", ("p", "p", "p", 5, "p", "p", "p", 2, "p", "p", "p")),
    ("ugo_fec_listen_route", "listen", ("p", "p", 16, "p", "n", "p", "p", "p", 2, "p")),
    ("ugo_fec_listen_remap", "listen", ("p", 2, 2, "p")),
    ("ugo_fec_listen_names", "listen", ("p", "n", "p", "p")),
    ("ugo_fec_listen_entries", "listen", ("p", 2)),
]
# (handle, host_out): no batch, no device pointer
STATES = [("ugo_fec_stream_set_state", "stream_rx"), ("ugo_fec_stream_tx_set_state", "stream_tx"),
          ("ugo_fec_ack_set_state", "ack"), ("ugo_fec_sent_set_state", "sent"), ("ugo_fec_cc_set_state", "cc"),
          ("ugo_fec_loop_set_state", "loop"), ("ugo_fec_listen_state", "listen")]
CREATES = ["ugo_fec_stream_set_create", "ugo_fec_stream_tx_set_create", "ugo_fec_ack_set_create",
           "ugo_fec_sent_set_create"]
IDS = [c[0][len("ugo_fec_"):] for c in CALLS]


def test_the_table_names_every_per_call_entry_point_of_the_families():
    """CPU: the literal table against the headers' stream-ordered calls."""
    want = {s for s in fec.header_stream_symbols()
            if any(k in s for k in ("_set_", "_cc_", "_listen_")) and not s.endswith(("_create", "_destroy"))}
    assert {c[0] for c in CALLS} == want
    assert len({c[0] for c in CALLS}) == len(CALLS)


class Families:
    """Every family at its smallest legal size: two members at the headers'
    minimum windows, a listen table of two."""

    def __init__(self, enc):
        self.enc = enc
        self.members = {
            "stream_rx": [fec.StreamRx(enc, fec.STREAM_MIN_WINDOW) for _ in range(2)],
            "stream_tx": [fec.StreamTx(enc, fec.STREAM_MIN_WINDOW, 1) for _ in range(2)],
            "ack": [fec.AckRx(enc, fec.ACK_MIN_WINDOW) for _ in range(2)],
            "sent": [fec.SentTx(enc, fec.SENT_MIN_WINDOW, 1) for _ in range(2)],
        }
        m = self.members
        self.sets = {"stream_rx": fec.StreamRxSet(enc, m["stream_rx"]), "stream_tx": fec.StreamTxSet(enc, m["stream_tx"]),
                     "ack": fec.AckRxSet(enc, m["ack"]), "sent": fec.SentTxSet(enc, m["sent"])}
        s = self.sets
        s["cc"] = fec.CcSet(enc, s["sent"])
        s["loop"] = fec.LoopSet(enc, s["stream_rx"], s["ack"], s["stream_tx"], s["sent"], now_us=0)
        s["listen"] = fec.ListenTable(enc, 2)

    def handle(self, family):
        return self.sets[family]._h

    def close(self):
        for k in ("loop", "cc", "listen", "stream_rx", "stream_tx", "ack", "sent"):
            self.sets[k].close()
        for ms in self.members.values():
            for x in ms:
                x.close()


@pytest.fixture(scope="module")
def fam(enc):
    f = Families(enc)
    yield f
    f.close()


@pytest.fixture(scope="module")
def room(gpu):
    """Sentinel-filled device memory for the pointer arguments, and pageable host memory no kernel can reach."""
    dev = torch.full((16 * ROOM,), SENTINEL, dtype=torch.uint8, device="cuda")
    host = np.full(2 * ROOM, SENTINEL, np.uint8)
    pageable = (host.ctypes.data + ROOM - 1) // ROOM * ROOM
    assert dev.data_ptr() % ROOM == 0
    torch.cuda.synchronize()
    return dev, host, pageable


def _args(spec, dev, n=2, swap=None, null=False):
    """The argument list of a row: pointer k of the row replaced by `swap[k]`, every pointer NULL with `null`."""
    out, k = [], 0
    for a in spec:
        if a == "p":
            p = dev.data_ptr() + k * ROOM
            out.append(None if null else (swap or {}).get(k, p))
            k += 1
        else:
            out.append(n if a == "n" else a)
    assert k * ROOM <= dev.numel()
    return out + [None]


def _untouched(dev, host):
    torch.cuda.synchronize()
    return bool((dev == SENTINEL).all()) and bool((host == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,spec", CALLS, ids=IDS)
def test_null_handle_is_an_argument_error(fam, room, name, family, spec):
    dev, host, _ = room
    fn = getattr(fec.load_library(), name)
    assert fn(None, *_args(spec, dev)) == BAD
    assert fn(None, *_args(spec, dev, n=0)) == BAD  # the handle comes before the empty batch
    assert _untouched(dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("name,family", STATES, ids=[s[0][len("ugo_fec_"):] for s in STATES])
def test_state_of_a_null_handle_or_into_null(fam, name, family):
    fn = getattr(fec.load_library(), name)
    out = np.full(4096, SENTINEL, np.uint8)
    assert fn(None, out.ctypes.data) == BAD
    assert fn(fam.handle(family), None) == BAD
    assert (out == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,spec", [c for c in CALLS if "n" in c[2]],
                         ids=[i for i, c in zip(IDS, CALLS) if "n" in c[2]])
def test_empty_batch_is_ok_and_writes_nothing(fam, room, name, family, spec):
    dev, host, pageable = room
    fn = getattr(fec.load_library(), name)
    h = fam.handle(family)
    assert fn(h, *_args(spec, dev, n=0)) == OK
    # ... before the argument rule and the device views are looked at
    assert fn(h, *_args(spec, dev, n=0, null=True)) == OK
    assert fn(h, *_args(spec, dev, n=0, swap={0: pageable})) == OK
    assert _untouched(dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,spec", CALLS, ids=IDS)
def test_pageable_pointer_is_an_argument_error(fam, room, name, family, spec):
    dev, host, pageable = room
    fn = getattr(fec.load_library(), name)
    h = fam.handle(family)
    for k in range(spec.count("p")):  # each pointer argument in turn, the others valid
        assert fn(h, *_args(spec, dev, swap={k: pageable})) == BAD, (name, k)
    assert _untouched(dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("create", CREATES)
def test_create_rejects_a_member_listed_twice_or_of_another_context(fam, create):
    family = {"ugo_fec_stream_set_create": "stream_rx", "ugo_fec_stream_tx_set_create": "stream_tx",
              "ugo_fec_ack_set_create": "ack", "ugo_fec_sent_set_create": "sent"}[create]
    make = {"stream_rx": lambda e: fec.StreamRx(e, fec.STREAM_MIN_WINDOW),
            "stream_tx": lambda e: fec.StreamTx(e, fec.STREAM_MIN_WINDOW, 1),
            "ack": lambda e: fec.AckRx(e, fec.ACK_MIN_WINDOW),
            "sent": lambda e: fec.SentTx(e, fec.SENT_MIN_WINDOW, 1)}[family]
    fn = getattr(fec.load_library(), create)
    a, b = (m._h.value for m in fam.members[family])
    other = fec.New(4, 2)
    stranger = make(other)
    third = make(fam.enc)

    def status(ctx, *handles):
        arr = (ctypes.c_void_p * len(handles))(*handles)
        out = ctypes.c_void_p(1)
        st = fn(ctx._h, ctypes.addressof(arr), len(handles), ctypes.byref(out))
        if st == OK:  # not expected: give it back
            getattr(fec.load_library(), create.replace("_create", "_destroy"))(out)
            return st, "made"
        return st, out.value

    try:
        assert status(fam.enc, a, a) == (BAD, None)
        assert status(fam.enc, a, b, a) == (BAD, None)                      # at the ends
        assert status(fam.enc, a, b, b, third._h.value) == (BAD, None)      # in the middle
        assert status(fam.enc, a, stranger._h.value) == (BAD, None)         # a member of another context
        assert status(other, a, b) == (BAD, None)                           # every member foreign
        assert status(fam.enc, a, None) == (BAD, None)
        assert status(fam.enc) == (BAD, None)                               # an empty list
    finally:
        third.close()
        stranger.close()
        other.close()


@pytest.mark.gpu
def test_loop_and_cc_calls_after_their_neighbour_is_gone(enc, room):  # noqa: F811
    """A set of their own: the neighbours go first, one at a time."""
    dev, host, _ = room
    lib = fec.load_library()
    loop_calls = [c for c in CALLS if c[1] == "loop"]
    cc_calls = [c for c in CALLS if c[1] == "cc"]
    assert len(loop_calls) == 5 and len(cc_calls) == 2
    for gone in ("stream_rx", "ack", "stream_tx", "sent"):
        f = Families(enc)
        try:
            f.sets[gone].close()
            for name, _, spec in loop_calls:
                assert getattr(lib, name)(f.handle("loop"), *_args(spec, dev)) == BAD, (gone, name)
                assert getattr(lib, name)(f.handle("loop"), *_args(spec, dev, n=0)) == BAD, (gone, name)
            for name, _, spec in cc_calls if gone == "sent" else ():
                assert getattr(lib, name)(f.handle("cc"), *_args(spec, dev)) == BAD, name
        finally:
            f.close()
    assert _untouched(dev, host)
