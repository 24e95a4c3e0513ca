"""One stream connection on the device beside the rule of tests/stream_ref.py,
shared by test_stream_deliver.py and test_stream_deliver_sizes.py; test
infrastructure only.

Every deliver and every read compares seg_status, every field of the record
and the whole window -- pre-filled with a sentinel, so that a byte written
outside an accepted segment shows -- with RuleRx, and ordered_segments with the
rule's contested count.  finish() is the last call of a history: fresh
segments over every uncovered byte of the window, so that a bit left behind in
any of the four bitmaps turns into a wrong status, record or ordered count.
"""
import numpy as np
import pytest
import torch

import stream_ref as sr
from stream_ref import Packet, Seg  # noqa: F401
from ugo_amd import fec

KEY = b"1234567890123456"  # ugo/listener.go:92, ugo/dial.go:132
SENTINEL = 0xA5
MAX_SLOT = 65520           # the largest slot: a multiple of 16, at most 0xffff


@pytest.fixture(scope="module")
def enc(gpu):
    e = fec.New(10, 3, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pad_bytes():
    """The keystream for the largest slot; a shorter slot uses its prefix."""
    return np.frombuffer(fec.rc4_keystream(KEY, MAX_SLOT), np.uint8).copy()


def rand_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def build_batch(packets, slot, max_segments, pad, data_off=None, seed=0):
    """The decoder's view of `packets`: (pkts [npk, slot] still encrypted, info,
    segs).  Segment j of packet i sits at data_off(i, j) -- default: packed
    behind a few header bytes -- and is XORed with pad by its position."""
    rng = np.random.default_rng(seed)
    npk = len(packets)
    pkts = rng.integers(0, 256, (npk, slot), dtype=np.uint8)   # header bytes and slack: noise
    info = np.zeros(npk, fec.PKT_INFO_DTYPE)
    segs = np.zeros((npk, max_segments), fec.PKT_SEGMENT_DTYPE)
    for i, p in enumerate(packets):
        info[i]["status"] = p.status
        info[i]["n_segments"] = len(p.segs)
        cur = int(rng.integers(1, 24))
        for j, s in enumerate(p.segs):
            off = cur + int(rng.integers(3, 12)) if data_off is None else data_off(i, j)
            av = len(s.data)
            assert off + av <= slot, (off, av, slot)
            body = np.frombuffer(s.data, np.uint8)
            pkts[i, off:off + av] = body ^ pad[off:off + av] if pad is not None else body
            segs[i, j] = (s.offset, off, s.length, av)
            cur = off + av
    return pkts, info, segs


def _place(arr, where):
    """A uint8 numpy array as a torch tensor in device or pinned host memory."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory() if where == "pinned" else t.cuda()


class Harness:
    """One connection on the device beside the rule (and, inside the common
    domain, the literal reference); every step is compared.

    pad: a keystream of at least `slot` bytes or None.  rule: a RuleRx to take
    over from (the device connection is then in that state already, its window
    holding rule.W); default a new connection, window filled with SENTINEL."""

    def __init__(self, enc, cap, slot=256, max_segments=4, pad=None, literal=False, rx=None, rule=None, ordered=0):
        self.rx = fec.StreamRx(enc, cap) if rx is None else rx
        self.lit = sr.LiteralConn() if literal else None
        self.cap, self.slot, self.max_segments = cap, slot, max_segments
        self.pad = pad
        self._dpad = {}
        self.ordered = ordered
        self.calls = 0
        if rule is not None:
            self.rule = rule
            return
        self.rule = sr.RuleRx(cap, SENTINEL)
        st = self.rx.state()
        assert st["ngaps"] == 1 and st["read_pos"] == 0 and st["err"] == 0
        assert not self.rx.window().any().item()               # create zeroes the window
        self.rx.window().fill_(SENTINEL)

    def close(self):
        self.rx.close()

    def device_pad(self, slot, where="device"):
        if self.pad is None:
            return None
        if (slot, where) not in self._dpad:
            self._dpad[slot, where] = _place(self.pad[:slot], where)
        return self._dpad[slot, where]

    def check(self):
        st = self.rx.state()
        want = self.rule.record()
        got = {k: int(st[k]) for k in want}
        assert got == want
        assert int(st["ordered_segments"]) == self.ordered
        win = self.rx.window().cpu().numpy()
        bad = np.flatnonzero(win != self.rule.W)
        assert bad.size == 0, f"window differs at {bad[:8]} (of {bad.size})"

    def deliver(self, packets, data_off=None, ordered="count", raw=None, slot=None, inputs="device",
                outputs="device", status_shift=0, pkts_guard=(0, 0), pad_room=None):
        """ordered: "count" -- ordered_segments must grow by exactly the rule's
        contested count; an int -- by exactly that; None -- it is read back.
        raw: (pkts, info, segs) numpy arrays as they are (pkts may be a view into
        a larger array); `packets` is then what the rule is to see.  slot: other
        than the connection's.  inputs / outputs: "device" or "pinned" (host).
        status_shift: seg_status starts that many bytes past a 256-B boundary.
        pkts_guard: raw pkts has that many slots of the test's own in front of
        and behind the batch, all in one allocation.  pad_room: the pad is the
        first `slot` bytes of this larger array, placed as one allocation."""
        self.calls += 1
        slot = self.slot if slot is None else slot
        pad = None if self.pad is None else self.pad[:slot]
        pkts, info, segs = raw if raw is not None else build_batch(packets, slot, self.max_segments, pad,
                                                                   data_off, seed=self.calls)
        npk = len(packets)
        dp = _place(pkts, inputs)[pkts_guard[0]:pkts_guard[0] + npk]
        assert tuple(dp.shape) == (npk, slot) and dp.shape[0] + sum(pkts_guard) == len(pkts)
        dpad = self.device_pad(slot, inputs) if pad_room is None else _place(pad_room, inputs)[:slot]
        di = _place(info.view(np.uint8).reshape(npk, 64), inputs)
        ds = _place(segs.view(np.uint8).reshape(npk, self.max_segments, 16), inputs)
        n = npk * self.max_segments
        if outputs == "pinned":
            room = torch.full((n + 256 + status_shift,), 0x77, dtype=torch.uint8).pin_memory()
        else:
            room = torch.full((n + 256 + status_shift,), 0x77, dtype=torch.uint8, device="cuda")
        at = (-room.data_ptr()) % 256 + status_shift
        status = room[at:at + n].view(npk, self.max_segments)
        assert status.data_ptr() % 256 == status_shift and status.is_contiguous()
        self.rx.deliver(dp, di, ds, pad=dpad, out=status)
        want = self.rule.deliver(packets, count_contested=ordered == "count")
        self.rx.state()                                        # waits for the call: pinned outputs are complete
        whole = room.cpu().numpy()
        got = whole[at:at + n].reshape(npk, self.max_segments)
        assert (whole[:at] == 0x77).all() and (whole[at + n:] == 0x77).all()   # nothing around seg_status
        exp = np.zeros_like(got)
        for i, row in enumerate(want):
            exp[i, :len(row)] = row
        assert np.array_equal(got, exp), (np.argwhere(got != exp)[:8], got[got != exp][:8], exp[got != exp][:8])
        if ordered == "count":
            self.ordered += self.rule.contested
        elif ordered is None:
            self.ordered = int(self.rx.state()["ordered_segments"])
        else:
            self.ordered += ordered
        self.check()
        if self.lit is not None:
            assert self.lit.deliver(packets) == want
        return got

    def read(self, n, discard=False, dst_shift=None, guard=64, outputs="device"):
        """dst_shift: dst is carved out of a sentinel-filled buffer, dst_shift
        bytes past a 16-B boundary and `guard` bytes from either end; every byte
        of that buffer outside [0, n_read) must come back untouched."""
        if discard:
            buf, n_read, eof = self.rx.read(n, discard=True)
        else:
            shift = 0 if dst_shift is None else dst_shift
            size = guard + 16 + shift + n + guard
            if outputs == "pinned":
                room = torch.full((size,), 0x5A, dtype=torch.uint8).pin_memory()
                n_read = torch.zeros(1, dtype=torch.int64).pin_memory()
                eof = torch.full((1,), 0x33, dtype=torch.uint8).pin_memory()
            else:
                room = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda")
                n_read = torch.zeros(1, dtype=torch.int64, device="cuda")
                eof = torch.full((1,), 0x33, dtype=torch.uint8, device="cuda")
            at = guard + (-(room.data_ptr() + guard)) % 16 + shift
            assert (room.data_ptr() + at) % 16 == shift
            dst = room[at:at + max(n, 1)]
            assert dst.data_ptr() == room.data_ptr() + at
            self.rx.read(n, out=dst, n_read=n_read, eof=eof)
            self.rx.state()                                    # waits for the call
        data, want_eof = self.rule.read(n)
        m = int(n_read.cpu().item())
        assert m == len(data) and int(eof.cpu().item()) == int(want_eof)
        if not discard:
            got = room.cpu().numpy()
            exp = np.full(size, 0x5A, np.uint8)
            exp[at:at + m] = np.frombuffer(data, np.uint8)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"read buffer differs at {bad[:8] - at} from dst (of {bad.size}), m = {m}"
        self.check()
        if self.lit is not None:
            assert self.lit.read(n) == (data, want_eof)
        return data, want_eof

    def finish(self, seed=0, ordered="count"):
        """The call after the history: fresh segments over every uncovered byte
        of [read_pos, read_pos + cap), compared like any other call.  A claim or
        contested bit left in the scratch bitmaps, or a C or S bit left below or
        beyond what the rule holds, changes a status, the record or the ordered
        count here.  A segment that starts on a queued empty segment is the
        rule's DUPLICATE."""
        assert self.rule.err == sr.NONE
        rng = np.random.default_rng(seed)
        slot = max(self.slot, 256) if self.cap < (1 << 20) else MAX_SLOT     # a large window in few packets
        assert self.pad is None or len(self.pad) >= slot
        packets = sr.tile_uncovered(self.rule, rng, slot - 16)
        assert packets
        per = max(1, (64 << 20) // slot)
        for k in range(0, len(packets), per):
            ms, self.max_segments = self.max_segments, 1
            try:
                got = self.deliver(packets[k:k + per], data_off=lambda i, j: 1 + (i % 15), ordered=ordered, slot=slot)
            finally:
                self.max_segments = ms
        assert self.rule.err == sr.NONE
        return got
