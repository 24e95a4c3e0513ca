"""Stream delivery (include/ugo_stream.h) past the sizes and inputs that
test_stream_deliver.py reaches: segments longer than one pass of the copy
loop, offsets at and above 2^32, offsets that alias live bits modulo the window
or modulo 2^32, batches of several tiles of the ordered pass, windows of
several grid-stride passes, reads into unaligned destinations with guards,
descriptors that lie, operands in pinned host memory -- and, after every
history that did not end in an error, one more call over every uncovered byte
of the window (Harness.finish), which a bit left behind in any bitmap fails.

The checker is the same: RuleRx of tests/stream_ref.py, whole statuses, whole
record, whole window, ordered count.  The CPU tests here hold the additions to
that checker: its translation to a base offset, the clamp of lying descriptors
and the out-of-window table, each against values written out by hand or
against the literal reference.
"""
import numpy as np
import pytest
import torch

import stream_ref as sr
from stream_harness import MAX_SLOT, SENTINEL, Harness, enc, pad_bytes, rand_bytes  # noqa: F401  (fixtures)
from stream_ref import ACCEPTED, DUPLICATE, OUT_OF_WINDOW, Packet, Seg
from ugo_amd import fec

P32, P63, P64 = 1 << 32, 1 << 63, 1 << 64
BASES = [4096, P32 - 3000, P32, (1 << 40) + 7]


# ------------------------------------------------------------------ CPU tests
def _trace(rule, steps):
    """Everything the rule answers over a history."""
    out = []
    for op, arg in steps:
        if op == "deliver":
            st = rule.deliver(arg, count_contested=True)
            out.append((st, rule.contested, dict(rule.record())))
        else:
            out.append((rule.read(arg), dict(rule.record())))
    return out


def _shift_record(rec, k):
    rec = dict(rec)
    rec["read_pos"] += k
    rec["hi"] += k
    if rec["head_valid"]:
        rec["head_off"] += k
    return rec


def test_rule_translation_covariance():
    """The same history K bytes further along: the same statuses, reads and
    contested counts, the record with its offsets shifted, the window rotated
    by K mod cap."""
    cap = 4096
    for seed in range(60):
        rng = np.random.default_rng(seed)
        steps, _ = sr.gen_history(rng, total_max=1500, in_batch_dups=seed % 2 == 1)
        r0 = sr.RuleRx(cap, SENTINEL)
        t0 = _trace(r0, steps)
        assert (r0.W != SENTINEL).any()
        for k in BASES:
            rk = sr.RuleRx.at(cap, k, SENTINEL)
            tk = _trace(rk, sr.shift_history(steps, k))
            assert len(tk) == len(t0)
            for a, b in zip(t0, tk):
                assert a[:-1] == b[:-1], (seed, k)
                assert _shift_record(a[-1], k) == b[-1], (seed, k)
            assert np.array_equal(np.roll(r0.W, k % cap), rk.W), (seed, k)


def test_rule_matches_literal_reference_at_high_bases():
    """RuleRx.at(base) against LiteralConn(base), the literal side taking the
    offsets as they are; then the closing call of Harness.finish through both."""
    n = 0
    for base in BASES:
        for seed in range(150):
            rng = np.random.default_rng(7000 + seed)
            steps, data = sr.gen_history(rng, total_max=1500, in_batch_dups=seed % 2 == 1, base=base,
                                         fin=seed % 3 != 0)
            rule, lit = sr.RuleRx.at(4096, base), sr.LiteralConn(base)
            got = bytearray()
            for op, arg in steps:
                if op == "deliver":
                    assert rule.deliver(arg) == lit.deliver(arg), (base, seed)
                    assert rule.ngaps == len(lit.gaps)
                else:
                    a, b = rule.read(arg), lit.read(arg)
                    assert a == b, (base, seed)
                    got += a[0]
            assert bytes(got) == data and rule.read_pos == base + len(data)
            assert rule.err == sr.NONE and lit.err == sr.NONE and not lit.hit_start_eq_gap_end
            last = sr.tile_uncovered(rule, rng, 240)
            want = rule.deliver(last, count_contested=True)
            assert want == lit.deliver(last) and rule.contested == 0
            flat = [s for row in want for s in row]
            # a queued empty segment at read_pos answers for the segment that starts on it
            assert flat[0] == (DUPLICATE if seed % 3 != 0 else ACCEPTED) and set(flat[1:]) == {ACCEPTED}
            assert rule.hi == rule.read_pos + 4096
            n += 1
    assert n == 4 * 150


def test_contested_count_matches_the_set_form():
    """_contested_count (byte maps) is _contested_count_sets at any state."""
    n = 0
    for seed in range(300):
        rng = np.random.default_rng(seed)
        steps, _ = sr.gen_history(rng, total_max=1500, in_batch_dups=True)
        rule = sr.RuleRx(4096)
        for op, arg in steps:
            if op == "deliver":
                a, b = rule._contested_count(arg), rule._contested_count_sets(arg)
                assert a == b, seed
                n += a
                rule.deliver(arg)
            else:
                rule.read(arg)
    assert n > 300


def test_generator_forced_tiles_and_base():
    rng = np.random.default_rng(5)
    steps, data = sr.gen_history(rng, seg_max=700, base=P32 - 4500, total=9000, fin=False,
                                 forced=[(4200, 300), (4500, 200), (6000, 1400)])
    segs = [s for op, arg in steps if op == "deliver" for p in arg for s in p.segs]
    assert all(s.length > 0 for s in segs)                              # no fin
    assert any(s.offset == P32 - 300 and s.length == 300 for s in segs)
    assert any(s.offset == P32 and s.length == 200 for s in segs)
    assert any(s.offset == P32 + 1500 and s.length == 1400 for s in segs)
    assert min(s.offset for s in segs) == P32 - 4500 and max(s.offset + s.length for s in segs) == P32 + 4500
    assert all(s.data == data[s.offset - (P32 - 4500):][:len(s.data)] for s in segs)


# (slot, data_off, len, avail) -> the avail that is used
CLAMP_TABLE = [
    ((64, 10, 20, 20), 20),
    ((64, 10, 20, 30), 20),                  # avail > len
    ((64, 10, 20, 0xFFFF), 20),
    ((64, 45, 20, 20), 19),                  # one byte past the slot
    ((64, 59, 20, 20), 5),                   # 15
    ((64, 60, 20, 20), 4),                   # 16
    ((64, 61, 20, 20), 3),                   # 17
    ((64, 63, 10, 10), 1),                   # data_off == slot - 1
    ((64, 64, 10, 10), 0),                   # data_off == slot
    ((64, 65, 10, 10), 0),                   # data_off > slot
    ((64, 1000, 40, 40), 0),
    ((64, P32 - 1, 40, 40), 0),              # the largest data_off: no 32-bit sum may wrap it back in
    ((64, 20, 0, 7), 0),                     # len == 0 with avail > 0
    ((64, 0, 64, 64), 64),
    ((64, 16, 64, 64), 48),
    ((64, 32, 200, 200), 32),
    ((65520, 1, 65519, 65519), 65519),
    ((65520, 16, 65535, 65535), 65504),
    ((65520, 65519, 65535, 65535), 1),
]


def test_clamp_table():
    for args, want in CLAMP_TABLE:
        assert sr.clamp_segment(*args) == want, args


def test_packets_from_raw():
    rng = np.random.default_rng(3)
    slot, ms = 64, 2
    pkts = rng.integers(0, 256, (4, slot), dtype=np.uint8)
    pad = rng.integers(0, 256, slot, dtype=np.uint8)
    info = np.zeros(4, fec.PKT_INFO_DTYPE)
    segs = np.zeros((4, ms), fec.PKT_SEGMENT_DTYPE)
    info["n_segments"] = [1, ms + 1, 0xFFFF, 2]
    info["status"][3] = 7
    segs[0, 0] = (100, 59, 20, 20)           # five bytes in the slot, fifteen zeros
    segs[1] = [(200, 10, 4, 9), (204, 64, 3, 3)]
    segs[2] = [(300, 0, 0, 5), (P32 + 1, 63, 2, 2)]
    out = sr.packets_from_raw(pkts, info, segs, pad)
    assert [len(p.segs) for p in out] == [1, ms, ms, 2] and [p.status for p in out] == [0, 0, 0, 7]
    s = out[0].segs[0]
    assert (s.offset, s.length, s.data) == (100, 20, (pkts[0, 59:64] ^ pad[59:64]).tobytes())
    assert s.body() == s.data + bytes(15)
    a, b = out[1].segs
    assert (a.offset, a.length, a.data) == (200, 4, (pkts[1, 10:14] ^ pad[10:14]).tobytes())
    assert (b.offset, b.length, b.data) == (204, 3, b"")
    a, b = out[2].segs
    assert (a.offset, a.length, a.data) == (300, 0, b"")
    assert (b.offset, b.length, b.data) == (P32 + 1, 2, bytes([pkts[2, 63] ^ pad[63]]))
    plain = sr.packets_from_raw(pkts, info, segs)
    assert plain[0].segs[0].data == pkts[0, 59:64].tobytes()


# The out-of-window and aliasing table.  Window 4096, read_pos 1003 (so the
# window is [1003, 5099)), live bits: a data segment [2000, 2100) (start bit at
# 2000, coverage without a start bit at 2050), an empty segment at 3000 (start
# bit only), a data segment [4500, 4600) (above cap, so that x - cap exists).
OOW_CAP, OOW_RP, OOW_LIVE = 4096, 1003, (2000, 2050, 3000, 4500)
O, D, A = OUT_OF_WINDOW, DUPLICATE, ACCEPTED
# per length: (offset, status), written out by hand
OOW_TABLE = {
    0: [(6096, O), (10192, O), (P32 + 2000, O),
        (6146, O), (10242, O), (P32 + 2050, O),
        (7096, O), (11192, O), (P32 + 3000, O),
        (8596, O), (12692, O), (P32 + 4500, O), (404, O),      # 404 < read_pos: an empty segment there is outside
        (P63, O), (P64 - 1, O),
        (5099, O),                                             # read_pos + cap: the first offset outside
        (5100, O)],
    1: [(6096, O), (10192, O), (P32 + 2000, O),
        (6146, O), (10242, O), (P32 + 2050, O),
        (7096, O), (11192, O), (P32 + 3000, O),
        (8596, O), (12692, O), (P32 + 4500, O), (404, D),      # wholly below read_pos: old data, not an alias
        (P63, O), (P64 - 1, O), (P64 - 1, O),                  # 2^64-1 + 1 wraps to 0
        (5098, A),                                             # the last byte of the window
        (5099, O)],
    40: [(6096, O), (10192, O), (P32 + 2000, O),
         (6146, O), (10242, O), (P32 + 2050, O),
         (7096, O), (11192, O), (P32 + 3000, O),
         (8596, O), (12692, O), (P32 + 4500, O), (404, D),
         (P63, O), (P64 - 1, O), (P64 - 40, O), (P64 - 39, O),  # o + len wraps to 0 and to 1
         (5059, A),                                            # ends exactly at read_pos + cap
         (5060, O)],
}


def _oow_setup(rng):
    return [("deliver", [Packet([Seg(0, rand_bytes(rng, OOW_RP))])]),
            ("read", OOW_RP),
            ("deliver", [Packet([Seg(2000, rand_bytes(rng, 100))]), Packet([Seg(3000)]),
                         Packet([Seg(4500, rand_bytes(rng, 100))])])]


def _oow_batch(rng, length):
    rows = sr.out_of_window_rows(OOW_RP, OOW_CAP, OOW_LIVE, length)
    assert [o for _, o in rows] == [o for o, _ in OOW_TABLE[length]], rows
    return [Packet([Seg(o, rand_bytes(rng, length))]) for _, o in rows], [s for _, s in OOW_TABLE[length]]


@pytest.mark.parametrize("length", [0, 1, 40])
def test_out_of_window_table_through_the_rule(length):
    rng = np.random.default_rng(31)
    for one_call in (True, False):
        rule = sr.RuleRx(OOW_CAP, SENTINEL)
        for op, arg in _oow_setup(rng):
            rule.deliver(arg) if op == "deliver" else rule.read(arg)
        assert rule.read_pos == OOW_RP and rule.S[[2000, 3000, 4500 - 4096]].all() and not rule.S[2050]
        assert rule.C[2050] and not rule.C[3000]
        batch, want = _oow_batch(rng, length)
        c0, s0 = rule.C.copy(), rule.S.copy()
        got = rule.deliver(batch) if one_call else [rule.deliver([p])[0] for p in batch]
        assert [r[0] for r in got] == want
        # the bitmaps' effect: only what was accepted
        for p, st in zip(batch, want):
            if st == A:
                s = p.segs[0]
                s0[s.offset & 4095] = True
                c0[np.arange(s.offset, s.offset + s.length) & 4095] = True
        assert np.array_equal(rule.C, c0) and np.array_equal(rule.S, s0)
        assert rule.out_of_window == want.count(O) and rule.duplicate == want.count(D)


# ------------------------------------------------------------------ GPU tests
# A. long segments
LONG = [2047, 2048, 2049, 2064, 4095, 4113, 9000, 65519, 65535]
CORNERS = (0, 1, 15)


@pytest.mark.gpu
@pytest.mark.parametrize("with_pad", [False, True])
def test_long_segments(enc, pad_bytes, with_pad):
    """One segment per packet, longer than one pass of the copy loop (128
    chunks, 2048 B) by nothing, a byte, a chunk, and up to the u16 limit; data_off
    and stream offset at the corner residues mod 16; tiled without a gap, sent
    in descending order, through a 262144-B window that they lap.  65519 bytes
    are present only at data_off 0 and 1 (the largest slot is 65520); 65535 is
    declared with the slot's rest present and a zero tail."""
    rng = np.random.default_rng(41)
    h = Harness(enc, 262144, slot=MAX_SLOT, max_segments=1, pad=pad_bytes if with_pad else None)
    packets, offs, seen, x = [], [], set(), 0
    for L in LONG:
        for r_doff in CORNERS:
            for r_off in CORNERS:
                if L == 65519 and r_doff == 15:
                    continue
                fill = (r_off - x) % 16
                if fill:
                    packets.append(Packet([Seg(x, rand_bytes(rng, fill))]))
                    offs.append(7)
                    x += fill
                if L == 65535:
                    doff = 16 + r_doff
                    seg = Seg(x, rand_bytes(rng, MAX_SLOT - doff - 3), length=L)
                else:
                    doff = r_doff if L == 65519 else 32 + r_doff
                    seg = Seg(x, rand_bytes(rng, L))
                packets.append(Packet([seg]))
                offs.append(doff)
                seen.add((L, doff % 16, x % 16))
                x += L
    want = {(L, a, b) for L in LONG for a in CORNERS for b in CORNERS if not (L == 65519 and a == 15)}
    assert seen == want and len(seen) == 78
    k = 0
    while k < len(packets):
        room, n = h.cap - h.rule.readable, 0
        while k + n < len(packets) and packets[k + n].segs[0].length <= room:
            room -= packets[k + n].segs[0].length
            n += 1
        part, part_offs = packets[k:k + n][::-1], offs[k:k + n][::-1]
        got = h.deliver(part, data_off=lambda i, j: part_offs[i], ordered=0)
        assert (got[:, 0] == ACCEPTED).all()
        h.read(h.cap, dst_shift=k % 16)
        k += n
    assert h.rule.read_pos == x and x > 4 * h.cap
    h.finish()
    h.close()


# B. crossing 2^32
def _advance(enc, cap, target):
    """A device connection whose read_pos and hi are `target`, reached by
    delivering gap-free tilings of len = 65535 / avail = 0 segments and
    discarding them; the record is checked in closed form after every call.
    Returns (rx, accepted)."""
    rx = fec.StreamRx(enc, cap)
    rx.window().fill_(SENTINEL)
    nseg = cap // 65535
    lap = nseg * 65535
    assert target >= 2 * lap
    info = np.zeros(nseg, fec.PKT_INFO_DTYPE)
    info["n_segments"] = 1
    segs = np.zeros((nseg, 1), fec.PKT_SEGMENT_DTYPE)
    segs["offset"][:, 0] = np.arange(nseg, dtype=np.uint64) * 65535
    segs["len"] = 65535
    pkts = torch.full((nseg, 16), 0xEE, dtype=torch.uint8, device="cuda")
    di = torch.from_numpy(info.view(np.uint8).reshape(nseg, 64)).cuda()
    ds = torch.from_numpy(segs.view(np.uint8).reshape(nseg, 1, 16)).cuda()
    offsets = ds.view(torch.int64).view(nseg, 2)[:, 0]
    status = torch.zeros((nseg, 1), dtype=torch.uint8, device="cuda")
    pos = accepted = 0

    def record(read_pos, hi, readable):
        st = rx.state()
        got = {k: int(st[k]) for k in ("read_pos", "hi", "readable", "accepted", "ngaps", "head_valid",
                                       "ordered_segments", "err", "duplicate", "out_of_window", "eof")}
        assert got == {"read_pos": read_pos, "hi": hi, "readable": readable, "accepted": accepted, "ngaps": 1,
                       "head_valid": 0, "ordered_segments": 0, "err": 0, "duplicate": 0, "out_of_window": 0,
                       "eof": 0}, got

    def step(n, nbytes):
        nonlocal pos, accepted
        rx.deliver(pkts[:n], di[:n], ds[:n], out=status[:n])
        accepted += n
        record(pos, pos + nbytes, nbytes)
        assert bool((status[:n] == ACCEPTED).all().item())
        _, n_read, eof = rx.read(nbytes + 1, discard=True)
        pos += nbytes
        record(pos, pos, 0)
        assert int(n_read.item()) == nbytes and not eof.item()

    while pos + lap <= target:
        step(nseg, lap)
        offsets += lap
    rest = target - pos
    if rest:
        n = -(-rest // 65535)
        last = rest - (n - 1) * 65535
        ds.view(torch.int16).view(nseg, 8)[n - 1, 6] = last if last < 32768 else last - 65536   # len of the last one
        step(n, rest)
    assert pos == target
    assert not rx.window().any().item()          # every lap wrote zeros, the laps shift by cap % 65535
    return rx, accepted


B_CAP = 1 << 24
B_BASE = P32 - 4500


def _takeover(enc, pad_bytes, slot, max_segments):
    rx, accepted = _advance(enc, B_CAP, B_BASE)
    rule = sr.RuleRx.at(B_CAP, B_BASE, sentinel=0, accepted=accepted)
    h = Harness(enc, B_CAP, slot=slot, max_segments=max_segments, pad=pad_bytes, rx=rx, rule=rule)
    h.lit = sr.LiteralConn(B_BASE)
    h.check()
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("forced", ["ends_and_starts", "straddles"])
def test_crossing_2_32_histories(enc, pad_bytes, forced):
    """One connection advanced to 2^32 - 4500, then in-domain batches with
    duplicates, retransmissions and reads up to 2^32 + 4500, compared in full:
    once with a segment that ends exactly at 2^32 and one that starts there,
    once with one that lies across it."""
    tiles = {"ends_and_starts": [(4200, 300), (4500, 200)], "straddles": [(3800, 1400)]}[forced]
    for seed in (51, 52):
        h = _takeover(enc, pad_bytes, 3008, 3)
        rng = np.random.default_rng(seed)
        steps, data = sr.gen_history(rng, seg_max=700, in_batch_dups=True, base=B_BASE, total=9000, fin=False,
                                     forced=tiles)
        sent = {(s.offset, s.length) for op, arg in steps if op == "deliver" for p in arg for s in p.segs}
        if forced == "straddles":
            assert (P32 - 700, 1400) in sent
        else:
            assert (P32 - 300, 300) in sent and (P32, 200) in sent
        got = bytearray()
        for op, arg in steps:
            if op == "deliver":
                h.deliver(arg)
            else:
                got += h.read(arg, dst_shift=arg % 16)[0]
        assert bytes(got) == data and h.rule.read_pos == P32 + 4500
        assert h.ordered > 0
        h.finish(seed)
        h.close()


@pytest.mark.gpu
def test_crossing_2_32_reads(enc, pad_bytes):
    """Reads that stop at 2^32 - 1, 2^32 and 2^32 + 1, with a partly read head
    segment whose head_off lies below 2^32 while read_pos does not."""
    rng = np.random.default_rng(53)
    h = _takeover(enc, pad_bytes, 3536, 1)
    s1, s2, s3 = Seg(B_BASE, rand_bytes(rng, 3500)), Seg(P32 - 1000, rand_bytes(rng, 1500)), \
        Seg(P32 + 500, rand_bytes(rng, 1000))
    # an empty segment above 2^32 while read_pos is below: in the window by 64-bit arithmetic only
    got = h.deliver([Packet([s3]), Packet([s1]), Packet([Seg(P32 + 2000)]), Packet([s2])], ordered=0)
    assert got[:, 0].tolist() == [1, 1, 1, 1] and h.rule.readable == 6000 and not h.rule.eof
    h.read(4499, dst_shift=1)
    st = h.rx.state()
    assert int(st["read_pos"]) == P32 - 1 and st["head_valid"] == 1 and int(st["head_off"]) == P32 - 1000
    h.read(1, dst_shift=15)
    st = h.rx.state()
    assert int(st["read_pos"]) == P32 and st["head_valid"] == 1 and int(st["head_off"]) == P32 - 1000
    # duplicates: through head_off, through S (data, empty); a fresh empty segment with read_pos at 2^32
    got = h.deliver([Packet([s2]), Packet([s3]), Packet([Seg(P32 + 2000)]), Packet([Seg(P32 + 2500)])], ordered=0)
    assert got[:, 0].tolist() == [2, 2, 2, 1]
    h.read(1, dst_shift=0)
    assert int(h.rx.state()["read_pos"]) == P32 + 1
    h.read(499)
    assert h.rx.state()["head_valid"] == 0                         # at a segment's start
    data, _ = h.read(5000, dst_shift=7)
    assert data == s3.data
    h.finish()
    h.close()


# C. out of window, aliasing
@pytest.mark.gpu
@pytest.mark.parametrize("length", [0, 1, 40])
@pytest.mark.parametrize("one_call", [True, False])
def test_out_of_window_and_aliases(enc, pad_bytes, one_call, length):
    rng = np.random.default_rng(31)
    h = Harness(enc, OOW_CAP, slot=1040, max_segments=1, pad=pad_bytes)
    for op, arg in _oow_setup(rng):
        h.deliver(arg, ordered=0) if op == "deliver" else h.read(arg)
    assert h.rule.read_pos == OOW_RP
    batch, want = _oow_batch(rng, length)
    if one_call:
        got = h.deliver(batch)[:, 0].tolist()
    else:
        got = [int(h.deliver([p])[0, 0]) for p in batch]
    assert got == want                                             # the hand-written column, not only the rule
    assert h.ordered == 0
    h.finish()
    h.close()


# D. the ordered pass over several tiles
TILE = 16 * 1024


def _tiled_batch(rng, case, max_segments):
    """(packets, index of the fatal packet or None): one 1..3-byte segment per
    packet, tiled without a gap; a packet at a chosen index repeats the
    segment of the packet before it, which makes both contested."""
    npk = 36000 if max_segments == 1 else 11004
    total = npk * max_segments
    assert total > 2 * TILE + 200 and (total % 16 == 0) == (max_segments == 1)
    # with three slots per packet the last packet's segment lies in the pass's partial last chunk of 16
    assert max_segments == 1 or (npk - 1) * max_segments >= total - total % 16
    start = [-(-TILE * t // max_segments) for t in range(3)]        # first packet of each tile
    if case == "last_tile":
        repeats = {start[2] + 2, start[2] + 50, start[2] + 51, npk - 40, npk - 1}
    elif case == "every_tile":
        repeats = {1, 900, start[1] + 2, start[1] + 700, start[2] + 2, start[2] + 40, npk - 1}
    else:
        repeats = {10, start[1] + 5, start[1] + 200, start[1] + 201, start[2] + 2, start[2] + 60, npk - 1}
    fatal = start[1] + 100 if case == "fatal" else None
    assert all(0 < i < npk for i in repeats)
    packets, x, prev = [], 0, None
    for i in range(npk):
        if i == fatal:
            seg = Seg(x - 1, rand_bytes(rng, 3))                   # one covered byte, two fresh ones
        elif i in repeats:
            seg = prev
        else:
            n = 1 + i % 3
            seg = Seg(x, rand_bytes(rng, n))
            x += n
        packets.append(Packet([seg]))
        prev = seg
    return packets, fatal, repeats


@pytest.mark.gpu
@pytest.mark.parametrize("status_shift", [0, 1])
@pytest.mark.parametrize("max_segments", [1, 3])
@pytest.mark.parametrize("case", ["last_tile", "every_tile", "fatal"])
def test_ordered_pass_over_three_tiles(enc, pad_bytes, case, max_segments, status_shift):
    """npackets * max_segments entries span three tiles of the ordered pass (a
    multiple of 16 with one segment slot per packet, not one with three);
    seg_status 16-B aligned and one byte past.  Contested segments only in the
    last tile; in every tile and in the batch's last entry; a fatal overlap in
    the middle tile with contested and clean segments after it."""
    rng = np.random.default_rng(61)
    h = Harness(enc, 131072, slot=16, max_segments=max_segments, pad=pad_bytes)
    packets, fatal, repeats = _tiled_batch(rng, case, max_segments)
    tiles = {i * max_segments // TILE for i in repeats}
    assert tiles == ({2} if case == "last_tile" else {0, 1, 2})
    got = h.deliver(packets, data_off=lambda i, j: i % 13, ordered=None if case == "fatal" else "count",
                    status_shift=status_shift)
    col = got[:, 0]
    if case == "fatal":
        assert col[fatal] == sr.OVERLAP and not got[fatal + 1:].any() and (col[:fatal] != 0).all()
        assert h.rule.err == sr.OVERLAP and (h.rule.err_packet, h.rule.err_segment) == (fatal, 0)
        end = packets[fatal - 1].segs[0].offset + packets[fatal - 1].segs[0].length
        assert h.rule.hi == end and not h.rule.C[end:].any() and not h.rule.S[end:].any()
        assert (h.rule.W[end:] == SENTINEL).all()                  # and so is the device's: h.check()
        assert fatal * max_segments // TILE == 1 and 1 <= h.ordered
        before = dict(h.rule.record())
        got = h.deliver(packets[:64], data_off=lambda i, j: i % 13, ordered=0, status_shift=status_shift)
        assert not got.any() and h.rule.record() == before         # inert
    else:
        # every repeat and every segment that is repeated (a run of repeats shares one)
        assert h.rule.contested == len(repeats) + sum(i - 1 not in repeats for i in repeats)
        assert [int(col[i]) for i in sorted(repeats)] == [DUPLICATE] * len(repeats)
        assert (np.delete(col, sorted(repeats)) == ACCEPTED).all()
        assert col[-1] == DUPLICATE                                 # the batch's last segment is contested
        h.read(1000, dst_shift=3)
        h.finish()
    h.close()


# E. grid-stride passes, large reads
E_CAP = 1 << 25
E_RP = 1003
E_B1 = (E_RP & ~63) + 64 * 1024 * 256     # where the second pass of k_apply<One> / k_scan<One> starts
E_B2 = E_CAP                              # the ring's physical end


def _far_segments(rng):
    """49 isolated 100-byte segments (the last: 35 bytes, ending at read_pos +
    cap): most of them beyond 16 MiB from read_pos, an uncovered run across
    word 262143 / 262144 of a pass, one across the ring's end."""
    offs = [E_B1 - 250, E_B1 - 130, E_B1 + 37, E_B2 - 250, E_B2 - 130, E_B2 + 41,
            5000, 70001, (1 << 20) + 3, (8 << 20) + 77]
    offs += [(17 << 20) + k * ((14 << 20) // 38) + 7 * k + 1 for k in range(38)]
    packets = [Packet([Seg(o, rand_bytes(rng, 100))]) for o in offs]
    packets.append(Packet([Seg(E_RP + E_CAP - 35, rand_bytes(rng, 35))]))
    assert len(packets) == 49 and sum(o - E_RP > (16 << 20) for o in offs) >= 40
    order = rng.permutation(len(packets))
    return [packets[i] for i in order]


def _large_window(enc, pad_bytes, rng):
    h = Harness(enc, E_CAP, slot=160, max_segments=1, pad=pad_bytes)
    h.deliver([Packet([Seg(0, rand_bytes(rng, E_RP))])], ordered=0, slot=1040)
    h.read(E_RP)
    return h


@pytest.mark.gpu
def test_grid_stride_passes_and_large_reads(enc, pad_bytes):
    rng = np.random.default_rng(71)
    h = _large_window(enc, pad_bytes, rng)
    got = h.deliver(_far_segments(rng), ordered=0)
    assert (got == ACCEPTED).all()
    assert h.rule.ngaps == 50 and h.rule.err == sr.NONE and h.rule.hi == E_RP + E_CAP and h.rule.readable == 0
    # the runs the passes must not lose or count twice
    assert not h.rule.C[(E_B1 - 30) & (E_CAP - 1)] and not h.rule.C[(E_B1 + 36) & (E_CAP - 1)]
    assert not h.rule.C[E_CAP - 30] and not h.rule.C[40]
    # real data up to beyond the ring's end: 32 MiB readable
    fill = sr.tile_uncovered(h.rule, rng, MAX_SLOT - 16, lo=E_RP, hi=E_B2 + 141)
    got = h.deliver(fill[::-1], data_off=lambda i, j: 1 + i % 15, slot=MAX_SLOT)
    assert (got == ACCEPTED).all() and h.rule.contested == 0
    assert h.rule.readable == E_B2 + 141 - E_RP >= (20 << 20) and h.rule.ngaps == 2
    h.read(h.rule.readable - 100, dst_shift=3)                     # four passes of k_read<One>, across the end
    assert h.rule.read_pos == E_B2 + 41 > E_B2                     # the one call went past the ring's end
    h.read(10000, dst_shift=9)
    assert h.rule.readable == 0
    h.finish()
    h.close()


@pytest.mark.gpu
def test_gap_limit_far_from_read_pos(enc, pad_bytes):
    """The same 49 segments and one more: 51 gaps, counted over three passes."""
    rng = np.random.default_rng(71)
    h = _large_window(enc, pad_bytes, rng)
    batch = _far_segments(rng) + [Packet([Seg(3000, rand_bytes(rng, 100))])]
    got = h.deliver(batch, ordered=0)
    assert (got == ACCEPTED).all() and h.rule.ngaps == 51 and h.rule.err == sr.TOO_MANY_GAPS
    got = h.deliver(batch[:3], ordered=0)
    assert not got.any()
    h.close()


# F. read destination extents
READ_M = [0, 1, 15, 16, 17, 33, 4096 + 5]


@pytest.mark.gpu
def test_read_destination_extents(enc, pad_bytes):
    """dst at every residue mod 16, read_pos at the corner residues, seven
    sizes; alternately n = m < readable and n > readable = m.  The buffer
    around [dst, dst + m) keeps its sentinel (Harness.read compares all of it)."""
    rng = np.random.default_rng(81)
    h = Harness(enc, 8192, slot=4160, max_segments=1, pad=pad_bytes)
    seen, kinds, idx = set(), [0, 0], 0
    for r in CORNERS:
        for d in range(16):
            for m in READ_M:
                short = idx % 2 == 1               # n > readable
                idx += 1
                if h.rule.readable:
                    h.read(h.rule.readable, discard=True)
                x = h.rule.read_pos
                pre = (r - x) % 16
                total = pre + m + (0 if short else 9)
                if total:
                    h.deliver([Packet([Seg(x, rand_bytes(rng, total))])], data_off=lambda i, j: 1 + idx % 15,
                              ordered=0)
                if pre:
                    h.read(pre, discard=True)      # dst == NULL: nothing is written, the record moves
                assert h.rule.read_pos % 16 == r and h.rule.readable == total - pre
                data, _ = h.read(m + 37 if short else m, dst_shift=d)
                assert len(data) == m
                seen.add((r, d, m))
                kinds[short] += 1
    assert seen == {(r, d, m) for r in CORNERS for d in range(16) for m in READ_M} and kinds == [168, 168]
    assert h.rule.read_pos > 8 * h.cap
    h.finish()
    h.close()


# G. hostile descriptors
@pytest.mark.gpu
def test_hostile_descriptors(enc, pad_bytes):
    """Descriptors that point past their slot.  The packets lie inside one
    noise-filled allocation with a slot in front and two behind, the pad in an
    equally large one, so a read past a slot stays in memory this test owns and
    shows as a byte that is not the clamp's zero."""
    rng = np.random.default_rng(91)
    slot, ms, front, back = 64, 2, 1, 2
    rows = [  # (n_segments, [(data_off, len, avail), ...])
        (1, [(10, 20, 30)]),                       # avail > len
        (1, [(45, 20, 20)]),                       # past the slot by 1
        (2, [(59, 20, 20), (60, 20, 20)]),         # by 15, by 16
        (1, [(61, 20, 20)]),                       # by 17
        (2, [(64, 10, 10), (63, 10, 10)]),         # data_off == slot, slot - 1
        (ms + 1, [(5, 7, 7), (12, 40, 40)]),       # n_segments past max_segments
        (0xFFFF, [(0, 64, 64), (16, 64, 64)]),
        (1, [(None, 40, 40)]),                     # the largest data_off inside the allocation
        (1, [(32, 200, 200)]),
        (2, [(20, 0, 7), (48, 17, 0xFFFF)]),       # len == 0 with avail > 0; avail far above len and the slot
        (1, [(65, 33, 33)]),
        (1, [(3, 5, 5)]),                          # the last packet is well formed
    ]
    npk = len(rows)
    room = rng.integers(0, 256, (front + npk + back, slot), dtype=np.uint8)
    pad_room = rng.integers(0, 256, (npk + back) * slot, dtype=np.uint8)
    info = np.zeros(npk, fec.PKT_INFO_DTYPE)
    segs = np.zeros((npk, ms), fec.PKT_SEGMENT_DTYPE)
    x = 0
    for i, (n, descs) in enumerate(rows):
        info[i]["n_segments"] = n
        for j, (off, ln, av) in enumerate(descs):
            if off is None:
                off = min((npk - i + back) * slot, pad_room.size) - 40 - 1
                assert off > 5 * slot
            # an unclamped kernel stays inside both allocations
            assert off + min(av, ln) <= min((npk - i + back) * slot, pad_room.size)
            segs[i, j] = (3000 if ln == 0 else x, off, ln, av)
            x += ln
    pkts = room[front:front + npk]
    packets = sr.packets_from_raw(pkts, info, segs, pad_room[:slot])
    assert [len(p.segs) for p in packets] == [min(n, ms) for n, _ in rows]
    avails = [len(s.data) for p in packets for s in p.segs]
    assert avails == [20, 19, 5, 4, 3, 0, 1, 7, 40, 64, 48, 0, 32, 0, 16, 0, 5]
    h = Harness(enc, 4096, slot=slot, max_segments=ms, pad=pad_room)
    got = h.deliver(packets, raw=(room, info, segs), pkts_guard=(front, back), pad_room=pad_room, ordered=0)
    want = [[1] * len(p.segs) + [0] * (ms - len(p.segs)) for p in packets]
    assert got.tolist() == want
    assert h.rule.readable == x and h.rule.eof == 0 and h.rule.S[3000]
    data, _ = h.read(x + 10, dst_shift=5)
    assert data == b"".join(s.body() for p in packets for s in p.segs)
    h.finish()
    h.close()


# H. pinned host operands
@pytest.mark.gpu
@pytest.mark.parametrize("inputs", ["pinned", "device"])
def test_pinned_host_operands(enc, pad_bytes, inputs):
    """pkts, pad, info, segs, seg_status, dst, n_read and eof in pinned host
    memory; then only the outputs."""
    rng = np.random.default_rng(101)
    h = Harness(enc, 4096, slot=256, max_segments=2, pad=pad_bytes, literal=True)
    a = Packet([Seg(0, rand_bytes(rng, 150)), Seg(150, rand_bytes(rng, 33))])
    b = Packet([Seg(183, rand_bytes(rng, 200))])
    c = Packet([Seg(383, rand_bytes(rng, 17), length=17), Seg(400)])
    got = h.deliver([b, a, c, a], inputs=inputs, outputs="pinned")          # the repeat goes through the ordered pass
    assert got.tolist() == [[1, 0], [1, 1], [1, 1], [2, 2]] and h.ordered == 4
    h.read(100, dst_shift=5, outputs="pinned")
    data, eof = h.read(1000, dst_shift=0, outputs="pinned")
    assert len(data) == 300 and eof
    h.finish()
    h.close()
