"""Receive-window sets (ugo_fec_stream_set_*, include/ugo_stream.h) at the
launch shapes that test_stream_set.py does not reach: several blocks per
connection in k_read<Many> (ticket, scan_head, the split copy), in k_apply<Many> and
k_scan<Many> (runs across the seam between two blocks' bitmap words, the first
uncovered byte found by a later block, a wrapped window), members of very
different sizes in one set, the ordered pass over an unaligned status array with
three segment slots per packet, a member across 2^32 beside one at 0, lying
descriptors between another member's packets, and the connection fold above
32,768 members.

The oracle is what it is for test_stream_set.py: one RuleRx per member through
stream_set_harness.demux_deliver, every status, record field, ordered count,
window byte and destination byte after every call, finish() at the end.  The
histories of groups A and B are plain functions over the harness's interface;
the CPU tests run them over the rules alone (RuleSet) and hold the positions
they aim at -- the block that owns a bitmap word, the seam a run straddles --
and the values written beside each case.  expected_rblocks / expected_wblocks
only assert that a shape is the shape a test claims.
"""
import numpy as np
import pytest

import stream_ref as sr
from stream_harness import MAX_SLOT, SENTINEL, enc, pad_bytes  # noqa: F401  (fixtures)
from stream_harness import rand_bytes as _bytes
from stream_ref import ACCEPTED, DUPLICATE, Packet, Seg
from stream_set_harness import SetHarness, demux_deliver, expected_rblocks, expected_wblocks, interleave
from test_stream_deliver_sizes import _advance
from ugo_amd import fec

P32 = 1 << 32
SHIFTS = (0, 1, 7, 15)

READ_SETS = {"two_blocks": [32768, 4096], "unequal": [1 << 20, 4096, 65536], "one_large": [1 << 22]}
READ_BLOCKS = {"two_blocks": 2, "unequal": 64, "one_large": 256}      # rblocks, as the issue states them
UNEQUAL = READ_SETS["unequal"]
FOLD_NCONN = 32769


def P(o, data, status=0):
    return Packet([Seg(o, data)], status=status)


class RuleSet:
    """SetHarness's interface over the rules alone: what a history does to the
    rules, with no device.  The CPU tests run the histories through it."""

    def __init__(self, caps, max_segments=1, rules=None):
        self.caps = list(caps)
        self.rules = [sr.RuleRx(cap, SENTINEL) for cap in caps] if rules is None else list(rules)
        self.nconn = len(self.caps)
        self.max_segments = max_segments
        self.ordered = [0] * self.nconn

    def deliver(self, packets, conn_of, ordered="count", **_):
        rows, contested = demux_deliver(self.rules, packets, conn_of, count_contested=ordered == "count")
        for c in range(self.nconn):
            self.ordered[c] += contested[c] if ordered == "count" else ordered[c]
        got = np.zeros((len(packets), self.max_segments), np.uint8)
        for i, row in enumerate(rows):
            got[i, :len(row)] = row
        return got

    def read(self, ns, **_):
        return [(b"", False) if v == 0 else self.rules[c].read(v) for c, v in enumerate(ns)]

    def reads(self, ns_list, **_):
        return [self.read(ns) for ns in ns_list]


def _tile(rng, lo, hi, seg_max=1400):
    """Fresh one-segment packets over [lo, hi), ascending, at most seg_max bytes each."""
    out, o = [], lo
    while o < hi:
        n = int(min(hi - o, seg_max - rng.integers(0, 64)))
        out.append(P(o, _bytes(rng, n)))
        o += n
    return out


def _cover_except(rng, lo, hi, holes):
    out, cur = [], lo
    for a, b in sorted(holes) + [(hi, hi)]:
        assert cur <= a <= b <= hi
        out += _tile(rng, cur, a)
        cur = b
    return out


def _round_robin(lists):
    packets, conn_of = [], []
    for k in range(max(len(l) for l in lists)):
        for c, l in enumerate(lists):
            if k < len(l):
                packets.append(l[k])
                conn_of.append(c)
    return packets, conn_of


def _top_up(h, rng, c, upto):
    """Member c, gap-free so far, receives fresh in-order segments up to `upto`."""
    r = h.rules[c]
    lo = r.read_pos + r.readable
    assert r.hi <= lo and upto - r.read_pos <= r.cap
    if upto > lo:
        pk = _tile(rng, lo, upto)
        got = h.deliver(pk, [c] * len(pk), ordered=[0] * h.nconn)
        assert (got[:, 0] == ACCEPTED).all()
        assert r.readable == upto - r.read_pos and r.ngaps == 1


# ------------------------------------------------------- A: the read histories
def reads_history(h, rng):
    """Group A over member 0 (the large one); the small members are read, or
    skipped with n == 0, in the same calls.  Copy seams between the blocks of
    k_read<Many> lie every 4096 bytes from 16 * c0, c0 = (read_pos + 15) >> 4;
    block b of rblocks clears bitmap words [256 b, 256 b + 256) from read_pos &
    ~63 in its first pass.  Returns the blocks whose words held a head segment's
    start bit."""
    cap, n = h.caps[0], h.nconn
    rb = expected_rblocks(max(h.caps), n)
    r = h.rules[0]
    step = [0]

    def small(k):
        for c in range(1, n):
            if h.rules[c].readable < 64:
                _top_up(h, rng, c, h.rules[c].read_pos + 2000)
        return ([0 if (k + c) % 2 else 1 + (7 * k + c) % 40 for c in range(1, n)],
                [SHIFTS[(k + c) % 4] for c in range(n)])

    def rd(n0, **kw):
        ns, shifts = small(step[0])
        step[0] += 1
        return h.read([n0] + ns, shifts=shifts, **kw)[0]

    # lengths 1, 15, 16, 17 (the last with n, n_read, eof and dst in pinned host memory)
    _top_up(h, rng, 0, 3 * 4096)
    for n0, kw in ((1, {}), (15, {}), (16, {}), (17, {"where": "pinned"})):
        data, eof = rd(n0, **kw)
        assert len(data) == n0 and not eof
    assert (r.read_pos, r.readable, r.head_valid, r.head_off) == (49, 3 * 4096 - 49, True, 0)
    # a chunk short of a copy seam, exactly to it, a byte past it: the seam between block 0 and 1,
    # in front of the last block, and between the last block and block 0's second pass
    for k in sorted({1, rb - 1, rb}):
        for d in (-16, 0, 1):
            rp = r.read_pos
            seam = 16 * ((rp + 15) >> 4) + 4096 * k
            _top_up(h, rng, 0, seam + 2000)
            end = rp + r.readable
            assert end >= seam + 2000
            data, _ = rd(seam + d - rp)
            assert len(data) == seam + d - rp and r.read_pos == seam + d and r.readable == end - seam - d
    # the whole window from a read_pos that is no multiple of 16 or 64: across the ring's physical end
    rp = r.read_pos
    assert rp % 16 == 1 and rp % 64 != 0 and rp & (cap - 1) != 0
    _top_up(h, rng, 0, rp + cap)
    assert r.readable == cap
    data, _ = rd(cap)
    assert len(data) == cap and r.read_pos == rp + cap and r.readable == 0 and not r.head_valid
    # more than readable
    _top_up(h, rng, 0, r.read_pos + 5000)
    data, eof = rd(5100)
    assert len(data) == 5000 and not eof and r.readable == 0
    # a partly read head whose start bit lies in a word of block 0, a middle block, the last block
    blocks = sorted({0, rb // 2, rb - 1})
    seen = []
    for discard, which in ((False, blocks), (True, blocks[-1:])):
        for b in which:
            rp = r.read_pos
            base = rp & ~63
            s = base + 64 * (256 * b + 5) + 3              # the head segment's offset: word 256 b + 5
            word = (s - base) // 64
            assert word < 256 * rb and word // 256 == b and r.readable == 0
            seen.append(word // 256)
            _top_up(h, rng, 0, s)
            got = h.deliver([P(s, _bytes(rng, 1300))], [0], ordered=[0] * n)
            assert got[0, 0] == ACCEPTED and r.readable == s + 1300 - rp
            e = s + 700                                    # the read ends inside it, 700 B above its start bit
            data, eof = rd(e - rp, discard=discard)
            assert len(data) == e - rp and not eof
            assert (r.head_valid, r.head_off, r.read_pos, r.readable, r.ngaps, r.eof) == (True, s, e, 600, 1, False)
            # the head again, 100 B longer than what is covered: a duplicate through head_off alone
            got = h.deliver([P(s, _bytes(rng, 1400))], [0], ordered=[0] * n)
            assert got[0, 0] == DUPLICATE and r.err == sr.NONE and r.readable == 600
            data, _ = rd(650, discard=discard)             # the rest: n > readable, ends where the segment ends
            assert len(data) == 600 and (r.head_valid, r.head_off, r.readable) == (False, 0, 0)
    # a read that ends on a segment's boundary with more behind it: no head
    rp = r.read_pos
    h.deliver([P(rp + 1000, _bytes(rng, 1000)), P(rp, _bytes(rng, 1000))], [0, 0], ordered=[0] * n)
    rd(1000)
    assert (r.head_valid, r.head_off, r.read_pos, r.readable, r.ngaps) == (False, 0, rp + 1000, 1000, 1)
    # two reads back to back, no state call in between: the second sees ticket and scan_head reset
    span = min(cap - 4096, 40000)
    _top_up(h, rng, 0, r.read_pos + 1000 + span)
    rp = r.read_pos
    first, second = 1000 + span // 2 + 33, span + 10
    (ns1, sh1), (ns2, sh2) = small(step[0]), small(step[0] + 1)
    step[0] += 2
    out = h.reads([[first] + ns1, [second] + ns2], shifts_list=[sh1, sh2])
    assert len(out[0][0][0]) == first and len(out[1][0][0]) == 1000 + span - first
    assert r.read_pos == rp + 1000 + span and r.readable == 0 and not r.head_valid
    # a read that ends in front of a queued empty segment
    x = r.read_pos
    _top_up(h, rng, 0, x + 20000)
    h.deliver([Packet([Seg(x + 20000, _bytes(rng, 100)), Seg(x + 20100)])], [0], ordered=[0] * n, max_segments=2)
    assert r.readable == 20100 and r.eof and r.ngaps == 1
    data, eof = rd(20100)
    assert len(data) == 20100 and eof and r.readable == 0 and r.read_pos == x + 20100
    return seen


# --------------------------------------------- B: apply and scan, unequal members
def _blk(pos, base):
    """The block of 16 that scans the bitmap word of stream position `pos`."""
    return ((pos - base) // 64 % 4096) // 256


def scan_start(h, rng, start):
    """read_pos of the large member at 0, at an odd value, or 1.5 windows on."""
    r, cap = h.rules[0], h.caps[0]
    if start == "odd":
        _top_up(h, rng, 0, 1003)
        h.read([1003, 0, 0], discard=True)
    elif start == "wrapped":
        _top_up(h, rng, 0, cap)
        h.read([cap, 0, 0], discard=True)
        _top_up(h, rng, 0, cap + cap // 2 + 777)
        h.read([cap, 0, 0], discard=True)
    assert r.read_pos == {"zero": 0, "odd": 1003, "wrapped": cap + cap // 2 + 777}[start] and r.readable == 0
    return r.read_pos


def scan_runs_history(h, rng, start):
    """Uncovered runs at the seams between the blocks of k_scan<Many>: block b of
    16 scans words 256 b + t + 4096 j from read_pos & ~63, so the seams lie every
    16,384 bytes from there.  Returns the holes."""
    r, cap = h.rules[0], h.caps[0]
    rp = scan_start(h, rng, start)
    base = rp & ~63
    X = lambda k: base + 16384 * k  # noqa: E731
    holes = [(X(1) - 10, X(1) + 10),        # across a seam: one run
             (X(2) - 10, X(2)),             # ends at a seam
             (X(3), X(3) + 10),             # starts at a seam
             (X(4) - 1, X(4) + 1),          # a byte on either side
             (X(5) - 1, X(5)),              # the last byte of a block's words
             (X(6), X(6) + 1),              # the first byte of the next block's
             (X(16) - 10, X(16) + 10),      # between block 15 and block 0's second pass
             (X(33) - 7, X(33) + 73)]       # a whole word and more
    if start == "wrapped":
        end = (rp | (cap - 1)) + 1          # the ring's physical end
        assert rp < end - 5 and end + 5 < rp + cap and all(abs(end - X(k)) > 64 for k in range(65))
        holes.append((end - 5, end + 5))
    for a, b in holes:                      # the run's bytes lie where the case says
        assert rp < a < b < rp + cap - 100
    assert [(_blk(a, base), _blk(b - 1, base)) for a, b in holes[:8]] == \
        [(0, 1), (1, 1), (3, 3), (3, 4), (4, 4), (6, 6), (15, 0), (0, 1)]
    hi = rp + cap - 100
    big = _cover_except(rng, rp, hi, holes)[::-1]       # descending: the first packets claim near the window's end
    lo1, lo2 = h.rules[1].read_pos, h.rules[2].read_pos
    one = [P(lo1 + 30 * k, _bytes(rng, 30)) for k in range(60)]
    two = [P(lo2 + 500 * k, _bytes(rng, 500)) for k in range(60)]
    packets, conn_of = _round_robin([big, one, two])
    assert conn_of[:180] == [0, 1, 2] * 60 and packets[0].segs[0].offset > rp + cap - 2000
    got = h.deliver(packets, conn_of, ordered=[0, 0, 0])
    assert (got[:, 0] == ACCEPTED).all()
    nholes = 9 if start == "wrapped" else 8
    assert len(holes) == nholes
    assert (r.ngaps, r.readable, r.hi, r.eof, r.err) == (nholes + 1, X(1) - 10 - rp, hi, False, sr.NONE)
    assert (h.rules[1].readable, h.rules[1].ngaps, h.rules[2].readable, h.rules[2].ngaps) == (1800, 1, 30000, 1)
    # the runs filled again, largest offset first: one gap, everything readable
    fill = [P(a, _bytes(rng, b - a)) for a, b in sorted(holes, reverse=True)]
    h.deliver(fill, [0] * len(fill), ordered=[0, 0, 0])
    assert (r.ngaps, r.readable) == (1, hi - rp)
    return holes


def first_uncovered_history(h, rng, where):
    """The first uncovered byte of the large member in a word of block 0, of
    block 7, in the last word below hi; other blocks see later ones."""
    r = h.rules[0]
    rp = scan_start(h, rng, "odd")
    base = rp & ~63
    word = lambda k, bit: base + 64 * k + bit  # noqa: E731
    hi = word(4096 + 256 * 11 + 40, 30)
    later = [word(4096 + 3, 5), word(256 * 12, 1)]      # block 0's second pass, block 12
    u = {"block0": word(9, 17), "block7": word(256 * 7 + 9, 17), "last_word": hi - 2}[where]
    holes = [(u, u + 1)] + ([] if where == "last_word" else [(x, x + 1) for x in later])
    assert _blk(u, base) == {"block0": 0, "block7": 7, "last_word": 11}[where]
    assert [_blk(x, base) for x in later] == [0, 12]
    assert where != "last_word" or (u - base) // 64 == (hi - 1 - base) // 64
    big = _cover_except(rng, rp, hi, holes)[::-1]
    one = [P(30 * k, _bytes(rng, 30)) for k in range(20)]
    packets, conn_of = _round_robin([big, one])
    h.deliver(packets, conn_of, ordered=[0, 0, 0])
    assert (r.readable, r.ngaps, r.hi, r.eof) == (u - rp, len(holes) + 1, hi, False)
    return u


def gap_limit_history(h, rng, nseg):
    """nseg isolated segments in the large member: nseg + 1 gaps, counted by all
    16 blocks; in-order data for the two small members in the same blocks."""
    r = h.rules[0]
    offs = [20007 * k + 500 for k in range(nseg)]
    assert {_blk(o, 0) for o in offs} == set(range(16)) and offs[-1] + 100 < h.caps[0]
    lists = [[P(o, _bytes(rng, 100)) for o in offs], [P(20 * k, _bytes(rng, 20)) for k in range(50)],
             [P(300 * k, _bytes(rng, 300)) for k in range(50)]]
    packets, conn_of = _round_robin(lists)
    assert len(packets) >= 130
    got = h.deliver(packets, conn_of, ordered=[0, 0, 0])
    assert (got[:, 0] == ACCEPTED).all()
    assert r.ngaps == nseg + 1 and r.readable == 0
    assert r.err == (sr.TOO_MANY_GAPS if nseg + 1 > sr.MAX_GAPS else sr.NONE)
    assert [(x.err, x.readable) for x in h.rules[1:]] == [(sr.NONE, 1000), (sr.NONE, 15000)]
    got = h.deliver([P(0, _bytes(rng, 500)), P(1000, _bytes(rng, 20)), P(15000, _bytes(rng, 300))], [0, 1, 2],
                    ordered=[0, 0, 0])
    assert got[:, 0].tolist() == [0 if nseg + 1 > sr.MAX_GAPS else 1, 1, 1]


# ----------------------------------------------------- C: the ordered pass
ORD_NPK, ORD_MS, ORD_TILE = 36001, 3, 16384


def _ord_nseg(i):
    return 3 if i % 100 in (2, 3) else 2 if i % 100 in (0, 1) else 1


def ordered_batch(rng, fatal):
    """36,001 packets of two connections (even / odd index), three segment slots
    a packet: 108,003 status entries, seven tiles of the ordered pass, the last
    16-entry run partial.  A packet repeated 200 packets later makes every
    segment of both contested.  Connection 0: in the first and the last tile, in
    slots 0, 1 and 2, and in the array's last entries; connection 1: in the
    middle tile only.  fatal: packet 33,050 of connection 0 (last tile) lies
    across covered and fresh bytes, and connection 1 has one more repeat after it.
    Returns (packets, conn_of, repeats per connection, ordered per connection,
    index of the fatal packet or None)."""
    tile = lambda i: i * ORD_MS // ORD_TILE  # noqa: E731
    total = ORD_NPK * ORD_MS
    assert total % 16 == 3 and (total - 1) // ORD_TILE == 6
    i_f = 33050 if fatal else None
    rep = [[1000, 3002, 34000, 35002, 36000], [17001, 18003] + ([35001] if fatal else [])]
    x, packets = [0, 0], []
    for i in range(ORD_NPK):
        c = i % 2
        if i == i_f:
            packets.append(P(x[c] - 1, _bytes(rng, 3)))        # one covered byte, two fresh ones
            continue
        segs = []
        for _ in range(_ord_nseg(i)):
            segs.append(Seg(x[c], _bytes(rng, 8)))
            x[c] += 8
        packets.append(Packet(segs))
    for c in (0, 1):
        for i in rep[c]:
            assert i % 2 == c and i != i_f and i - 200 != i_f
            packets[i] = packets[i - 200]
    assert {tile(i) for i in rep[0]} | {tile(i - 200) for i in rep[0]} == {0, 6}
    assert {tile(i) for i in rep[1][:2]} | {tile(i - 200) for i in rep[1][:2]} == {3}
    assert {len(packets[i].segs) for i in rep[0]} == {2, 3} and len(packets[3002].segs) == 3
    assert ORD_MS * 36000 >= total - 16 and 36000 in rep[0]     # contested entries in the partial last run
    if fatal:
        assert tile(i_f) == 6 and tile(35001) == 6 and 35001 > i_f
        assert len(packets[i_f - 2].segs) == 1 and len(packets[i_f + 2].segs) == 1
        # connection 0 stops at its fatal segment: the repeats before it, the covered neighbour, itself
        ordered = [2 * 2 + 2 * 3 + 2, 2 * 2 + 2 * 3 + 2 * 2]
        assert ordered == [12, 14]
    else:
        ordered = [2 * (2 + 3 + 2 + 3 + 2), 2 * (2 + 3)]
        assert ordered == [24, 10]
    return packets, [i % 2 for i in range(ORD_NPK)], rep, ordered, i_f


# ------------------------------------------------- E: a member across 2^32
E_CAP, E_BASE = 1 << 24, P32 - 4500
E_TILES = {"ends_and_starts": [(4200, 300), (4500, 200)], "straddles": [(3800, 1400)]}


def crossing_rounds(seed, forced):
    """Member 0's history around 2^32 and member 1's from 0, call by call;
    member 1 is delayed so that its segment at 700 and member 0's at 2^32 + 700
    meet in one batch.  Returns (rounds of (lists, ns), data per member, the
    round in which they meet)."""
    rng = np.random.default_rng(seed)
    s0, d0 = sr.gen_history(rng, seg_max=700, in_batch_dups=True, base=E_BASE, total=9000, fin=False,
                            forced=E_TILES[forced] + [(5200, 100)])
    s1, d1 = sr.gen_history(rng, total=1500, in_batch_dups=True, forced=[(700, 100)])

    def holds(steps, off):
        return min(k for k, (op, arg) in enumerate(steps)
                   if op == "deliver" and any(s.offset == off for p in arg for s in p.segs))

    k0, k1 = holds(s0, P32 + 700), holds(s1, 700)
    s0 = [("read", 0)] * max(0, k1 - k0) + list(s0)
    s1 = [("read", 0)] * max(0, k0 - k1) + list(s1)
    rounds = []
    for k in range(max(len(s0), len(s1))):
        lists, ns = [[], []], [0, 0]
        for c, steps in enumerate((s0, s1)):
            if k < len(steps):
                op, arg = steps[k]
                if op == "deliver":
                    lists[c] = arg
                else:
                    ns[c] = arg
        rounds.append((lists, ns))
    meet = max(k0, k1)
    offs = [{s.offset for p in rounds[meet][0][c] for s in p.segs} for c in (0, 1)]
    assert P32 + 700 in offs[0] and 700 in offs[1]          # equal modulo 2^32, in one batch
    sent = {(s.offset, s.length) for lists, _ in rounds for p in lists[0] for s in p.segs}
    if forced == "straddles":
        assert (P32 - 700, 1400) in sent
    else:
        assert (P32 - 300, 300) in sent and (P32, 200) in sent
    return rounds, (d0, d1), meet


def run_rounds(h, rounds, seed):
    rng = np.random.default_rng(seed)
    got = [bytearray(), bytearray()]
    for lists, ns in rounds:
        if any(lists):
            packets, conn_of = interleave(rng, lists)
            h.deliver(packets, conn_of)
        if any(ns):
            out = h.read(ns, shifts=[n % 16 for n in ns])
            for c in (0, 1):
                got[c] += out[c][0]
    return got


# ------------------------------------------------- F: lying descriptors in a set
HOSTILE_ROWS = [  # (n_segments, [(data_off, len, avail), ...]): the table of test_stream_deliver_sizes
    (1, [(10, 20, 30)]),                       # avail > len
    (1, [(45, 20, 20)]),                       # past the slot by 1
    (2, [(59, 20, 20), (60, 20, 20)]),         # by 15, by 16
    (1, [(61, 20, 20)]),                       # by 17
    (2, [(64, 10, 10), (63, 10, 10)]),         # data_off == slot, slot - 1
    (3, [(5, 7, 7), (12, 40, 40)]),            # n_segments past max_segments
    (0xFFFF, [(0, 64, 64), (16, 64, 64)]),
    (1, [(None, 40, 40)]),                     # the largest data_off inside the allocation
    (1, [(32, 200, 200)]),
    (2, [(20, 0, 7), (48, 17, 0xFFFF)]),       # len == 0 with avail > 0; avail far above len and the slot
    (1, [(65, 33, 33)]),
    (1, [(3, 5, 5)]),                          # well formed
]
HOSTILE_SLOT, HOSTILE_MS, HOSTILE_FRONT, HOSTILE_BACK = 64, 2, 1, 2


def hostile_set_batch(rng):
    """The lying packets for member 0, an honest packet of member 1 in front of
    and behind each, and between them one packet whose conn_of is nconn and one
    whose conn_of is 0x80000000: 27 packets, one copy block.  Returns (room,
    pad_room, info, segs, conn_of)."""
    slot, ms, front, back = HOSTILE_SLOT, HOSTILE_MS, HOSTILE_FRONT, HOSTILE_BACK
    plan = ["honest"]
    for k in range(len(HOSTILE_ROWS)):
        plan += [k, "honest"]
    plan.insert(8, "nconn")
    plan.insert(15, "high")
    npk = len(plan)
    assert npk == 27 and npk <= 64
    room = rng.integers(0, 256, (front + npk + back, slot), dtype=np.uint8)
    pad_room = rng.integers(0, 256, (npk + back) * slot, dtype=np.uint8)
    info = np.zeros(npk, fec.PKT_INFO_DTYPE)
    segs = np.zeros((npk, ms), fec.PKT_SEGMENT_DTYPE)
    conn_of, x, y = [], 0, 0
    for i, what in enumerate(plan):
        if what in ("honest", "nconn", "high"):
            info[i]["n_segments"] = 1
            segs[i, 0] = (y, 8, 20, 20)
            conn_of.append({"honest": 1, "nconn": 2, "high": 0x80000000}[what])
            y += 20 if what == "honest" else 0
            continue
        n, descs = HOSTILE_ROWS[what]
        info[i]["n_segments"] = n
        for j, (off, ln, av) in enumerate(descs):
            if off is None:
                off = min((npk - i + back) * slot, pad_room.size) - 40 - 1
                assert off > 5 * slot
            assert off + min(av, ln) <= min((npk - i + back) * slot, pad_room.size)   # an unclamped kernel stays inside
            segs[i, j] = (3000 if ln == 0 else x, off, ln, av)
            x += ln
        conn_of.append(0)
    for i in range(npk):                       # every lying packet between two of member 1, strangers aside
        if conn_of[i] == 0:
            assert 1 in conn_of[max(0, i - 2):i] and 1 in conn_of[i + 1:i + 3]
    return room, pad_room, info, segs, conn_of


def hostile_packets(batch):
    room, pad_room, info, segs, _ = batch
    pkts = room[HOSTILE_FRONT:HOSTILE_FRONT + len(info)]
    return sr.packets_from_raw(pkts, info, segs, pad_room[:HOSTILE_SLOT])


# ------------------------------------------------------------------ CPU tests
def test_shapes_are_what_the_tests_claim():
    for name, caps in READ_SETS.items():
        assert expected_rblocks(max(caps), len(caps)) == READ_BLOCKS[name] >= 2
    assert expected_wblocks(max(UNEQUAL)) == 16 and expected_wblocks(1 << 22) == 64 and expected_wblocks(32768) == 1
    assert expected_wblocks(1 << 19) == 8 and expected_rblocks(1 << 19, 2) == 32           # group C
    assert expected_rblocks(4096, 1024) == 1 and expected_wblocks(4096) == 1               # group D: blockIdx.y alone
    assert FOLD_NCONN > 32768 and expected_rblocks(4096, FOLD_NCONN) == 1
    # the formulas at their clamps
    assert expected_wblocks(1 << 40) == 1024 and expected_rblocks(1 << 40, 1) == 2048
    assert expected_rblocks(1 << 40, 4095) == 1 and expected_rblocks(1 << 40, 4096) == 1
    assert expected_rblocks(16384, 1) == 1 and expected_rblocks(16385, 1) == 2 and expected_wblocks(65537) == 2


@pytest.mark.parametrize("name", list(READ_SETS))
def test_read_histories_through_the_rule(name):
    caps = READ_SETS[name]
    rb = READ_BLOCKS[name]
    seen = reads_history(RuleSet(caps, max_segments=2), np.random.default_rng(11))
    assert seen == sorted({0, rb // 2, rb - 1}) + [rb - 1]


@pytest.mark.parametrize("start", ["zero", "odd", "wrapped"])
def test_scan_histories_through_the_rule(start):
    h = RuleSet(UNEQUAL)
    holes = scan_runs_history(h, np.random.default_rng(12), start)
    rp, cap = h.rules[0].read_pos, UNEQUAL[0]
    assert (rp & (cap - 1)) + cap - 100 > cap or start == "zero"     # the covered range passes the ring's end
    if start == "wrapped":
        assert holes[-1][0] & (cap - 1) == cap - 5


def test_first_uncovered_and_gap_limit_through_the_rule():
    for where in ("block0", "block7", "last_word"):
        h = RuleSet(UNEQUAL)
        u = first_uncovered_history(h, np.random.default_rng(13), where)
        assert not h.rules[0].C[u & (UNEQUAL[0] - 1)] and h.rules[0].C[(u - 1) & (UNEQUAL[0] - 1)]
    for nseg, err in ((49, sr.NONE), (50, sr.TOO_MANY_GAPS)):
        h = RuleSet(UNEQUAL)
        gap_limit_history(h, np.random.default_rng(14), nseg)
        # the second call fills the first gap of a live member; an ended one keeps its record
        assert h.rules[0].err == err and h.rules[0].ngaps == {49: 49, 50: 51}[nseg]


def test_ordered_batch_places_its_contested_entries():
    for fatal in (False, True):
        packets, conn_of, rep, ordered, i_f = ordered_batch(np.random.default_rng(15), fatal)
        assert len(packets) == ORD_NPK and max(len(p.segs) for p in packets) == ORD_MS
        assert all(packets[i] is packets[i - 200] and conn_of[i] == conn_of[i - 200] for c in (0, 1) for i in rep[c])


@pytest.mark.parametrize("forced", list(E_TILES))
def test_crossing_rounds_through_the_rule(forced):
    """The seeds of group E: with the rule alone the forced segments are sent,
    the two members' offsets meet modulo 2^32 in one batch, the ordered pass is
    entered, and both streams read back whole."""
    for seed in (51, 52):
        rounds, data, meet = crossing_rounds(seed, forced)
        h = RuleSet([E_CAP, 4096], max_segments=3, rules=[sr.RuleRx.at(E_CAP, E_BASE), sr.RuleRx(4096, SENTINEL)])
        got = run_rounds(h, rounds, seed)
        assert bytes(got[0]) == data[0] and bytes(got[1]) == data[1]
        assert h.rules[0].read_pos == P32 + 4500 and h.rules[1].eof and h.rules[1].err == sr.NONE
        assert h.ordered[0] > 0 and h.ordered[1] > 0 and any(rounds[meet][0][c] for c in (0, 1))


def test_demultiplexing_raw_descriptors_agrees_with_hand_split():
    batch = hostile_set_batch(np.random.default_rng(91))
    conn_of = batch[4]
    packets = hostile_packets(batch)
    avails = [len(s.data) for p, c in zip(packets, conn_of) if c == 0 for s in p.segs]
    assert avails == [20, 19, 5, 4, 3, 0, 1, 7, 40, 64, 48, 0, 32, 0, 16, 0, 5]     # the clamp, as in the single test
    rules = [sr.RuleRx(4096, SENTINEL), sr.RuleRx(4096, SENTINEL)]
    rows, contested = demux_deliver(rules, packets, conn_of)
    for c in (0, 1):
        alone = sr.RuleRx(4096, SENTINEL)
        want = alone.deliver([p for p, k in zip(packets, conn_of) if k == c], count_contested=True)
        assert [rows[i] for i, k in enumerate(conn_of) if k == c] == want
        assert alone.record() == rules[c].record() and np.array_equal(alone.W, rules[c].W)
        assert contested[c] == alone.contested == 0
    assert all(rows[i] == [sr.NONE] for i, k in enumerate(conn_of) if k > 1) and sum(k > 1 for k in conn_of) == 2
    assert rules[1].readable == 20 * conn_of.count(1) == 260 and rules[1].accepted == 13
    assert set(sum((rows[i] for i, k in enumerate(conn_of) if k == 0), [])) == {ACCEPTED}


# ------------------------------------------------------------------ GPU tests
# A. reads with several blocks per connection
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(READ_SETS))
def test_reads_with_several_blocks_per_connection(enc, pad_bytes, name):
    """reads_history on the device: every length, seam, partly read head,
    back-to-back pair and the end of stream, in sets whose k_read<Many> runs 2, 64
    and 256 blocks per connection."""
    caps = READ_SETS[name]
    assert expected_rblocks(max(caps), len(caps)) == READ_BLOCKS[name] >= 2
    h = SetHarness(enc, caps, slot=1488, max_segments=1, pad=pad_bytes)
    seen = reads_history(h, np.random.default_rng(11))
    assert seen[0] == 0 and seen[-1] == READ_BLOCKS[name] - 1
    h.finish(slot=4096)
    h.close()


# B. apply and scan with several blocks per connection, unequal members, wrapped
@pytest.mark.gpu
@pytest.mark.parametrize("start", ["zero", "odd", "wrapped"])
def test_scan_runs_at_block_seams(enc, pad_bytes, start):
    assert expected_wblocks(max(UNEQUAL)) == 16 and expected_rblocks(max(UNEQUAL), 3) == 64
    h = SetHarness(enc, UNEQUAL, slot=1488, max_segments=1, pad=pad_bytes)
    scan_runs_history(h, np.random.default_rng(12), start)
    h.finish(slot=4096)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["block0", "block7", "last_word"])
def test_first_uncovered_byte_by_block(enc, pad_bytes, where):
    assert expected_wblocks(max(UNEQUAL)) == 16
    h = SetHarness(enc, UNEQUAL, slot=1488, max_segments=1, pad=pad_bytes)
    first_uncovered_history(h, np.random.default_rng(13), where)
    h.read([h.rules[0].readable + 5, 100, 0], shifts=[7, 1, 0])       # up to the first uncovered byte
    h.finish(slot=4096)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nseg", [49, 50])
def test_gap_limit_counted_by_every_block(enc, pad_bytes, nseg):
    """50 gaps are allowed, 51 end the large member alone."""
    assert expected_wblocks(max(UNEQUAL)) == 16
    h = SetHarness(enc, UNEQUAL, slot=1488, max_segments=1, pad=pad_bytes)
    gap_limit_history(h, np.random.default_rng(14), nseg)
    h.finish(slot=4096)
    h.close()


# C. the ordered pass: unaligned statuses, three slots a packet, later tiles
@pytest.mark.gpu
@pytest.mark.parametrize("status_shift,fatal", [(0, False), (1, False), (8, False), (1, True)])
def test_ordered_pass_unaligned_statuses_three_slots(enc, status_shift, fatal):
    packets, conn_of, rep, ordered, i_f = ordered_batch(np.random.default_rng(15), fatal)
    h = SetHarness(enc, [1 << 19, 1 << 19], slot=64, max_segments=ORD_MS)
    got = h.deliver(packets, conn_of, data_off=lambda i, j: 4 + 12 * j, ordered=ordered, status_shift=status_shift)
    assert h.ordered == ordered and min(ordered) > 0
    last = 33050 if fatal else ORD_NPK
    for c in (0, 1):
        for i in rep[c]:
            k = len(packets[i].segs)
            want = [0] * ORD_MS if (c == 0 and i > last) else [DUPLICATE] * k + [0] * (ORD_MS - k)
            assert got[i].tolist() == want, i
    if fatal:
        a, b = h.rules
        assert got[i_f].tolist() == [sr.OVERLAP, 0, 0] and (a.err, a.err_packet, a.err_segment) == (sr.OVERLAP, i_f, 0)
        assert not got[i_f + 2::2].any()                           # connection 0's later accepts come back as 0
        assert got[35001].tolist() == [DUPLICATE, DUPLICATE, 0] and (got[i_f + 1::2, 0] != 0).all()
        assert b.err == sr.NONE
    h.finish(slot=4096)
    h.close()


# D. many connections in the ordered pass at once
@pytest.mark.gpu
def test_ordered_pass_in_342_of_1024_members(enc, pad_bytes):
    rng = np.random.default_rng(16)
    n = 1024
    h = SetHarness(enc, [4096] * n, slot=128, max_segments=1, pad=pad_bytes)
    lists = []
    for c in range(n):
        p = P(0, _bytes(rng, 40))
        lists.append([p, p] if c % 3 == 0 else [p])
    packets, conn_of = interleave(rng, lists)
    ordered = [2 if c % 3 == 0 else 0 for c in range(n)]
    assert sum(1 for v in ordered if v) == 342 and len(packets) == n + 342
    got = h.deliver(packets, conn_of, ordered=ordered)
    assert sorted(got[:, 0].tolist()) == [ACCEPTED] * n + [DUPLICATE] * 342
    assert all(r.accepted == 1 and r.duplicate == (c % 3 == 0) for c, r in enumerate(h.rules))
    h.finish(slot=1488)
    h.close()


# E. a member across 2^32 beside one at 0
@pytest.mark.gpu
@pytest.mark.parametrize("forced", list(E_TILES))
def test_member_across_2_32_beside_one_at_0(enc, pad_bytes, forced):
    ordered_seen = 0
    for seed in (51, 52):
        rounds, data, meet = crossing_rounds(seed, forced)
        rx0, accepted = _advance(enc, E_CAP, E_BASE)
        rx1 = fec.StreamRx(enc, 4096)
        rx1.window().fill_(SENTINEL)
        rules = [sr.RuleRx.at(E_CAP, E_BASE, sentinel=0, accepted=accepted), sr.RuleRx(4096, SENTINEL)]
        h = SetHarness(enc, [E_CAP, 4096], slot=3008, max_segments=3, pad=pad_bytes, rxs=[rx0, rx1], rules=rules)
        h.check()
        got = run_rounds(h, rounds, seed)
        assert bytes(got[0]) == data[0] and bytes(got[1]) == data[1]
        assert h.rules[0].read_pos == P32 + 4500 and h.rules[1].eof
        assert h.ordered[0] > 0 and h.ordered[1] > 0
        ordered_seen += sum(h.ordered)
        h.finish(seed, slot=MAX_SLOT)
        h.close()
        rx0.close()
        rx1.close()
    assert ordered_seen > 0


# F. lying descriptors through a set
@pytest.mark.gpu
def test_hostile_descriptors_between_another_members_packets(enc):
    batch = hostile_set_batch(np.random.default_rng(91))
    room, pad_room, info, segs, conn_of = batch
    packets = hostile_packets(batch)
    h = SetHarness(enc, [4096, 4096], slot=HOSTILE_SLOT, max_segments=HOSTILE_MS, pad=pad_room)
    got = h.deliver(packets, conn_of, raw=(room, info, segs), pkts_guard=(HOSTILE_FRONT, HOSTILE_BACK),
                    pad_room=pad_room, ordered=[0, 0])
    for i, (p, c) in enumerate(zip(packets, conn_of)):
        k = len(p.segs) if c < 2 else 0
        assert got[i].tolist() == [ACCEPTED] * k + [0] * (HOSTILE_MS - k), i
    # member 1: exactly what it is without the lying packets
    alone = sr.RuleRx(4096, SENTINEL)
    alone.deliver([p for p, c in zip(packets, conn_of) if c == 1])
    b = h.rules[1]
    assert alone.record() == b.record() and np.array_equal(alone.W, b.W) and b.readable == 260
    a = h.rules[0]
    want = b"".join(s.body() for p, c in zip(packets, conn_of) if c == 0 for s in p.segs)
    assert a.readable == len(want) and a.eof == 0 and a.S[3000]
    out = h.read([len(want) + 10, 260], shifts=[5, 9])
    assert out[0][0] == want
    h.finish()
    h.close()


# G. the fold: more than 32,768 members
@pytest.fixture(scope="module")
def fold(enc):
    rxs = [fec.StreamRx(enc, 4096) for _ in range(FOLD_NCONN)]
    yield rxs
    for rx in rxs:
        rx.close()


@pytest.mark.gpu
def test_the_fold_32769_members(enc, pad_bytes, fold):
    """Members 32,768 and above come from blockIdx.z; the last z-slice holds one
    member and 32,767 blocks that leave.  Measured on an MI355X: 1.6 s to create
    the 32,769 windows, 0.5 s for the calls, 0.2 s to destroy the windows."""
    rxs = fold
    rng = np.random.default_rng(17)
    untouched = sr.RuleRx(4096)                # shared by the members that never get a packet
    named, held = [0, 1, 32766, 32767, 32768], [12345, 31999]
    rules = [untouched] * FOLD_NCONN
    for c in named + held:
        rules[c] = sr.RuleRx(4096)             # create zeroes a window
    h = SetHarness(enc, [4096] * FOLD_NCONN, slot=128, max_segments=1, pad=pad_bytes, rxs=rxs, rules=rules)
    try:                                       # the members outlive the set, whatever fails
        assert h.nconn == FOLD_NCONN > 32768 and expected_rblocks(4096, h.nconn) == 1
        zero = h.set.states()
        assert zero.shape == (FOLD_NCONN,) and zero[0]["ngaps"] == 1 and zero[0]["read_pos"] == 0
        assert all(zero[c].tobytes() == zero[0].tobytes() for c in (1, 32767, 32768, FOLD_NCONN - 1))
        others = np.ones(FOLD_NCONN, bool)

        def rest_is_zero(states):
            raw = states.view(np.uint8).reshape(FOLD_NCONN, -1)
            assert (raw[others] == zero[:1].view(np.uint8)).all()

        lists = [[] for _ in range(FOLD_NCONN)]
        for c in named:
            lists[c] = [P(50 * k, _bytes(rng, 50 if k != 5 else 30)) for k in range(8)]     # one gap
            lists[c].insert(4, lists[c][2])                                                 # and one repeat
        packets, conn_of = interleave(rng, lists)
        assert len(packets) == 45
        others[named] = False
        h.deliver(packets, conn_of, members=named)
        after_first = h.set.states()
        rest_is_zero(after_first)
        assert [int(after_first[c]["accepted"]) for c in named] == [8] * 5 and h.ordered[32768] == 2
        assert [int(after_first[c]["readable"]) for c in named] == [280] * 5
        lists = [[] for _ in range(FOLD_NCONN)]
        for c in held:
            lists[c] = [P(70 * k, _bytes(rng, 70)) for k in range(5)]
        packets, conn_of = interleave(rng, lists)
        others[held] = False
        h.deliver(packets, conn_of, members=named + held)
        after_second = h.set.states()
        rest_is_zero(after_second)
        for c in named:                            # no packet in that call: bit for bit
            assert after_second[c].tobytes() == after_first[c].tobytes(), c
        ns = [0] * FOLD_NCONN
        ns[32767], ns[32768] = 100, 300
        out = h.read(ns, shifts=[c % 16 for c in range(FOLD_NCONN)], guard=16, members=named + held)
        assert len(out[32767][0]) == 100 and len(out[32768][0]) == 280
        rest_is_zero(h.set.states())
        h.finish(slot=1488, members=named + held)
        rest_is_zero(h.set.states())
        assert untouched.record() == sr.RuleRx(4096).record() and not untouched.W.any()
    finally:
        h.close()
