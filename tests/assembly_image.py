"""Whole-storage images for the RX / TX assembly calls; test infrastructure only.

The assembly tests compare what a kernel places with the per-packet reference
path; this module also pins what a kernel leaves alone.  A batch is carved out
of ONE flat device buffer, sentinel-filled, with a guard on either side in the
same allocation:

    | guard >= 256 B | extent(round_up(W,16), row_stride, n, group_stride, G) B | guard >= 256 B |

so a kernel that writes past what include/ugo_fec.h allows -- into a row's
slack behind round_up(W, 16), into a neighbouring slot, or behind the batch's
last row -- lands in memory the test owns and shows up as a mismatch, never as
a fault.  The expected image of the entire buffer is built on the CPU from the
reference placement: a placed row holds its W bytes, then zeros to
round_up(W, 16); every other byte, guards included, is the sentinel.
"""
import functools

import numpy as np

import rc4_ref

SENTINEL = 0xA5
GUARD = 256
KEY = b"1234567890123456"  # ugo/listener.go:92, ugo/dial.go:132


@functools.lru_cache(maxsize=None)
def keystream():
    """The fixed key's RC4 keystream (oracle/rc4_ref.py), computed once."""
    return np.frombuffer(rc4_ref.keystream(KEY, 3072), np.uint8)


def crypt(w):
    """crypt.Encrypt / Decrypt of one packet of at most 3072 bytes: XOR with the
    fixed-key keystream, i.e. rc4_ref.xor_stream(KEY, w)."""
    return (np.frombuffer(w, np.uint8) ^ keystream()[:len(w)]).tobytes()


def round_up(v, a):
    return (v + a - 1) // a * a


def extent(width, row_stride, n, group_stride, G):
    """Bytes from the first byte of row 0 of group 0 to the last byte of the
    furthest row slot of `width` bytes."""
    return (n - 1) * row_stride + (G - 1) * group_stride + width


def expected_placement(wire, G, n, S, pitch, first_group, frames=False):
    """The batch ugo's per-packet path builds from `wire` in ring order
    (decrypted packets): FEC.decode (ugo/fec.go:78-89), the flag filter of
    Conn.handlePacket (ugo/conn.go:395), the group/slot of input
    (ugo/fec.go:145,175), and its dedupe -- a seqid already queued drops the
    new packet, so the first copy stays (ugo/fec.go:123-129).  Returns the
    group-major batch, presence masks and stats [accepted, bad flag, out of
    window, too short, duplicate].  frames: a row holds the decrypted packet's
    first S + 6 bytes (ugo_fec_rx_assemble_frames: header, then the payload
    at column 6) instead of its payload."""
    want = np.zeros((G, n, pitch), np.uint8)
    masks = np.zeros(G, np.uint64)
    stats = [0, 0, 0, 0, 0]
    seen = set()
    for w in wire:
        if len(w) < 6:
            stats[3] += 1
            continue
        seq = int.from_bytes(w[:4], "little")
        flag = int.from_bytes(w[4:6], "little")
        if flag not in (0xF1, 0xF2):
            stats[1] += 1
            continue
        g = seq // n - first_group
        if not 0 <= g < G:
            stats[2] += 1
            continue
        if seq in seen:
            stats[4] += 1
            continue
        seen.add(seq)
        stats[0] += 1
        pl = w[:S + 6] if frames else w[6:6 + S]
        want[g, seq % n, :] = 0
        want[g, seq % n, :len(pl)] = np.frombuffer(pl, np.uint8)
        masks[g] |= np.uint64(1 << (seq % n))
    return want, masks, stats


def ring(wire, slot):
    """Packets -> (slots uint8 [npk, slot], lens uint16 [npk])."""
    npk = len(wire)
    slots = np.zeros((npk, slot), np.uint8)
    lens = np.zeros(npk, np.uint16)
    for i, w in enumerate(wire):
        slots[i, :len(w)] = np.frombuffer(w, np.uint8)
        lens[i] = len(w)
    return slots, lens


def packet(rng, seq, flag, L):
    """A decrypted wire packet of L >= 6 bytes: header, then random payload."""
    b = bytearray(rng.integers(0, 256, L, dtype=np.uint8).tobytes())
    b[0:4] = int(seq).to_bytes(4, "little")
    b[4:6] = int(flag).to_bytes(2, "little")
    return bytes(b)


def build_rx_ring(d, p, S, G, first_group, seed):
    """A small received ring (decrypted packets, arrival order shuffled) for the
    window [first_group, first_group + G) of a (d, p) code with shard size S:
    about 80 % of the (group, row) pairs present with lengths drawn from
    [6, S + 6], some of them repeated with another payload, and at least one
    full-length packet, one header-only packet, one repeated seqid whose second
    copy in ring order is longer and different, one bad-flag packet (aimed at a
    row nothing else claims), out-of-window packets either side of the window
    and two short packets."""
    n = d + p
    rng = np.random.default_rng(seed)
    pairs = [(g, r) for g in range(G) for r in range(n)]
    here = rng.random(len(pairs)) < 0.8
    order = rng.permutation(len(pairs))
    full, honly, twice, bad = (int(order[k]) for k in range(4))
    here[[full, honly, twice]] = True
    here[bad] = False

    def seq_of(k):
        g, r = pairs[k]
        return (first_group + g) * n + r, (0xF1 if r < d else 0xF2)

    wire = []
    for k in range(len(pairs)):
        if not here[k] or k == twice:
            continue
        seq, flag = seq_of(k)
        L = S + 6 if k == full else 6 if k == honly else int(rng.integers(6, S + 7))
        wire.append(packet(rng, seq, flag, L))
        if k not in (full, honly) and rng.random() < 0.15:  # a later (or earlier) copy, another payload
            wire.append(packet(rng, seq, flag, int(rng.integers(6, S + 7))))
    seq, _ = seq_of(bad)
    wire.append(packet(rng, seq, 0x77, int(rng.integers(6, S + 7))))
    for g in (first_group - 1, first_group + G):
        for r in range(n):
            if rng.random() < 0.5 or r == 0:
                wire.append(packet(rng, g * n + r, 0xF1 if r < d else 0xF2, int(rng.integers(6, S + 7))))
    wire.append(b"\x01\x02\x03")
    wire.append(packet(rng, seq_of(full)[0], 0xF1, 6)[:5])
    wire = [wire[i] for i in rng.permutation(len(wire))]
    # the repeated seqid: the first copy in ring order shorter than the second
    seq, flag = seq_of(twice)
    L1 = int(rng.integers(6, S + 6))
    L2 = int(rng.integers(L1 + 1, S + 7))
    i1, i2 = sorted(int(x) for x in rng.choice(len(wire) + 1, 2, replace=False))
    wire.insert(i1, packet(rng, seq, flag, L1))
    wire.insert(i2 + 1, packet(rng, seq, flag, L2))
    return wire


class Layout:
    """Where the rows of a batch of G groups x n rows of W bytes sit: row r of
    group g at base + r*row_stride + g*group_stride, base at `residue` modulo
    64.  planar: the batch is passed as [n][G][w16] (shard-major), else as
    [G][n][w16] (group-major); w16 = round_up(W, 16) is the width of the view
    whatever the strides -- a wider pitch is a narrowed view of its storage."""

    def __init__(self, name, W, n, G, row_stride, group_stride, planar=True, residue=0):
        self.name, self.W, self.n, self.G = name, W, n, G
        self.w16 = round_up(W, 16)
        self.row_stride, self.group_stride = row_stride, group_stride
        self.planar, self.residue = planar, residue
        self.extent = extent(self.w16, row_stride, n, group_stride, G)
        assert row_stride % 16 == 0 and group_stride % 16 == 0 and residue % 16 == 0 and 0 <= residue < 64
        starts = sorted(r * row_stride + g * group_stride for g in range(G) for r in range(n))
        assert all(b - a >= self.w16 for a, b in zip(starts, starts[1:])), "row slots overlap"

    def start(self, g, r):
        return r * self.row_stride + g * self.group_stride


def rx_layouts(W, n, G):
    """The five layouts of tests/test_assembly_extents.py, by number."""
    w16, w64 = round_up(W, 16), round_up(W, 64)
    rs = w16 + 16
    return {
        1: Layout("planar-dense", W, n, G, G * w16, w16),
        2: Layout("planar-pitch64-narrowed", W, n, G, G * w64, w64),
        3: Layout("planar-pitch64+64-narrowed", W, n, G, G * (w64 + 64), w64 + 64),
        4: Layout("group-major-padded", W, n, G, rs, n * rs + 32, planar=False),
        5: Layout("planar-pitch64-base+16", W, n, G, G * w64, w64, residue=16),
    }


class Image:
    """The flat buffer of one batch (module docstring).  `flat` is the device
    buffer, `batch` the strided view to pass to the call, `base` the offset of
    the batch's first byte in `flat`.  Device work needs torch; `expected` and
    `decode` do not (device=None builds no buffer)."""

    def __init__(self, layout, device="cuda"):
        self.layout = L = layout
        self.flat = self.batch = None
        self.base = GUARD
        if device is not None:
            import torch

            self.flat = torch.full((GUARD + 64 + L.extent + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
            self.base = GUARD + (L.residue - (self.flat.data_ptr() + GUARD)) % 64
            if L.planar:
                size, stride = (L.n, L.G, L.w16), (L.row_stride, L.group_stride, 1)
            else:
                size, stride = (L.G, L.n, L.w16), (L.group_stride, L.row_stride, 1)
            self.batch = torch.as_strided(self.flat, size, stride, self.base)
            assert self.batch.data_ptr() % 64 == L.residue
        self.size = self.base + L.extent + GUARD
        if self.flat is not None:
            self.flat = self.flat[:self.size]  # both guards at least GUARD bytes, the tail one exactly

    def expected(self, want, masks, sentinel=SENTINEL):
        """The whole buffer after the placement (want [G][n][>= w16], masks) of
        expected_placement: placed rows in [0, w16), the sentinel elsewhere."""
        L = self.layout
        img = np.full(self.size, sentinel, np.uint8)
        for g in range(L.G):
            for r in range(L.n):
                if (int(masks[g]) >> r) & 1:
                    o = self.base + L.start(g, r)
                    img[o:o + L.w16] = want[g, r, :L.w16]
        return img

    def rows(self, img):
        """The (G, n, w16) rows of a whole-buffer image (a copy)."""
        L = self.layout
        out = np.empty((L.G, L.n, L.w16), np.uint8)
        for g in range(L.G):
            for r in range(L.n):
                o = self.base + L.start(g, r)
                out[g, r] = img[o:o + L.w16]
        return out

    def decode(self, off):
        """Where byte `off` of the buffer lies: "guard", or (group, row, column)
        of the row slot it belongs to (the nearest slot starting at or before
        it; a column at or past w16 is the slack behind that row)."""
        L = self.layout
        rel = off - self.base
        if rel < 0 or rel >= L.extent:
            return "guard"
        best = None
        for g in range(L.G):
            for r in range(L.n):
                s = L.start(g, r)
                if s <= rel and (best is None or s > best[0]):
                    best = (s, g, r)
        return (best[1], best[2], rel - best[0])

    def got(self):
        return self.flat.cpu().numpy()

    def check(self, want_img, what=""):
        """Whole-buffer equality; the first differing offset decoded."""
        check_equal(self.got(), want_img, self.decode, what)


def check_equal(got, want, decode, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    if np.array_equal(got, want):
        return
    diff = np.flatnonzero(got != want)
    off = int(diff[0])
    where = decode(off)
    kind = "guard" if where == "guard" else "(group, row, column) = %r" % (where,)
    raise AssertionError(
        "%s: %d bytes differ, first at buffer offset %d, %s: got 0x%02x, want 0x%02x (last differing offset %d, %s)"
        % (what, diff.size, off, kind, got[off], want[off], int(diff[-1]), decode(int(diff[-1]))))


class SlotImage:
    """The same for an array of `count` slots of `slot` bytes (the TX wire
    buffer): a contiguous [count, slot] view between two guards."""

    def __init__(self, count, slot, device="cuda"):
        import torch

        self.count, self.slot, self.base = count, slot, GUARD
        self.size = GUARD + count * slot + GUARD
        self.flat = torch.full((self.size,), SENTINEL, dtype=torch.uint8, device=device)
        self.view = self.flat[GUARD:GUARD + count * slot].view(count, slot)

    def blank(self):
        return np.full(self.size, SENTINEL, np.uint8)

    def put(self, img, i, data, pad_to=16):
        """Slot i of the expected image: `data`, then zeros to round_up(len, pad_to)."""
        o = self.base + i * self.slot
        w = round_up(len(data), pad_to)
        assert w <= self.slot
        img[o:o + w] = 0
        img[o:o + len(data)] = np.frombuffer(bytes(data), np.uint8)

    def decode(self, off):
        rel = off - self.base
        if rel < 0 or rel >= self.count * self.slot:
            return "guard"
        return ("slot", rel // self.slot, rel % self.slot)

    def check(self, want_img, what=""):
        check_equal(self.flat.cpu().numpy(), want_img, self.decode, what)
