"""Write extents of the assembly calls: what they place AND what they leave alone.

Every case runs a call on a batch carved out of one sentinel-filled buffer
with guards on both sides (tests/assembly_image.py) and compares the WHOLE
buffer with the image the per-packet reference path gives: the bytes
include/ugo_fec.h says a call writes -- a placed RX row in
[0, round_up(W, 16)), a TX wire slot in [0, round_up(wire_len, 16)), a
recovered row in [0, shard_size) -- and the sentinel everywhere else: the slack
between a row and its stride, unclaimed rows, the slots of rejected groups, the
rows past max_out and the guards.  An overfill therefore lands in memory the
test owns and is reported as a mismatch at a decoded (group, row, column).

RX: both layouts of rows (ugo_fec_rx_assemble, W = S; _frames, W = S + 6) over
the row widths at which the launcher changes kernel or pass count and over five
storage layouts (assembly_image.rx_layouts).  TX: ugo_fec_tx_assemble over the
chunk counts either side of the per-lane / scalar length loads, with slot_in
!= slot_out.  Host RX: ugo_fec_rx_recover_host's out rows and out_index.
"""
import functools

import numpy as np
import pytest
import torch

import assembly_image as ai
import fec_ref
import rs_ref
from ugo_amd import fec

pytestmark = pytest.mark.gpu

G, FIRST_GROUP = 5, 2
# row widths: both sides of every pass boundary of both kernel families (32 chunks of 16 B per pass,
# 4 passes, then the looping kernels), and round_up(W, 64) - round_up(W, 16) = 0 (512, 1470, ...),
# 16 (40), 32 (17) and 48 (7, 16, 513, 1476, ...)
FRAME_W = [7, 16, 17, 40, 512, 513, 1024, 1025, 1470, 1472, 1476, 1536, 1537, 2048, 2049, 3006]
PAYLOAD_W = [1] + FRAME_W[1:]


_keystream, _crypt = ai.keystream, ai.crypt


@pytest.fixture(scope="module")
def codecs(gpu):
    made = {}

    def get(d, p):
        if (d, p) not in made:
            made[(d, p)] = fec.New(d, p)
        return made[(d, p)]

    yield get
    for c in made.values():
        c.close()


# ---- RX ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rx_wire(d, p, S):
    """The ring of one (code, shard size): decrypted packets, computed once."""
    return tuple(ai.build_rx_ring(d, p, S, G, FIRST_GROUP, 1000 * d + S))


@functools.lru_cache(maxsize=None)
def _rx_reference(d, p, S, frames):
    """The reference placement of that ring (rows at a round_up(W, 16) pitch),
    computed once and shared; nothing writes it."""
    W = S + 6 if frames else S
    want, masks, stats = ai.expected_placement(_rx_wire(d, p, S), G, d + p, S, ai.round_up(W, 16), FIRST_GROUP, frames)
    want.setflags(write=False)
    masks.setflags(write=False)
    return want, masks, tuple(stats)


_dev_rings = {}


def _device_ring(wire, slot):
    """(ring, lens, pad) on the device for a tuple of decrypted packets."""
    key = (id(wire), slot)
    if key not in _dev_rings:
        slots, lens = ai.ring([_crypt(w) for w in wire], slot)
        pad = torch.from_numpy(_keystream()[:slot].copy()).cuda()
        _dev_rings[key] = (wire, torch.from_numpy(slots).cuda(), torch.from_numpy(lens.view(np.int16)).cuda(), pad)
    return _dev_rings[key][1:]


def _rx_call(codec, wire, slot, img, present, S, frames):
    ring, lens, pad = _device_ring(wire, slot)
    st = torch.zeros(5, dtype=torch.int32, device="cuda")
    codec.rx_assemble(ring, lens, img.batch, present, first_group=FIRST_GROUP, shard_size=S, pad=pad, stats=st,
                      shard_major=img.layout.planar, frames=frames)
    torch.cuda.synchronize()
    return st.cpu().tolist()


def _rx_extent_case(codecs, d, p, W, layout, frames):
    n, S = d + p, (W - 6 if frames else W)
    slot = ai.round_up(S + 6, 16)
    wire = _rx_wire(d, p, S)
    want, masks, stats = _rx_reference(d, p, S, frames)
    L = ai.rx_layouts(W, n, G)[layout]
    img = ai.Image(L)
    present = torch.zeros(G, dtype=torch.int64, device="cuda")
    got_stats = _rx_call(codecs(d, p), wire, slot, img, present, S, frames)
    what = "%s W=%d layout %d (%s)" % ("frames" if frames else "payload", W, layout, L.name)
    assert got_stats == list(stats), what
    assert np.array_equal(present.cpu().numpy().view(np.uint64), masks), what
    img.check(img.expected(want, masks), what)


def _rx_params():
    out = []
    for frames, widths in ((False, PAYLOAD_W), (True, FRAME_W)):
        for W in widths:
            for layout in (1, 2, 3, 4, 5):
                out.append(pytest.param(W, layout, frames,
                                        id="%s-W%d-layout%d" % ("frames" if frames else "payload", W, layout)))
    return out


@pytest.mark.parametrize("W,layout,frames", _rx_params())
def test_rx_assemble_whole_buffer(codecs, W, layout, frames):
    """(10,3): placed rows written in [0, round_up(W, 16)) and nowhere else, in
    every layout, at every row width where the launcher changes kernel or pass
    count; masks and stats equal the reference's."""
    _rx_extent_case(codecs, 10, 3, W, layout, frames)


@pytest.mark.parametrize("frames", [False, True], ids=["payload", "frames"])
@pytest.mark.parametrize("S,layout", [(1470, 2), (507, 4)])
def test_rx_assemble_whole_buffer_code_3_2(codecs, S, layout, frames):
    """The same with n = 5 rows per group (the kernels depend on n only)."""
    _rx_extent_case(codecs, 3, 2, S + 6 if frames else S, layout, frames)


@pytest.mark.parametrize("frames", [False, True], ids=["payload", "frames"])
@pytest.mark.parametrize("layout", [2, 4])
def test_rx_assemble_second_call_duplicates_write_nothing(codecs, layout, frames):
    """Three calls into one batch.  The second call's ring holds only copies --
    other lengths, other payloads -- of seqids the first call placed: the whole
    buffer stays byte for byte what the first call left.  The third mixes new
    packets with such copies."""
    d, p, n, S = 10, 3, 13, 1470
    W = S + 6 if frames else S
    slot = ai.round_up(S + 6, 16)
    stream = _rx_wire(d, p, S)
    cut = len(stream) // 2
    first, rest = tuple(stream[:cut]), stream[cut:]
    rng = np.random.default_rng(5)
    _, m1, _ = ai.expected_placement(first, G, n, S, ai.round_up(W, 16), FIRST_GROUP, frames)
    placed = [(FIRST_GROUP + g) * n + r for g in range(G) for r in range(n) if (int(m1[g]) >> r) & 1]
    copies = tuple(ai.packet(rng, s, 0xF1 if s % n < d else 0xF2, int(rng.integers(6, S + 7)))
                   for s in placed for _ in range(2))
    third = tuple(list(rest) + [ai.packet(rng, s, 0xF1 if s % n < d else 0xF2, S + 6) for s in placed[::3]])
    third = tuple(third[i] for i in rng.permutation(len(third)))
    w16 = ai.round_up(W, 16)

    def ref(wire):
        return ai.expected_placement(wire, G, n, S, w16, FIRST_GROUP, frames)

    L = ai.rx_layouts(W, n, G)[layout]
    img = ai.Image(L)
    present = torch.zeros(G, dtype=torch.int64, device="cuda")
    codec = codecs(d, p)
    what = "%s layout %d" % ("frames" if frames else "payload", layout)
    want1, masks1, stats1 = ref(first)
    assert _rx_call(codec, first, slot, img, present, S, frames) == stats1
    image1 = img.expected(want1, masks1)
    img.check(image1, what + " call 1")
    assert _rx_call(codec, copies, slot, img, present, S, frames) == [0, 0, 0, 0, len(copies)]
    assert np.array_equal(present.cpu().numpy().view(np.uint64), masks1)
    img.check(image1, what + " call 2 (duplicates only)")
    want3, masks3, stats3 = ref(first + copies + third)
    _, _, stats2 = ref(first + copies)
    assert masks3.tolist() != masks1.tolist()
    assert _rx_call(codec, third, slot, img, present, S, frames) == [a - b for a, b in zip(stats3, stats2)]
    assert np.array_equal(present.cpu().numpy().view(np.uint64), masks3)
    img.check(img.expected(want3, masks3), what + " call 3")


# ---- TX ----------------------------------------------------------------------
TX_KINDS = ("over", "under", "header_only", "short_longest", "full")
TX_SLOTS = [(0, 0), (0, 16), (0, 48), (32, 0), (32, 16), (32, 48)]  # (slot_in, slot_out) - need


def _tx_params():
    """codes x max_len x G x pad.  A batch of 7 groups holds every kind of
    group: one with a length above max_len, one with a length below 6, one
    all-header-only, one whose longest packet is well short of max_len, one
    reaching max_len and two random ones.  Batches of 3 and 1 groups cannot
    hold them all: they take 3 (1) consecutive kinds of the cycle TX_KINDS,
    starting one further on with each case, so every kind is met at every G,
    code and max_len boundary.  The slot paddings rotate through TX_SLOTS:
    slot_in != slot_out in 5 cases of 6."""
    out, i, turn = [], 0, {1: 0, 3: 0, 7: 0}
    for d, p in ((10, 3), (5, 3), (32, 8)):
        for max_len in (6, 22, 500, 1008, 1009, 1024, 1025, 1476):
            for groups in (1, 3, 7):
                for pad in (True, False):
                    t = turn[groups]
                    turn[groups] += 1
                    if groups == 7:
                        kinds = ("random", "over", "full", "header_only", "short_longest", "under", "random")
                    else:
                        kinds = tuple(TX_KINDS[(t + k) % 5] for k in range(groups))
                    add_in, add_out = TX_SLOTS[(i + i // 6) % 6]
                    i += 1
                    out.append(pytest.param(d, p, max_len, groups, pad, add_in, add_out, kinds,
                                            id="%d+%d-len%d-G%d-%s-in+%d-out+%d" % (
                                                d, p, max_len, groups, "pad" if pad else "plain", add_in, add_out)))
    return out


def _tx_lengths(rng, kind, d, max_len):
    lens = rng.integers(6, max_len + 1, d)
    k = int(rng.integers(0, d))
    if kind == "full":
        lens[k] = max_len
    elif kind == "header_only":
        lens[:] = 6
    elif kind == "short_longest":  # the parity packets end chunks before max_len
        lens = rng.integers(6, max(6, max_len // 2) + 1, d)
    elif kind == "over":
        lens[k] = max_len + 1
    elif kind == "under":
        lens[k] = int(rng.integers(0, 6))
    return lens


@pytest.mark.parametrize("d,p,max_len,groups,pad,add_in,add_out,kinds", _tx_params())
def test_tx_assemble_whole_wire_buffer(codecs, d, p, max_len, groups, pad, add_in, add_out, kinds):
    """ugo_fec_tx_assemble: a wire slot is written in [0, round_up(wire_len, 16))
    only, zeros in [wire_len, round_up(wire_len, 16)); a slot whose wire_len
    comes back 0 (a bad-length group, the parity of a header-only group) is not
    written; pkts and lens are only read.  Expected packets: fec_ref.tx_group."""
    n = d + p
    need = ai.round_up(max_len, 16)
    slot_in, slot_out = need + add_in, need + add_out
    rng = np.random.default_rng(max_len * 1000 + d * 10 + groups + (5 if pad else 0))
    lens = np.concatenate([_tx_lengths(rng, k, d, max_len) for k in kinds]).astype(np.uint16)
    host = rng.integers(0, 256, (groups * d, slot_in), dtype=np.uint8)  # random past each length too
    first_seq = 26 * n
    # expected: the sender loop per group
    wire = ai.SlotImage(groups * n, slot_out)
    want = wire.blank()
    want_wl = np.zeros(groups * n, np.uint16)
    want_st = np.zeros(groups, np.int8)
    tx = fec_ref.FEC.new(128, d, p, clock=lambda: 0)
    for g in range(groups):
        gl = lens[g * d:(g + 1) * d]
        if (gl < 6).any() or (gl > max_len).any():
            want_st[g] = fec.ErrShardSize.code
            continue
        tx.next = first_seq + g * n  # the batch spends n seqids on every group (include/ugo_fec.h)
        out = fec_ref.tx_group(tx, [host[g * d + k, :gl[k]].tobytes() for k in range(d)], None)
        if len(out) == d:
            assert (gl == 6).all()
            want_st[g] = fec.ErrShardNoData.code
        for r, w in enumerate(out):
            w = _crypt(w) if pad else w
            wire.put(want, g * n + r, w)
            want_wl[g * n + r] = len(w)
    dp = torch.from_numpy(host).cuda()
    dl = torch.from_numpy(lens.view(np.int16)).cuda()
    dp0, dl0 = dp.clone(), dl.clone()
    # the lengths and statuses between guards of their own
    wl_all = torch.full((groups * n + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
    st_all = torch.full((groups + 64,), -7, dtype=torch.int8, device="cuda")
    dpad = torch.from_numpy(_keystream()[:need].copy()).cuda() if pad else None
    codecs(d, p).tx_assemble(dp, dl, wire.view, wl_all[32:32 + groups * n], first_seq=first_seq, pad=dpad,
                             max_len=max_len, status=st_all[32:32 + groups])
    torch.cuda.synchronize()
    what = "(%d,%d) max_len %d G %d slots %d -> %d kinds %s" % (d, p, max_len, groups, slot_in, slot_out, kinds)
    wl = wl_all.cpu().numpy().view(np.uint16)
    st = st_all.cpu().numpy()
    assert np.array_equal(wl[32:32 + groups * n], want_wl), what
    assert (wl[:32] == 0x5A5A).all() and (wl[32 + groups * n:] == 0x5A5A).all(), what
    assert np.array_equal(st[32:32 + groups], want_st), what
    assert (st[:32] == -7).all() and (st[32 + groups:] == -7).all(), what
    wire.check(want, what)
    assert torch.equal(dp, dp0) and torch.equal(dl, dl0), what


# ---- host RX: the output rows ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _recover_case():
    """A (10,3) ring of 40 groups, S = 1470, ~14 % loss (some groups past
    recovery), repeated packets, shuffled; the oracle's recovered shards in
    ugo's `recovered` order."""
    d, p, n, S, groups = 10, 3, 13, 1470, 40
    rng = np.random.default_rng(404)
    wire = []
    for g in range(groups):
        for r in range(n):
            if rng.random() < 0.14:
                continue
            w = ai.packet(rng, g * n + r, 0xF1 if r < d else 0xF2, int(rng.integers(6, S + 7)))
            wire.append(w)
            if rng.random() < 0.05:
                wire.append(w)
    wire = [wire[i] for i in rng.permutation(len(wire))]
    want, masks, stats = ai.expected_placement(wire, groups, n, S, 1472, 0)
    exp = np.ascontiguousarray(want[:, :, :S])
    _, exp_st = rs_ref.c_reconstruct(d, p, exp, masks, data_only=True)
    rec = [(g, r) for g in range(groups) if exp_st[g] == 0 for r in range(d) if not (int(masks[g]) >> r) & 1]
    lossy = [g for g in range(groups) if (~int(masks[g])) & ((1 << d) - 1)]
    assert any(exp_st[g] != 0 for g in lossy), "the case should hold an unrecoverable lossy group"
    assert len(rec) >= 8
    exp.setflags(write=False)
    return tuple(_crypt(w) for w in wire), exp, masks, stats, rec


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("stride", [1470, 1488], ids=["stride-S", "stride-padded"])
def test_rx_recover_host_output_extents(codecs, stride, pinned):
    """More recovered rows than max_out, out rows at a stride of S and of
    round_up(S, 16) + 16: rows below max_out hold the oracle's shard in [0, S);
    every other byte of out -- the row tails, the rows at or past max_out --
    and every out_index entry past max_out keep the caller's bytes."""
    d, p, n, S, groups, slot = 10, 3, 13, 1470, 40, 1488
    assert stride in (S, ai.round_up(S, 16) + 16)
    enc, exp, masks, stats, rec = _recover_case()
    max_out = len(rec) // 2
    rows, nidx = max_out + 3, max_out + 5
    npk = len(enc)
    bufs = []

    def buf(nbytes):
        if not pinned:
            return np.zeros(nbytes, np.uint8)
        a = fec.host_alloc(nbytes)
        bufs.append(a)
        return a

    try:
        slots = buf(npk * slot).reshape(npk, slot)
        lens = buf(npk * 2).view(np.uint16)
        slots[:] = 0
        for i, w in enumerate(enc):
            slots[i, :len(w)] = np.frombuffer(w, np.uint8)
            lens[i] = len(w)
        out = buf(rows * stride).reshape(rows, stride)
        out[:] = ai.SENTINEL
        index = buf(nidx * 4).view(np.uint32)
        index[:] = 0xA5A5A5A5
        pres = np.zeros(groups, np.uint64)
        nrec, got_index, got_out, got_stats = codecs(d, p).rx_recover_host(
            slots, lens, S, groups, pad=_keystream()[:slot].tobytes(), out=out, max_out=max_out, present_out=pres,
            out_index=index)
        assert got_index is index and got_out is out
        assert nrec == len(rec) and nrec > max_out
        assert np.array_equal(pres, masks) and got_stats.tolist() == stats
        assert index[:max_out].tolist() == [g * n + r for g, r in rec[:max_out]]
        assert (index[max_out:] == 0xA5A5A5A5).all()
        want = np.full((rows, stride), ai.SENTINEL, np.uint8)
        for j, (g, r) in enumerate(rec[:max_out]):
            want[j, :S] = exp[g, r]
        ai.check_equal(out.reshape(-1), want.reshape(-1), lambda o: ("out row", o // stride, o % stride),
                       "stride %d %s" % (stride, "pinned" if pinned else "pageable"))
    finally:
        for a in bufs:
            fec.host_free(a)
