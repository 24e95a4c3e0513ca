"""ugo_fec_packet_decode against the directed corpus of tests/packet_vectors.py,
through the whole-output image: every byte of info, ranges and segs that
include/ugo_pkt.h specifies equals oracle/packet_ref.py's, every byte it says
the call leaves alone -- entries past the counts, other packets' rows, the
guards round the arrays -- still holds the caller's 0xA5.  Bit-exact, no
tolerances.

Beyond the corpus: the bytes of a slot past lens[i] (a reused ring slot holds
the tail of an older packet there) must not change a single output byte;
every ufloat16 and every short string over a small alphabet; slots of 0xfff0
with lens above 32767 (negative as the binding's int16) and above the slot;
batch sizes round the 256-thread block; pinned host memory; the argument
checks.
"""
import numpy as np
import pytest
import torch

import packet_vectors as pv
from ugo_amd import fec

INVALID_ARG = fec.ErrInvalidArg.code
CAPS = [(32, 8), (2, 1), (256, 8), (0, 0)]


@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(10, 3)


def _round16(v):
    return (v + 15) & ~15


def _i16(lens):
    return torch.from_numpy(np.ascontiguousarray(lens, np.uint16).view(np.int16))


def _decode(enc, packets, R, S, slot=None, framed=False, encrypt=False, lens=None, **slack):
    """One call over `packets` in a fresh image; returns (image, what it holds)."""
    slot = slot or max(16, _round16(max(len(b) for b in packets)))
    slots, ln = pv.ring(packets, slot, encrypt=encrypt, **slack)
    pad = torch.from_numpy(pv.keystream(slot).copy()).cuda() if encrypt else None
    im = pv.DecodeImage(len(packets), R, S)
    enc.packet_decode(torch.from_numpy(slots).cuda(), _i16(ln if lens is None else lens).cuda(), pad=pad, framed=framed,
                      max_ranges=R, max_segments=S, out=im.out)
    torch.cuda.synchronize()
    return im, im.got()


def _corpus(framed):
    """Every directed vector and every prefix of one.  Framed, the corpus is
    taken twice, the flag rotation two on the second time, so that each vector
    meets a typeData header (stripped) and another flag (decoded from byte 0)."""
    pk = [full[:cut] for _, full, cut in pv.with_prefixes()]
    return pv.frame_both(pk) if framed else pk


# ------------------------------------------------------------------- corpus
@pytest.mark.gpu
@pytest.mark.parametrize("encrypt", [False, True], ids=["plain", "rc4"])
@pytest.mark.parametrize("framed", [False, True], ids=["unframed", "framed"])
@pytest.mark.parametrize("caps", CAPS, ids=lambda c: "caps%d-%d" % c)
def test_directed_corpus_image(enc, caps, framed, encrypt):
    R, S = caps
    pk = _corpus(framed)
    im, got = _decode(enc, pk, R, S, framed=framed, encrypt=encrypt)
    want, mask = im.expected(pk, framed)
    im.check(got, want, mask, "caps %r framed %r rc4 %r" % (caps, framed, encrypt), pk)
    codes = set(im.info(got)["status"].tolist())
    assert codes == {0, 1, 2, 3, 4, 5, 6}, codes
    if not framed:
        assert max(len(b) for b in pk) == 528  # lens[i] == slot is in the batch


# ---------------------------------------------------------------- stale ring
@pytest.mark.gpu
@pytest.mark.parametrize("encrypt", [False, True], ids=["plain", "rc4"])
@pytest.mark.parametrize("framed", [False, True], ids=["unframed", "framed"])
def test_stale_ring_bytes_change_nothing(enc, framed, encrypt):
    """The same packets over slots whose slack holds zeros, the rest of the
    longer packet each one is a prefix of (truncation is only a smaller
    lens[i]), 0xff, 0x80 -- a continuation byte: a varint reader that looks
    past the end keeps going --, the rest and then 0x80, and random bytes.  Every
    output byte is the same in all six, specified or not, and what is specified
    is the oracle's."""
    fulls = [full for _, full, _ in pv.with_prefixes()]
    cuts = [cut for _, _, cut in pv.with_prefixes()]
    if framed:
        fulls = pv.frame_both(fulls)
        cuts = [c + 6 for c in cuts + cuts]
        # shorter than the FEC header, with `f1 00` left in bytes 4..5 of the slot:
        # not framed, payload_off 0, fec_flag_lo 0
        stale = b"\x00\x00\x00\x00\xf1\x00" + b"\x20\x01\x05\x00\x02\xaa\xbb"
        fulls += [stale] * 6
        cuts += list(range(6))
    pk = [f[:c] for f, c in zip(fulls, cuts)]
    rng = np.random.default_rng(7)
    first = None
    for name, slack in [("zeros", dict(slack=0)), ("rest", dict(slack=0, fulls=fulls)), ("ff", dict(slack=0xFF)),
                        ("80", dict(slack=0x80)), ("rest, then 80", dict(slack=0x80, fulls=fulls)),
                        ("random", dict(slack="random", rng=rng))]:
        im, got = _decode(enc, pk, 32, 8, slot=_round16(max(len(f) for f in fulls)) + 16, framed=framed,
                          encrypt=encrypt, **slack)
        if first is None:
            first = got
            want, mask = im.expected(pk, framed)
        im.check(got, want, mask, "slack %s" % name, pk)
        im.check(got, first, np.ones_like(mask), "slack %s against slack zeros" % name, pk)
    if framed:
        tail = im.info(first)[-6:]
        assert not tail["payload_off"].any() and not tail["fec_flag_lo"].any()


# ---------------------------------------------------------------- exhaustive
@pytest.mark.gpu
def test_every_ufloat16(enc):
    pk = [b for _, b in pv.ufloat16_vectors()]
    im, got = _decode(enc, pk, 2, 2)
    want, mask = im.expected(pk)
    assert mask.all() and not im.info(want)["status"].any()
    im.check(got, want, mask, "ufloat16", pk)
    assert im.info(got)["delay_us"][0xFFFF] == 0x3FFC0000000


@pytest.mark.gpu
def test_every_short_string_over_the_small_alphabet(enc):
    pk = [b for _, b in pv.small_alphabet_vectors()]
    assert len(pk) == 66430
    im, got = _decode(enc, pk, 2, 2, slot=16, slack=0x80)
    want, mask = im.expected(pk)
    im.check(got, want, mask, "small alphabet", pk)
    assert np.bincount(im.info(got)["status"]).tolist() == [3552, 42313, 20565]


# ----------------------------------------------------------------- oversized
@pytest.mark.gpu
@pytest.mark.parametrize("S", [pv.MANY_SEGMENTS, pv.MANY_SEGMENTS - 1], ids=["fits", "one-over"])
def test_slot_fff0(enc, S):
    """lens above 32767, lens == slot == 0xfff0, and 21,839 segments in one
    packet against a cap that holds them all and one that does not."""
    many, big = (b for _, b in pv.oversized_vectors())
    whole = b"\x20\x01\x00" + (65515).to_bytes(2, "big") + bytes(range(256)) * 255 + bytes(235)
    assert len(whole) == 0xFFF0
    pk = [b"\x20\x07", many, big, many[:-1], whole, many[:-3], b"\x80\x20\x14\x00\x00\x02\x02\x01\x02\x01\x01"]
    im, got = _decode(enc, pk, 2, S, slot=0xFFF0, slack=0x80)
    want, mask = im.expected(pk)
    im.check(got, want, mask, "slot 0xfff0, max_segments %d" % S)
    info = im.info(got)
    assert info["status"].tolist() == [0, 0 if S == pv.MANY_SEGMENTS else 6, 0, 2, 0, 0, 6]
    assert info["n_segments"][[1, 2, 4, 5]].tolist() == [S, 1, 1, pv.MANY_SEGMENTS - 1]
    assert im.segs(got)[2, 0].tolist() == (0, 10, 39990, 39990) and im.segs(got)[4, 0].tolist() == (0, 5, 65515, 65515)


@pytest.mark.gpu
def test_lens_above_slot_reads_as_slot(enc):
    rng = np.random.default_rng(11)
    body = [b"\x20\x01\x00\x00\x3b" + bytes(59),                 # exactly the slot
            b"\x20\x01\x00\x01\x00" + bytes(59),                 # declares 256 bytes, 59 present
            b"\x20\x01" + b"\x01\x00\x00" * 18 + b"\x80" * 8,   # an offset still continuing at the end of the slot
            b"\x20\x01" + b"\x01\x00\x00" * 20 + b"\x01\x00",    # half a BE16 at the end of the slot
            rng.integers(0, 256, 64, dtype=np.uint8).tobytes()]
    assert all(len(b) == 64 for b in body)
    lens = np.array([65, 100, 0x7FFF, 0x8000, 0xFFFF], np.uint16)
    im, got = _decode(enc, body, 4, 24, slot=64, lens=lens)
    want, mask = im.expected(body)
    im.check(got, want, mask, "lens > slot", body)
    # the last two end inside a field: status 2 only if the read stops at the slot
    assert im.info(got)["status"][:4].tolist() == [0, 0, 2, 2]
    assert im.segs(got)[1, 0].tolist() == (0, 5, 256, 59)


# --------------------------------------------------------------- batch shape
@pytest.mark.gpu
@pytest.mark.parametrize("npk", [1, 255, 256, 257, 513])
def test_batch_sizes_round_the_block(enc, npk):
    """Pairwise distinct packets, so a slipped index shows in the image."""
    pk = []
    for i in range(npk):
        if i % 3 == 2:  # a SACK with two ranges under largest 1000 + i
            pk.append(b"\xa0\x20" + pv.uv(1000 + i) + b"\x07\x00\x01\x01\x01\x02" + pv.uv(i) + b"\x00\x00\x00")
        else:
            pk.append(b"\x20" + pv.uv(70000 + i) + pv.uv(i) + b"\x00\x02" + bytes([i & 0xFF, i >> 8]) + b"\x09\x00\x00")
    assert len(set(pk)) == npk
    im, got = _decode(enc, pk, 2, 2)
    want, mask = im.expected(pk)
    assert mask.all()
    im.check(got, want, mask, "npk %d" % npk, pk)
    assert im.info(got)["packet_number"].tolist() == [i if i % 3 == 2 else 70000 + i for i in range(npk)]


# -------------------------------------------------------------- memory kinds
@pytest.mark.gpu
def test_pinned_host_buffers_give_the_device_image(enc):
    """Ring, lens, pad and all three outputs in pinned host memory (zero-copy,
    as the header promises): the same image as with device buffers."""
    pk = pv.frame([b for _, b in pv.directed()])
    slot = _round16(max(len(b) for b in pk))
    slots, lens = pv.ring(pk, slot, slack=0x80, encrypt=True)
    dev_im, dev_got = _decode(enc, pk, 32, 8, slot=slot, framed=True, encrypt=True, slack=0x80)
    bufs = [fec.host_alloc(n) for n in (slots.size, lens.size * 2, slot, pv.DecodeImage.bytes_needed(len(pk), 32, 8))]
    im = None
    try:
        h_slots, h_lens, h_pad, h_out = bufs
        h_slots[:] = slots.reshape(-1)
        h_lens[:] = lens.view(np.uint8)
        h_pad[:] = pv.keystream(slot)
        im = pv.DecodeImage(len(pk), 32, 8, buffer=h_out)
        enc.packet_decode(torch.from_numpy(h_slots).view(len(pk), slot), torch.from_numpy(h_lens.view(np.int16)),
                          pad=torch.from_numpy(h_pad), framed=True, max_ranges=32, max_segments=8, out=im.out)
        torch.cuda.synchronize()
        got = h_out[:im.size].copy()
    finally:
        del im
        for b in bufs:
            fec.host_free(b)
    want, mask = dev_im.expected(pk, True)
    dev_im.check(got, want, mask, "pinned", pk)
    dev_im.check(got, dev_got, np.ones_like(mask), "pinned against device", pk)


@pytest.mark.gpu
def test_pageable_memory_is_rejected(enc):
    pk = [b"\x20\x01\x05\x00\x02\xaa\xbb"] * 4
    slots, lens = pv.ring(pk, 16)
    d_slots, d_lens = torch.from_numpy(slots).cuda(), _i16(lens).cuda()
    im = pv.DecodeImage(4, 2, 2)
    with pytest.raises(fec.ErrInvalidArg):  # a pageable ring
        enc.packet_decode(torch.from_numpy(slots), d_lens, max_ranges=2, max_segments=2, out=im.out)
    host = pv.DecodeImage(4, 2, 2, buffer=np.zeros(pv.DecodeImage.bytes_needed(4, 2, 2), np.uint8))
    with pytest.raises(fec.ErrInvalidArg):  # a pageable info
        enc.packet_decode(d_slots, d_lens, max_ranges=2, max_segments=2, out=(host.out[0],) + im.out[1:])
    torch.cuda.synchronize()
    assert (im.got() == pv.SENTINEL).all() and (host.flat.numpy() == pv.SENTINEL).all()


# ----------------------------------------------------------------- arguments
PK = [b"\x20\x01\x05\x00\x02\xaa\xbb", b"\x80\x20\x14\x00\x00\x02\x02\x01\x02\x01\x01", b"\x20\x01\x00\xff",
      b"\x20\x01", b""]


class _Args:
    """A valid call over PK, to be spoiled one argument at a time."""

    def __init__(self, enc):
        slots, lens = pv.ring(PK, 48, encrypt=True)
        self.keep = (torch.from_numpy(slots).cuda(), _i16(lens).cuda(),
                     torch.from_numpy(pv.keystream(64).copy()).cuda())
        self.im = pv.DecodeImage(len(PK), 4, 2)
        info, ranges, segs = self.im.out
        self.a = dict(ctx=enc._h, pkts=self.keep[0].data_ptr(), slot=48, lens=self.keep[1].data_ptr(), npk=len(PK),
                      pad=self.keep[2].data_ptr(), flags=0, info=info.data_ptr(), ranges=ranges.data_ptr(),
                      max_ranges=4, segs=segs.data_ptr(), max_segments=2)

    def call(self, **spoil):
        a = dict(self.a, **spoil)
        st = fec.load_library().ugo_fec_packet_decode(
            a["ctx"], a["pkts"], a["slot"], a["lens"], a["npk"], a["pad"], a["flags"], a["info"], a["ranges"],
            a["max_ranges"], a["segs"], a["max_segments"], None)
        torch.cuda.synchronize()
        return st


REJECTED = {
    "null-ctx": dict(ctx=None),
    "null-pkts": dict(pkts=None),
    "null-lens": dict(lens=None),
    "null-info": dict(info=None),
    "slot-0": dict(slot=0),
    "slot-24": dict(slot=24),
    "slot-0x10000": dict(slot=0x10000),
    "pkts-plus-8": dict(pkts=+8),
    "pad-plus-4": dict(pad=+4),
    "flags-2": dict(flags=2),
    "flags-3": dict(flags=3),
    "max-ranges-0x10000": dict(max_ranges=0x10000),
    "max-segments-0x10000": dict(max_segments=0x10000),
    "null-ranges": dict(ranges=None),
    "null-segs": dict(segs=None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejected_arguments_touch_nothing(enc, case):
    args = _Args(enc)
    spoil = dict(REJECTED[case])
    for k in ("pkts", "pad"):  # an offset into the valid buffer, off the 16-byte boundary
        if isinstance(spoil.get(k), int):
            spoil[k] += args.a[k]
    assert args.call(**spoil) == INVALID_ARG
    assert (args.im.got() == pv.SENTINEL).all(), "a rejected call wrote to its outputs"


@pytest.mark.gpu
def test_accepted_argument_edges(enc):
    args = _Args(enc)
    lib_call = fec.load_library().ugo_fec_packet_decode
    # no packets: a no-op whatever else is passed
    assert lib_call(enc._h, None, 0, None, 0, None, 0, None, None, 0, None, 0, None) == fec.OK
    assert args.call(npk=0) == fec.OK
    assert (args.im.got() == pv.SENTINEL).all()
    # the untouched call is valid, with and without the pad, framed flag alone
    want, mask = args.im.expected(PK)
    assert args.call() == fec.OK
    args.im.check(args.im.got(), want, mask, "valid call", PK)
    args.im.refill()
    assert args.call(flags=fec.PKT_FEC_FRAMED) == fec.OK
    args.im.check(args.im.got(), *args.im.expected(PK, True), "framed flag", PK)
    # NULL ranges and segs under zero caps: packets that carry either get CAPACITY, counts 0
    args.im.refill()
    assert args.call(ranges=None, max_ranges=0, segs=None, max_segments=0) == fec.OK
    got = args.im.got()
    zero = pv.DecodeImage(len(PK), 0, 0, device=None)
    want0, _ = zero.expected(PK)
    info, winfo = args.im.info(got), zero.info(want0)
    assert info["status"].tolist() == winfo["status"].tolist() == [6, 6, 2, 0, 1]
    ok = info["status"] != 2
    assert info[ok & (info["status"] != 1)].tobytes() == winfo[ok & (winfo["status"] != 1)].tobytes()
    assert not info["n_ranges"][[0, 1, 3]].any() and not info["n_segments"][[0, 1, 3]].any()
    assert (got[args.im.ranges_off - pv.GUARD:] == pv.SENTINEL).all(), "ranges / segs written under zero caps"
    # one cap zero with its array NULL, the other in use
    args.im.refill()
    assert args.call(ranges=None, max_ranges=0) == fec.OK
    got = args.im.got()
    assert args.im.info(got)["status"].tolist() == [0, 6, 2, 0, 1] and args.im.info(got)["n_segments"][0] == 1
    assert (args.im.ranges(got) == 0xA5A5A5A5A5A5A5A5).all()
    assert args.im.segs(got)[0, 0].tolist() == (5, 5, 2, 2)
