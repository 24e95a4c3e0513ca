"""ugo_fec_packet_encode and ugo_fec_stream_tx_set_encode against the directed
corpus of tests/packet_encode_vectors.py, through the whole-output image: wire,
wire_lens and status lie in one sentinel-filled allocation between guards, and
every byte of it is compared with an image built from the oracle alone under
the rules of include/ugo_pkt.h -- bytes [0, round_up(len, 16)) of a slot
written, zeros behind len, a failed slot untouched with wire_lens 0.  The
operands are compared with what went in after every call.  Bit-exact, no
tolerances.

Every family runs unframed, framed and under the RC4 pad, from one flat
payload buffer and from a row of payload per packet (payload_stride); families
a and c also into pinned host memory; a and b at batch sizes round the 64
packets of a block and over payload buffers whose other bytes are zeros, ff
and random; a, b and c through the send windows, the window's wrap point at
every place of a segment's copy.
"""
import numpy as np
import pytest
import torch

import packet_encode_vectors as ev
from stream_harness import enc, pad_bytes  # noqa: F401  (fixtures)
from stream_tx_harness import SENTINEL as SENTINEL_TX
from stream_tx_harness import TxHarness
from ugo_amd import fec

MODES = {"unframed": (False, False), "framed": (True, False), "rc4": (False, True)}
_images = {}


def _expected_image(im, fam, framed, ks, sentinel=ev.SENTINEL):
    key = (fam.name, im.n, im.slot, framed, ks is not None, sentinel)
    if key not in _images:
        _images[key] = im.expected(fam.expected(framed), framed, ks, sentinel)
        _images[key].setflags(write=False)
    return _images[key]


def _run(enc, fam, pad_bytes, mode="unframed", per_packet=False, surround=None, buffer=None, seed=5):
    """One call over the family into a fresh image; returns the image read back."""
    framed, with_pad = MODES[mode]
    rng = np.random.default_rng(seed)
    n, slot = len(fam.pkts), fam.slot
    info, ranges, segs, payload = ev._describe(fam.pkts, rng, fam.max_ranges, fam.max_segments, fam.residues,
                                               surround, per_packet)
    ks = pad_bytes[:slot] if with_pad else None
    host = [info.view(np.uint8).reshape(n, 64), ranges.view(np.int64),
            segs.view(np.uint8).reshape(n, fam.max_segments, 16), payload] + ([ks] if with_pad else [])
    dev = [torch.from_numpy(np.array(h)).cuda() for h in host]
    im = ev.EncodeImage(n, slot, buffer=buffer)
    enc.packet_encode(dev[0], dev[1], dev[2], dev[3], slot, payload_stride=payload.shape[1] if per_packet else 0,
                      pad=dev[4] if with_pad else None, framed=framed, out=im.out)
    torch.cuda.synchronize()
    got = im.got()
    what = "family %s, %s, %s payload" % (fam.name, mode, "a row per packet of" if per_packet else "flat")
    im.check(got, _expected_image(im, fam, framed, ks), what, fam.label)
    for name, h, d in zip(("info", "ranges", "segs", "payload", "pad"), host, dev):
        assert np.array_equal(d.cpu().numpy(), h), "%s: the call changed %s" % (what, name)
    return got


# ------------------------------------------------------------------- corpus
@pytest.mark.gpu
@pytest.mark.parametrize("per_packet", [False, True], ids=["flat", "stride"])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(ev.FAMILIES))
def test_family_image(enc, pad_bytes, name, mode, per_packet):
    _run(enc, ev.FAMILIES[name](), pad_bytes, mode, per_packet)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_sizes_past_every_length_field(enc, pad_bytes, mode):
    """Family d on its own.  ugo_pkt_segment.len is a uint16, so the largest
    segments the interface can state are 0xffff bytes: 0x8000 twice, 0xffff
    three times and 0xffff once make packets of 0x1000e, 0x30011 and 0x10007
    bytes -- 14, 17 and 7 in the 16 bits of wire_lens.  Each is
    UGO_PKT_CAPACITY, wire_lens 0 and an untouched slot, between packets that
    encode.  A failed packet's segments are not read; their bytes are in the
    payload buffer all the same, so that an encoder whose sum is too narrow
    copies them over the neighbours' slots, inside the image, and fails by
    bytes.  (A 32-bit sum wraps only at 65,535 segments of 65,535 bytes in one
    packet, and what an encoder would do with that packet if it got the sum
    wrong is write 4 GiB: that packet is in no test.)"""
    fam = ev.family_d()
    got = _run(enc, fam, pad_bytes, mode)
    im = ev.EncodeImage(len(fam.pkts), fam.slot, layout_only=True)
    assert im.status(got).tolist() == [0, 6, 0, 6, 0, 6, 0] and not im.lens(got)[1::2].any()
    assert (im.wire(got)[1::2] == ev.SENTINEL).all() and im.lens(got)[0::2].all()


# -------------------------------------------------------------- memory kind
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["framed", "rc4"])
@pytest.mark.parametrize("name", ["a", "c", "c-9000", "c-fff0"])
def test_outputs_in_pinned_host_memory(enc, pad_bytes, name, mode):
    """wire, wire_lens and status in pinned host memory (zero-copy, as the
    header allows): the image of the device run."""
    fam = ev.FAMILIES[name]()
    buf = fec.host_alloc(ev.EncodeImage.bytes_needed(len(fam.pkts), fam.slot))
    try:
        pinned = _run(enc, fam, pad_bytes, mode, buffer=buf)
    finally:
        fec.host_free(buf)
    assert np.array_equal(pinned, _run(enc, fam, pad_bytes, mode))


# -------------------------------------------------------------- batch shape
@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["a", "b"])
def test_batch_sizes_round_the_block(enc, pad_bytes, name, mode):
    """One block with one packet, one short of full, full, and a second block
    with one packet: the packets spread over the family, so that a slipped
    index shows."""
    fam = ev.FAMILIES[name]()
    for n in (1, 63, 64, 65):
        _run(enc, fam.pick(n), pad_bytes, mode, per_packet=n == 63)


# ----------------------------------------------------- round the segments
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["framed", "rc4"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_bytes_round_the_segments_change_nothing(enc, pad_bytes, name, mode):
    """The copy reads 16 bytes at a time from unaligned segments: what lies in
    the payload buffer before and behind a segment must not reach the wire."""
    fam = ev.FAMILIES[name]()
    first = None
    for surround in ("zeros", "ff", "random"):
        for per_packet in (False, True):
            got = _run(enc, fam, pad_bytes, mode, per_packet, surround)
            first = got if first is None else first
            assert np.array_equal(got, first), (surround, per_packet)


# ------------------------------------------------------------- send windows
@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_same_body_through_the_send_windows(enc, pad_bytes, name, mode):
    """k_packet_encode<WinSrc>: the family's packets as hand-made descriptors
    over five windows, each just large enough, the wrap point nowhere in a
    segment, in its first and its last 16 bytes, and in its interior at and
    off a chunk boundary.  The harness compares every output byte with its
    own statement; the wire, lengths and statuses are then those of the flat
    encoder's oracle image."""
    framed, with_pad = MODES[mode]
    fam = ev.FAMILIES[name]()
    moved, conn, caps, bases, streams, met = ev.window_layout(fam, framed)
    assert [met[m] for m in range(5)] == [set()] + [{p} for p in ev.PLACEMENTS[1:]]
    n, slot = len(moved.pkts), moved.slot
    info = np.zeros(n, fec.PKT_INFO_DTYPE)
    segs = np.zeros((n, moved.max_segments), fec.PKT_SEGMENT_DTYPE)
    for i, p in enumerate(moved.pkts):
        info[i]["packet_number"], info[i]["stop_waiting"], info[i]["n_segments"] = p["pn"], p["sw"], len(p["segments"])
        for j, (o, d) in enumerate(p["segments"]):
            segs[i, j] = (o, o & (caps[conn[i]] - 1), len(d), len(d))
    h = TxHarness(enc, caps, rq_caps=2, starts=bases)
    try:
        assert h.write(streams) == [len(s) for s in streams]
        wire, lens, status = h.encode(info, segs, np.array(conn, np.uint32), n, slot=slot, framed=framed,
                                      pad=pad_bytes if with_pad else None)
        torch.cuda.synchronize()
        wire, lens = wire.cpu().numpy(), lens.cpu().numpy()
    finally:
        h.close()
    # the harness's slots are filled with its own sentinel: the oracle image over that one
    im = ev.EncodeImage(n, slot, layout_only=True)
    want = _expected_image(im, moved, framed, pad_bytes[:slot] if with_pad else None, SENTINEL_TX)
    got = np.full(im.size, SENTINEL_TX, np.uint8)
    im.wire(got)[:] = wire
    im.lens(got)[:] = lens.view(np.uint16)
    im.status(got)[:] = status
    im.check(got, want, "family %s through the send windows, %s" % (name, mode), moved.label)
