"""Stream order on a non-blocking stream that is behind its host.

Every header from ugo_pkt.h to ugo_loop.h promises calls that are
stream-ordered with no host copy and no synchronisation.  On the legacy
default stream, which waits for every blocking stream of the process, a launch
on the wrong stream, a fill on the null stream or a state read that waits for
the wrong stream still gives the right bytes.  Here every call goes to a
torch.cuda.Stream() -- hipStreamNonBlocking -- on which a device-side delay
(chain_harness.behind) is enqueued in front of every run of calls: the host
enqueues the whole run while the delay still runs, so work that goes anywhere
but the call's stream executes before its operands exist and reads what the
buffers held before.

  * the chain, the server and the chain alternating between two streams, with
    the harnesses' deferred comparison (chain_harness, defer=True);
  * single calls the chain does not make, each with a late write: the operand
    buffers hold a valid decoy batch, operand.copy_(real) is enqueued behind
    the delay, then the call, and the outputs must be the reference's of the
    real batch, which differs from the decoy's;
  * the data path of one ring, run once over a decoy ring and then, behind one
    delay and a late write, over the real ring into the same buffers;
  * a census: every entry point whose prototype ends in `void* stream` was
    called with the side stream's handle, or stands in EXEMPT with its reason.

A run proves something only if stream.query() is False right after its last
enqueue; a test fails with "the stream was not behind" when more than 5 % of
its runs proved nothing.
"""
import copy
import re
import time

import numpy as np
import pytest

import chain_ref as ch
import listen_ref as lr
import packet_ref as pr
import sent_ref as sr
import stream_ref as rr
import test_chain as tc
from ugo_amd import fec

# What the census does not ask for, and why.
_CORE = "a call of the FEC core of ugo_fec.h, which "
EXEMPT = {
    "ugo_fec_encode_strided": _CORE + "test_concurrency.py runs on streams of its own (encode_batch)",
    "ugo_fec_reconstruct_into": _CORE + "test_concurrency.py runs on streams of its own",
    "ugo_fec_encode": _CORE + "only checks pitch and forwards to ugo_fec_encode_strided",
    "ugo_fec_reconstruct": _CORE + "only checks pitch and forwards to ugo_fec_reconstruct_strided",
    "ugo_fec_reconstruct_strided": _CORE + "copies the masks to the host and synchronises its stream by contract",
    "ugo_fec_reconstruct_rows": _CORE + "copies the masks to the host and synchronises its stream by contract",
}
N_STREAMED = 43                                 # prototypes in include/*.h that end in `void* stream`


def test_the_entry_points_with_a_stream_argument_are_found():
    """The census's expected set, pinned where no GPU is."""
    syms = fec.header_stream_symbols()
    assert "ugo_fec_cc_set_ack" in syms and "ugo_fec_listen_route" in syms
    assert "ugo_fec_cc_set_state" not in syms and "ugo_fec_stream_rx_create" not in syms
    assert len(syms) == len(set(syms)) == N_STREAMED
    plain = "".join(re.sub(r"/\*.*?\*/", "", open(p).read(), flags=re.S) for p in fec.HEADER_PATHS)
    assert len(re.findall(r"\bvoid\s*\*\s*stream\s*\)\s*;", plain)) == N_STREAMED     # counted another way
    assert set(syms) <= set(fec.header_symbols())
    lib = fec.load_library()
    for s in syms:
        assert getattr(lib, s).argtypes[-1] is fec.ctypes.c_void_p, s
    for s, why in EXEMPT.items():
        assert s in syms and why, f"the exemption {s} names no entry point with a stream argument"


# ---------------------------------------------------------------- the inputs of the data path (CPU)
D, P, N, S, SLOT, G = 10, 3, 13, 1470, 1488, 8
FS, PITCH_F, PITCH_P = S + 6, 1488, 1472
FIRST_SEQ, FIRST_GROUP = 130, 10
RX_CAP = 1 << 17
REAL_LOSS = {1: [4], 3: [0], 5: [9], 6: [2, 7], 2: [11]}           # group: rows lost; row 11 is a parity packet
DECOY_LOSS = {0: [1], 2: [3, 8], 4: [0], 7: [5], 5: [12]}
FILL = 0xA5


def _ring_batch(seed, loss):
    """80 packets of one stream segment each, contiguous from offset 0, as the
    encoder's input, and which of the 104 wire packets the link keeps."""
    import test_packet_encode as tpe

    rng = np.random.default_rng(seed)
    pk, x = [], 0
    for i in range(G * D):
        data = rng.integers(0, 256, int(rng.integers(1, 1401)), dtype=np.uint8).tobytes()
        pk.append(tpe._pkt(pn=1000 * seed + i, sw=5 if i % 7 == 0 else 0, segments=[(x, data)]))
        x += len(data)
    info, ranges, segs, payload = tpe._describe(pk, rng, 1, 1)
    keep = np.ones(G * N, np.int16)
    for g, rows in loss.items():
        for r in rows:
            keep[g * N + r] = 0
    raws = []
    for q in pk:
        st, raw = tpe._ref_encode(q)
        assert st == 0
        raws.append(raw)
    return dict(info=info.view(np.uint8).reshape(-1, 64).copy(), ranges=ranges.view(np.int64).copy(),
                segs=segs.view(np.uint8).reshape(len(pk), 1, 16).copy(), payload=payload.copy(), keep=keep, raws=raws,
                stream=b"".join(q["segments"][0][1] for q in pk))


def _fresh_images():
    """What the buffers of the data path hold before the first pass."""
    z = lambda *s, dt=np.uint8, v=FILL: np.full(s, v, dt)  # noqa: E731
    return dict(framed=z(G * D, SLOT), wl=z(G * D, dt=np.uint16, v=0), est=z(G * D),
                wire=z(G * N, SLOT), wlen=z(G * N, dt=np.uint16, v=0), tst=z(G, dt=np.int8, v=-1),
                sh_f=z(N, G, PITCH_F), sh_p=z(N, G, PITCH_P), lout=z(G, P, PITCH_F), lst_st=z(G, dt=np.int8, v=-1),
                rout=z(P * G, PITCH_P), rindex=z(P * G, dt=np.uint32, v=0x77777777),
                oinfo=z(G * N, 64), oranges=z(G * N, 1, 2, dt=np.uint64, v=0xA5A5A5A5A5A5A5A5),
                osegs=z(G * N, 1, 16), seg_status=z(G * N, 1, v=0x77), dst=z(RX_CAP, v=0x5A))


def _data_path_model(b, img, defined=None):
    """The data path over the batch b on the CPU -- packet_ref, fec_ref /
    rs_ref, the placement of assembly_image, stream_ref -- written over the
    images `img` of the buffers as the calls may write them.  Returns what is
    compared besides the images; `defined` masks the bytes the headers leave
    unspecified, and is carried from pass to pass: what an earlier ring left
    unspecified stays so until a later one writes it."""
    import assembly_image as ai
    import fec_ref
    import rs_ref

    r16 = ai.round_up
    out, defined = {}, dict(defined or {})
    for i, raw in enumerate(b["raws"]):         # packet_encode, framed: 6 zero bytes, the packet, zeros to the chunk
        w = r16(6 + len(raw), 16)
        img["framed"][i, :w] = 0
        img["framed"][i, 6:6 + len(raw)] = np.frombuffer(raw, np.uint8)
        img["wl"][i], img["est"][i] = 6 + len(raw), 0
    tx = fec_ref.FEC.new(128, D, P, clock=lambda: 0)                 # tx_assemble: the sender loop per group
    tx.next = FIRST_SEQ
    sent = []
    for g in range(G):
        sent += fec_ref.tx_group(tx, [bytes(6) + raw for raw in b["raws"][g * D:(g + 1) * D]], ai.KEY)
        img["tst"][g] = 0
    for i, w in enumerate(sent):
        img["wire"][i, :r16(len(w), 16)] = 0
        img["wire"][i, :len(w)] = np.frombuffer(w, np.uint8)
        img["wlen"][i] = len(w)
    plain = [ai.crypt(w) if b["keep"][i] else b"" for i, w in enumerate(sent)]     # the link: a lost packet is empty
    out["lens2"] = np.asarray([len(w) for w in plain], np.uint16)
    want_f, masks, stats = ai.expected_placement(plain, G, N, S, PITCH_F, FIRST_GROUP, frames=True)
    want_p, masks_p, stats_p = ai.expected_placement(plain, G, N, S, PITCH_P, FIRST_GROUP)
    assert np.array_equal(masks, masks_p) and stats == stats_p
    for g in range(G):
        for r in range(N):
            if (int(masks[g]) >> r) & 1:
                img["sh_f"][r, g], img["sh_p"][r, g] = want_f[g, r], want_p[g, r]
    out["present"], out["stats"] = masks, np.asarray(stats, np.int32)
    lossy = [g for g in range(G) if (~int(masks[g])) & ((1 << D) - 1)]
    out["lossy"] = np.asarray(lossy, np.int32)
    exp = np.ascontiguousarray(want_p[:, :, :S])
    _, exp_st = rs_ref.c_reconstruct(D, P, exp, masks, data_only=True)
    for k in ("lout", "rout"):
        defined[k] = defined[k].copy() if k in defined else np.ones(img[k].shape, bool)
    r = 0
    for j, g in enumerate(lossy):               # reconstruct_list on the frames, recover_data on the payload rows
        assert exp_st[g] == 0
        img["lst_st"][j] = 0
        for i, row in enumerate(k for k in range(D) if not (int(masks[g]) >> k) & 1):
            img["lout"][j, i, 6:FS], defined["lout"][j, i, 6:FS] = exp[g, row], True
            defined["lout"][j, i, :6] = defined["lout"][j, i, FS:] = False        # a recovered header; the chunk's end
            img["rout"][r, :S], img["rindex"][r], defined["rout"][r, :S] = exp[g, row], g * N + row, True
            defined["rout"][r, S:] = False
            r += 1
    out["n_recovered"] = r
    ok = np.zeros(G * N, bool)                  # packet_decode, framed, of the data packets that arrived
    defined["oinfo"] = np.zeros(img["oinfo"].shape, bool)
    iv, sv = ch._iv(img["oinfo"]), ch._sv(img["osegs"])
    off = {f: ch.I_T.fields[f][1] for f in ("status", "payload_off", "fec_flag_lo", "reserved")}
    for i, w in enumerate(plain):
        w = w if i % N < D else b""
        framed = len(w) >= 6 and w[4] | (w[5] << 8) == 0xF1
        st, dec = pr.decode(w[6:] if framed else w)
        rec = np.zeros(1, ch.I_T)
        rec["payload_off"], rec["fec_flag_lo"] = 6 if framed else 0, w[4] if len(w) >= 6 else 0
        for f, o in off.items():                # all a failed packet's record defines
            defined["oinfo"][i, o:o + ch.I_T.fields[f][0].itemsize] = True
        if st != pr.PKT_OK:
            rec["status"] = st
            for f in off:
                iv[f][i] = rec[f][0]
            continue
        assert framed and dec["sack"] is None and len(dec["segments"]) == 1
        ok[i], defined["oinfo"][i] = True, True
        for f in ("flags", "packet_number", "stop_waiting"):
            rec[f] = dec[f]
        rec["n_segments"] = 1
        iv[i] = rec[0]
        o, d, n, a = dec["segments"][0]
        sv[i, 0] = (o, d + 6, n, a)
    out["decoded"] = ok
    info = np.zeros(G * N, ch.I_T)              # stream_deliver and stream_read: what the rule sees of the ring
    info["status"], info["n_segments"] = np.where(ok, 0, 1), ok
    pkts = rr.packets_from_raw(img["wire"], info, sv, ch.pad_bytes())
    rule = rr.RuleRx(RX_CAP, FILL)
    rows = rule.deliver(pkts)
    img["seg_status"][:] = 0
    for i, row in enumerate(rows):
        img["seg_status"][i, :len(row)] = row
    data, eof = rule.read(RX_CAP)
    img["dst"][:len(data)] = np.frombuffer(data, np.uint8)
    out.update(n_read=len(data), eof=int(eof), data=data, window=rule.W, record=rule.record())
    assert rule.err == rr.NONE
    return out, defined


def test_the_rings_of_the_data_path_are_what_the_test_is_for():
    """Conditions on the inputs of test_data_path_of_one_ring_on_a_stream_that_is_behind."""
    img = _fresh_images()
    decoy, real = _ring_batch(3, DECOY_LOSS), _ring_batch(4, REAL_LOSS)
    od, defined = _data_path_model(decoy, img)
    before = copy.deepcopy(img)
    o, defined = _data_path_model(real, img, defined)
    assert o["lossy"].tolist() == [1, 3, 5, 6] and o["n_recovered"] == 5 and o["stats"].tolist() == [98, 0, 0, 6, 0]
    assert od["lossy"].tolist() == [0, 2, 4, 7] and not np.array_equal(o["present"], od["present"])
    assert 0 < o["n_read"] < len(real["stream"]) and o["data"] == real["stream"][:o["n_read"]]   # up to the first loss
    assert o["decoded"].sum() == G * D - 5 and o["data"] != od["data"][:o["n_read"]]
    for k in set(img) - {"est", "tst", "lst_st", "oranges", "wl"}:   # those hold the same after either ring, or may
        m = defined.get(k, True)
        assert ((img[k] != before[k]) & m).any(), f"{k}: the decoy ring leaves what the real ring writes"


# ---------------------------------------------------------------- GPU
import torch  # noqa: E402

from chain_harness import ChainHarness, ServerHarness, behind, calibrate_sleep, differ  # noqa: E402
from listen_harness import Guarded, ListenHarness  # noqa: E402
from sent_harness import NO_CONN, SentHarness, _put  # noqa: E402
from stream_harness import build_batch  # noqa: E402

WARM_DELAY_S = 1e-3


@pytest.fixture(scope="module")
def enc(gpu):
    return fec.New(D, P)


@pytest.fixture(scope="module")
def side(gpu):
    return torch.cuda.Stream()                  # non-blocking: the legacy default stream does not wait for it


def chain(enc, name, delay):
    """test_chain.run_on_device with the deferred harness."""
    made = []

    def make(n, now, **kw):
        made.append(ChainHarness(enc, n, now, kw.pop("max_ranges"), kw.pop("max_packets"), defer=True, delay=delay,
                                 **kw))
        return made[-1]

    try:
        scr, A, B, st = tc.run(name, make)
        tc.lives_hold(scr, A, B, st)
        return st
    finally:
        for h in made:
            h.close()


def server(enc, delay):
    made = []

    def make(max_conn, now, **kw):
        made.append(ServerHarness(enc, max_conn, now, kw.pop("max_ranges"), kw.pop("max_packets"), defer=True,
                                  delay=delay, **kw))
        return made[-1]

    try:
        tc.server_holds(tc.run_server(make, True)[1])
    finally:
        for s in made:
            s.close()


@pytest.fixture(scope="module")
def tempo(enc, side):
    """The delay: at least 4 x the host time to enqueue the longest run (the 13
    calls of receive), measured over a warm-up run of n3, and a millisecond at
    the least.  A preempted host thread can double its enqueue time."""
    with torch.cuda.stream(side):
        cps = calibrate_sleep()
        warm = behind(side, WARM_DELAY_S, cps)
        chain(enc, "n3", warm)
    took = sorted(r[1] for r in warm.runs if r[0] == "receive")
    enqueue = took[len(took) // 2]
    t = dict(cycles_per_s=cps, enqueue_s=enqueue, delay_s=max(WARM_DELAY_S, 4 * enqueue))
    print(f"\nreceive's 13 calls take the host {enqueue * 1e6:.0f} us to enqueue (median of {len(took)}, "
          f"slowest {took[-1] * 1e6:.0f} us); the delay is {t['delay_s'] * 1e3:.2f} ms")
    return t


def make_delay(side, tempo):
    return behind(side, tempo["delay_s"], tempo["cycles_per_s"])


def report(what, delay):
    idle = sum(1 for r in delay.runs if r[2])
    print(f"\n{what}: {len(delay.runs)} runs behind a delay of {delay.seconds * 1e3:.2f} ms "
          f"({delay.longest * 1e3:.2f} ms at the longest), {idle} of them "
          f"({100.0 * idle / max(len(delay.runs), 1):.1f} %) had finished at their last enqueue; the slowest took the "
          f"host {max((r[1] for r in delay.runs), default=0) * 1e6:.0f} us")
    delay.assert_was_behind()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 257])
def test_chain_on_a_stream_that_is_behind(enc, side, tempo, n):
    """test_chain_equals_the_rules_call_by_call with no host wait inside a run
    of calls.  257 stays: the smallest size at which the one-lane-per-member
    kernels take a second block and the multi-launch scans their second level."""
    delay = make_delay(side, tempo)
    with torch.cuda.stream(side):
        chain(enc, f"n{n}", delay)
    report(f"n{n}", delay)


@pytest.mark.gpu
def test_server_on_a_stream_that_is_behind(enc, side, tempo):
    delay = make_delay(side, tempo)
    with torch.cuda.stream(side):
        server(enc, delay)
    report("server", delay)


class alternating(behind):
    """Every run on the other of two non-blocking streams, which first waits
    for the one before: the sets are last used on different streams."""

    def __init__(self, streams, seconds, cycles_per_s):
        super().__init__(streams[0], seconds, cycles_per_s)
        self.streams, self.used = streams, [0, 0]

    def __call__(self, seconds=0.0):
        cur = torch.cuda.current_stream()
        k = 1 - self.streams.index(cur)
        self.streams[k].wait_stream(cur)
        torch.cuda.set_stream(self.streams[k])
        self.stream = self.streams[k]
        self.used[k] += 1
        super().__call__(seconds)


@pytest.mark.gpu
def test_chain_alternating_between_two_streams(enc, side, tempo):
    """Nothing may depend on state kept per stream, and every *_set_state has
    to wait for the stream its own set was last used on."""
    delay = alternating([side, torch.cuda.Stream()], tempo["delay_s"], tempo["cycles_per_s"])
    with torch.cuda.stream(side):               # leaving restores the stream current before, whatever was set inside
        chain(enc, "n3", delay)
    assert min(delay.used) > 10, delay.used
    report("n3 on two streams in turn", delay)


# ---------------------------------------------------------------- single calls with a late write
def A(c, la, lio, ranges=(), w=0, delay=0, status=0, flags=0x80, nr=None):
    return (status, c, flags, sr.Ack(la, lio, ranges, w, delay), nr)


def _ack_operands(packets, max_ranges, seed):
    """SentHarness.ack's operands for `packets`: (info, ranges, conn_of, what the rule is given)."""
    npk = len(packets)
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (npk, 64), dtype=np.uint8)
    iv = raw.view(fec.PKT_INFO_DTYPE).reshape(-1)
    ranges = rng.integers(0, 2 ** 62, (npk, max_ranges, 2), dtype=np.int64)
    conn = np.zeros(npk, np.uint32)
    model = []
    for i, (st, c, flags, a, nr) in enumerate(packets):
        nr = len(a.ranges) if nr is None else nr
        conn[i] = c & 0xffffffff
        iv["status"][i], iv["flags"][i], iv["n_ranges"][i] = st, flags, nr
        iv["packet_number"][i], iv["largest_acked"][i], iv["largest_in_order"][i] = a.w, a.la, a.lio
        iv["delay_us"][i] = a.delay
        for k, (f, l) in enumerate(a.ranges[:max_ranges]):
            ranges[i, k] = (f, l)
        rows = [(int(ranges[i, k, 0]), int(ranges[i, k, 1])) for k in range(max_ranges)]
        model.append((st, c & 0xffffffff, flags, sr.Ack(a.la, a.lio, rows, a.w, a.delay), nr))
    return raw, ranges, conn.view(np.int32), model


def _events(want):
    out = np.zeros(len(want), fec.SENT_EVENT_DTYPE)
    for k in sr.RuleSent.EVENT_FIELDS:
        out[k] = [w[k] & ch.M64 for w in want]
    return out


def _late(delay, label, writes, call, seconds=0.0):
    """The late write: behind the delay the operands get the real batch from
    copies that are on the device already, then the call is enqueued."""
    delay(seconds)
    t0 = time.perf_counter()
    for operand, real in writes:
        operand.copy_(real)
    out = call()
    delay.ran(label, time.perf_counter() - t0)
    return out


def late_sent_set_ack(enc, delay):
    """3 members, window 1024, 30 packets outstanding, and in one call the ACKs
    of test_cc.py::test_sent_ack_is_set_ack_for_the_sent_histories."""
    MR, now = 3, 77_000
    h = SentHarness(enc, [1024, 1024, 1024], 2)
    try:
        for c in range(3):
            h.send(c, range(1, 31))
        real = [A(0, la, 0, [(2, la), (0, 0)], w=la) for la in (5, 6, 7)] + \
            [A(1, 20, 0, [(2, 20), (0, 0)], delay=1), A(1, 20, 20, (), delay=2), A(1, 21, 21, (), delay=5),
             A(1, 21, 0, [(3, 21), (0, 0)], delay=6)] + \
            [A(2, 31, 31, w=1), A(2, 10, 10, w=2, status=3), A(7, 9, 9, w=3), A(NO_CONN, 9, 9, w=4), A(2, 12, 12, w=5)]
        decoy = [A(i % 3, 14 + i, 14 + i, (), w=40 + i, delay=9) for i in range(len(real))]
        ri, rr_, rc, model = _ack_operands(real, MR, 1)
        di, dr, dc, dmodel = _ack_operands(decoy, MR, 2)
        want_decoy = _events(sr.ack_set(copy.deepcopy(h.rules), dmodel, now, MR))
        want = _events(sr.ack_set(h.rules, model, now, MR))
        assert (want["largest_acked"] != want_decoy["largest_acked"]).all(), "the decoy's events are the real batch's"
        fill = np.random.default_rng(3).integers(0, 256, (3, 64), dtype=np.uint8)
        ops, reals, ev = [_put(x) for x in (di, dr, dc)], [_put(x) for x in (ri, rr_, rc)], _put(fill)
        _late(delay, "sent_set_ack", zip(ops, reals),
              lambda: h.set.ack(ops[0], ops[1], ops[2], now, npackets=len(real), events=ev))
        h.check()                               # waits for the call; every record and ring against the rule
        got = ev.cpu().numpy().view(fec.SENT_EVENT_DTYPE).reshape(-1)
        for k in sr.RuleSent.EVENT_FIELDS:
            differ("sent_set_ack", f"event field {k}", got[k].astype(np.uint64), want[k].astype(np.uint64))
        assert not got["reserved"].any()
        for t, x in zip(ops, (ri, rr_, rc)):
            assert np.array_equal(t.cpu().numpy(), x), "sent_set_ack wrote an operand"
    finally:
        h.close()


def late_listen_names(enc, delay):
    """64 packets over 5 members, two of them under v6 names."""
    h = ListenHarness(enc, 8)
    try:
        rows = [lr.name_v4(bytes([10, 0, 0, k]), 4000 + k) for k in range(3)] + \
            [lr.name_v6(bytes([0x20, 1] + [k] * 14), 5000 + k, scope=k) for k in (3, 4)]
        names = np.stack([np.frombuffer(r, np.uint8) for r in rows])
        pkts = np.zeros((5, 48), np.uint8)
        for k in range(5):
            pkts[k, :22] = np.frombuffer(lr.init_packet(0x100 + k), np.uint8)
        assert h.route(names, pkts, np.full(5, 22, np.uint16))[3] == 5 and h.rule.nconn == 5
        rng = np.random.default_rng(5)
        real = rng.integers(0, 5, 64).astype(np.uint32)
        decoy = ((real + rng.integers(1, 5, 64)) % 5).astype(np.uint32)          # another member everywhere, in range
        w_rows, w_lens = h.rule.names([int(v) for v in real])
        d_rows, d_lens = h.rule.names([int(v) for v in decoy])
        assert all(a != b for a, b in zip(w_rows, d_rows)) and w_lens != d_lens
        dc, dreal = _put(decoy.view(np.int32)), _put(real.view(np.int32))
        g_rows, g_lens = Guarded(32 * 64, 601), Guarded(4 * 64, 701)
        _late(delay, "listen_names", [(dc, dreal)],
              lambda: h.table.names(dc, names_out=g_rows.view(torch.uint8, 64, 32),
                                    name_lens=g_lens.view(torch.int32, 64)))
        h.check(entries=False)                  # waits for the call
        differ("listen_names", "name_lens", g_lens.read().view(np.uint32), np.asarray(w_lens, np.uint32))
        differ("listen_names", "names", g_rows.read(), np.frombuffer(b"".join(w_rows), np.uint8))
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), real), "listen_names wrote conn_of"
    finally:
        h.close()


def _history(seed, npk=30, max_segments=2):
    """npk packets of max_segments segments each, contiguous from offset 0, in another order."""
    rng = np.random.default_rng(seed)
    pk, x = [], 0
    for _ in range(npk):
        row = []
        for _ in range(max_segments):
            data = rng.integers(0, 256, int(rng.integers(1, 100)), dtype=np.uint8).tobytes()
            row.append(rr.Seg(x, data))
            x += len(data)
        pk.append(rr.Packet(row))
    return [pk[i] for i in rng.permutation(npk)], x


def late_stream_deliver_read(enc, delay):
    """ugo_fec_stream_deliver and ugo_fec_stream_read of one connection on a
    4096-byte window: read is enqueued behind deliver and must see its bytes."""
    cap, slot, ms = 4096, 256, 2
    pad = ch.pad_bytes()[:slot].copy()
    real, total = _history(11)
    decoy, _ = _history(12)
    rp, ri, rs = build_batch(real, slot, ms, pad, seed=1)
    dp, di, ds = build_batch(decoy, slot, ms, pad, seed=2)
    rule, drule = rr.RuleRx(cap, FILL), rr.RuleRx(cap, FILL)
    want_st, decoy_st = rule.deliver(real), drule.deliver(decoy)
    data, eof = rule.read(cap)
    assert len(data) == total and data != drule.read(cap)[0][:total] and not np.array_equal(rule.W, drule.W)
    npk = len(real)
    as_bytes = lambda i, s: (i.view(np.uint8).reshape(npk, 64), s.view(np.uint8).reshape(npk, ms, 16))  # noqa: E731
    ops = [_put(x) for x in (dp, *as_bytes(di, ds))]
    reals = [_put(x) for x in (rp, *as_bytes(ri, rs))]
    dpad = _put(pad)
    rx = fec.StreamRx(enc, cap)
    try:
        rx.window().fill_(FILL)
        status = torch.full((len(real), ms), 0x77, dtype=torch.uint8, device="cuda")
        dst = torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda")
        n_read = torch.zeros(1, dtype=torch.int64, device="cuda")
        deof = torch.full((1,), 0x33, dtype=torch.uint8, device="cuda")

        def calls():
            rx.deliver(ops[0], ops[1], ops[2], pad=dpad, out=status)
            rx.read(cap, out=dst, n_read=n_read, eof=deof)

        _late(delay, "stream_deliver, stream_read", zip(ops, reals), calls)
        st = rx.state()                         # waits for the calls
        exp = np.zeros((len(real), ms), np.uint8)
        for i, row in enumerate(want_st):
            exp[i, :len(row)] = row
        differ("stream_deliver", "seg_status", status.cpu().numpy(), exp)
        assert {k: int(st[k]) for k in rule.record()} == rule.record()
        differ("stream_deliver", "the window", rx.window().cpu().numpy(), rule.W)
        assert int(n_read.item()) == total and int(deof.item()) == int(eof)
        want_dst = np.full(cap, 0x5A, np.uint8)
        want_dst[:total] = np.frombuffer(data, np.uint8)
        differ("stream_read", "dst", dst.cpu().numpy(), want_dst)
    finally:
        rx.close()


@pytest.mark.gpu
def test_sent_set_ack_sees_a_late_write(enc, side, tempo):
    delay = make_delay(side, tempo)
    with torch.cuda.stream(side):
        late_sent_set_ack(enc, delay)
    report("sent_set_ack", delay)


@pytest.mark.gpu
def test_listen_names_sees_a_late_write(enc, side, tempo):
    delay = make_delay(side, tempo)
    with torch.cuda.stream(side):
        late_listen_names(enc, delay)
    report("listen_names", delay)


@pytest.mark.gpu
def test_stream_deliver_and_read_see_a_late_write(enc, side, tempo):
    delay = make_delay(side, tempo)
    with torch.cuda.stream(side):
        late_stream_deliver_read(enc, delay)
    report("stream_deliver, stream_read", delay)


# ---------------------------------------------------------------- the data path of one ring
def data_path(enc, delay):
    """packet_encode(framed) -> tx_assemble -> the loss -> rx_assemble(frames)
    -> lossy_groups -> reconstruct_list -> packet_decode(framed) ->
    stream_deliver -> stream_read, then rx_assemble into payload rows ->
    recover_data: first over the decoy ring, in the usual way; then, behind a
    delay and a late write of the encoder's operands and of what the link
    keeps, over the real ring into the same buffers.  A call that overtook its
    operands computes on the decoy's."""
    img = _fresh_images()
    decoy, real = _ring_batch(3, DECOY_LOSS), _ring_batch(4, REAL_LOSS)
    _, defined = _data_path_model(decoy, img)
    want, defined = _data_path_model(real, img, defined)
    dev = {k: _put(v.view(np.int16) if v.dtype == np.uint16 else v.view(np.int32) if v.dtype == np.uint32 else
                   v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in _fresh_images().items()}
    room = max(len(decoy["payload"]), len(real["payload"]))
    keys = ("info", "ranges", "segs", "keep")
    ops = {k: _put(decoy[k]) for k in keys}
    reals = {k: _put(real[k]) for k in keys}
    ops["payload"] = torch.zeros(room, dtype=torch.uint8, device="cuda")
    ops["payload"][:len(decoy["payload"])] = _put(decoy["payload"])
    reals["payload"] = torch.zeros(room, dtype=torch.uint8, device="cuda")
    reals["payload"][:len(real["payload"])] = _put(real["payload"])
    dpad = _put(ch.pad_bytes())
    is_data = _put(np.asarray([1 if i % N < D else 0 for i in range(G * N)], np.int16))
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    lens2, lens3 = z(G * N, torch.int16), z(G * N, torch.int16)
    present_f, present_p = z(G, torch.int64), z(G, torch.int64)
    stats_f, stats_p = z(5, torch.int32), z(5, torch.int32)
    lst, cnt, rcnt = z(G, torch.int32), z(1, torch.int32), z(1, torch.int32)
    n_read, eof = z(1, torch.int64), z(1, torch.uint8)
    rxs = [fec.StreamRx(enc, RX_CAP), fec.StreamRx(enc, RX_CAP)]

    def path(rx):
        rx.window().fill_(FILL)
        enc.packet_encode(ops["info"], ops["ranges"], ops["segs"], ops["payload"], SLOT, framed=True,
                          out=(dev["framed"], dev["wl"], dev["est"]))
        enc.tx_assemble(dev["framed"], dev["wl"], dev["wire"], dev["wlen"], first_seq=FIRST_SEQ, pad=dpad,
                        status=dev["tst"])
        torch.mul(dev["wlen"], ops["keep"], out=lens2)                  # the loss: a lost packet has length 0
        present_f.zero_()
        stats_f.zero_()
        enc.rx_assemble(dev["wire"], lens2, dev["sh_f"], present_f, first_group=FIRST_GROUP, shard_size=S, pad=dpad,
                        stats=stats_f, frames=True)
        enc.lossy_groups(present_f, data_only=True, out=lst, count=cnt)
        enc.reconstruct_list(dev["sh_f"], present_f, lst, cnt, dev["lout"], shard_size=FS, data_only=True,
                             status=dev["lst_st"])
        torch.mul(lens2, is_data, out=lens3)                            # the connection decodes the data packets
        enc.packet_decode(dev["wire"], lens3, pad=dpad, framed=True, max_ranges=1, max_segments=1,
                          out=(dev["oinfo"], dev["oranges"], dev["osegs"]))
        rx.deliver(dev["wire"], dev["oinfo"], dev["osegs"], pad=dpad, out=dev["seg_status"])
        rx.read(RX_CAP, out=dev["dst"], n_read=n_read, eof=eof)

    def payload_rows():
        """The same ring placed as payload rows, and `input`'s recovered list of it."""
        present_p.zero_()
        stats_p.zero_()
        enc.rx_assemble(wire_b, lens_b, dev["sh_p"], present_p, first_group=FIRST_GROUP, shard_size=S, pad=dpad,
                        stats=stats_p)
        enc.recover_data(dev["sh_p"], present_p, dev["rout"], dev["rindex"], count=rcnt, shard_size=S)

    # Two runs, a synchronisation between them: a second rx_assemble behind the first on a busy stream keeps the
    # host until the stream has caught up (its scratch comes from a stream-ordered pool, and the runtime waits for
    # the first call's pending free), so what followed it would not be behind.  The second run's operands are its
    # own copies of the ring, which hold the decoy's until the late write.
    wire_b, lens_b = torch.zeros_like(dev["wire"]), torch.zeros_like(lens2)
    ring = [(wire_b, dev["wire"]), (lens_b, lens2)]
    try:
        t0 = time.perf_counter()
        path(rxs[0])
        took = time.perf_counter() - t0             # the same calls: the delay is 4 x their enqueue time at least,
        for operand, src in ring:                   # and 50 ms at most where the first pass loaded its kernels
            operand.copy_(src)
        payload_rows()
        torch.cuda.current_stream().synchronize()
        _late(delay, "the data path of one ring", [(ops[k], reals[k]) for k in ops], lambda: path(rxs[1]),
              seconds=min(4 * took, 0.05))
        torch.cuda.current_stream().synchronize()
        _late(delay, "the ring as payload rows", ring, payload_rows)
        torch.cuda.current_stream().synchronize()                       # then every output whole
        host = lambda t: t.cpu().numpy()  # noqa: E731
        for k, w in img.items():
            got = host(dev[k]).view(w.dtype)
            if k == "oinfo":                    # of a packet that failed only four fields are defined
                got, w = np.where(defined[k], got, 0), np.where(defined[k], w, 0)
            elif k in ("osegs", "oranges"):
                got, w = got[want["decoded"]], w[want["decoded"]]
            elif k in defined:
                got, w = np.where(defined[k], got, 0), np.where(defined[k], w, 0)
            differ("the data path", k, got, w)
        differ("the loss", "lens", host(lens2).view(np.uint16), want["lens2"])
        for what, present, stats in (("frames", present_f, stats_f), ("payload rows", present_p, stats_p)):
            differ(f"rx_assemble, {what}", "present", host(present).view(np.uint64), want["present"])
            differ(f"rx_assemble, {what}", "stats", host(stats), want["stats"])
        k = len(want["lossy"])
        assert int(cnt.item()) == k and int(rcnt.item()) == want["n_recovered"]
        differ("lossy_groups", "list", host(lst)[:k], want["lossy"])
        assert int(n_read.item()) == want["n_read"] and int(eof.item()) == want["eof"]
        st = rxs[1].state()
        assert {f: int(st[f]) for f in want["record"]} == want["record"]
        differ("stream_deliver", "the window", host(rxs[1].window()), want["window"])
    finally:
        for rx in rxs:
            rx.close()


@pytest.mark.gpu
def test_data_path_of_one_ring_on_a_stream_that_is_behind(enc, side, tempo):
    """8 groups of (10, 3), slot 1488, S = 1470, the RC4 pad; a data packet
    lost in groups 1, 3 and 5, two in group 6, a parity packet in group 2."""
    delay = make_delay(side, tempo)
    with torch.cuda.stream(side):
        data_path(enc, delay)
    report("the data path of one ring", delay)


# ---------------------------------------------------------------- the census
class _Census:
    """The library, noting for every entry point with a stream argument the handles it was given."""

    def __init__(self, lib, names):
        self._lib, self._names, self.seen = lib, frozenset(names), {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._names:
            return fn

        def call(*args):
            self.seen.setdefault(name, set()).add(args[-1] or 0)
            return fn(*args)

        return call


@pytest.mark.gpu
def test_every_entry_point_with_a_stream_argument_runs_off_the_default_stream(enc, side, monkeypatch):
    """n3, the server run and the calls above with load_library replaced by a
    proxy that notes the stream handle of every call.  It needs no stream that
    is behind and says which entry point went elsewhere even where a run then
    fails by a wrong value."""
    census = _Census(fec.load_library(), fec.header_stream_symbols())
    monkeypatch.setattr(fec, "load_library", lambda path=None: census)
    failed = None
    try:
        with torch.cuda.stream(side):
            delay = behind(side, WARM_DELAY_S, calibrate_sleep())
            chain(enc, "n3", delay)
            server(enc, delay)
            late_sent_set_ack(enc, delay)
            late_listen_names(enc, delay)
            late_stream_deliver_read(enc, delay)
            data_path(enc, delay)
    except AssertionError as e:
        failed = e
    finally:
        monkeypatch.undo()
    handle = side.cuda_stream
    assert handle != 0
    wrong = {s: sorted(h) for s, h in census.seen.items() if h != {handle}}
    assert not wrong, f"called on another stream than the side stream {handle}: {wrong}" + \
        (f"; and a run failed: {failed}" if failed else "")
    if failed is not None:
        raise failed
    missing = sorted(set(fec.header_stream_symbols()) - set(census.seen) - set(EXEMPT))
    assert not missing, f"never called off the default stream, and not exempt: {missing}"
    needless = sorted(set(EXEMPT) & set(census.seen))
    assert not needless, f"exempt, yet called on the side stream: {needless}"
