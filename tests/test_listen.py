"""The connection table (include/ugo_listen.h): listener.handlePacket per ring.

CPU: the rule of tests/listen_ref.py against a per-packet replay of
ugo/listener.go:64-119 on random traffic, the closed form of THE RULE against
the walk, and one directed case per deviation.  GPU: the device against the
rule through tests/listen_harness.py -- every output array, the state and the
entry dump after every call.
"""
import ctypes
import struct

import numpy as np
import pytest
import torch

import listen_ref as lr
from listen_harness import Guarded, ListenHarness, _put
from stream_harness import enc, pad_bytes  # noqa: F401  (fixtures)
from ugo_amd import fec

NO_CONN = lr.NO_CONN
SLOT = 48


def batch_of(items, slot=SLOT, seed=0):
    """[(name row, packet bytes, lens or None)] -> (names, pkts, lens); what
    follows a packet's bytes in its slot is arbitrary."""
    n = len(items)
    names = np.zeros((n, 32), np.uint8)
    pkts = np.random.default_rng(seed).integers(0, 256, (n, slot), dtype=np.uint8)
    lens = np.zeros(n, np.uint16)
    for i, (row, data, length) in enumerate(items):
        names[i] = np.frombuffer(row, np.uint8)
        pkts[i, :len(data)] = np.frombuffer(bytes(data), np.uint8)
        lens[i] = len(data) if length is None else length
    return names, pkts, lens


def v4(k, port=4000):
    return lr.name_v4(bytes([10, (k >> 16) & 255, (k >> 8) & 255, k & 255]), port)


def data(n=30, first=0x41):
    return bytes([first]) + bytes(range(1, n))


def init(cid, byte1=0):
    return lr.init_packet(cid, byte1)


# ================================================================ CPU
def test_symbols_constants_and_layouts():
    lib = fec.load_library()
    want = {"ugo_fec_listen_" + s for s in ("create", "destroy", "state", "route", "remap", "names", "entries")}
    assert want <= set(fec.header_symbols())
    for s in want:
        assert hasattr(lib, s)
    assert lib.ugo_fec_abi_version() == 9
    assert fec.KERNEL_NAMES[15] == "listen" and fec.KERNEL_IDS["listen"] == 15
    assert (fec.LISTEN_FED, fec.LISTEN_FED_NEW, fec.LISTEN_DUP_INIT, fec.LISTEN_ACCEPT, fec.LISTEN_STRANGER,
            fec.LISTEN_REFUSED, fec.LISTEN_BAD_NAME) == (lr.FED, lr.FED_NEW, lr.DUP_INIT, lr.ACCEPT, lr.STRANGER,
                                                         lr.REFUSED, lr.BAD_NAME)
    assert fec.LISTEN_FULL == lr.FULL and fec.STREAM_NO_CONN == NO_CONN
    src = open(fec.LISTEN_HEADER_PATH).read()
    for name, value in (("UGO_LISTEN_REFUSED", 5), ("UGO_LISTEN_BAD_NAME", 6), ("UGO_LISTEN_FULL", 1),
                        ("UGO_FEC_KERNEL_LISTEN", 15), ("UGO_LISTEN_REMAP_LENGTH", 8)):
        assert f"#define {name} {value}" in src
    # no table: every entry point is an argument error, nothing is launched
    assert lib.ugo_fec_listen_create(None, 8, None) == 6
    assert lib.ugo_fec_listen_state(None, None) == 6
    assert lib.ugo_fec_listen_route(None, None, None, 48, None, 1, None, None, None, 0, None, None) == 6
    assert lib.ugo_fec_listen_remap(None, None, 0, 0, None, None) == 6
    assert lib.ugo_fec_listen_names(None, None, 1, None, None, None) == 6
    assert lib.ugo_fec_listen_entries(None, None, 1, None) == 6
    lib.ugo_fec_listen_destroy(None)
    with pytest.raises(ValueError):
        fec.ListenTable(None, 0)
    with pytest.raises(ValueError):
        fec.ListenTable(None, (1 << 20) + 1)


def test_the_key_is_what_the_string_distinguishes():
    ip4, ip6 = bytes([192, 0, 2, 7]), bytes([0x20, 1, 0xd, 0xb8]) + bytes(11) + b"\x01"
    same = [lr.name_v4(ip4, 5000), lr.name_v4(ip4, 5000, tail=b"\x99" * 16), lr.name_v6(lr.mapped(ip4), 5000),
            lr.name_v6(lr.mapped(ip4), 5000, flowinfo=77, tail=b"\x01\x02\x03\x04")]
    assert len({lr.addr_string(r) for r in same}) == 1 and lr.addr_string(same[0]) == "192.0.2.7:5000"
    apart = [same[0], lr.name_v4(ip4, 5001), lr.name_v6(lr.mapped(ip4), 5000, scope=3), lr.name_v6(ip6, 5000),
             lr.name_v6(ip6, 5000, scope=2), lr.name_v6(ip6, 5000, scope=5), lr.name_v6(ip6, 5001),
             lr.name_v4(bytes([192, 0, 2, 8]), 5000)]
    assert len({lr.addr_string(r) for r in apart}) == len(apart)
    assert lr.addr_string(lr.name_v6(ip6, 5000, scope=2)) == "[2001:db8::1%2]:5000"
    assert lr.addr_string(lr.name_v6(ip6, 5000, flowinfo=9)) == lr.addr_string(lr.name_v6(ip6, 5000))
    assert lr.addr_string(lr.name_other(17)) is None and lr.addr_string(lr.name_other(0)) is None
    assert lr.entry_of(lr.clean_row(same[0]), 3) == lr.entry_of(lr.clean_row(same[3]), 3)
    assert lr.clean_row(same[3]) == lr.name_v6(lr.mapped(ip4), 5000) and lr.clean_row(same[1]) == lr.name_v4(ip4, 5000, tail=b"\x99" * 8)


def _replay(seed, batches, n):
    """Random traffic through GoListener one packet at a time and through
    RuleListener one batch at a time; returns what was seen, for coverage."""
    tr = lr.Traffic(seed)
    go, rule = lr.GoListener(), lr.RuleListener(4096)
    seen = set()
    for _ in range(batches):
        names, pkts, lens = tr.batch(n)
        known = dict(rule.members)
        nconn = rule.nconn
        conn_of, cls, accepted = rule.route(names, pkts, lens, tr.slot)
        assert not rule.unspecified and rule.n_dead == 0
        # THE RULE in the header's words is the walk
        assert (conn_of, cls, [(a[0], a[1]) for a in accepted]) == lr.rule_by_first(known, names, pkts, lens,
                                                                                    tr.slot, nconn, 4096)
        acc = {a[0]: a for a in accepted}
        for i in range(n):
            key = lr.addr_string(bytes(names[i]))
            if key is None:
                assert cls[i] == lr.BAD_NAME and conn_of[i] == NO_CONN   # not a *net.UDPAddr: never reaches Go
                continue
            buf = bytes(pkts[i, :min(int(lens[i]), tr.slot)])
            what, conn = go.handle_packet(key, buf)
            want = {"fed": (lr.FED, lr.FED_NEW), "dup": (lr.DUP_INIT,), "accept": (lr.ACCEPT,),
                    "drop": (lr.STRANGER,)}[what]
            assert cls[i] in want, (i, what, cls[i])
            assert conn_of[i] == (conn if what == "fed" else NO_CONN)
            if what == "fed":
                assert (cls[i] == lr.FED_NEW) == (conn >= nconn)
            if what == "accept":
                assert acc[i][1] == conn and go.pending[conn] == (key, acc[i][2])
                assert lr.addr_string(acc[i][3]) == key
            seen.add((what, len(buf) if len(buf) in (21, 22, 23) else 0, buf[1] != 0 if len(buf) > 1 else None))
        assert len(go.pending) == rule.nconn and go.connections == rule.members
    return seen, tr, rule


def test_rule_against_a_replay_of_listener_go():
    seen = set()
    for seed in range(6):
        s, tr, rule = _replay(seed, batches=4, n=700)
        seen |= s
    labels = {l for l, _ in tr.pool}
    assert {"v4", "v4 other port", "v4-mapped, the same key as v4", "v4-mapped with a scope", "v6",
            "v6 other flowinfo, the same key", "v6 scope", "v6 other scope", "v6 no scope"} == labels
    # a known key's INIT with byte 1 != 0 is fed, an unknown key's accepted: the asymmetry
    assert ("fed", 22, True) in seen and ("accept", 22, True) in seen and ("dup", 22, False) in seen
    for what in ("fed", "drop"):
        for length in (21, 22, 23):
            assert any(w == what and l == length for w, l, _ in seen), (what, length)
    # the same key under two spellings is one connection
    row4 = tr.pool[0][1]
    row6 = tr.pool[2][1]
    assert lr.addr_string(row4) == lr.addr_string(row6)


def test_deviation_a_no_queue_of_1024():
    a = v4(1)
    items = [(a, init(7), None)] + [(a, data(), None)] * (lr.QUEUE + 6)
    names, pkts, lens = batch_of(items)
    go, rule = lr.GoListener(), lr.RuleListener(4)
    got = [go.handle_packet(lr.addr_string(bytes(r)), bytes(p[:l]))[0] for r, p, l in zip(names, pkts, lens)]
    assert got == ["accept"] + ["fed"] * lr.QUEUE + ["full"] * 6
    conn_of, cls, _ = rule.route(names, pkts, lens, SLOT)
    assert cls == [lr.ACCEPT] + [lr.FED_NEW] * (lr.QUEUE + 6) and conn_of[1:] == [0] * (lr.QUEUE + 6)


def test_deviation_b_refusal_past_max_conn():
    rule = lr.RuleListener(2)
    items = [(v4(1), init(1), None), (v4(2), init(2), None), (v4(3), data(), None), (v4(3), init(3), None),
             (v4(3), data(), None), (v4(3), init(33), None), (v4(4), init(4, 9), None), (v4(1), data(), None)]
    conn_of, cls, acc = rule.route(*batch_of(items), SLOT)
    assert cls == [lr.ACCEPT, lr.ACCEPT, lr.STRANGER, lr.REFUSED, lr.STRANGER, lr.STRANGER, lr.REFUSED, lr.FED_NEW]
    assert conn_of == [NO_CONN] * 7 + [0] and len(acc) == 2 and rule.n_dead == 2 and rule.nconn == 2
    # a dead key stays unknown: refused again, no other dead slot; the reference would have accepted
    conn_of, cls, acc = rule.route(*batch_of([(v4(3), data(), None), (v4(3), init(3), None)]), SLOT)
    assert cls == [lr.STRANGER, lr.REFUSED] and rule.n_dead == 2 and not acc
    assert rule.remap([0, NO_CONN], 1) == 0 and rule.n_dead == 0 and rule.nconn == 1
    conn_of, cls, acc = rule.route(*batch_of([(v4(3), init(3), None), (v4(3), data(), None)]), SLOT)
    assert cls == [lr.ACCEPT, lr.FED_NEW] and conn_of == [NO_CONN, 1] and acc[0][:3] == (0, 1, 3)


def test_deviation_c_the_table_fills():
    rule = lr.RuleListener(8)
    assert rule.n_slots == 16
    rule.route(*batch_of([(v4(k), init(k), None) for k in range(16)]), SLOT)
    assert (rule.nconn, rule.n_dead, rule.err, rule.unspecified) == (8, 8, 0, False)   # 16 of 16 slots held
    rule.route(*batch_of([(v4(3), data(), None), (v4(12), init(1), None)]), SLOT)      # a dead key has its slot
    assert rule.err == 0
    conn_of, cls, _ = rule.route(*batch_of([(v4(3), data(), None), (v4(99), init(1), None)]), SLOT)
    assert rule.err == lr.FULL and rule.unspecified and (conn_of[0], cls[0]) == (3, lr.FED)
    assert rule.remap(list(range(8)), 8) == 0 and rule.err == 0 and rule.n_dead == 0


def test_deviation_d_ciphertext_that_looks_like_an_init():
    """22 bytes of data whose first byte is 0: an unknown key is accepted on it,
    a known key loses it as a dup-INIT when byte 1 is 0 too -- as the reference."""
    go, rule = lr.GoListener(), lr.RuleListener(4)
    look = bytes([0, 0]) + bytes(range(20))
    items = [(v4(1), look, None), (v4(1), look, None), (v4(1), bytes([0, 5]) + bytes(20), None)]
    names, pkts, lens = batch_of(items)
    assert [go.handle_packet(lr.addr_string(bytes(r)), bytes(p[:l]))[0] for r, p, l in zip(names, pkts, lens)] == \
        ["accept", "dup", "fed"]
    conn_of, cls, acc = rule.route(names, pkts, lens, SLOT)
    assert cls == [lr.ACCEPT, lr.DUP_INIT, lr.FED_NEW] and acc[0][2] == struct.unpack(">I", look[18:22])[0]


def test_rule_remap_statuses():
    rule = lr.RuleListener(4)
    rule.route(*batch_of([(v4(k), init(k), None) for k in range(3)]), SLOT)
    before = (dict(rule.members), dict(rule.rows), rule.nconn)
    assert rule.remap([0, 0, 1], 3) == lr.REMAP_NOT_INJECTIVE
    assert rule.remap([0, 1, 3], 3) == lr.REMAP_OUT_OF_RANGE
    assert rule.remap([0, 1, 2], 5) == lr.REMAP_TOO_MANY
    assert rule.remap([0, 1], 3) == lr.REMAP_LENGTH
    assert rule.remap([5, 5, 1], 3) == lr.REMAP_OUT_OF_RANGE      # both out of range: not counted as a clash
    assert before == (rule.members, rule.rows, rule.nconn)
    assert rule.remap([2, NO_CONN, 0], 3) == 0
    assert rule.entries() == [lr.entry_of(v4(2), 0), lr.entry_of(v4(0), 2)]
    assert rule.names([0, 1, 2, 3, NO_CONN])[1] == [16, 0, 16, 0, 0]


# ================================================================ GPU
@pytest.fixture()
def harness(enc):
    made = []

    def make(max_conn):
        made.append(ListenHarness(enc, max_conn))
        return made[-1]

    yield make
    for h in made:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["device", "pinned"])
def test_directed_one_wave(harness, where):
    h = harness(16)
    a, b, c, d = v4(1), lr.name_v6(bytes([0x20, 1]) + bytes(range(14)), 700, scope=0, flowinfo=5), v4(3), v4(4)
    b_other_flow = lr.name_v6(bytes([0x20, 1]) + bytes(range(14)), 700, flowinfo=0xdeadbeef, tail=b"\x77" * 4)
    h.route(*batch_of([(a, init(0xA1), None), (b, init(0xB1), None)]), where=where)   # a and b known from here on
    items = [
        (c, data(), None),                 # before its INIT: STRANGER
        (c, data(22, first=1), None),      # 22 bytes, byte 0 != 0: no INIT
        (c, init(0xC1, 7), None),          # ACCEPT (an unknown key's INIT is judged by byte 0)
        (c, data(), None),                 # FED_NEW
        (c, init(0xC2), None),             # the key's second INIT, a dup-INIT now
        (c, init(0xC3, 7), None),          # byte 1 != 0 from a key known by now: fed
        (a, init(0xA2), None),             # dup-INIT of a known key
        (a, init(0xA3, 1), None),          # byte 1 != 0 from a known key: FED
        (a, data(), None),
        (b_other_flow, data(), None),      # another flowinfo, junk behind the address: the same key
        (lr.name_v6(lr.mapped(bytes([10, 0, 0, 1])), 4000), data(), None),   # v4-mapped a
        (lr.name_other(17), init(1), None),                                # no address
        (lr.name_other(0x0a00), data(), None),
        (a, b"", 0),                       # lens 0
        (a, init(0xA4), 21), (a, init(0xA5) + b"\0", 23),                  # 21 and 23 bytes: data
        (d, init(0xD1)[:21] + b"\x55" * 27, SLOT + 9),                     # lens > slot: clamped to the slot, no INIT
        (d, init(0xD1), None),                                           # d's INIT
        (d, init(0xD2), None), (d, data(), SLOT + 1000),
    ]
    conn, cls, acc, n_acc = h.route(*batch_of(items), where=where)
    assert cls.tolist() == [4, 4, 3, 1, 2, 1, 2, 0, 0, 0, 0, 6, 6, 0, 0, 0, 4, 3, 2, 1]
    assert n_acc == 2 and acc["client_id"].tolist() == [0xC1, 0xD1] and acc["member"].tolist() == [2, 3]
    h.names([0, 1, 2, 3, 4, NO_CONN], where=where)


@pytest.mark.gpu
def test_first_init_tie_break(harness):
    """One new key's INITs in two lanes of a wave, in two waves of a block and
    in two blocks; member numbers follow the batch order of the first INITs,
    which crosses the pieces of the numbering scan."""
    h = harness(64)
    known = [v4(100 + k) for k in range(5)]
    h.route(*batch_of([(r, init(k), None) for k, r in enumerate(known)]))
    n = 4099
    rng = np.random.default_rng(5)
    items = [(known[int(rng.integers(5))], data(int(rng.integers(23, 40))), None) for _ in range(n)]
    k1, k2, k3, k4, k5 = (v4(200 + k) for k in range(5))
    inits = {5: (k1, 0x15), 9: (k1, 0x19), 70: (k2, 0x270), 200: (k2, 0x2200), 3900: (k3, 0x33900),
             4098: (k3, 0x34098), 4000: (k4, 0x44000), 100: (k4, 0x40100), 4097: (k5, 0x54097), 300: (k5, 0x50300),
             2: (k5, 0x50002)}
    for i, (row, cid) in inits.items():
        items[i] = (row, init(cid, byte1=i % 2), None)
    for i, row in ((0, k1), (7, k1), (12, k1), (150, k2), (255, k2), (256, k2), (50, k4), (3000, k4), (4096, k3),
                   (3899, k3), (3901, k3), (1, k5), (3, k5)):
        items[i] = (row, data(), None)
    conn, cls, acc, n_acc = h.route(*batch_of(items))
    assert acc["packet"].tolist() == [2, 5, 70, 100, 3900] and acc["member"].tolist() == [5, 6, 7, 8, 9]
    assert acc["client_id"].tolist() == [0x50002, 0x15, 0x270, 0x40100, 0x33900]
    assert cls[[0, 7, 12, 9]].tolist() == [lr.STRANGER, lr.FED_NEW, lr.FED_NEW, lr.FED_NEW]   # 9: byte 1 != 0
    assert cls[[200, 4098, 4000, 300]].tolist() == [lr.DUP_INIT] * 4 and conn[4097] == 5


@pytest.mark.gpu
def test_pieces_of_two_tiles(harness):
    """More than 1,024 tiles: a block of the numbering scan walks two tiles."""
    h = harness(256)
    n = 1024 * 256 + 300
    rng = np.random.default_rng(9)
    known = np.stack([np.frombuffer(v4(k), np.uint8) for k in range(40)])
    h.route(known, *batch_of([(v4(0), init(k), None) for k in range(40)])[1:])
    names = known[rng.integers(0, 40, n)]
    pkts = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens = rng.integers(23, 33, n).astype(np.uint16)
    at = np.sort(rng.choice(n, 150, replace=False))
    at[-1] = n - 1
    for j, i in enumerate(at):                      # 50 new keys, three INITs each, the last in the last lane
        names[i] = np.frombuffer(v4(1000 + j % 50), np.uint8)
        pkts[i, :22] = np.frombuffer(init(int(i)), np.uint8)
        lens[i] = 22
    conn, cls, acc, n_acc = h.route(names, pkts, lens, entries=False)
    assert n_acc == 50 and acc["packet"].tolist() == at[:50].tolist()
    h.check()


@pytest.mark.gpu
def test_probing_refusal_fill_and_remap(harness):
    """The smallest table: 8 members in 16 slots.  Keys arrive in random order
    over several calls; dead slots then fill the table until chains wrap its
    end and every probe walks all of it; every key is still found."""
    h = harness(8)
    rng = np.random.default_rng(11)
    rows = [v4(int(k), port=int(p)) for k, p in zip(rng.integers(0, 1 << 24, 40), rng.integers(1, 65536, 40))]
    order = rng.permutation(8)
    for part in (order[:3], order[3:4], order[4:]):
        h.route(*batch_of([(rows[k], init(int(k)), None) for k in part] + [(rows[k], data(), None) for k in order]))
    everyone = [(rows[k], data(), None) for k in range(8)]
    conn, cls, _, _ = h.route(*batch_of(everyone))
    assert sorted(conn.tolist()) == list(range(8))
    # past max_conn: REFUSED, and n_dead rises
    conn, cls, acc, n_acc = h.route(*batch_of([(rows[8], data(), None), (rows[8], init(8), None),
                                               (rows[8], init(88), None)] + everyone))
    assert cls[:3].tolist() == [lr.STRANGER, lr.REFUSED, lr.STRANGER] and n_acc == 0 and h.rule.n_dead == 1
    h.route(*batch_of([(rows[k], init(int(k)), None) for k in range(9, 15)] + everyone + [(rows[8], init(8), None)]))
    assert h.rule.n_dead == 7                        # 15 of 16 slots held: one chain round the table's end
    conn, cls, _, _ = h.route(*batch_of(everyone + [(rows[15], init(1), None), (rows[30], data(), None)]))
    assert h.rule.n_dead == 8 and sorted(conn[:8].tolist()) == list(range(8))          # 16 of 16
    conn, cls, _, _ = h.route(*batch_of(everyone + [(rows[12], init(1), None), (rows[31], data(), None)]))
    assert cls[8:].tolist() == [lr.REFUSED, lr.STRANGER] and int(h.table.state()["err"]) == 0
    # deviation (c): two more keys than slots
    items = everyone + [(rows[20], init(1), None), (rows[0], init(5), None), (rows[21], init(2), None)] + everyone
    names, pkts, lens = batch_of(items)
    dn, dp, dl = _put(names), _put(pkts), _put(lens.view(np.int16))
    conn, cls, acc, n_acc = h.table.route(dn, dp, dl)
    dead = set(h.rule.dead)
    w_conn, w_cls, _ = h.rule.route(names, pkts, lens, SLOT)
    assert h.rule.unspecified
    st = h.table.state()
    assert (int(st["err"]), int(st["nconn"]), int(st["n_dead"])) == (lr.FULL, 8, 8) and int(n_acc.item()) == 0
    conn, cls = conn.cpu().numpy().view(np.uint32), cls.cpu().numpy()
    keep = [i for i in range(len(items)) if i not in (8, 10)]
    assert cls[keep].tolist() == [w_cls[i] for i in keep] and conn[keep].tolist() == [w_conn[i] for i in keep]
    assert cls[9] == lr.DUP_INIT                                                 # a known key routes exactly
    assert set(cls[[8, 10]].tolist()) == {lr.STRANGER} and (conn[[8, 10]] == NO_CONN).all()
    got = h.table.entries()
    assert got["member"].tolist() == list(range(8)) and len({e.tobytes() for e in got[["ip", "scope", "port"]]}) == 8
    # the rule takes the device's word for what is unspecified, then both go on together
    h.rule.dead = dead
    h.rule.counts = st["counts"].tolist()
    h.remap(list(range(8)), 8)                       # clears the error and the dead slots
    assert int(h.table.state()["err"]) == 0 and int(h.table.state()["n_dead"]) == 0
    conn, cls, _, _ = h.route(*batch_of(everyone + [(rows[20], init(1), None)]))
    assert cls[8] == lr.REFUSED and sorted(conn[:8].tolist()) == list(range(8))


@pytest.mark.gpu
def test_remap_renumber_close_and_accept_again(harness):
    h = harness(12)
    rows = [v4(1), lr.name_v6(bytes([0xfe, 0x80]) + bytes(13) + b"\x01", 9, scope=2), v4(3), v4(4),
            lr.name_v6(lr.mapped(bytes([9, 9, 9, 9])), 9), v4(6)]
    h.route(*batch_of([(r, init(k), None) for k, r in enumerate(rows)]))
    everyone = [(r, data(), None) for r in rows]
    h.remap([5, 4, 3, 2, 1, 0], 6)                                   # renumbering
    conn, _, _, _ = h.route(*batch_of(everyone))
    assert conn.tolist() == [5, 4, 3, 2, 1, 0]
    h.remap([0, NO_CONN, 1, NO_CONN, 2, 3], 4)                       # closing two
    conn, cls, _, _ = h.route(*batch_of(everyone))
    assert conn.tolist() == [3, 2, NO_CONN, 1, NO_CONN, 0] and cls[[2, 4]].tolist() == [lr.STRANGER] * 2
    conn, cls, acc, _ = h.route(*batch_of([(rows[2], init(0x22), None)] + everyone))   # the same address again
    assert acc["member"].tolist() == [4] and conn[3] == 4 and cls[3] == lr.FED_NEW
    h.names(list(range(8)))
    # maps that are refused leave every byte as it was
    all_names = h.names(list(range(12)))[0].tobytes()
    for bad, nconn_new, want in (([0, 1, 2, 3, 3], 5, lr.REMAP_NOT_INJECTIVE), ([0, 1, 2, 3, 5], 5, 2),
                                 ([0, 1, 2, 3, 4], 13, lr.REMAP_TOO_MANY), ([0, 1, 2, 3], 4, lr.REMAP_LENGTH),
                                 ([7, 7, NO_CONN, 1, 1], 3, 3), ([0, 1, 2, 3, 4, 5], 6, lr.REMAP_LENGTH)):
        assert h.remap(bad, nconn_new) == want
        assert h.names(list(range(12)))[0].tobytes() == all_names
    conn, _, _, _ = h.route(*batch_of(everyone))
    assert conn.tolist() == [3, 2, 4, 1, NO_CONN, 0]
    h.remap([1, 2, 3, 4, 6], 8)                                       # numbers 0, 5 and 7 without an entry
    h.names(list(range(9)))
    conn, _, acc, _ = h.route(*batch_of(everyone + [(rows[4], init(1), None)]))
    assert conn[:6].tolist() == [4, 3, 6, 2, NO_CONN, 1] and acc["member"].tolist() == [8]
    h.remap([NO_CONN] * 9, 0)                                         # everything closed
    assert len(h.table.entries()) == 0


@pytest.mark.gpu
def test_32769_members(harness):
    n = 32769
    h = harness(n)
    rng = np.random.default_rng(3)
    names = np.zeros((n, 32), np.uint8)
    names[:, 0] = 2
    names[:, 2:4] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    names[:, 4:8] = np.arange(n, dtype=">u4").view(np.uint8).reshape(n, 4)
    pkts = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pkts[:, 0] = 0
    lens = np.full(n, 22, np.uint16)
    conn, cls, acc, n_acc = h.route(names, pkts, lens)
    assert n_acc == n and (cls == lr.ACCEPT).all()
    idx = (n - 1 - np.arange(n)).astype(np.uint32)
    h.remap(idx, n)
    pkts[:, 0] = 1
    conn, cls, _, _ = h.route(names, pkts, lens, entries=False)
    assert np.array_equal(conn, idx) and (cls == lr.FED).all()
    keep = np.arange(n) % 7 != 0
    idx = np.where(keep, np.cumsum(keep) - 1, NO_CONN).astype(np.uint32)
    h.remap(idx, int(keep.sum()))
    conn, cls, _, _ = h.route(names, pkts, lens, entries=False)
    assert np.array_equal(conn[::-1], idx)


@pytest.mark.gpu
def test_replay_is_deterministic(enc):
    """100,000 packets with 3,000 new keys of 2-5 INITs each into two fresh
    tables: byte-identical outputs and entry dumps, and the rule's."""
    n, nk = 100000, 3000
    rng = np.random.default_rng(17)
    keys = np.zeros((nk + 500, 32), np.uint8)
    for k in range(nk + 500):
        row = lr.name_v6(bytes(rng.integers(0, 256, 16, dtype=np.uint8)), int(rng.integers(1, 65536)),
                         scope=int(rng.integers(0, 3))) if k % 3 else v4(k, port=int(rng.integers(1, 65536)))
        keys[k] = np.frombuffer(row, np.uint8)
    names = keys[rng.integers(0, nk + 500, n)]
    pkts = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens = rng.integers(20, 33, n).astype(np.uint16)
    lens[lens == 22] = 24
    for k in range(nk):
        for i in rng.choice(n, int(rng.integers(2, 6)), replace=False):
            names[i] = keys[k]
            pkts[i, :22] = np.frombuffer(init(int(i), byte1=int(i) % 3 == 0), np.uint8)
            lens[i] = 22
    h = ListenHarness(enc, 4096)                          # the first replay is held against the rule
    conn, cls, acc, n_acc = h.route(names, pkts, lens)
    first = (conn.tobytes(), cls.tobytes(), acc.tobytes(), n_acc, h.table.state().tobytes(),
             h.table.entries().tobytes())
    h.close()
    t = fec.ListenTable(enc, 4096)                        # the second against the first
    conn, cls, acc, n = t.route(_put(names), _put(pkts), _put(lens.view(np.int16)))
    n = int(n.item())
    second = (conn.cpu().numpy().tobytes(), cls.cpu().numpy().tobytes(), acc.cpu().numpy()[:n].tobytes(), n,
              t.state().tobytes(), t.entries().tobytes())
    t.close()
    assert first == second and 2900 <= n_acc <= nk


@pytest.mark.gpu
def test_names_rows_and_lengths(harness):
    h = harness(5)
    rows = [v4(1), lr.name_v6(bytes([0x20, 1]) + bytes(14), 443, scope=4, flowinfo=0x01020304, tail=b"\xee" * 4),
            lr.name_v4(bytes([1, 2, 3, 4]), 80, tail=b"\xcc" * 24)]
    h.route(*batch_of([(r, init(k), None) for k, r in enumerate(rows)]))
    got, lens = h.names([1, 0, 2, 2, NO_CONN, 3, 4, 5, 1 << 31, 0xfffffffe, 1])
    assert lens.tolist() == [28, 16, 16, 16, 0, 0, 0, 0, 0, 0, 28]
    assert got[0].tobytes() == lr.name_v6(bytes([0x20, 1]) + bytes(14), 443, scope=4)
    assert got[2].tobytes() == lr.name_v4(bytes([1, 2, 3, 4]), 80, tail=b"\xcc" * 8)
    h.names([2] * 300 + [7], where="pinned")


@pytest.mark.gpu
def test_argument_rules(enc):
    lib = fec.load_library()
    t = fec.ListenTable(enc, 8)
    n = 4
    names, pkts, lens = batch_of([(v4(k), init(k), None) for k in range(n)])
    g = [Guarded(32 * n + 16, 1), Guarded(SLOT * n + 16, 2), Guarded(2 * n + 2, 3), Guarded(4 * n + 4, 4),
         Guarded(n, 5), Guarded(48 * n + 16, 6), Guarded(8, 7)]
    dn, dp, dl, dc, dk, da, dna = (x.t.data_ptr() for x in g)
    ok = [t._h, dn, dp, SLOT, dl, n, dc, dk, da, n, dna, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.ugo_fec_listen_route(*a)

    host = np.zeros(4096, np.uint8)
    pageable = host.ctypes.data + (-host.ctypes.data) % 16
    bad = [dict(_0=None), dict(_1=None), dict(_2=None), dict(_4=None), dict(_6=None), dict(_7=None), dict(_8=None),
           dict(_10=None), dict(_1=dn + 8), dict(_1=dn + 4), dict(_2=dp + 8), dict(_3=0), dict(_3=24), dict(_3=65536),
           dict(_3=65552), dict(_4=dl + 1), dict(_6=dc + 2), dict(_8=da + 8), dict(_10=dna + 2),
           dict(_5=(1 << 31) + 1), dict(_1=pageable), dict(_2=pageable), dict(_4=pageable), dict(_6=pageable),
           dict(_7=pageable), dict(_8=pageable), dict(_10=pageable)]
    for kw in bad:
        assert call(**kw) == 6, kw
    assert call(_5=0) == 0 and call(_5=0, _1=None, _2=None, _6=None) == 0          # npackets == 0: a no-op
    assert lib.ugo_fec_listen_names(t._h, None, n, dn, dc, None) == 6
    assert lib.ugo_fec_listen_names(t._h, dc, n, dn + 8, dc, None) == 6
    assert lib.ugo_fec_listen_names(t._h, dc, n, dn, None, None) == 6
    assert lib.ugo_fec_listen_names(t._h, pageable, n, dn, dc, None) == 6
    assert lib.ugo_fec_listen_names(t._h, None, 0, None, None, None) == 0
    assert lib.ugo_fec_listen_remap(t._h, dc, n, n, None, None) == 6
    assert lib.ugo_fec_listen_remap(t._h, None, n, n, dna, None) == 6
    assert lib.ugo_fec_listen_remap(t._h, dc + 2, n, n, dna, None) == 6
    assert lib.ugo_fec_listen_remap(t._h, dc, n, n, pageable, None) == 6
    assert lib.ugo_fec_listen_remap(t._h, dc, (1 << 20) + 1, n, dna, None) == 6
    assert lib.ugo_fec_listen_entries(t._h, None, 8, None) == 6
    assert lib.ugo_fec_listen_entries(t._h, da + 8, 2, None) == 6
    assert lib.ugo_fec_listen_entries(t._h, da, 0, None) == 6
    assert lib.ugo_fec_listen_entries(t._h, pageable, 8, None) == 6
    assert lib.ugo_fec_listen_state(t._h, None) == 6
    h = ctypes.c_void_p()
    assert lib.ugo_fec_listen_create(enc._h, 0, ctypes.byref(h)) == 6 and not h.value
    assert lib.ugo_fec_listen_create(enc._h, (1 << 20) + 1, ctypes.byref(h)) == 6
    assert lib.ugo_fec_listen_create(enc._h, 8, None) == 6
    st = t.state()
    assert int(st["nconn"]) == 0 and not st["counts"].any() and int(st["n_slots"]) == 16
    for x in g:                                             # nothing was written by any of it
        assert np.array_equal(x.read(), x.fill[64:64 + x.nbytes])
    with pytest.raises(ValueError):
        t.route(torch.zeros((n, 31), dtype=torch.uint8, device="cuda"), g[1].t[:SLOT * n].view(n, SLOT),
                g[2].t[:2 * n].view(torch.int16))
    # no list wanted: the members exist and the full count is reported
    g[0].t[:32 * n].copy_(torch.from_numpy(names).reshape(-1))
    g[1].t[:SLOT * n].copy_(torch.from_numpy(pkts).reshape(-1))
    g[2].t[:2 * n].copy_(torch.from_numpy(lens.view(np.uint8)))
    assert call(_8=None, _9=0) == 0
    assert int(t.state()["nconn"]) == n and g[6].read().view(np.uint32)[0] == n
    assert np.array_equal(g[5].read(), g[5].fill[64:64 + g[5].nbytes])
    t.close()


@pytest.mark.gpu
def test_max_accepted_truncates_the_list_only(harness):
    h = harness(16)
    items = [(v4(k), init(k), None) for k in range(6)]
    conn, cls, acc, n_acc = h.route(*batch_of(items), max_accepted=4)
    assert n_acc == 6 and len(acc) == 4 and int(h.table.state()["nconn"]) == 6
    conn, _, _, _ = h.route(*batch_of([(v4(k), data(), None) for k in range(6)]), max_accepted=0)
    assert conn.tolist() == list(range(6))


@pytest.mark.gpu
def test_chain_route_decode_deliver_read(enc, pad_bytes):
    """Two batches through route -> packet_decode -> set_deliver with conn_of
    never leaving the device.  A connects in batch 1 and is served in it; B
    connects in batch 2, the set is rebuilt, and both streams are read back."""
    rng = np.random.default_rng(23)
    slot, ms = 512, 1
    dpad = torch.from_numpy(pad_bytes[:slot]).cuda()

    def wire_of(stream_bytes, first_number):
        """The stream as encrypted one-segment packets of 300 bytes."""
        npk = len(stream_bytes) // 300
        info = np.zeros(npk, fec.PKT_INFO_DTYPE)
        segs = np.zeros((npk, ms), fec.PKT_SEGMENT_DTYPE)
        for i in range(npk):
            info[i]["packet_number"], info[i]["n_segments"] = first_number + i, 1
            segs[i, 0] = (300 * i, 300 * i, 300, 300)
        wire, wl, status = enc.packet_encode(
            torch.from_numpy(info.view(np.uint8).reshape(npk, 64)).cuda(),
            torch.zeros((npk, 1, 2), dtype=torch.int64, device="cuda"),
            torch.from_numpy(segs.view(np.uint8).reshape(npk, ms, 16)).cuda(),
            torch.from_numpy(np.frombuffer(stream_bytes, np.uint8).copy()).cuda(), slot, pad=dpad)
        assert not status.any().item()
        return wire.cpu().numpy(), wl.cpu().numpy().view(np.uint16)

    sa, sb = rng.integers(0, 256, 6000, dtype=np.uint8).tobytes(), rng.integers(0, 256, 1500, dtype=np.uint8).tobytes()
    wa, la = wire_of(sa, 1)
    wb, lb = wire_of(sb, 1)
    A, B, X = v4(1), lr.name_v6(bytes([0x20, 1]) + bytes(range(14)), 9000), v4(9)

    def ring(parts):
        """[(name, wire rows, lens)] -> device names, pkts, lens"""
        names = np.concatenate([np.tile(np.frombuffer(r, np.uint8), (len(w), 1)) for r, w, _ in parts])
        return (torch.from_numpy(names).cuda(), torch.from_numpy(np.concatenate([w for _, w, _ in parts])).cuda(),
                torch.from_numpy(np.concatenate([l for _, _, l in parts]).view(np.int16)).cuda())

    def raw(data_bytes):
        w = np.zeros((1, slot), np.uint8)
        w[0, :len(data_bytes)] = np.frombuffer(data_bytes, np.uint8)
        return w, np.array([len(data_bytes)], np.uint16)

    table = fec.ListenTable(enc, 4)
    rxs, sets = [], []

    def batch(parts, want_new):
        names, pkts, lens = ring(parts)
        conn_of, cls, acc, n_acc = table.route(names, pkts, lens)
        info, _, segs = enc.packet_decode(pkts, lens, pad=dpad, max_ranges=1, max_segments=ms)
        assert int(n_acc.item()) == want_new                   # the one word the host reads, with the sizes
        for _ in range(want_new):                               # the host's share: windows and the set
            rxs.append(fec.StreamRx(enc, 8192))
        if sets:
            sets.pop().close()
        sets.append(fec.StreamRxSet(enc, rxs))
        sets[-1].deliver(pkts, info, segs, conn_of, pad=dpad)
        return conn_of, cls

    conn_of, cls = batch([(X, wa[:2], la[:2]), (A, *raw(init(0xAA))), (A, wa[:10], la[:10]), (X, wa[10:12], la[10:12])], 1)
    assert cls.tolist() == [4, 4, 3] + [1] * 10 + [4, 4]
    conn_of, cls = batch([(B, *raw(init(0xBB))), (A, wa[10:], la[10:]), (B, wb, lb), (X, wb[:1], lb[:1]),
                          (A, *raw(init(0xAA)))], 1)
    assert cls.tolist() == [3] + [0] * 10 + [1] * 5 + [4, 2]
    want = torch.tensor([7000, 7000], dtype=torch.int64, device="cuda")
    dst = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    n_read, eof = sets[-1].read(want, dst=dst, dst_off=torch.tensor([0, 8192], dtype=torch.int64, device="cuda"))
    assert n_read.tolist() == [6000, 1500]
    got = dst.cpu().numpy()
    assert got[:6000].tobytes() == sa and got[8192:8192 + 1500].tobytes() == sb
    nm, nl = table.names(conn_of)
    assert nl.tolist() == [0] + [16] * 10 + [28] * 5 + [0, 0]
    sets.pop().close()
    for rx in rxs:
        rx.close()
    table.close()
