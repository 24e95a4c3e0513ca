"""The connection table restated on the CPU; test infrastructure only.

GoListener is listener.handlePacket (ugo/listener.go:64-119) one packet at a
time, with its map keyed by remoteAddr.String() and its receivedPackets queue.

RuleListener is THE RULE of include/ugo_listen.h: the same per-packet walk, its
dict keyed by the string net.UDPAddr.String() would produce for the name row --
so the key normalisation of the device (16-byte IP, port, scope) is held
against the reference's own notion of equality -- plus the deviations (a)-(d),
remap, names and the entry dump.

rule_by_first() is THE RULE as the header words it (per key, with f the lowest
INIT of the call), the closed form the kernels compute; the tests hold it
against the walk.
"""
import functools
import ipaddress
import struct

import numpy as np

AF_INET, AF_INET6 = 2, 10
NO_CONN = 0xffffffff
FED, FED_NEW, DUP_INIT, ACCEPT, STRANGER, REFUSED, BAD_NAME = range(7)
NCLASS = 8
FULL = 1
REMAP_NOT_INJECTIVE, REMAP_OUT_OF_RANGE, REMAP_TOO_MANY, REMAP_LENGTH = 1, 2, 4, 8
QUEUE = 1024  # receivedPackets of conn.go


# ---------------------------------------------------------------- name rows
def name_v4(ip4: bytes, port: int, tail: bytes = b"") -> bytes:
    """sockaddr_in in a 32-byte row; tail fills what follows the address."""
    row = struct.pack("<H", AF_INET) + struct.pack(">H", port) + bytes(ip4)
    return (row + tail + bytes(32))[:32]


def name_v6(ip16: bytes, port: int, scope: int = 0, flowinfo: int = 0, tail: bytes = b"") -> bytes:
    """sockaddr_in6 in a 32-byte row."""
    row = (struct.pack("<H", AF_INET6) + struct.pack(">H", port) + struct.pack("<I", flowinfo) + bytes(ip16) +
           struct.pack("<I", scope))
    return (row + tail + bytes(32))[:32]


def name_other(family: int, fill: int = 0x5a) -> bytes:
    return struct.pack("<H", family) + bytes([fill]) * 30


def mapped(ip4: bytes) -> bytes:
    return bytes(10) + b"\xff\xff" + bytes(ip4)


@functools.lru_cache(maxsize=1 << 16)
def addr_string(row: bytes):
    """What remoteAddr.String() gives for the *net.UDPAddr recvmsg makes of the
    row (net/udpsock.go, ipsock.go): IP.String() prints a v4-mapped address as
    a dotted quad; a zone follows after '%'; JoinHostPort brackets a host with
    ':' or '%'.  A zone is rendered as its number.  None: no address."""
    family = struct.unpack_from("<H", row)[0]
    port = struct.unpack_from(">H", row, 2)[0]
    if family == AF_INET:
        host = ".".join(str(b) for b in row[4:8])
    elif family == AF_INET6:
        ip, scope = bytes(row[8:24]), struct.unpack_from("<I", row, 24)[0]
        if ip[:12] == bytes(10) + b"\xff\xff":
            host = ".".join(str(b) for b in ip[12:])
        else:
            host = ipaddress.IPv6Address(ip).compressed
        if scope:
            host += "%" + str(scope)
    else:
        return None
    if ":" in host or "%" in host:
        host = "[" + host + "]"
    return f"{host}:{port}"


def clean_row(row: bytes) -> bytes:
    """The row as accepted[] and the table keep it."""
    family = struct.unpack_from("<H", row)[0]
    if family == AF_INET:
        return bytes(row[:16]) + bytes(16)
    assert family == AF_INET6
    return bytes(row[:4]) + bytes(4) + bytes(row[8:28]) + bytes(4)


def entry_of(row: bytes, member: int):
    """(ip16, scope, port, member) of a kept row: the entry dump's row."""
    family = struct.unpack_from("<H", row)[0]
    port = struct.unpack_from(">H", row, 2)[0]
    if family == AF_INET:
        return (mapped(row[4:8]), 0, port, member)
    return (bytes(row[8:24]), struct.unpack_from("<I", row, 24)[0], port, member)


def name_len(row: bytes) -> int:
    return {AF_INET: 16, AF_INET6: 28}.get(struct.unpack_from("<H", row)[0], 0)


# ---------------------------------------------------------------- packets
def init_packet(client_id: int, byte1: int = 0, fill: int = 0x11) -> bytes:
    """22 bytes as Dial sends them: packetInit, the cipher, 16 bytes, the client's id."""
    return bytes([0, byte1]) + bytes([fill]) * 16 + struct.pack(">I", client_id)


def packet_len(length: int, slot: int) -> int:
    return min(length, slot)


def is_init(buf: bytes) -> bool:
    return len(buf) == 22 and buf[0] == 0


def is_dup_init(buf: bytes) -> bool:
    return len(buf) == 22 and buf[0] == 0 and buf[1] == 0


# ---------------------------------------------------------------- listener.go, one packet at a time
class GoListener:
    def __init__(self, queue=QUEUE):
        self.connections = {}  # remoteAddr.String() -> index into pending
        self.pending = []      # (string, clientConnectionID)
        self.queued = []       # len(conn.receivedPackets); nothing drains it inside a replay
        self.queue = queue

    def handle_packet(self, addr: str, buf: bytes):
        """('fed', conn) | ('full', conn) | ('dup', conn) | ('accept', conn) | ('drop', None)"""
        if addr in self.connections:
            conn = self.connections[addr]
            if len(buf) == 22 and buf[0] == 0 and buf[1] == 0:
                return ("dup", conn)
            if self.queued[conn] < self.queue:
                self.queued[conn] += 1
                return ("fed", conn)
            return ("full", conn)
        if len(buf) == 22:
            if buf[0] == 0:
                conn = len(self.pending)
                self.pending.append((addr, struct.unpack(">I", buf[18:22])[0]))
                self.queued.append(0)
                self.connections[addr] = conn
                return ("accept", conn)
        return ("drop", None)

    def close(self, addr: str):
        del self.connections[addr]


# ---------------------------------------------------------------- THE RULE
def slots_for(max_conn: int) -> int:
    n = 16
    while n < 2 * max_conn:
        n *= 2
    return n


class RuleListener:
    def __init__(self, max_conn: int):
        self.max_conn = max_conn
        self.n_slots = slots_for(max_conn)
        self.members = {}   # string -> member
        self.rows = {}      # member -> kept row
        self.dead = set()   # strings, deviation (b)
        self.nconn = 0
        self.err = 0
        self.counts = [0] * NCLASS
        self.unspecified = False  # deviation (c) struck in the last call

    @property
    def n_dead(self):
        return len(self.dead)

    def route(self, names, pkts, lens, slot):
        """names [n] rows, pkts [n] byte strings of slot bytes, lens [n].
        Returns (conn_of, cls, accepted) with accepted rows (packet, member,
        client_id, row)."""
        base, held = self.nconn, len(self.rows) + len(self.dead)
        conn_of, cls, accepted = [], [], []
        refused_now, claims = set(), set()
        for i, (row, raw, length) in enumerate(zip(names, pkts, lens)):
            buf = bytes(raw[:packet_len(length, slot)])
            key = addr_string(bytes(row))
            c, m = STRANGER, NO_CONN
            if key is None:
                c = BAD_NAME
            elif key in self.members:
                if is_dup_init(buf):
                    c = DUP_INIT
                else:
                    m = self.members[key]
                    c = FED if m < base else FED_NEW
            elif is_init(buf) and key not in refused_now:
                if key not in self.dead:
                    claims.add(key)
                if self.nconn < self.max_conn:
                    member = self.nconn
                    self.nconn += 1
                    self.members[key] = member
                    self.rows[member] = clean_row(bytes(row))
                    accepted.append((i, member, struct.unpack(">I", buf[18:22])[0], self.rows[member]))
                    c = ACCEPT
                else:
                    refused_now.add(key)
                    self.dead.add(key)
                    c = REFUSED
            conn_of.append(m)
            cls.append(c)
            self.counts[c] += 1
        # deviation (c): more keys in need of a slot than free slots
        self.unspecified = held + len(claims) > self.n_slots
        if self.unspecified:
            self.err = FULL
        return conn_of, cls, accepted

    def remap(self, new_index, nconn_new):
        status = 0
        if len(new_index) != self.nconn:
            status |= REMAP_LENGTH
        if nconn_new > self.max_conn:
            status |= REMAP_TOO_MANY
        kept = [v for v in new_index[:self.nconn] if v != NO_CONN]
        if any(v >= nconn_new for v in kept):
            status |= REMAP_OUT_OF_RANGE
        inside = [v for v in kept if v < nconn_new]
        if len(set(inside)) != len(inside):
            status |= REMAP_NOT_INJECTIVE
        if status:
            return status
        by_member = {m: k for k, m in self.members.items()}
        members, rows = {}, {}
        for m, v in enumerate(new_index):
            if v != NO_CONN and m in by_member:
                members[by_member[m]] = v
                rows[v] = self.rows[m]
        self.members, self.rows = members, rows
        self.dead = set()
        self.nconn, self.err = nconn_new, 0
        return 0

    def names(self, conn_of):
        rows, lens = [], []
        for m in conn_of:
            row = self.rows.get(m) if m < self.nconn else None
            rows.append(row if row is not None else bytes(32))
            lens.append(name_len(row) if row is not None else 0)
        return rows, lens

    def entries(self):
        return [entry_of(self.rows[m], m) for m in sorted(self.rows)]


def rule_by_first(known, names, pkts, lens, slot, nconn, max_conn):
    """THE RULE in the header's words, with room for every new key: known maps
    string -> member.  Returns (conn_of, cls, accepted as (packet, member))."""
    n = len(names)
    keys = [addr_string(bytes(r)) for r in names]
    bufs = [bytes(p[:packet_len(l, slot)]) for p, l in zip(pkts, lens)]
    first = {}
    for i in range(n):
        if keys[i] is not None and keys[i] not in known and is_init(bufs[i]):
            first.setdefault(keys[i], i)
    order = sorted(first.values())
    number = {keys[i]: nconn + r for r, i in enumerate(order)}
    assert nconn + len(order) <= max_conn
    conn_of, cls = [], []
    for i in range(n):
        k, c, m = keys[i], STRANGER, NO_CONN
        if k is None:
            c = BAD_NAME
        elif k in known or (k in first and i > first[k]):
            if is_dup_init(bufs[i]):
                c = DUP_INIT
            elif k in known:
                c, m = FED, known[k]
            else:
                c, m = FED_NEW, number[k]
        elif k in first and i == first[k]:
            c = ACCEPT
        conn_of.append(m)
        cls.append(c)
    return conn_of, cls, [(i, number[keys[i]]) for i in order]


# ---------------------------------------------------------------- traffic
class Traffic:
    """Random batches over a pool of addresses that covers what the key must
    tell apart and what it must not."""

    def __init__(self, seed, n_addr=40, slot=48):
        self.rng = np.random.default_rng(seed)
        self.slot = slot
        rng, pool = self.rng, []
        for _ in range(n_addr):
            ip4 = bytes(rng.integers(1, 255, 4, dtype=np.uint8))
            ip6 = bytes([0x20, 0x01]) + bytes(rng.integers(0, 256, 14, dtype=np.uint8))
            ll = bytes([0xfe, 0x80]) + bytes(6) + bytes(rng.integers(0, 256, 8, dtype=np.uint8))
            port = int(rng.integers(1024, 65535))
            pool += [
                ("v4", name_v4(ip4, port)),
                ("v4 other port", name_v4(ip4, port ^ 1)),
                ("v4-mapped, the same key as v4", name_v6(mapped(ip4), port)),
                ("v4-mapped with a scope", name_v6(mapped(ip4), port, scope=3)),
                ("v6", name_v6(ip6, port)),
                ("v6 other flowinfo, the same key", name_v6(ip6, port, flowinfo=int(rng.integers(1, 1 << 32)))),
                ("v6 scope", name_v6(ll, port, scope=2)),
                ("v6 other scope", name_v6(ll, port, scope=5)),
                ("v6 no scope", name_v6(ll, port)),
            ]
        self.pool = pool

    def batch(self, n, p_init=0.15, p_bad=0.02, junk=True):
        """(names [n,32], pkts [n,slot], lens [n]) as numpy arrays."""
        rng, slot = self.rng, self.slot
        names = np.zeros((n, 32), np.uint8)
        pkts = rng.integers(0, 256, (n, slot), dtype=np.uint8)
        lens = np.zeros(n, np.uint16)
        for i in range(n):
            row = bytearray(self.pool[int(rng.integers(len(self.pool)))][1])
            if junk:  # what follows the address is ignored
                row[name_len(bytes(row)):] = bytes(rng.integers(0, 256, 32 - name_len(bytes(row)), dtype=np.uint8))
                if name_len(bytes(row)) == 16:
                    row[8:16] = bytes(8)  # sin_zero stays: it is inside the address length
            if rng.random() < p_bad:
                row = bytearray(name_other(int(rng.choice([0, 1, 17, 0x0a00, 0x0200]))))
            names[i] = np.frombuffer(bytes(row), np.uint8)
            u = rng.random()
            if u < p_init:
                byte1 = 0 if rng.random() < 0.7 else int(rng.integers(1, 256))
                pk = init_packet(int(rng.integers(0, 1 << 32)), byte1, fill=int(rng.integers(0, 256)))
                pkts[i, :22] = np.frombuffer(pk, np.uint8)
                lens[i] = int(rng.choice([22, 22, 22, 21, 23]))
            elif u < p_init + 0.1:  # deviation (d): data of 22 bytes, some of it looking like an INIT
                lens[i] = 22
                pkts[i, 0] = int(rng.choice([0, 0, 1, 7]))
                pkts[i, 1] = int(rng.choice([0, 0, 9]))
            else:
                lens[i] = int(rng.choice([0, 1, 21, 22, 23, slot, slot + 7, int(rng.integers(0, slot + 1))]))
        return names, pkts, lens
