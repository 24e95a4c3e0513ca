"""A connection table on the device (ugo_fec_listen_*) beside the RuleListener
of tests/listen_ref.py; test infrastructure only.

After every call every output array, the state and the entry dump are compared
in whole with the rule.  Outputs are written into arrays filled with arbitrary
bytes, with guard bytes on both sides that must survive; operand arrays are
compared with what went in.
"""
import numpy as np
import torch

import listen_ref as lr
from ugo_amd import fec

GUARD = 64


def _put(arr, where="device"):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory() if where == "pinned" else t.cuda()


class Guarded:
    """nbytes of output between two guards, all of it arbitrary bytes."""

    def __init__(self, nbytes, seed, where="device"):
        self.nbytes = nbytes
        self.fill = np.random.default_rng(seed).integers(0, 256, nbytes + 2 * GUARD, dtype=np.uint8)
        self.whole = _put(self.fill, where)
        self.t = self.whole[GUARD:GUARD + nbytes]

    def view(self, dtype, *shape):
        return self.t.view(dtype).reshape(*shape)

    def read(self):
        """The output bytes, after checking both guards."""
        got = self.whole.cpu().numpy()
        assert np.array_equal(got[:GUARD], self.fill[:GUARD]), "bytes before the output were written"
        assert np.array_equal(got[GUARD + self.nbytes:], self.fill[GUARD + self.nbytes:]), \
            "bytes after the output were written"
        return got[GUARD:GUARD + self.nbytes].copy()


def entry_array(entries):
    out = np.zeros(len(entries), fec.LISTEN_ENTRY_DTYPE)
    for j, (ip, scope, port, member) in enumerate(entries):
        out[j]["ip"] = np.frombuffer(ip, np.uint8)
        out[j]["scope"], out[j]["port"], out[j]["member"] = scope, port, member
    return out


class ListenHarness:
    def __init__(self, enc, max_conn):
        self.enc = enc
        self.table = fec.ListenTable(enc, max_conn)
        self.rule = lr.RuleListener(max_conn)
        self.max_conn = max_conn
        self.calls = 0
        self.check()

    def close(self):
        self.table.close()

    # ---------------------------------------------------------------- state and entries
    def check(self, entries=True):
        st = self.table.state()                            # waits for the last call
        r = self.rule
        assert int(st["n_slots"]) == r.n_slots
        assert (int(st["nconn"]), int(st["n_dead"]), int(st["err"])) == (r.nconn, r.n_dead, r.err), (st, r.nconn,
                                                                                                    r.n_dead, r.err)
        assert st["counts"].tolist() == r.counts, (st["counts"].tolist(), r.counts)
        if entries:
            got = self.table.entries()
            want = entry_array(r.entries())
            assert got.tobytes() == want.tobytes(), "the entry dump differs from the rule's"
        return st

    # ---------------------------------------------------------------- ugo_fec_listen_route
    def route(self, names, pkts, lens, max_accepted=None, where="device", entries=True):
        """names uint8 [n, 32], pkts uint8 [n, slot], lens uint16 [n] (numpy).
        Returns (conn_of, cls, accepted records, n_accepted) as numpy."""
        self.calls += 1
        n, slot = pkts.shape
        cap = min(n, self.max_conn) if max_accepted is None else max_accepted
        dn, dp, dl = _put(names, where), _put(pkts, where), _put(lens.view(np.int16), where)
        g_conn = Guarded(4 * n, 100 + self.calls, where)
        g_cls = Guarded(n, 200 + self.calls, where)
        g_acc = Guarded(48 * cap, 300 + self.calls, where)
        g_n = Guarded(4, 400 + self.calls, where)
        self.table.route(dn, dp, dl, conn_of=g_conn.view(torch.int32, n), cls=g_cls.view(torch.uint8, n),
                         accepted=g_acc.view(torch.uint8, cap, 48), n_accepted=g_n.view(torch.int32, 1))
        w_conn, w_cls, w_acc = self.rule.route(names, pkts, lens, slot)
        assert not self.rule.unspecified, "deviation (c): use route_full"
        self.check(entries)
        conn = g_conn.read().view(np.uint32)
        cls = g_cls.read()
        n_acc = int(g_n.read().view(np.uint32)[0])
        bad = np.flatnonzero(cls != np.asarray(w_cls, np.uint8))
        assert bad.size == 0, f"cls differs at {bad[:8]}: {cls[bad[:8]]} vs {np.asarray(w_cls)[bad[:8]]}"
        bad = np.flatnonzero(conn != np.asarray(w_conn, np.uint32))
        assert bad.size == 0, f"conn_of differs at {bad[:8]}: {conn[bad[:8]]} vs {np.asarray(w_conn)[bad[:8]]}"
        assert n_acc == len(w_acc), (n_acc, len(w_acc))
        acc_bytes = g_acc.read()
        rows = min(n_acc, cap)
        acc = acc_bytes[:48 * rows].view(fec.LISTEN_ACCEPT_DTYPE)
        want = np.zeros(rows, fec.LISTEN_ACCEPT_DTYPE)
        for j, (i, m, cid, row) in enumerate(w_acc[:rows]):
            want[j]["packet"], want[j]["member"], want[j]["client_id"] = i, m, cid
            want[j]["name"] = np.frombuffer(row, np.uint8)
        assert acc.tobytes() == want.tobytes(), "accepted[] differs"
        assert np.array_equal(acc_bytes[48 * rows:], g_acc.fill[GUARD + 48 * rows:GUARD + 48 * cap]), \
            "accepted[] was written past the rows the call accepted"
        assert np.array_equal(dn.cpu().numpy(), names) and np.array_equal(dp.cpu().numpy(), pkts) and \
            np.array_equal(dl.cpu().numpy().view(np.uint16), lens), "an operand was written"
        return conn, cls, acc, n_acc

    # ---------------------------------------------------------------- ugo_fec_listen_remap
    def remap(self, new_index, nconn_new, where="device"):
        self.calls += 1
        idx = np.asarray(new_index, np.uint32)
        di = _put(idx.view(np.int32), where)
        g_st = Guarded(4, 500 + self.calls, where)
        before = None
        want = self.rule.remap([int(v) for v in idx], nconn_new)
        if want:
            before = (self.table.state().tobytes(), self.table.entries().tobytes())
        self.table.remap(di, nconn_new, status=g_st.view(torch.int32, 1))
        got = int(g_st.read().view(np.uint32)[0])
        assert got == want, (got, want)
        self.check()
        if want:
            assert before == (self.table.state().tobytes(), self.table.entries().tobytes())
        assert np.array_equal(di.cpu().numpy().view(np.uint32), idx), "new_index was written"
        return got

    # ---------------------------------------------------------------- ugo_fec_listen_names
    def names(self, conn_of, where="device"):
        self.calls += 1
        c = np.asarray(conn_of, np.uint32)
        n = len(c)
        dc = _put(c.view(np.int32), where)
        g_rows, g_lens = Guarded(32 * n, 600 + self.calls, where), Guarded(4 * n, 700 + self.calls, where)
        self.table.names(dc, names_out=g_rows.view(torch.uint8, n, 32), name_lens=g_lens.view(torch.int32, n))
        w_rows, w_lens = self.rule.names([int(v) for v in c])
        self.check(entries=False)
        rows, lens = g_rows.read().reshape(n, 32), g_lens.read().view(np.uint32)
        assert lens.tolist() == w_lens
        assert rows.tobytes() == b"".join(w_rows)
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), c)
        return rows, lens
