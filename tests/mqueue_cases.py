"""Cases of the mqueue stage shared by the CPU and the GPU suite: named ones for every edge the
contract (include/emqx_mqueue.h) names, and seeded random ones of a few thousand deliveries or
sessions.  A case holds its tables as numpy arrays (never changed: every run works on copies) and
answers ``reference()`` from the sequential restatement (tests/mqueue_ref.py); the verdicts of a put
case come from the window stage's restatement (tests/window_ref.py), as they do on the stream."""
import numpy as np

from tests import mqueue_ref as R
from tests import window_ref as WR

TILE = 1024  # deliveries a tile of the put passes (emqx_amd/csrc/mqueue.h MQ_TILE)
ENTRY = np.dtype([("ref", "<u4"), ("opts", "u1"), ("rsv", "u1", (3,))])
RING = np.dtype([("head", "<u4"), ("len", "<u4")])
SESSION = np.dtype([("inflight", "<u4"), ("inflight_max", "<u4"), ("mq_len", "<u4"), ("mq_max", "<u4"),
                    ("next_pkt_id", "<u4"), ("flags", "<u4"), ("dropped", "<u8")])
PRESENT, CONNECTED, STORE_QOS0, PASS = 1, 2, 4, 8
DISC = PRESENT | STORE_QOS0   # a disconnected session that stores QoS 0: every delivery is a candidate
CONN = PRESENT | CONNECTED
NOW = 1_700_000_000_000
JUNK = 0xAB000000  # refs of ring positions no queue holds: the stage never clears, so they must survive


def rec(inflight=0, inflight_max=32, mq_len=0, mq_max=1000, next_pkt_id=1, flags=CONN, dropped=0):
    return dict(inflight=inflight, inflight_max=inflight_max, mq_len=mq_len, mq_max=mq_max, next_pkt_id=next_pkt_id,
                flags=flags, dropped=dropped)


def np_sessions(recs):
    t = np.zeros(len(recs), dtype=SESSION)
    for i, r in enumerate(recs):
        for k, v in r.items():
            t[k][i] = v
    return t


def build_tables(q, rows):
    """``rows``: one (head, [(ref, opts), ...]) or (head, entries, raw_header) a session.  The ring
    with junk wherever no queue entry lies, and the headers."""
    n = len(rows)
    ring = np.zeros((n, q), dtype=ENTRY)
    ring["ref"] = JUNK + np.arange(n * q, dtype=np.uint32).reshape(n, q)
    ring["opts"] = 0x55
    heads = np.zeros(n, dtype=RING)
    for s, row in enumerate(rows):
        head, entries = row[0], row[1]
        for i, (ref, opts) in enumerate(entries):
            ring[s, (head + i) % q] = (ref, opts, (0, 0, 0))
        heads[s] = row[2] if len(row) > 2 else (head, len(entries))
    return ring, heads


def lists_of(ring, heads):
    """The tables as the restatement takes them."""
    return ([[[int(e["ref"]), int(e["opts"])] for e in row] for row in ring], [[int(h["head"]), int(h["len"])] for h in heads])


class PutCase:
    """``boxes``: one dict an inbox with sub, opts (the deliveries' bytes) and, for a subscriber the
    table holds, nothing else: its record is ``recs[sub]`` with mq_len set to the row's."""

    def __init__(self, name, q, rows, recs, boxes, refs=False, verdicts=None, check_len=True, stale_len=()):
        self.name, self.q = name, q
        self.ring, self.heads = build_tables(q, rows)
        before = [dict(r) for r in recs]
        for s, r in enumerate(before):
            r["mq_len"] = min(int(self.heads["len"][s]), q)
        self.subs = np.array([b["sub"] for b in boxes], dtype=np.uint32)
        self.offsets = np.zeros(len(boxes) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(b["opts"]) for b in boxes])
        self.opts = np.array([o for b in boxes for o in b["opts"]], dtype=np.uint8)
        after = [dict(r) for r in before]
        w = WR.run(self.subs, self.offsets, self.opts, after, update_table=True)
        self.verdicts = np.array(w["verdicts"] if verdicts is None else verdicts, dtype=np.uint8)
        for s in stale_len:
            after[s]["mq_len"] += 1
        self.sessions = np_sessions(after) if check_len else None
        self.session_dicts = after if check_len else None
        total = int(self.offsets[-1])
        self.refs = (np.arange(total, dtype=np.uint32) * 7 + 1000) if refs else None

    def reference(self):
        ring, heads = lists_of(self.ring, self.heads)
        out = R.put(self.subs, self.offsets, self.opts, self.verdicts, self.refs, ring, heads, self.q, sessions=self.session_dicts)
        return out, ring, heads


def check_put(ref, got, ring, heads):
    """``ref``: PutCase.reference(); ``got``: a Put; the tables after the call."""
    out, r_ring, r_heads = ref
    assert [got.summary[k] for k in ("flags", "deliveries", "inboxes", "stored", "evicted", "unstored", "full_rows",
                                     "len_mismatch")] == out["summary"]
    assert [[int(e["ref"]), int(e["opts"])] for e in got.evicted] == out["evicted"]
    assert not got.evicted["rsv"].any()
    assert got.unstored.tolist() == out["unstored"]
    assert lists_of(ring, heads) == (r_ring, r_heads)
    assert not ring["rsv"].any()


def queue(n, first_ref=100, qos=lambda i: 1):
    return [(first_ref + i, qos(i)) for i in range(n)]


def put_cases():
    q1 = [1] * 3
    mixed = [0, 1, 2, 1, 0x10 | 1, 0x40 | 2, 2, 1]
    cases = [
        PutCase("empty_row", 8, [(0, [])], [rec(flags=DISC, mq_max=4)], [dict(sub=0, opts=q1)]),
        PutCase("head_wraps", 8, [(6, queue(3))], [rec(flags=DISC, mq_max=8)], [dict(sub=0, opts=[1, 0, 2])], refs=True),
        # L = M = Q: the survivors overwrite the evicted positions; out_evicted still shows the old entries
        PutCase("full_row_evicts", 8, [(5, queue(8))], [rec(flags=DISC, mq_max=8)], [dict(sub=0, opts=q1)]),
        PutCase("full_row_evicts_all", 8, [(3, queue(8))], [rec(flags=DISC, mq_max=8)], [dict(sub=0, opts=[1] * 8)]),
        # e > M: every old entry evicted, the first e - M candidates QUEUED_DROPPED
        PutCase("more_than_max", 8, [(7, queue(2))], [rec(flags=DISC, mq_max=4)], [dict(sub=0, opts=[1, 2, 1, 0, 1, 2, 1])]),
        # L > M: never drops, then overflows Q
        PutCase("beyond_max_row_full", 8, [(2, queue(6))], [rec(flags=DISC, mq_max=4)], [dict(sub=0, opts=[1] * 5)]),
        PutCase("no_queued", 8, [(1, queue(2))], [rec(flags=CONN, inflight_max=32, mq_max=8)], [dict(sub=0, opts=[1, 2, 0])]),
        PutCase("connected_window_full", 8, [(1, queue(2))], [rec(flags=CONN, inflight=2, inflight_max=3, mq_max=4)],
                [dict(sub=0, opts=mixed)]),
        PutCase("bad_sub", 8, [(0, queue(1))], [rec(flags=DISC, mq_max=8)], [dict(sub=0, opts=[1]), dict(sub=9, opts=[1, 1])],
                verdicts=[3, 3, 3]),
        PutCase("no_inboxes", 8, [(0, queue(1))], [rec(flags=DISC)], []),
        PutCase("empty_inboxes", 8, [(0, []), (0, queue(1)), (0, [])], [rec(flags=DISC, mq_max=8)] * 3,
                [dict(sub=2, opts=[]), dict(sub=0, opts=[1, 1]), dict(sub=1, opts=[])]),
        PutCase("bad_ring_header", 8, [(5, queue(3), (13, 20))], [rec(flags=DISC, mq_max=8)], [dict(sub=0, opts=[1, 1])]),
        PutCase("len_mismatch", 8, [(0, queue(2)), (0, queue(1))], [rec(flags=DISC, mq_max=8)] * 2,
                [dict(sub=0, opts=[1]), dict(sub=1, opts=[1])], stale_len=(1,)),
        PutCase("no_sessions_given", 16, [(15, queue(4))], [rec(flags=DISC, mq_max=16)], [dict(sub=0, opts=[1, 2])], check_len=False),
    ]
    # one inbox holds every delivery, over more than two tiles; its neighbours are empty
    big = 2 * TILE + 300
    cases.append(PutCase("one_inbox_has_all", 1024, [(0, []), (1000, queue(900)), (0, [])], [rec(flags=DISC, mq_max=1000)] * 3,
                         [dict(sub=0, opts=[]), dict(sub=1, opts=[1 + (i % 2) for i in range(big)]), dict(sub=2, opts=[])], refs=True))
    # inboxes that begin and end at the tile size - 1, the tile size and the tile size + 1
    sizes = [TILE - 1, 1, 1, TILE - 2, 1, 1, 40]
    cases.append(PutCase("tile_bounds", 8, [((3 * s) % 8, queue(s % 7, 100 * s)) for s in range(len(sizes))],
                         [rec(flags=DISC, mq_max=4 + s % 5) for s in range(len(sizes))],
                         [dict(sub=len(sizes) - 1 - k, opts=[(k + i) % 3 for i in range(n)]) for k, n in enumerate(sizes)]))
    for seed, q in ((1, 8), (2, 64)):
        cases.append(random_put(seed, q))
    return cases


def random_put(seed, q, n_sessions=400):
    rng = np.random.default_rng(seed)
    rows, recs, boxes = [], [], []
    for s in range(n_sessions):
        mq_max = int(rng.integers(1, q + 1))
        L = int(rng.integers(0, q + 1 if rng.random() < 0.1 else mq_max + 1))
        rows.append((int(rng.integers(0, q)), queue(L, 1000 * s, lambda i: int(rng.integers(0, 3)))))
        flags = [DISC, PRESENT, CONN, CONN | PASS, 0][int(rng.choice(5, p=[0.4, 0.2, 0.3, 0.05, 0.05]))]
        recs.append(rec(flags=flags, inflight=int(rng.integers(0, 4)), inflight_max=int(rng.integers(0, 4)), mq_max=mq_max))
    for s in rng.permutation(n_sessions)[: n_sessions * 3 // 4]:
        n = int(rng.choice([0, 1, 2, 5, 3 * q], p=[0.1, 0.3, 0.3, 0.2, 0.1]))
        boxes.append(dict(sub=int(s), opts=[int(x) for x in rng.choice([0, 1, 2, 0x11, 0x42], size=n, p=[0.2, 0.4, 0.3, 0.05, 0.05])]))
    return PutCase("random_q%d" % q, q, rows, recs, boxes, refs=bool(seed & 1))


# ---- take ---------------------------------------------------------------------------------------

class TakeCase:
    """``rows`` as in build_tables, ``recs`` the records (mq_len is set from the row unless
    ``keep_len``); ``subs`` None: the whole table; ``deadlines``: a list indexed by ref or None."""

    def __init__(self, name, q, rows, recs, subs="all", now=NOW, deadlines=None, cap_out=None, keep_len=()):
        self.name, self.q, self.now, self.cap_out = name, q, now, cap_out
        self.ring, self.heads = build_tables(q, rows)
        recs = [dict(r) for r in recs]
        for s, r in enumerate(recs):
            if s not in keep_len:
                r["mq_len"] = min(int(self.heads["len"][s]), q)
        self.session_dicts = recs
        self.sessions = np_sessions(recs)
        self.subs = list(range(len(rows))) if isinstance(subs, str) else subs
        self.deadlines = None if deadlines is None else np.array(deadlines, dtype=np.uint64)

    def reference(self, update_table=True, cap_out="case"):
        ring, heads = lists_of(self.ring, self.heads)
        recs = [dict(r) for r in self.session_dicts]
        cap = self.cap_out if cap_out == "case" else cap_out
        out = R.take(self.subs, recs, ring, heads, self.q, now=self.now, deadlines=self.deadlines, cap_out=cap,
                     update_table=update_table)
        return out, recs, heads


def check_take(ref, got, sessions, heads, ring, case):
    out, r_recs, r_heads = ref
    assert [got.summary[k] for k in ("flags", "ok_sessions", "sessions", "items", "sends", "sends_qos0", "expired",
                                     "len_mismatch")] == out["summary"]
    assert got.offsets.tolist() == out["offsets"]
    assert got.status.tolist() == out["status"] and got.counts.tolist() == out["counts"]
    assert (got.opts.tolist(), got.verdicts.tolist(), got.pkt_ids.tolist(), got.refs.tolist()) == (
        out["opts"], out["verdicts"], out["pkt_ids"], out["refs"])
    assert sessions.tobytes() == np_sessions(r_recs).tobytes()
    assert [[int(h["head"]), int(h["len"])] for h in heads] == r_heads
    assert ring.tobytes() == case.ring.tobytes()  # a take never writes a ring


def _deadlines(n=4096):
    """ref % 3 == 0: passed; == 1: not yet; == 2: never."""
    return [NOW - 1 if r % 3 == 0 else NOW + 5 if r % 3 == 1 else R.NO_EXPIRY for r in range(n)]


def take_cases():
    live1, live2, dead = 4, 7, 3  # refs by _deadlines: not yet (4), not yet (7), passed (3)
    cases = [
        TakeCase("budget_zero_qos0_head", 8, [(0, [(1, 0), (2, 1)])], [rec(inflight=4, inflight_max=4)]),
        TakeCase("budget_ends_at_last", 8, [(6, [(1, 1), (2, 0), (3, 2)])], [rec(inflight=2, inflight_max=4)]),
        TakeCase("trailing_qos0_stays", 8, [(6, [(1, 1), (2, 2), (3, 0), (4, 1)])], [rec(inflight=2, inflight_max=4)]),
        TakeCase("fewer_than_budget", 8, [(3, [(1, 0), (2, 1), (3, 0)])], [rec(inflight=0, inflight_max=4)]),
        TakeCase("all_expired", 8, [(1, [(dead, 1), (dead + 3, 0), (dead + 6, 2)])], [rec(inflight=3, inflight_max=4)],
                 deadlines=_deadlines()),
        TakeCase("expired_between_counting", 8, [(7, [(live1, 1), (dead, 1), (live2, 2), (dead + 3, 2), (live1 + 3, 1), (2, 1)])],
                 [rec(inflight=1, inflight_max=4)], deadlines=_deadlines()),
        TakeCase("expired_head_budget_zero", 8, [(0, [(dead, 1), (live1, 1)])], [rec(inflight=4, inflight_max=4)], deadlines=_deadlines()),
        TakeCase("unbounded_window", 1024, [(1000, queue(1024, 0, lambda i: 1 + i % 2))], [rec(inflight=7, inflight_max=0)]),
        TakeCase("inflight_above_max", 8, [(0, [(1, 0), (2, 1)])], [rec(inflight=9, inflight_max=4)]),
        TakeCase("ids_wrap", 8, [(2, queue(5, 10, lambda i: 1 + i % 2))], [rec(inflight=0, inflight_max=8, next_pkt_id=65534)]),
        TakeCase("pass_absent_bad_sub", 8, [(0, queue(2)), (0, queue(2)), (0, queue(2))],
                 [rec(flags=CONN | PASS), rec(flags=0), rec()], subs=[0, 1, 7, 2]),
        TakeCase("bad_ring_header", 8, [(5, queue(3), (13, 20))], [rec(inflight=0, inflight_max=0)]),
        TakeCase("bad_ref", 8, [(0, [(live1, 1), (5000, 1), (dead, 1), (6000, 2)])], [rec(inflight=1, inflight_max=3)],
                 deadlines=_deadlines()),
        TakeCase("no_deadlines", 8, [(0, [(dead, 1), (live1, 2)])], [rec()], deadlines=None),
        TakeCase("len_mismatch", 8, [(0, queue(2)), (0, queue(3))], [rec(mq_len=5), rec()], keep_len=(0,)),
        TakeCase("empty_queues", 8, [(3, []), (0, [])], [rec(), rec(inflight=32)]),
        TakeCase("whole_table", 64, [(s * 5 % 64, queue(s % 9, 10 * s, lambda i: i % 3)) for s in range(70)],
                 [rec(inflight=s % 4, inflight_max=4) for s in range(70)], subs=None),
        # Q = 256: the group's trip loop (16 entries a trip) runs many times, with a wrapped and an odd head
        TakeCase("q256_trips", 256, [(251, queue(200, 0, lambda i: (i * 7) % 3)), (255, queue(256, 300, lambda i: 1)),
                                     (100, queue(130, 600, lambda i: 0)), (7, queue(70, 800, lambda i: 2))],
                 [rec(inflight=0, inflight_max=0), rec(inflight=0, inflight_max=150), rec(inflight=32), rec(inflight=0, inflight_max=65)],
                 deadlines=_deadlines()),
        # a full ring with an odd head: the pair at the head is loaded twice, once for each of its entries
        TakeCase("full_ring_odd_head", 8, [(3, queue(8, 50, lambda i: 1)), (1, queue(8, 70, lambda i: i % 2))],
                 [rec(inflight=0, inflight_max=0), rec(inflight=0, inflight_max=0)]),
        TakeCase("no_sessions", 8, [(0, queue(1))], [rec()], subs=[]),
    ]
    for seed, q in ((5, 8), (6, 64), (7, 256)):
        cases.append(random_take(seed, q))
    return cases


def overflow_case():
    """Two sessions with three and two items: cap_out 4 is one short."""
    return TakeCase("output_full", 8, [(6, [(1, 1), (2, 0), (3, 2)]), (0, [(4, 1), (5, 1)])], [rec(), rec()], cap_out=4)


def random_take(seed, q, n_sessions=None):
    rng = np.random.default_rng(seed)
    n_sessions = n_sessions or (2500 if q == 8 else 600 if q == 64 else 150)
    rows, recs = [], []
    for s in range(n_sessions):
        L = int(rng.choice([0, int(rng.integers(0, q + 1)), q], p=[0.2, 0.7, 0.1]))
        entries = [(int(rng.integers(0, 5000)), int(rng.choice([0, 1, 2], p=[0.3, 0.4, 0.3]))) for _ in range(L)]
        row = (int(rng.integers(0, q)), entries)
        if rng.random() < 0.03:
            row = row + ((int(rng.integers(0, 4 * q)), int(rng.integers(0, 4 * q))),)
        rows.append(row)
        flags = [CONN, PRESENT, CONN | PASS, 0][int(rng.choice(4, p=[0.8, 0.1, 0.05, 0.05]))]
        imax = int(rng.choice([0, 2, 4, 32, q]))
        recs.append(rec(flags=flags, inflight=int(rng.integers(0, imax + 2)), inflight_max=imax,
                        next_pkt_id=int(rng.choice([1, 65535, int(rng.integers(1, 65536))]))))
    subs = [int(s) for s in rng.permutation(n_sessions)[: n_sessions * 4 // 5]]
    subs.insert(len(subs) // 2, n_sessions + 3)
    return TakeCase("random_q%d" % q, q, rows, recs, subs=subs, deadlines=_deadlines(4096))
