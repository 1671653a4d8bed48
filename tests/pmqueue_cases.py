"""The cases of the priority mqueue stage (include/emqx_pmqueue.h), shared by the CPU and the GPU
tests: a world of tables, session records, class rings and heads, a put or a take call on it, and the
literal restatement's answer (tests/pmqueue_ref.py), computed once a case."""

import functools
import random

import numpy as np

from emqx_amd import pmqueue as P
from emqx_amd import window
from tests import pmqueue_ref as R

INF = "infinity"
# (prios, default_class, max_len, mult, base)
T_ONE = ([0], 0, 3, 10, 0)
T_TWO = ([5, 0], 1, 3, 1, 0)
T_THREE = ([INF, 2, 0], 2, 3, 1, 0)
T_EIGHT = ([INF, 7, 6, 5, 4, 3, 2, -1], 6, 4, 1, 0)
T_NEG = ([2, 0, -1, -3], 1, 2, 10, 0)


class World:
    """Tables, records, rings and heads of ``n`` sessions."""

    def __init__(self, configs, n, c, qc, table=0, **session_columns):
        self.tables = P.pack_tables(configs)
        session_columns.setdefault("mq_max", 0)
        session_columns.setdefault("mq_len", 0)
        self.sessions = window.pack_sessions(n, **session_columns)
        self.ring = P.empty_ring(n, c, qc)
        self.heads = P.empty_heads(n, table)
        self.qc = qc

    def fill(self, sub, queues, order=None, head=None, credit=0, last=0):
        """``queues``: {class: [(ref, opts), ...]}; ``order``: the list (default: ascending classes);
        ``head``: {class: ring position of its oldest entry}."""
        head = head or {}
        for c, entries in queues.items():
            h = head.get(c, 0)
            self.ring[sub, c] = R.as_rows(entries, self.qc, h, P.ENTRY)
            self.heads["head"][sub][c] = h
            self.heads["len"][sub][c] = len(entries)
        order = sorted(c for c, e in queues.items() if e) if order is None else order
        word = 0xFFFFFFFF
        for p, c in enumerate(order):
            word = (word & ~(0xF << (4 * p))) | (c << (4 * p))
        self.heads["order"][sub] = word
        self.heads["credit"][sub] = credit
        self.heads["flags"][sub] = last
        self.sessions["mq_len"][sub] = sum(len(e) for e in queues.values())
        return self


class PutCase:
    def __init__(self, name, world, subs, offsets, classes, opts=None, verdicts=None, refs="auto", src=None, msg_class=None):
        """``classes``: per delivery the class byte of its message for every table (the message index is
        the delivery's position unless ``src`` / ``msg_class`` are given)."""
        self.name = name
        self.tables, self.sessions, self.ring, self.heads = world.tables, world.sessions, world.ring, world.heads
        self.subs = np.asarray(subs, dtype=np.uint32)
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        total = int(self.offsets[-1]) if self.offsets.size else 0
        self.opts = np.asarray([1] * total if opts is None else opts, dtype=np.uint8)
        self.verdicts = np.asarray([R.W_QUEUED] * total if verdicts is None else verdicts, dtype=np.uint8)
        self.refs = (np.arange(1000, 1000 + total, dtype=np.uint32) if isinstance(refs, str) else
                     None if refs is None else np.asarray(refs, dtype=np.uint32))
        self.src = np.arange(total, dtype=np.uint32) if src is None else np.asarray(src, dtype=np.uint32)
        if msg_class is None:
            msg_class = np.repeat(np.asarray(classes, dtype=np.uint8).reshape(-1, 1), max(self.tables.size, 1), axis=1)
        self.msg_class = np.ascontiguousarray(np.asarray(msg_class, dtype=np.uint8).reshape(-1, max(self.tables.size, 1)))

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return R.put_reference(self)


class TakeCase:
    def __init__(self, name, world, subs, now=0, deadlines=None, cap_out=None):
        self.name = name
        self.tables, self.sessions, self.ring, self.heads = world.tables, world.sessions, world.ring, world.heads
        self.subs = None if subs is None else np.asarray(subs, dtype=np.uint32)
        self.now = now
        self.deadlines = None if deadlines is None else np.asarray(deadlines, dtype=np.uint64)
        self.cap_out = cap_out

    @functools.lru_cache(maxsize=None)
    def reference(self, cap_out="case"):
        return R.take_reference(self, self.cap_out if cap_out == "case" else cap_out)


def msgs(first, n, opts=1):
    return [(first + i, opts) for i in range(n)]


def put_cases():
    cases = []
    # C 1, 2, 3, 8 and Qc 8, 64; every class empty, one short of full, full; e below, at and above M
    for configs, c in ((T_ONE, 1), (T_TWO, 2), (T_THREE, 3), (T_EIGHT, 8)):
        for qc in (8, 64):
            ncls, m = len(configs[0]), configs[2]
            for fill, tag in ((0, "empty"), (m - 1, "short"), (m, "full")):
                for e in (m - 1, m, m + 2):
                    w = World([configs], 2, c, qc)
                    w.fill(1, {k: msgs(100 * (k + 1), fill) for k in range(ncls)}, head={k: (qc - 1 + k) % qc for k in range(ncls)})
                    classes = [k for k in reversed(range(ncls)) for _ in range(e)]  # the lowest class arrives first
                    random.Random(e + qc).shuffle(classes)
                    cases.append(PutCase("c%d_q%d_%s_e%d" % (c, qc, tag, e), w, [1], [0, len(classes)], classes,
                                         opts=[(i % 3) for i in range(len(classes))]))
    # L > M: nothing is evicted; then the ring itself is full
    w = World([T_TWO], 1, 2, 8).fill(0, {0: msgs(10, 5), 1: msgs(20, 7)})
    cases.append(PutCase("len_above_max", w, [0], [0, 6], [0, 0, 1, 1, 0, 1]))
    w = World([T_TWO], 1, 2, 8).fill(0, {0: msgs(10, 7), 1: msgs(20, 8)}, head={0: 5, 1: 3})
    cases.append(PutCase("row_full", w, [0], [0, 5], [0, 0, 0, 1, 1]))
    # the order list: a class activated onto a rotated list; infinity first, last, rotated away then a keysort
    w = World([T_EIGHT], 1, 8, 8).fill(0, {3: msgs(30, 2), 5: msgs(50, 1), 1: msgs(10, 2)}, order=[3, 5, 1], credit=0, last=0)
    cases.append(PutCase("activate_onto_rotated", w, [0], [0, 3], [3, 4, 5]))
    w = World([T_THREE], 1, 3, 8)
    cases.append(PutCase("infinity_first", w, [0], [0, 4], [0, 2, 1, 0]))
    cases.append(PutCase("infinity_last", World([T_THREE], 1, 3, 8), [0], [0, 4], [2, 1, 1, 0]))
    w = World([T_THREE], 1, 3, 8).fill(0, {0: msgs(1, 2), 2: msgs(5, 1)}, order=[2, 0], credit=0, last=0)
    cases.append(PutCase("infinity_rotated_then_keysort", w, [0], [0, 2], [2, 1]))
    w = World([T_THREE], 1, 3, 8).fill(0, {0: msgs(1, 2), 2: msgs(5, 1)}, order=[0, 2])
    cases.append(PutCase("infinity_head_held", w, [0], [0, 1], [1]))
    # the default class through 0xFF and through a byte not below n_classes; box_src beyond n_msgs
    cases.append(PutCase("default_class", World([T_THREE], 1, 3, 8), [0], [0, 4], [0xFF, 3, 7, 1]))
    cases.append(PutCase("bad_src", World([T_TWO], 1, 2, 8), [0], [0, 3], [0, 0, 0], src=[0, 9, 3]))
    # two tables: the class byte of one message differs per table
    w = World([T_TWO, T_THREE], 2, 3, 8, table=np.array([0, 1]))
    cases.append(PutCase("two_tables", w, [0, 1], [0, 2, 4], None, src=[0, 1, 0, 1], msg_class=[[0, 2], [1, 0]]))
    # unfit tables of each kind; PASS, absent and out-of-range subscribers
    unfit = [([0], 0, 0, 1, 0), ([0], 0, 1, 1, 0), ([0], 0, 9, 1, 0), ([3, 2, 1, 0], 0, 3, 1, 0), ([1, 2], 0, 3, 1, 0),
             ([5, INF], 0, 3, 1, 0), ([0], 1, 3, 1, 0), ([0], 0, 3, 0, 0), T_TWO]
    w = World(unfit, 10, 3, 8, table=np.arange(10) % 10)
    w.heads["table"][9] = 77
    cases.append(PutCase("unfit_tables", w, list(range(10)), list(range(0, 22, 2)), [0] * 20))
    w = World([T_TWO], 4, 2, 8, flags=np.array([window.PRESENT | window.PASS, 0, window.PRESENT, window.PRESENT]))
    cases.append(PutCase("pass_absent_bad_sub", w, [0, 1, 9, 3], [0, 1, 2, 3, 5], [0, 0, 0, 1, 0]))
    # malformed heads
    w = World([T_TWO], 5, 2, 8)
    for s in range(5):
        w.fill(s, {0: msgs(10, 2), 1: msgs(20, 1)})
    w.heads["order"][0] = 0xFFFFFF11  # a class twice
    w.heads["order"][1] = 0xFFFFFFF0  # misses a non-empty class
    w.heads["len"][2][1] = 200        # len > Qc
    w.heads["head"][3][0] = 9         # head >= Qc
    w.heads["credit"][4] = -7
    w.heads["len"][4][1] = 0          # the order lists an empty class
    cases.append(PutCase("malformed_heads", w, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5], [1, 0, 1, 0, 1]))
    # a record with a limit: the window evicted, the verdicts say so
    w = World([T_TWO], 1, 2, 8, mq_max=4)
    cases.append(PutCase("limited_record", w, [0], [0, 4], [0, 1, 0, 1],
                         verdicts=[R.W_QUEUED, R.W_QUEUED_DROPPED, R.W_QUEUED | R.W_EVICTS, R.W_SEND]))
    cases.append(PutCase("no_refs", World([T_TWO], 1, 2, 8), [0], [0, 3], [0, 1, 0], refs=None))
    # inbox sizes around the block; several inboxes; none
    for n in (0, 1, 1023, 1024, 1025, 2349):
        w = World([T_THREE], 3, 3, 8)
        w.fill(1, {0: msgs(1, 2), 1: msgs(5, 3)}, head={0: 7, 1: 6})
        rnd = random.Random(n)
        cases.append(PutCase("inbox_%d" % n, w, [2, 1, 0], [0, 2, 2 + n, 4 + n], [rnd.randrange(3) for _ in range(n + 4)],
                             opts=[rnd.randrange(3) for _ in range(n + 4)],
                             verdicts=[rnd.choice([R.W_QUEUED, R.W_QUEUED, R.W_SEND, R.W_SEND_QOS0]) for _ in range(n + 4)]))
    cases.append(PutCase("no_inboxes", World([T_TWO], 2, 2, 8), [], [0], []))
    # many small inboxes of three tables: more than one block at every group width
    rnd = random.Random(7)
    n = 300
    w = World([T_TWO, T_THREE, T_NEG], n, 4, 8, table=np.arange(n) % 3)
    for s in range(n):
        ncls = int(w.tables["n_classes"][s % 3])
        q = {k: msgs(1000 * s + 10 * k, rnd.randrange(0, 4)) for k in range(ncls)}
        q = {k: v[:int(w.tables["max_len"][s % 3])] for k, v in q.items()}
        order = [k for k in q if q[k]]
        rnd.shuffle(order)
        w.fill(s, q, order=order, head={k: rnd.randrange(8) for k in q}, credit=rnd.choice([0, 3, -1]), last=rnd.randrange(2))
    sizes = [rnd.randrange(0, 9) for _ in range(n)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    subs = list(range(n))
    rnd.shuffle(subs)
    cases.append(PutCase("many_inboxes", w, subs, off, [rnd.randrange(5) for _ in range(int(off[-1]))],
                         opts=[rnd.randrange(3) for _ in range(int(off[-1]))]))
    return cases


def take_cases():
    cases = []
    m = T_EIGHT[2]
    # budgets 0, 1, M and 1000 on a full 8 x 64 row
    for budget, inflight_max, inflight in ((0, 4, 4), (1, 4, 3), (m, 4, 0), (1000, 0, 5)):
        w = World([([INF, 7, 6, 5, 4, 3, 2, -1], 6, 64, 1, 0)], 1, 8, 64, inflight_max=inflight_max, inflight=inflight)
        w.fill(0, {k: msgs(100 * k, 64, opts=1 + k % 2) for k in range(8)}, head={k: (9 * k) % 64 for k in range(8)})
        cases.append(TakeCase("full_row_budget_%d" % budget, w, [0]))
    # credit 0 at entry: the shift comes first; credit negative: never a shift; the head class empties mid-credit
    w = World([T_TWO], 1, 2, 8, inflight_max=0).fill(0, {0: msgs(10, 3), 1: msgs(20, 3)}, order=[0, 1], credit=0, last=1)
    cases.append(TakeCase("credit_zero_at_entry", w, [0]))
    w = World([T_NEG], 1, 4, 8, inflight_max=0).fill(0, {2: msgs(10, 2), 0: msgs(20, 2), 3: msgs(30, 2)}, order=[2, 0, 3], credit=-1, last=1)
    cases.append(TakeCase("credit_negative", w, [0]))
    w = World([T_NEG], 1, 4, 8, inflight_max=0).fill(0, {0: msgs(20, 2), 1: msgs(40, 2), 3: msgs(30, 2)})
    cases.append(TakeCase("negative_priority_reached", w, [0]))
    w = World([([5, 0], 1, 3, 1, 0)], 1, 2, 8, inflight_max=0).fill(0, {0: msgs(10, 2), 1: msgs(20, 3)})
    cases.append(TakeCase("head_class_empties_mid_credit", w, [0]))
    w = World([T_TWO], 1, 2, 8, inflight_max=0).fill(0, {0: msgs(10, 3), 1: msgs(20, 3)}, order=[1, 0], credit=2, last=1)
    cases.append(TakeCase("rotated_list", w, [0]))
    # expired and QoS 0 entries at the head, between the others and at the end
    w = World([T_TWO], 1, 2, 8, inflight_max=3)
    w.fill(0, {0: [(0, 1), (1, 0), (2, 1), (3, 1)], 1: [(4, 0), (5, 1), (6, 2), (7, 0)]}, head={0: 6, 1: 7})
    cases.append(TakeCase("expired_and_qos0", w, [0], now=50, deadlines=[10, 99, 99, 20, 99, 10, 99, 10]))
    cases.append(TakeCase("bad_ref", w, [0], now=50, deadlines=[10, 99, 99]))
    cases.append(TakeCase("no_deadlines", w, [0], now=50))
    # ids across 65535 -> 1
    w = World([T_TWO], 1, 2, 8, inflight_max=0, next_pkt_id=65534).fill(0, {0: msgs(10, 3), 1: msgs(20, 2)})
    cases.append(TakeCase("ids_wrap", w, [0]))
    # statuses; subs NULL; malformed heads
    w = World([T_TWO, ([0], 0, 1, 1, 0)], 5, 2, 8, table=np.array([0, 0, 0, 1, 0]), inflight_max=0,
              flags=np.array([window.PRESENT | window.PASS, 0, window.PRESENT, window.PRESENT, window.PRESENT]))
    for s in range(5):
        w.fill(s, {0: msgs(10 * s, 2), 1: msgs(10 * s + 5, 1)})
    cases.append(TakeCase("statuses", w, [0, 1, 2, 3, 9, 4]))
    cases.append(TakeCase("subs_null", w, None))
    w = World([T_TWO], 5, 2, 8, inflight_max=0)
    for s in range(5):
        w.fill(s, {0: msgs(10, 2), 1: msgs(20, 1)})
    w.heads["order"][0] = 0xFFFFFF11
    w.heads["order"][1] = 0xFFFFFFF0
    w.heads["len"][2][1] = 200
    w.heads["head"][3][0] = 9
    w.heads["credit"][4] = -7
    w.heads["flags"][4] = 1
    cases.append(TakeCase("malformed_heads", w, [4, 3, 2, 1, 0]))
    w = World([T_TWO], 1, 2, 8, inflight_max=0, mq_max=5).fill(0, {0: msgs(10, 1)})
    cases.append(TakeCase("limited_record", w, [0]))
    # more sessions than a block takes at every group width, of three tables, in every state
    rnd = random.Random(11)
    n = 300
    w = World([T_TWO, T_THREE, T_NEG], n, 4, 16, table=np.arange(n) % 3,
              inflight_max=np.array([rnd.choice([0, 2, 5]) for _ in range(n)]), inflight=np.array([rnd.randrange(4) for _ in range(n)]),
              next_pkt_id=np.array([rnd.choice([1, 65535, 4000]) for _ in range(n)]))
    for s in range(n):
        ncls = int(w.tables["n_classes"][s % 3])
        q = {k: [(rnd.randrange(64), rnd.randrange(3)) for _ in range(rnd.randrange(0, 4))] for k in range(ncls)}
        order = [k for k in q if q[k]]
        rnd.shuffle(order)
        w.fill(s, q, order=order, head={k: rnd.randrange(16) for k in q}, credit=rnd.choice([0, 1, 5, -1]), last=rnd.randrange(2))
    subs = list(range(n))
    rnd.shuffle(subs)
    cases.append(TakeCase("many_sessions", w, subs, now=100, deadlines=[rnd.choice([50, 150, 0xFFFFFFFFFFFFFFFF]) for _ in range(64)]))
    return cases


def overflow_case():
    w = World([T_TWO], 2, 2, 8, inflight_max=2).fill(0, {0: [(1, 1), (2, 0)], 1: [(3, 1)]}).fill(1, {1: [(4, 1), (5, 2)]})
    return TakeCase("overflow", w, [0, 1], cap_out=4)


# ---- comparisons -----------------------------------------------------------------------------------

def check_put(ref, got, case, sessions, ring, heads, update_table=True):
    assert list(got.summary.values()) == ref["summary"], (got.summary, ref["summary"])
    assert got.verdicts.tolist() == ref["verdicts"]
    assert got.classes.tolist() == ref["classes"]
    assert [[int(e["ref"]), int(e["opts"])] for e in got.evicted] == ref["evicted"]
    assert got.counts.tolist() == ref["counts"]
    models = {sub: (mq, t, after) for sub, (mq, t, after) in ref["models"].items()}
    R.check_tables(models, sessions, ring, heads, update_table, (case.sessions, case.ring, case.heads),
                   lambda after: {"dropped": after})
    check_dead_positions(case, ring, heads if update_table else None, ref)


def check_dead_positions(case, ring, heads, ref):
    """A ring position outside the live queues after the call is what it was; rows of sessions the call
    did not own are untouched."""
    qc = ring.shape[2]
    for sub in range(ring.shape[0]):
        if sub not in ref["models"] or heads is None:
            if sub not in ref["models"]:
                assert ring[sub].tobytes() == case.ring[sub].tobytes(), sub
            continue
        for c in range(ring.shape[1]):
            h, n = int(heads["head"][sub][c]), int(heads["len"][sub][c])
            live = {(h + i) % qc for i in range(n)}
            for pos in set(range(qc)) - live:
                assert ring[sub, c, pos].tobytes() == case.ring[sub, c, pos].tobytes(), (sub, c, pos)


def check_take(ref, got, case, sessions, ring, heads, update_table=True):
    assert list(got.summary.values()) == ref["summary"], (got.summary, ref["summary"])
    assert got.offsets.tolist() == ref["offsets"] and got.status.tolist() == ref["status"]
    assert got.counts.tolist() == ref["counts"]
    full = ref.get("full", False)
    if not full:
        assert got.refs.tolist() == ref["refs"] and got.opts.tolist() == ref["opts"]
        assert got.verdicts.tolist() == ref["verdicts"] and got.pkt_ids.tolist() == ref["pkt_ids"]
        assert got.classes.tolist() == ref["classes"]
    assert ring.tobytes() == case.ring.tobytes()  # a take only reads the rings
    R.check_tables(ref["models"], sessions, ring, heads, update_table and not full, (case.sessions, case.ring, case.heads),
                   lambda extra: extra)
