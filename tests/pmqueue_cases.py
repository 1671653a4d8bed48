"""The cases of the priority mqueue stage (include/emqx_pmqueue.h), shared by the CPU and the GPU
tests: a world of tables, session records, class rings and heads, a put or a take call on it, and the
literal restatement's answer (tests/pmqueue_ref.py), computed once a case.  The second half is the
lattice: seeded worlds over C x Qc whose put and take rounds are sized around a group width G, chained
through the restatement's own models."""

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


def clone_models(models, events):
    """The models of a chain, for one evaluation: a reference computed twice starts from the same queues."""
    if models is None:
        return None
    out = {}
    for sub, mq in models.items():
        new = R.MQ(mq.max_len, mq.mult, mq.base, events)
        new.q = [[key, type(dq)(dq)] for key, dq in mq.q]
        new.len, new.dropped, new.last_prio, new.p_credit = mq.len, mq.dropped, mq.last_prio, mq.p_credit
        out[sub] = new
    return out


class PutCase:
    def __init__(self, name, world, subs, offsets, classes, opts=None, verdicts=None, refs="auto", src=None, msg_class=None,
                 events=None, models=None):
        """``classes``: per delivery the class byte of its message for every table (the message index is
        the delivery's position unless ``src`` / ``msg_class`` are given).  ``models``: the restatement's
        own queues from the calls before (a chain), ``events``: its counters."""
        self.name = name
        self.events, self.models, self._ref = events, models, None
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

    def reference(self):
        if self._ref is None:
            self._ref = R.put_reference(self, self.events, clone_models(self.models, self.events))
        return self._ref


class TakeCase:
    def __init__(self, name, world, subs, now=0, deadlines=None, cap_out=None, events=None, models=None):
        self.name = name
        self.events, self.models, self._ref = events, models, None
        self.tables, self.sessions, self.ring, self.heads = world.tables, world.sessions, world.ring, world.heads
        self.subs = None if subs is None else np.asarray(subs, dtype=np.uint32)
        self.now = now
        self.deadlines = None if deadlines is None else np.asarray(deadlines, dtype=np.uint64)
        self.cap_out = cap_out

    def reference(self, cap_out="case"):
        """The fold is evaluated once; a capacity below its items only sets the flag, as take_reference does."""
        cap = self.cap_out if cap_out == "case" else cap_out
        if self._ref is None:
            self._ref = R.take_reference(self, None, self.events, clone_models(self.models, self.events))
        ref = self._ref
        if cap is not None and ref["summary"][3] > cap:
            ref = dict(ref, full=True, summary=[ref["summary"][0] | R.F_OUTPUT_FULL] + ref["summary"][1:])
        return ref


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
    # the top of the byte fields: 8 full rings of 128, heads up to 127; 1, 2 and 130 candidates a class
    w = q128_world(3)
    per = [1, 2, 130]
    rnd = random.Random(128)
    classes = []
    for e in per:
        box = [k for k in range(8) for _ in range(e)]
        rnd.shuffle(box)
        classes += box
    off = np.concatenate([[0], np.cumsum([8 * e for e in per])])
    cases.append(PutCase("q128_full_bytes", w, [2, 0, 1], off, classes, opts=[i % 3 for i in range(len(classes))],
                         refs=np.arange(5000, 5000 + len(classes))))
    # L > M on the large ring: room for all, for some, for none
    w = World([T_Q128_ABOVE], 2, 3, 128).fill(1, {0: msgs(1000, 101), 1: msgs(2000, 127), 2: msgs(3000, 128)}, head={0: 120, 1: 5, 2: 127})
    cases.append(PutCase("q128_above_max", w, [1], [0, 10], [0, 1, 0, 2, 1, 0, 0, 2, 1, 0]))
    # a table of 3 classes on 7 rings; a length in ring 5 is flagged and read as empty
    w = classes_below_c_world()
    cases.append(PutCase("classes_below_c", w, [1, 0], [0, 6, 12], [5, 0, 1, 2, 6, 0xFF, 5, 0, 1, 2, 6, 0xFF]))
    # 65 inboxes: at G = 4 the second tile holds one group, and that one has the work
    w = one_group_world()
    sizes = [i % 3 for i in range(64)] + [11]
    off = np.concatenate([[0], np.cumsum(sizes)])
    cases.append(PutCase("one_group_last_tile", w, list(range(65)), off, [i % 2 for i in range(int(off[-1]))],
                         opts=[i % 3 for i in range(int(off[-1]))]))
    return cases


T_Q128 = ([INF, 7, 6, 5, 4, 3, 2, -1], 6, 128, 1, 0)
T_Q128_ABOVE = ([5, 2, 0], 1, 100, 1, 0)
Q128_HEADS = (127, 0, 1, 64, 126, 63, 65, 2)


def q128_world(n, **columns):
    """Every class of every session full at 128; the entry at ring position p has QoS p % 3, its ref
    is 1024 * session + 128 * class + age."""
    w = World([T_Q128], n, 8, 128, **columns)
    for s in range(n):
        w.fill(s, {k: [(1024 * s + 128 * k + i, (Q128_HEADS[k] + i) % 128 % 3) for i in range(128)] for k in range(8)},
               head=dict(enumerate(Q128_HEADS)))
    return w


def classes_below_c_world(**columns):
    w = World([T_THREE], 2, 7, 32, **columns)
    for s in range(2):
        w.fill(s, {0: msgs(100 * s, 2), 1: msgs(100 * s + 10, 3), 2: msgs(100 * s + 20, 2)}, head={0: 31, 1: 30, 2: 5})
    w.ring[1, 5] = R.as_rows(msgs(900, 3), 32, 7, P.ENTRY)  # what the length below would name
    w.heads["len"][1][5] = 3
    w.heads["head"][1][5] = 7
    return w


def one_group_world(**columns):
    """65 sessions; of the last tile at G = 4 (session 64 alone) the only one is OK and holds work."""
    flags = np.array([window.PRESENT | window.CONNECTED, 0, window.PRESENT | window.PASS, window.PRESENT] * 16 + [window.PRESENT | window.CONNECTED])
    w = World([T_TWO, ([0], 0, 1, 1, 0)], 65, 2, 8, table=np.array([0, 0, 0, 1] * 16 + [0]), flags=flags, **columns)
    for s in range(65):
        w.fill(s, {0: msgs(10 * s, 1 + s % 3, opts=s % 3), 1: msgs(10 * s + 5, s % 4)}, head={0: s % 8, 1: 7})
    w.fill(64, {0: msgs(640, 3), 1: [(645, 0), (646, 1), (647, 2)]}, head={0: 6, 1: 7}, order=[1, 0], credit=1, last=1)
    return w


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
    # all 1024 entries of 8 full rings of 128: QoS 0 / 1 / 2 by ring position, every 5th ref expired
    w = q128_world(1, inflight_max=0, next_pkt_id=65000)
    cases.append(TakeCase("q128_full_bytes", w, [0], now=50, deadlines=[10 if r % 5 == 0 else 99 for r in range(1024)]))
    # Qc 32: head 15, 20 entries; position 15 is a plain send, every expired or QoS 0 entry stands in word 1
    # or behind the ring end; the budget of 6 ends at position 22
    w = World([([5, 0], 1, 32, 1, 0)], 1, 2, 32, inflight_max=6)
    w.fill(0, {0: [(i, 1 if i == 0 else (0, 1, 1, 2)[i % 4]) for i in range(20)], 1: msgs(40, 4)}, head={0: 15, 1: 30})
    cases.append(TakeCase("q32_bits_word1", w, [0], now=50, deadlines=[10 if 0 < i < 20 and i % 4 == 1 else 99 for i in range(44)]))
    w = classes_below_c_world(inflight_max=0)
    cases.append(TakeCase("classes_below_c", w, [1, 0]))
    w = one_group_world(inflight_max=np.array([s % 4 for s in range(65)]))
    cases.append(TakeCase("one_group_last_tile", w, list(range(65)), now=50, deadlines=[10 if r % 7 == 0 else 99 for r in range(650)]))
    # mult 3, base 2: class 1 (priority 0) has credit (0 + 2 + 1) * 3 - 1 = 8; the ninth send is the budget's last
    # and leaves credit 0; the second take of the session shifts before anything else
    for name, w in zip(("credit_ends_with_budget", "credit_ends_with_budget_again"), credit_worlds()):
        cases.append(TakeCase(name, w, [0]))
    return cases


T_CREDIT = ([5, 0], 1, 16, 3, 2)


def credit_worlds():
    """The session before its first take, and what that take leaves (the acks reopened the window)."""
    first = World([T_CREDIT], 1, 2, 16, inflight_max=9).fill(0, {0: msgs(10, 2), 1: msgs(20, 12)}, head={0: 3, 1: 10}, order=[1, 0])
    second = World([T_CREDIT], 1, 2, 16, inflight_max=9, next_pkt_id=10)
    second.fill(0, {0: msgs(10, 2), 1: msgs(29, 3)}, head={0: 3, 1: 3}, order=[1, 0], credit=0, last=1)
    second.ring[:] = first.ring  # (a take only reads the rings: the consumed entries are still there)
    return first, second


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
    n, c, qc = ring.shape
    as_bytes = lambda r: np.ascontiguousarray(r).view(np.uint8).reshape(n, c, qc, -1)  # noqa: E731
    same = (as_bytes(ring) == as_bytes(case.ring)).all(axis=-1)
    owned = np.zeros(n, dtype=bool)
    owned[list(ref["models"])] = True
    assert same[~owned].all(), np.argwhere(~same & ~owned[:, None, None])[:4].tolist()
    if heads is None:
        return
    h, ln = heads["head"][:, :c].astype(np.int64), heads["len"][:, :c].astype(np.int64)
    live = ((np.arange(qc) - h[..., None]) % qc) < ln[..., None]
    assert (same | live)[owned].all(), np.argwhere(~same & ~live & owned[:, None, None])[:4].tolist()


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


# ---- the lattice -----------------------------------------------------------------------------------

LATTICE_SHAPES = ((1, 128), (2, 32), (3, 16), (5, 8), (5, 64), (7, 32), (8, 8), (8, 128))
LATTICE_N = 129        # 1 mod 64: the last tile holds one group at every group width
LATTICE_SEED = 20260301
LATTICE_PRIOS = [INF, 9, 5, 2, 0, -1, -3]  # (an eighth class draws 7 as well: the priorities of a table differ)
LATTICE_FIT, LATTICE_UNFIT = 10, [([0], 0, 1, 1, 0), ([1, 2], 0, 2, 1, 0), ([0], 0, 2, 0, 0)]
REF_BASE = 1 << 16     # a put without refs stores delivery positions, which stay below; every other ref is unique above
WILD_REF = 0xFFFF0000  # a few old entries name no deadline
CONN = window.PRESENT | window.CONNECTED
NOW = 1000


class Snapshot:
    def __init__(self, w):
        self.tables, self.sessions, self.ring, self.heads = w.tables, w.sessions.copy(), w.ring.copy(), w.heads.copy()


class Lattice:
    """A seeded world of ``n`` sessions at C x Qc and its rounds.  ``rounds(g)`` yields put and take
    cases in turn, each on a snapshot of the world as the calls before left it; the caller runs the
    case and hands the tables it leaves to ``advance``.  The restatement's models, its event counters,
    the flags it raised and what went into and came out of every queue are kept across the rounds."""

    def __init__(self, c, qc, n=LATTICE_N, seed=LATTICE_SEED):
        self.rnd = rnd = random.Random(1000003 * seed + 1009 * c + qc)
        self.c, self.qc, self.n = c, qc, n
        self.events, self.models = R.all_events(), {}
        self.flags = {"put": 0, "take": 0}
        configs = []
        for i in range(LATTICE_FIT):
            k = c if i == 0 else rnd.randrange(1, c + 1)
            prios = sorted(rnd.sample(LATTICE_PRIOS + ([7] if k == 8 else []), k), key=lambda p: 10 ** 7 if p == INF else p, reverse=True)
            configs.append((prios, rnd.randrange(k), rnd.choice([2, qc // 2, qc - 1, qc]), rnd.choice([1, 3, 1024]), rnd.choice([0, 2])))
        self.configs = configs
        table = np.array([rnd.randrange(LATTICE_FIT) if x < 0.92 else LATTICE_FIT + rnd.randrange(3) if x < 0.97 else 77
                          for x in (rnd.random() for _ in range(n))])
        imax = np.array([rnd.choice([0, 1, 3, 40]) for _ in range(n)])
        flags = np.array([rnd.choice([CONN] * 6 + [window.PRESENT, window.PRESENT | window.PASS, CONN | window.PASS, 0]) for _ in range(n)])
        table[0], flags[0] = 0, CONN  # session 0: every put brings it 3 * Qc candidates of one class
        self.world = w = World(configs + LATTICE_UNFIT, n, c, qc, table=table, flags=flags, inflight_max=imax,
                               inflight=np.array([rnd.randrange(m + 2) for m in imax]),
                               next_pkt_id=np.array([rnd.choice([1, 4000, 65534, 65535]) for _ in range(n)]),
                               mq_max=np.array([0 if s == 0 or rnd.random() < 0.97 else 5 for s in range(n)]),
                               dropped=np.array([rnd.choice([0, 0, 7, 0xFFFFFFFE]) for _ in range(n)], dtype=np.uint64))
        # every ring position holds an entry of its own: the live ones are the queues, the others must stay
        gen = np.random.default_rng(rnd.randrange(1 << 30))
        ground = P.empty_ring(n, c, qc)
        ground["ref"] = REF_BASE + np.arange(n * c * qc).reshape(n, c, qc)
        ground["opts"] = gen.choice([0, 1, 2, 1, 2, 0x11, 0x42], size=(n, c, qc))
        wild = gen.random((n, c, qc)) < 0.002
        ground["ref"][wild] = WILD_REF + np.arange(int(wild.sum()))
        self.next_ref = REF_BASE + n * c * qc
        for s in range(n):
            if table[s] >= LATTICE_FIT:
                self._fill(s, ground, {0: 2}, [0])
                continue
            m, k = configs[table[s]][2], len(configs[table[s]][0])
            lens = {cl: rnd.choice([0, 1, m - 1, m, m + 1 if m < qc else m, qc]) for cl in range(k)}
            order = [cl for cl in lens if lens[cl]]
            rnd.shuffle(order)
            self._fill(s, ground, lens, order)
            if s and rnd.random() < 0.03:
                self._malform(s, k)
        w.ring[:] = ground  # (the same entries at the live positions)
        self.put_in, self.came_out, self.lost = ({s: [] for s in range(n)} for _ in range(3))
        for s in range(n):
            if R.session_status(w.sessions, w.heads, w.tables, s, c, qc)[0] == R.A_OK:
                t = w.tables[int(w.heads["table"][s])]
                mq, _ = R.model_of(w.heads[s], t, w.ring[s], qc)
                self.put_in[s] = [(m[0], cl) for cl, q in R.logical(mq, t)["queues"].items() for m in q]

    def _fill(self, s, ground, lens, order):
        rnd, qc = self.rnd, self.qc
        head = {cl: rnd.choice([rnd.randrange(qc), rnd.randrange(qc), qc - 1]) for cl in lens}
        queues = {cl: [(int(ground["ref"][s, cl, (head[cl] + i) % qc]), int(ground["opts"][s, cl, (head[cl] + i) % qc])) for i in range(ln)]
                  for cl, ln in lens.items()}
        self.world.fill(s, queues, order=order, head=head, credit=rnd.choice([-1, 0, 1, 5]), last=rnd.randrange(2))

    def _malform(self, s, k):
        """One of the ways of the case malformed_heads, or a length in a ring the table has no class for."""
        h, rnd = self.world.heads, self.rnd
        how = rnd.randrange(8)
        if how == 0:
            h["order"][s] = 0xFFFFFF00 | (int(h["order"][s]) & 0xF) * 0x11  # a class twice
        elif how == 1:
            h["order"][s] = int(h["order"][s]) >> 4 | 0xF0000000            # misses a non-empty class
        elif how == 2:
            h["len"][s][rnd.randrange(k)] = 200
        elif how == 3:
            h["head"][s][rnd.randrange(k)] = self.qc + 1
        elif how == 4:
            h["credit"][s] = -7
        elif how == 5:
            h["len"][s][rnd.randrange(k)] = 0                               # the order may list an empty class
        elif how == 6:
            h["flags"][s] = int(h["flags"][s]) | 4
        else:
            h["len"][s][rnd.randrange(k, 8) if k < 8 else 7] = 3            # a ring the table has no class for (with 8: the order misses it)

    # ---- the rounds
    def rounds(self, g, rounds=3):
        for i in range(rounds):
            yield "put", self.put_round(i, g[i % len(g)] if isinstance(g, tuple) else g)
            yield "take", self.take_round(i)

    def put_round(self, i, g):
        rnd, n, qc = self.rnd, self.n, self.qc
        subs = rnd.sample(range(1, n), rnd.randrange(n // 2, n - 1))
        subs.insert(rnd.randrange(len(subs) + 1), 0)
        if i == 2:
            subs.insert(rnd.randrange(len(subs)), n + 5)  # a subscriber the table lacks
        sizes = [3 * qc if s == 0 else rnd.choice([0, 1, g - 1, g, g + 1, 2 * g + 1, 3 * qc]) for s in subs]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        total = int(off[-1])
        assert total < REF_BASE
        n_msgs, n_tables = total // 3 + 2, self.world.tables.size
        gen = np.random.default_rng(rnd.randrange(1 << 30))
        msg_class = gen.choice(list(range(self.c + 2)) + [200, 0xFF], size=(n_msgs, n_tables)).astype(np.uint8)
        msg_class[0] = rnd.randrange(self.c)  # message 0 is session 0's: one class, whatever the table
        src = gen.integers(1, n_msgs, size=total)
        src[gen.random(total) < 0.02] = n_msgs + 3
        verdicts = gen.choice([R.W_QUEUED, R.W_SEND, R.W_SEND_QOS0, R.W_QUEUED_DROPPED, R.W_QUEUED | R.W_EVICTS], size=total,
                              p=[0.75, 0.1, 0.1, 0.025, 0.025])
        at = subs.index(0)
        src[int(off[at]):int(off[at + 1])] = 0
        verdicts[int(off[at]):int(off[at + 1])] = R.W_QUEUED
        refs = None
        if i % 2 == 0:
            refs = np.arange(self.next_ref, self.next_ref + total)
            self.next_ref += total
        return PutCase("lattice_put_%d" % i, Snapshot(self.world), subs, off, None, opts=gen.choice([0, 1, 2, 0x11, 0x42], size=total),
                       verdicts=verdicts, refs=refs, src=src, msg_class=msg_class, events=self.events, models=self.models)

    def take_round(self, i):
        """Round 1 is one item short (``case.cap_out``); ``case.room`` is what it needs."""
        rnd, n = self.rnd, self.n
        rec = self.world.sessions = self.world.sessions.copy()  # (what the call before left stays as it was)
        rec["inflight"] = [rnd.randrange(int(m) + 2) for m in rec["inflight_max"]]  # the acks reopened some windows
        subs = None
        if i % 3 != 2:
            subs = rnd.sample(range(n), rnd.randrange(n // 2, n))
            if i == 0:
                subs.insert(rnd.randrange(len(subs)), n + 9)
        gen = np.random.default_rng(rnd.randrange(1 << 30))
        deadlines = gen.choice(np.array([NOW - 500, NOW + 500, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64), size=self.next_ref, p=[0.2, 0.4, 0.4])
        case = TakeCase("lattice_take_%d" % i, Snapshot(self.world), subs, now=NOW, deadlines=deadlines, events=self.events, models=self.models)
        case.room = case.reference(None)["summary"][3]
        assert case.room > 0
        case.cap_out = case.room - 1 if i == 1 else case.room
        return case

    def advance(self, kind, case, sessions, ring, heads, cap_out="case"):
        """The world becomes what the call left; the models, flags, and the ledger follow the restatement."""
        ref = case.reference() if kind == "put" else case.reference(cap_out)
        self.flags[kind] |= ref["summary"][0]
        if ref.get("full"):
            return
        w = self.world
        w.sessions, w.ring, w.heads = sessions, ring, heads
        for sub, (mq, _, _) in ref["models"].items():
            self.models[sub] = mq
        if kind == "put":
            left_out = set(ref["left_out"])
            for k, sub in enumerate(int(s) for s in case.subs):
                if sub not in ref["models"]:
                    continue
                for d in range(int(case.offsets[k]), int(case.offsets[k + 1])):
                    if ref["verdicts"][d] == 0 or d in left_out:
                        continue
                    name = int(case.refs[d]) if case.refs is not None else d
                    self.put_in[sub].append((name, ref["classes"][d]))
                    if ref["verdicts"][d] & R.W_MASK == R.W_QUEUED_DROPPED:
                        self.lost[sub].append(name)
                    if ref["evicted"][d][0] != R.NO_REF:
                        self.lost[sub].append(ref["evicted"][d][0])
        else:
            subs = range(self.n) if case.subs is None else [int(s) for s in case.subs]
            for k, sub in enumerate(subs):
                lo, hi = ref["offsets"][k], ref["offsets"][k + 1]
                if hi > lo:
                    self.came_out[sub] += list(zip(ref["refs"][lo:hi], ref["classes"][lo:hi]))

    def drained(self, got):
        """A take of every session (subs NULL) outside the rounds."""
        for sub in range(self.n):
            lo, hi = int(got.offsets[sub]), int(got.offsets[sub + 1])
            self.came_out[sub] += list(zip(got.refs[lo:hi].tolist(), got.classes[lo:hi].tolist()))

    def check_conservation(self):
        """Everything put and neither evicted nor left outside a full ring came out once, FIFO within a class."""
        assert int(self.world.sessions["mq_len"][[s for s in range(self.n) if self.put_in[s]]].sum()) == 0
        for sub in range(self.n):
            gone = list(self.lost[sub])
            kept = []
            for name, cl in self.put_in[sub]:
                if name in gone:
                    gone.remove(name)
                else:
                    kept.append((name, cl))
            assert not gone, (sub, gone)
            assert sorted(self.came_out[sub]) == sorted(kept), sub
            for cl in range(self.c):
                assert [r for r, k in self.came_out[sub] if k == cl] == [r for r, k in kept if k == cl], (sub, cl)
