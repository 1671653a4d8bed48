"""Cases of the ack stage shared by the CPU and the GPU tests: every cell of the table of
include/emqx_ack.h alone, the orders in which one id can be acked, list lengths around the wave and
the tile (emqx_amd/csrc/ack.h: AK_TILE), skewed lists, sessions that take no acks, a randomised
batch; and for the record call rows with holes, sends across a tile border, a bad subscriber.  A
case computes its reference (tests/ack_ref.py) once."""

import numpy as np

from emqx_amd import ack as A
from emqx_amd import window as W
from tests import ack_ref as R

T = A.TILE
E, M, P = R.EMPTY, R.MSG, R.PUBREL_AWAIT
ACK, REC, COMP = R.PUBACK, R.PUBREC, R.PUBCOMP
LIVE = W.PRESENT | W.CONNECTED


def rows_of(slots):
    return [[[int(s["pkt_id"]), int(s["phase"]), int(s["qos"]), int(s["ref"])] for s in row] for row in slots]


def slots_of(rows, w):
    t = A.empty_slots(len(rows), w)
    for i, row in enumerate(rows):
        for j, s in enumerate(row):
            t[i, j] = tuple(s)
    return t


def records_of(table):
    return [{f: int(table[f][i]) for f in W.SESSION.names} for i in range(table.size)]


def row(entries, w, at=None):
    """A row of w slots holding `entries` ([pkt_id, phase, qos, ref]) at the slot indices `at`
    (default: the first ones)."""
    r = [[0, E, 0, 0] for _ in range(w)]
    for i, e in enumerate(entries):
        r[i if at is None else at[i]] = list(e)
    return r


def acks(pairs):
    return [(k << 16) | i for k, i in pairs]


class RunCase:
    """Sessions given as (record fields or None, row, acks): None is a subscriber id at or above
    sub_limit.  Sessions no list names lie between them in the tables."""

    def __init__(self, sessions, w=16, spare=2):
        self.w = w
        recs, rows, subs, bad = [], [], [], 0
        lens = []
        flat = []
        for i, (rec, r, a) in enumerate(sessions):
            lens.append(len(a))
            flat.extend(a)
            if rec is None:
                subs.append(None)
                continue
            for j in range((i + 1) % (spare + 1)):  # sessions no list names, with rows that must not change
                recs.append(dict(flags=LIVE, inflight=3, inflight_max=w))
                rows.append(row([[100 + j, M, 1, 5], [7, P, 2, 6]], w, at=[1, w - 1]))
            subs.append(len(recs))
            recs.append(dict(dict(flags=LIVE, inflight=sum(1 for s in r if s[1] != E), inflight_max=w), **rec))
            rows.append(r)
        recs.append(dict(flags=LIVE, inflight=1, inflight_max=w))
        rows.append(row([[9, M, 1, 1]], w))
        for k, s in enumerate(subs):
            if s is None:
                subs[k] = len(recs) + 3 * bad  # the first of them is sub_limit itself
                bad += 1
        self.subs = np.asarray(subs, dtype=np.uint32)
        self.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.acks = np.asarray(flat, dtype=np.uint32)
        self.table = W.pack_sessions(len(recs), inflight=[r["inflight"] for r in recs], inflight_max=[r["inflight_max"] for r in recs],
                                     flags=[r["flags"] for r in recs], next_pkt_id=77, mq_len=4, dropped=1 << 33)
        self.slots = slots_of(rows, w)
        self.m, self.total, self.sub_limit = len(sessions), len(flat), len(recs)
        self._ref = {}

    def reference(self, update_table=False):
        if update_table not in self._ref:
            recs, rows = records_of(self.table), rows_of(self.slots)
            r = R.run(self.subs, self.offsets, self.acks, recs, rows, update_table=update_table)
            table = self.table.copy()
            table["inflight"] = [x["inflight"] for x in recs]
            self._ref[update_table] = {
                "verdicts": np.asarray(r["verdicts"], dtype=np.uint8), "refs": np.asarray(r["refs"], dtype=np.uint32),
                "counts": np.asarray(r["counts"], dtype=np.uint32).reshape(-1, 4), "summary": r["summary"],
                "slots": slots_of(rows, self.w), "table": table}
        return self._ref[update_table]


def check_run(ref, got, slots=None, table=None):
    """``got``: an emqx_amd.ack.Acked; ``slots`` and ``table``: the tables after the call."""
    assert [got.summary[k] for k in A.RUN_SUMMARY] == ref["summary"], (got.summary, ref["summary"])
    bad = np.flatnonzero(got.verdicts != ref["verdicts"])
    assert bad.size == 0, ("verdicts", bad[:8], got.verdicts[bad[:8]], ref["verdicts"][bad[:8]])
    bad = np.flatnonzero(got.refs != ref["refs"])
    assert bad.size == 0, ("refs", bad[:8], got.refs[bad[:8]], ref["refs"][bad[:8]])
    assert got.verdicts.dtype == np.uint8 and got.refs.dtype == np.uint32
    assert got.counts.tobytes() == ref["counts"].tobytes(), (got.counts, ref["counts"])
    if slots is not None:
        bad = np.flatnonzero((slots != ref["slots"]).any(axis=1))
        assert bad.size == 0, ("rows", bad[:4], slots[bad[:2]], ref["slots"][bad[:2]])
    if table is not None:
        assert table.tobytes() == ref["table"].tobytes(), (table["inflight"], ref["table"]["inflight"])


def same_run(x, y):
    assert x.summary == y.summary
    for a, b in zip(x[:-1], y[:-1]):
        assert a.tobytes() == b.tobytes()


# ---- the run call ------------------------------------------------------------------------------

def filler(seed, w=16):
    """A session with a few inflight entries and a short valid list."""
    ids = [1000 + 10 * seed + i for i in range(3)]
    return ({}, row([[ids[0], M, 1, 11 + seed], [ids[1], M, 2, 12 + seed], [ids[2], P, 2, 13 + seed]], w, at=[0, 3, w - 2]),
            acks([(ACK, ids[0]), (REC, ids[1]), (COMP, ids[2])][:1 + seed % 3]))


def around(session, w=16):
    """The session between two short ones."""
    return RunCase([filler(1, w), session, filler(2, w)], w)


def one(entries, pairs, w=16, rec=None, at=None):
    return around((rec or {}, row(entries, w, at), acks(pairs)), w)


def mixed_list(n, seed, w=16):
    """n acks drawn from a row's ids, their neighbours and random ids, every kind."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.arange(2, 60000), size=w - 3, replace=False)
    entries = [[int(i), int(rng.choice([M, M, P])), int(rng.integers(1, 3)), int(rng.integers(0, 1 << 32))] for i in ids]
    pool = np.concatenate([ids, ids, ids + 1, rng.integers(0, 65536, 4)])
    kinds = rng.choice([ACK, REC, COMP, COMP, 0, 4, 65535], size=n, p=[0.3, 0.25, 0.2, 0.2, 0.02, 0.02, 0.01])
    return ({}, row(entries, w, at=list(range(1, w - 2))), acks(zip(kinds.tolist(), rng.choice(pool, size=n).tolist())))


def skew(w=16):
    """2 T + 1 acks to one session, the only valid ids at ranks 0, T and 2 T."""
    pairs = [(ACK, 60000 + (i % 5000)) for i in range(2 * T + 1)]
    pairs[0], pairs[T], pairs[2 * T] = (REC, 5), (COMP, 5), (ACK, 6)
    return around(({}, row([[5, M, 2, 50], [6, M, 1, 60], [7, M, 1, 70]], w, at=[2, 9, w - 1]), acks(pairs)), w)


def same_id_repeated(w=16):
    """The same valid id T + 1 times: the first is OK, every other NOT_FOUND."""
    return around(({}, row([[5, M, 1, 50]], w, at=[4]), acks([(ACK, 5)] * (T + 1))), w)


def full_row_reversed(w):
    entries = [[i + 1, M if i % 2 else P, 1 + i % 2, 1000 + i] for i in range(w)]
    return one(entries, [(ACK if i % 2 else COMP, i + 1) for i in reversed(range(w))], w)


CELLS = {
    "puback_msg": one([[4, M, 1, 40]], [(ACK, 4)]),
    "puback_await": one([[4, P, 2, 40]], [(ACK, 4)]),
    "puback_none": one([[4, M, 1, 40]], [(ACK, 5)]),
    "pubrec_msg": one([[4, M, 2, 40]], [(REC, 4)]),
    "pubrec_await": one([[4, P, 2, 40]], [(REC, 4)]),
    "pubrec_none": one([[4, M, 2, 40]], [(REC, 3)]),
    "pubcomp_msg": one([[4, M, 2, 40]], [(COMP, 4)]),
    "pubcomp_await": one([[4, P, 2, 40]], [(COMP, 4)]),
    "pubcomp_none": one([], [(COMP, 4)]),
}

RUNS = {
    "pubrec_then_pubcomp": lambda: one([[4, M, 2, 40]], [(REC, 4), (COMP, 4)]),
    "pubcomp_before_pubrec": lambda: one([[4, M, 2, 40]], [(COMP, 4), (REC, 4)]),
    "puback_twice": lambda: one([[4, M, 1, 40]], [(ACK, 4), (ACK, 4)]),
    "pubrec_puback_pubcomp_pubcomp": lambda: one([[4, M, 2, 40]], [(REC, 4), (ACK, 4), (COMP, 4), (COMP, 4)]),
    "pubrec_twice_then_pubcomp_twice": lambda: one([[4, M, 2, 40]], [(REC, 4), (REC, 4), (COMP, 4), (COMP, 4), (REC, 4)]),
    "ids_0_1_65535": lambda: one([[0, M, 1, 1], [1, M, 1, 2], [65535, P, 2, 3]], [(ACK, 65535), (ACK, 0), (COMP, 65535), (ACK, 1), (ACK, 2)],
                                 at=[0, 7, 15]),
    "kind_0_and_4": lambda: one([[4, M, 1, 40]], [(0, 4), (4, 4), (65535, 4), (ACK, 4)]),
    "id_held_twice": lambda: one([[4, M, 1, 40], [4, P, 2, 41]], [(COMP, 4), (ACK, 4), (COMP, 4), (ACK, 4)], at=[3, 8]),
    "unknown_phase": lambda: one([[4, 3, 1, 40], [5, 255, 1, 41]], [(ACK, 4), (REC, 5), (COMP, 4), (COMP, 5)]),
    "full_row_reversed_w8": lambda: full_row_reversed(8),
    "full_row_reversed_w32": lambda: full_row_reversed(32),
    "full_row_reversed_w64": lambda: full_row_reversed(64),
    "empty_row": lambda: one([], [(ACK, 1), (REC, 2), (COMP, 3)]),
    "skew_2T+1": skew,
    "same_id_T+1_times": same_id_repeated,
    "not_present": lambda: one([[4, M, 1, 40]], [(ACK, 4), (0, 4)], rec=dict(flags=W.CONNECTED)),
    "pass": lambda: one([[4, M, 1, 40]], [(ACK, 4), (9, 4)], rec=dict(flags=LIVE | W.PASS)),
    "sub_at_sub_limit": lambda: RunCase([filler(1), (None, None, acks([(ACK, 4), (COMP, 5)])), filler(2), (None, None, acks([(REC, 1)]))]),
    "empty_lists_before_between_after": lambda: RunCase([({}, row([[1, M, 1, 1]], 16), []), ({}, row([], 16), []), filler(1),
                                                         ({}, row([[2, P, 2, 2]], 16), []), filler(2), ({}, row([], 16), [])]),
    "no_sessions": lambda: RunCase([]),
    "inflight_below_released": lambda: one([[4, M, 1, 40], [5, P, 2, 50], [6, M, 2, 60]], [(ACK, 4), (COMP, 5), (REC, 6)],
                                           rec=dict(inflight=1, inflight_max=2)),
    "inflight_max_0": lambda: one([[4, M, 1, 40]], [(ACK, 4)], rec=dict(inflight=9, inflight_max=0)),
    "inflight_over_max": lambda: one([[4, M, 1, 40]], [(ACK, 4)], rec=dict(inflight=40, inflight_max=16)),
}
for _n in (0, 1, 63, 64, 65, T - 1, T, T + 1):
    RUNS["list_of_%d" % _n] = (lambda n: lambda: around(mixed_list(n, seed=n)))(_n)
for _name in CELLS:
    RUNS[_name] = (lambda c: lambda: c)(CELLS[_name])

# what each cell of the table answers: verdict, ref, the slot's phase after, released, to_pubrel
CELL_ANSWERS = {
    "puback_msg": (R.A_OK, 40, E, 1, 0), "puback_await": (R.A_IN_USE, R.NO_REF, P, 0, 0), "puback_none": (R.A_NOT_FOUND, R.NO_REF, M, 0, 0),
    "pubrec_msg": (R.A_OK, 40, P, 0, 1), "pubrec_await": (R.A_IN_USE, R.NO_REF, P, 0, 0), "pubrec_none": (R.A_NOT_FOUND, R.NO_REF, M, 0, 0),
    "pubcomp_msg": (R.A_IN_USE, R.NO_REF, M, 0, 0), "pubcomp_await": (R.A_OK, 40, E, 1, 0), "pubcomp_none": (R.A_NOT_FOUND, R.NO_REF, E, 0, 0),
}


def fuzz(seed=3, n_sessions=2500, w=16):
    """A few thousand sessions with random rows (some holding an id twice) and ack lists drawn from
    the row's ids, their neighbours and random ids; a few without a record, with PASS, or beyond
    the table; a few long lists."""
    rng = np.random.default_rng(seed)
    sessions = []
    for i in range(n_sessions):
        n = int(rng.integers(0, 9)) if rng.random() < 0.99 else int(rng.integers(200, 1500))
        rec, r, a = mixed_list(n, seed=seed * 100003 + i, w=w)
        if rng.random() < 0.1:
            r[0] = list(r[int(rng.integers(1, w - 2))])  # an id held twice, the copy in the lower slot
            r[0][3] = 1
        if rng.random() < 0.3:
            r = [s if rng.random() < 0.5 else [0, E, 0, 0] for s in r]
        kind = rng.random()
        rec = dict(inflight=int(rng.integers(0, w + 3)), inflight_max=int(rng.choice([0, 1, w])))
        if kind < 0.03:
            rec["flags"] = W.CONNECTED
        elif kind < 0.06:
            rec["flags"] = LIVE | W.PASS
        sessions.append((None if 0.06 <= kind < 0.08 else rec, r, a))
    return RunCase(sessions, w)


def strided_run(w=16):
    """7 T + 5 acks over more than 100 sessions, for a grid capped below the 8 tiles and the four
    or more groups of rows: one list over tiles 0, 1 and 2 with the PUBREC and the PUBCOMP of one
    slot in different tiles (in order twice, the PUBCOMP first once); lists that start exactly at
    3 T, 5 T and 6 T; empty lists at the 3 T border and behind the last ack; a session that is not
    present whose list crosses the 4 T border; a subscriber beyond the table."""
    sessions, at = [], [0]

    def add(session):
        sessions.append(session)
        at[0] += len(session[2])

    def fill_to(pos):
        while at[0] < pos:
            k = len(sessions)
            add(mixed_list(min(pos - at[0], 20 + 7 * k % 31), seed=9000 + 100 * w + k, w=w))

    add(filler(1, w))  # two acks: rank i of the next list is position 2 + i
    pairs = [(ACK, 60000 + i % 5000) for i in range(2 * T + 200)]
    pairs[10], pairs[T + 10] = (REC, 5), (COMP, 5)          # tiles 0 and 1
    pairs[T + 20], pairs[2 * T + 20] = (REC, 6), (COMP, 6)  # tiles 1 and 2
    pairs[30], pairs[2 * T + 30] = (COMP, 7), (REC, 7)      # the PUBCOMP first: tiles 0 and 2
    pairs[-1] = (ACK, 8)
    add(({}, row([[5, M, 2, 50], [6, M, 2, 60], [7, M, 2, 70], [8, M, 1, 80]], w, at=[2, 5, w // 2 + 1, w - 1]), acks(pairs)))
    fill_to(3 * T)
    add(({}, row([[1, M, 1, 1]], w), []))
    add(({}, row([], w), []))
    add(mixed_list(70, seed=71, w=w))  # starts at 3 T
    fill_to(4 * T - 10)
    add((dict(flags=W.CONNECTED), row([[4, M, 1, 40]], w, at=[3]), acks([(ACK, 4), (REC, 4)] * 10)))  # not present, over 4 T
    add((dict(flags=LIVE | W.PASS), row([[4, P, 2, 40]], w), acks([(COMP, 4)])))
    add((None, None, acks([(ACK, 4), (COMP, 5), (REC, 6)])))
    fill_to(5 * T)
    add(mixed_list(T, seed=72, w=w))  # starts at 5 T, the next one at 6 T
    fill_to(7 * T + 5)
    add(({}, row([[2, P, 2, 2]], w), []))
    add(({}, row([], w), []))
    case = RunCase(sessions, w)
    assert case.total == 7 * T + 5 and case.m > 100 and int(case.offsets[2]) > 2 * T
    return case


# ---- the record call ---------------------------------------------------------------------------

class RecCase:
    """Inboxes given as (row or None, [(verdict, opts, pkt_id), ...]): None is a subscriber id at
    or above sub_limit."""

    def __init__(self, boxes, w=16, refs=False, spare=2):
        self.w = w
        rows, subs, bad = [], [], 0
        ver, opts, ids, lens = [], [], [], []
        for i, (r, ds) in enumerate(boxes):
            lens.append(len(ds))
            ver += [d[0] for d in ds]
            opts += [d[1] for d in ds]
            ids += [d[2] for d in ds]
            if r is None:
                subs.append(None)
                continue
            for j in range((i + 1) % (spare + 1)):
                rows.append(row([[100 + j, M, 1, 5]], w, at=[2]))
            subs.append(len(rows))
            rows.append(r)
        rows.append(row([], w))
        for k, s in enumerate(subs):
            if s is None:
                subs[k] = len(rows) + 3 * bad
                bad += 1
        self.subs = np.asarray(subs, dtype=np.uint32)
        self.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.verdicts, self.opts = np.asarray(ver, dtype=np.uint8), np.asarray(opts, dtype=np.uint8)
        self.pkt_ids = np.asarray(ids, dtype=np.uint16)
        self.m, self.total, self.sub_limit = len(boxes), len(ver), len(rows)
        self.refs = (np.arange(self.total, dtype=np.uint32) * 2654435761 + 17).astype(np.uint32) if refs else None
        self.slots = slots_of(rows, w)
        self._ref = None

    def reference(self):
        if self._ref is None:
            rows = rows_of(self.slots)
            r = R.record(self.subs, self.offsets, self.opts, self.verdicts, self.pkt_ids, self.refs, rows)
            self._ref = {"unrecorded": np.asarray(r["unrecorded"], dtype=np.uint32), "summary": r["summary"],
                         "slots": slots_of(rows, self.w)}
        return self._ref


def check_rec(ref, got, slots):
    assert [got.summary[k] for k in A.RECORD_SUMMARY] == ref["summary"], (got.summary, ref["summary"])
    assert got.unrecorded.tobytes() == ref["unrecorded"].tobytes(), (got.unrecorded, ref["unrecorded"])
    bad = np.flatnonzero((slots != ref["slots"]).any(axis=1))
    assert bad.size == 0, ("rows", bad[:4], slots[bad[:2]], ref["slots"][bad[:2]])


SEND, SEND0, QUEUED = W.W_SEND, W.W_SEND_QOS0, W.W_QUEUED


def deliveries(n, sends, seed, first_id=1):
    """n deliveries of which `sends` are EMQX_W_SEND with consecutive ids, the rest QoS 0 sends,
    queued (some with the EVICTS bit) and skips, shuffled in place."""
    rng = np.random.default_rng(seed)
    is_send = np.zeros(n, dtype=bool)
    is_send[rng.choice(n, size=sends, replace=False)] = True
    out, nid = [], first_id
    for s in is_send:
        if s:
            out.append((SEND, int(rng.integers(1, 3)) | int(rng.integers(0, 2)) * 4, nid))
            nid = 1 if nid == 65535 else nid + 1
        else:
            v = int(rng.choice([SEND0, QUEUED, QUEUED | W.W_EVICTS, W.W_SKIP_NO_LOCAL, W.W_DROP_QOS0]))
            out.append((v, int(rng.integers(0, 3)), 0))
    return out


def holes(w=8):
    return row([[11, M, 1, 1], [12, P, 2, 2], [13, M, 1, 3], [14, M, 2, 4], [15, M, 1, 5]], w, at=[1, 3, 4, 6, 7])  # free: 0, 2, 5


def rec_filler(seed, w):
    return (row([[500 + seed, M, 1, 9]], w, at=[seed % w]), deliveries(5, 2, seed, first_id=600 + seed))


RECORDS = {
    "free_0_2_5_takes_1": lambda refs=False: RecCase([rec_filler(1, 8), (holes(), deliveries(4, 1, 1, 65535)), rec_filler(2, 8)], 8, refs),
    "free_0_2_5_takes_3": lambda refs=False: RecCase([rec_filler(1, 8), (holes(), deliveries(7, 3, 2, 65534)), rec_filler(2, 8)], 8, refs),
    "free_0_2_5_takes_4": lambda refs=False: RecCase([rec_filler(1, 8), (holes(), deliveries(9, 4, 3, 20)), rec_filler(2, 8)], 8, refs),
    "sends_interleaved_across_a_tile_border": lambda refs=False: RecCase(
        [(row([], 16), deliveries(T - 7, 5, 4)), (row([[1, M, 1, 1]], 16, at=[3]), deliveries(15, 8, 5, 100)), rec_filler(3, 16)], 16, refs),
    "one_inbox_over_3_tiles": lambda refs=False: RecCase(
        [rec_filler(1, 32), (row([[i, M, 1, i] for i in range(1, 13)], 32, at=list(range(0, 24, 2))), deliveries(3 * T + 7, 40, 6, 65520)),
         rec_filler(2, 32)], 32, refs),
    "bad_subscriber": lambda refs=False: RecCase([rec_filler(1, 16), (None, deliveries(6, 3, 7)), rec_filler(2, 16), (None, deliveries(2, 0, 8))],
                                                 16, refs),
    "no_deliveries": lambda refs=False: RecCase([(row([], 16), []), (holes(16), [])], 16, refs),
    "no_inboxes": lambda refs=False: RecCase([], 16, refs),
    "full_row_w64": lambda refs=False: RecCase([(row([[i + 1, M, 1, i] for i in range(64)], 64), deliveries(5, 3, 9)),
                                               (row([], 64), deliveries(80, 70, 10))], 64, refs),
    "total_T": lambda refs=False: RecCase([(row([], 16), deliveries(T // 2, 9, 11)), (row([], 16), deliveries(T - T // 2, 30, 12))], 16, refs),
}


def rec_fuzz(seed=5, n_boxes=1500, w=16):
    rng = np.random.default_rng(seed)
    boxes = []
    for i in range(n_boxes):
        n = int(rng.integers(0, 12)) if rng.random() < 0.99 else int(rng.integers(300, 1800))
        r = [[int(rng.integers(0, 65536)), int(rng.choice([M, P])), 1, i] if rng.random() < 0.4 else [0, E, 0, 0] for _ in range(w)]
        ds = deliveries(n, int(rng.integers(0, min(n, 20) + 1)), seed * 7919 + i, first_id=int(rng.integers(1, 65536)))
        if rng.random() < 0.05:
            ds = [(int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 65536))) for _ in range(n)]  # any bytes
        boxes.append((None if rng.random() < 0.02 else r, ds))
    return RecCase(boxes, w, refs=True)


def strided_record(refs=False, w=16):
    """7 T + 5 positions over more than 100 inboxes, for a grid capped below the 8 tiles and the
    four groups of rows: one inbox over tiles 0, 1 and 2 that takes more sends than its row has
    free slots; inboxes that start exactly at 3 T and 4 T; a full row; a subscriber beyond the
    table; empty inboxes at the end."""
    boxes, at = [], [0]

    def add(r, ds):
        boxes.append((r, ds))
        at[0] += len(ds)

    def fill_to(pos):
        while at[0] < pos:
            k = len(boxes)
            n = min(pos - at[0], 20 + 11 * k % 37)
            free = [j for j in range(w) if (j + k) % 3]
            add(row([[700 + j, M if j % 2 else P, 1 + j % 2, k] for j in range(w) if (j + k) % 3 == 0], w,
                    at=[j for j in range(w) if (j + k) % 3 == 0]), deliveries(n, min(n, len(free) - 3 + k % 6), 8000 + k, first_id=65530 - 7 * k))

    add(*rec_filler(1, w))
    add(row([[i, M, 1, i] for i in range(1, 7)], w, at=list(range(0, 12, 2))), deliveries(2 * T + 300, 40, 21, 65520))
    fill_to(3 * T)
    add(row([], w), deliveries(T, 9, 22))  # starts at 3 T, the next one at 4 T
    add(row([[i + 1, M, 1, i] for i in range(w)], w), deliveries(8, 3, 23))
    add(None, deliveries(6, 3, 24))
    fill_to(7 * T + 5)
    add(row([], w), [])
    add(holes(w), [])
    case = RecCase(boxes, w, refs)
    assert case.total == 7 * T + 5 and case.m > 100 and int(case.offsets[2]) > 2 * T
    return case
