"""A literal restatement of emqx_mqueue with a priority table (apps/emqx/src/emqx_mqueue.erl:159-254 over
apps/emqx/src/emqx_pqueue.erl:98-211) and of emqx_session:dequeue/1 on top of it, one message at a time:
the queue is a Python list of ``[key, deque]`` in list order, the key is ``-P`` or the atom ``infinity``,
``lists:keysort`` compares keys in Erlang term order (every number is below every atom), credits are
plain signed integers.  It models ``max_len`` 0 (unbounded) and 1 too, which the device stage refuses.
It counts its own events, so that a test can say what a workload reached.

The second half reads and writes the tables of include/emqx_pmqueue.h (the head normalisation rule is
restated here, not imported), and plays a put or a take call over the model."""

from collections import deque

import numpy as np

INF = "infinity"
INF_CREDIT = 1000000
W_SEND_QOS0, W_SEND, W_QUEUED, W_QUEUED_DROPPED, W_EVICTS, W_MASK = 1, 2, 3, 4, 0x80, 0x0F
EXPIRED = 10
A_OK, A_NO_SESSION, A_PASS, UNFIT = 1, 4, 5, 7
PRESENT, PASS = 1, 8
NO_REF, NO_CLASS = 0xFFFFFFFF, 0xFF
(F_INPUT_REFUSED, F_BAD_SUB, F_OUTPUT_FULL, F_BAD_REF, F_BAD_HEAD, F_ROW_FULL, F_UNFIT, F_BAD_VERDICT, F_BAD_SRC,
 F_LIMITED) = 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400
PRIO_INFINITY = 0x7FFFFFFF
EVENTS = ("shifts", "unsorted_activations", "infinity_last", "evictions", "negative_credit_steps",
          # what the calls count on top of the model (the ring positions are the tables', the model has none)
          "evictions_across_ring_end", "len_above_max_puts", "row_full_inboxes", "expired_at_16_up", "qos0_at_16_up",
          "credit_zero_on_last_send")


def term_key(key):
    """Erlang term order over the keys: number < atom."""
    return (1, 0) if key == INF else (0, key)


def keysort(lst):
    return sorted(lst, key=lambda e: term_key(e[0]))  # stable, as lists:keysort/2


def negate(p):  # maybe_negate_priority/1
    return INF if p == INF else -p


class MQ:
    """#mqueue{} with a p_table."""

    def __init__(self, max_len=0, mult=10, base=0, events=None):
        self.max_len, self.mult, self.base = max_len, mult, base
        self.q = []  # [[key, deque], ...] in list order
        self.len = 0
        self.dropped = 0
        self.last_prio = None  # undefined
        self.p_credit = None
        self.events = events if events is not None else dict.fromkeys(EVENTS, 0)

    def plen(self, p):
        for key, dq in self.q:
            if key == negate(p):
                return len(dq)
        return 0

    def priorities(self):
        return [negate(key) for key, _ in self.q]


def pq_in(x, p, mq):
    """emqx_pqueue:in/3 on the list."""
    key = negate(p)
    for e in mq.q:
        if e[0] == key:
            e[1].append(x)
            return
    new = [key, deque([x])]
    if key == INF:
        mq.q = [new] + mq.q  # pushed at the head, no sort
        return
    if mq.q != keysort(mq.q):
        mq.events["unsorted_activations"] += 1
    if mq.q and mq.q[0][0] == INF:
        mq.q = [mq.q[0]] + keysort([new] + mq.q[1:])
    else:
        if any(e[0] == INF for e in mq.q):
            mq.events["infinity_last"] += 1
        mq.q = keysort([new] + mq.q)


def pq_out_head(mq):
    """emqx_pqueue:out/1: from the head element, which is deleted when it empties."""
    key, dq = mq.q[0]
    x = dq.popleft()
    if not dq:
        mq.q.pop(0)
    return x, negate(key)


def pq_out_prio(p, mq):
    """emqx_pqueue:out/2."""
    key = negate(p)
    for i, e in enumerate(mq.q):
        if e[0] == key:
            x = e[1].popleft()
            if not e[1]:
                mq.q.pop(i)
            return x
    raise AssertionError("empty priority")


def mq_in(msg, p, mq):
    """emqx_mqueue:in/2; returns the dropped message or None."""
    if mq.max_len != 0 and mq.plen(p) == mq.max_len:
        dropped = pq_out_prio(p, mq)
        pq_in(msg, p, mq)
        mq.dropped += 1
        mq.events["evictions"] += 1
        return dropped
    mq.len += 1
    pq_in(msg, p, mq)
    return None


def credits(p, mq):
    return ((INF_CREDIT if p == INF else p) + mq.base + 1) * mq.mult - 1


def mq_out(mq):
    """emqx_mqueue:out/1; returns (message, priority it came from) or None."""
    while True:
        if mq.len == 0:
            return None
        if mq.last_prio is None:
            x, p = pq_out_head(mq)
            mq.len -= 1
            mq.last_prio = p
            mq.p_credit = credits(p, mq)
            return x, p
        if mq.p_credit == 0:
            mq.q = mq.q[1:] + mq.q[:1]  # shift
            mq.last_prio = None
            mq.events["shifts"] += 1
            continue
        if mq.p_credit < 0:
            mq.events["negative_credit_steps"] += 1
        x, p = pq_out_head(mq)
        mq.len -= 1
        mq.p_credit -= 1
        return x, p


def batch_n(inflight_max, inflight):
    return 1000 if inflight_max == 0 else max(0, inflight_max - inflight)


def dequeue(cnt, mq, is_expired):
    """emqx_session:dequeue/3: [(message, priority, expired)] in order."""
    out = []
    while cnt > 0:
        got = mq_out(mq)
        if got is None:
            break
        msg, p = got
        if is_expired(msg):
            out.append((msg, p, True))
            continue
        out.append((msg, p, False))
        if msg[1] & 3:
            cnt -= 1
    return out


# ---- the tables of include/emqx_pmqueue.h ----------------------------------------------------------

def table_prios(t):
    return [INF if int(p) == PRIO_INFINITY else int(p) for p in t["prio"][:int(t["n_classes"])]]


def table_fit(t, c, qc):
    n = int(t["n_classes"])
    if not 1 <= n <= min(8, c) or int(t["default_class"]) >= n:
        return False
    if not 2 <= int(t["max_len"]) <= qc or not 1 <= int(t["mult"]) <= 1024 or int(t["base"]) > 1000000:
        return False
    prios = table_prios(t)
    if INF in prios[1:] or any(abs(p) > 1000000 for p in prios if p != INF):
        return False
    nums = [p for p in prios if p != INF]
    return all(a > b for a, b in zip(nums, nums[1:]))


def read_head(head, t, qc):
    """The head as the stage reads it: (heads, lens, order, credit, last_defined, malformed)."""
    n = int(t["n_classes"])
    bad = False
    heads, lens = [], []
    for c in range(8):
        h, ln = int(head["head"][c]), int(head["len"][c])
        if h >= qc or ln > qc or (c >= n and ln):
            bad = True
        heads.append(h % qc)
        lens.append(0 if c >= n else min(ln, qc))
    nibs = [(int(head["order"]) >> (4 * p)) & 0xF for p in range(8)]
    order = nibs[:nibs.index(0xF)] if 0xF in nibs else nibs
    want = [c for c in range(8) if lens[c]]
    if any(x != 0xF for x in nibs[len(order):]) or sorted(order) != want or len(set(order)) != len(order):
        order, bad = want, True
    credit = int(head["credit"])
    if credit < -1:
        credit, bad = -1, True
    if int(head["flags"]) & ~1:
        bad = True
    return heads, lens, order, credit, int(head["flags"]) & 1, bad


def model_of(head, t, rows, qc, events=None):
    """The MQ a normalised head and its class rings hold; messages are (ref, opts, None)."""
    heads, lens, order, credit, last, bad = read_head(head, t, qc)
    prios = table_prios(t)
    mq = MQ(int(t["max_len"]), int(t["mult"]), int(t["base"]), events)
    for c in order:
        dq = deque((int(rows[c][(heads[c] + i) % qc]["ref"]), int(rows[c][(heads[c] + i) % qc]["opts"]), None) for i in range(lens[c]))
        mq.q.append([negate(prios[c]), dq])
        mq.len += len(dq)
    mq.last_prio = "?" if last else None
    mq.p_credit = credit
    return mq, bad


def logical(mq, t):
    """What the tables must hold for the model: per class the (ref, opts) oldest first, the order list as
    class indices, the credit as the stage stores it (every negative value is -1; undefined is what it
    was), last_prio defined."""
    prios = table_prios(t)
    queues = {c: [] for c in range(8)}
    for key, dq in mq.q:
        queues[prios.index(negate(key))] = [(m[0], m[1]) for m in dq]
    credit = 0 if mq.p_credit is None else max(mq.p_credit, -1)
    return dict(queues=queues, order=[prios.index(negate(key)) for key, _ in mq.q], credit=credit,
                last=0 if mq.last_prio is None else 1, len=mq.len)


def session_status(sessions, heads, tables, sub, c, qc):
    """(status, flags) of a session for either call."""
    if sub >= sessions.size:
        return A_NO_SESSION, F_BAD_SUB
    fl = int(sessions["flags"][sub])
    if not fl & PRESENT:
        return A_NO_SESSION, 0
    if fl & PASS:
        return A_PASS, 0
    t = int(heads["table"][sub])
    if t >= tables.size or not table_fit(tables[t], c, qc):
        return UNFIT, F_UNFIT
    return A_OK, 0


def _model(case, sub, t, qc, events, models):
    """The model of an OK session: read from the tables, or the caller's own from the calls before (its
    messages become old ones)."""
    mq, bad = model_of(case.heads[sub], t, case.ring[sub], qc, events)
    if models is not None and sub in models:
        mq = models[sub]
        for e in mq.q:
            e[1] = deque((m[0], m[1], None) for m in e[1])
    return mq, bad


def put_reference(case, events=None, models=None):
    """One put call over the model: the outputs, and per OK session the model after it."""
    c, qc = case.ring.shape[1:]
    total = int(case.offsets[-1])
    out = dict(verdicts=[0] * total, classes=[NO_CLASS] * total, evicted=[[NO_REF, 0]] * total, counts=[], models={},
               left_out=[])  # (for a test's ledger: the candidates a full ring had no place for)
    flags = 0
    sums = [0, 0, 0, 0, 0]
    for k, sub in enumerate(int(s) for s in case.subs):
        lo, hi = int(case.offsets[k]), int(case.offsets[k + 1])
        status, f = session_status(case.sessions, case.heads, case.tables, sub, c, qc)
        flags |= f
        if status != A_OK:
            out["counts"].append([0, 0, 0, 0, 0, 0, 0, status])
            continue
        ti = int(case.heads["table"][sub])
        t = case.tables[ti]
        prios = table_prios(t)
        mq, bad = _model(case, sub, t, qc, events, models)
        flags |= F_BAD_HEAD if bad else 0
        flags |= F_LIMITED if int(case.sessions["mq_max"][sub]) else 0
        dropped0, evicted, qdropped, unstored = int(case.sessions["dropped"][sub]), 0, 0, 0
        alive = set()
        at = list(read_head(case.heads[sub], t, qc)[0])  # counting only: the ring position of every class's oldest entry
        above = set()
        for d in range(lo, hi):
            v = int(case.verdicts[d])
            if (v & W_MASK) == W_QUEUED_DROPPED or v & W_EVICTS:
                flags |= F_BAD_VERDICT
            if (v & W_MASK) != W_QUEUED or v & W_EVICTS:
                continue
            src = int(case.src[d])
            if src >= case.msg_class.shape[0]:
                flags |= F_BAD_SRC
                cl = int(t["default_class"])
            else:
                cl = int(case.msg_class[src, ti])
                cl = cl if cl < len(prios) else int(t["default_class"])
            out["classes"][d] = cl
            out["verdicts"][d] = W_QUEUED
            if mq.plen(prios[cl]) > mq.max_len and cl not in above and events is not None:
                above.add(cl)
                events["len_above_max_puts"] += 1
            if mq.plen(prios[cl]) >= qc and mq.plen(prios[cl]) != mq.max_len:  # a full ring beyond max_len: the stage's own limit
                unstored += 1
                flags |= F_ROW_FULL
                out["left_out"].append(d)
                continue
            ref = int(case.refs[d]) if case.refs is not None else d
            gone = mq_in((ref, int(case.opts[d]), d), prios[cl], mq)
            alive.add(d)
            if gone is not None:
                out["verdicts"][d] |= W_EVICTS
                if gone[2] is None:
                    out["evicted"][d] = [gone[0], gone[1]]
                    evicted += 1
                    at[cl] += 1
                    if at[cl] > qc and events is not None:  # an old entry behind the ring end, after ones in front of it
                        events["evictions_across_ring_end"] += 1
                else:
                    out["verdicts"][gone[2]] = W_QUEUED_DROPPED | (out["verdicts"][gone[2]] & W_EVICTS)
                    alive.discard(gone[2])
                    qdropped += 1
        if unstored and events is not None:
            events["row_full_inboxes"] += 1
        after = dropped0 + evicted + qdropped
        out["counts"].append([len(alive), evicted, qdropped, unstored, mq.len, after & 0xFFFFFFFF, after >> 32, A_OK])
        out["models"][sub] = (mq, t, after)
        for i, x in enumerate((len(alive), evicted, qdropped, unstored, 1)):
            sums[i] += x
    out["summary"] = [flags, total, len(case.subs)] + sums
    return out


def take_reference(case, cap_out=None, events=None, models=None):
    """One take call over the model."""
    c, qc = case.ring.shape[1:]
    subs = range(case.sessions.size) if case.subs is None else [int(s) for s in case.subs]
    out = dict(offsets=[0], opts=[], verdicts=[], pkt_ids=[], refs=[], classes=[], status=[], counts=[], models={})
    flags = 0
    sums = [0, 0, 0, 0, 0]  # OK, sends, sends0, expired, unfit
    for sub in subs:
        status, f = session_status(case.sessions, case.heads, case.tables, sub, c, qc)
        flags |= f
        out["status"].append(status)
        if status != A_OK:
            sums[4] += status == UNFIT
            out["counts"].append([0, 0, 0, 0])
            out["offsets"].append(len(out["refs"]))
            continue
        sums[0] += 1
        t = case.tables[int(case.heads["table"][sub])]
        prios = table_prios(t)
        mq, bad = _model(case, sub, t, qc, events, models)
        flags |= F_BAD_HEAD if bad else 0
        flags |= F_LIMITED if int(case.sessions["mq_max"][sub]) else 0
        rec = case.sessions[sub]

        def is_expired(msg):
            nonlocal flags
            if case.deadlines is None:
                return False
            if msg[0] >= len(case.deadlines):
                flags |= F_BAD_REF
                return False
            return case.now > int(case.deadlines[msg[0]])

        budget = batch_n(int(rec["inflight_max"]), int(rec["inflight"]))
        items = dequeue(budget, mq, is_expired)
        pkt = int(rec["next_pkt_id"])
        cnt = [0, 0, 0, mq.len]
        at = list(read_head(case.heads[sub], t, qc)[0])  # counting only
        for msg, p, expired in items:
            pos, at[prios.index(p)] = at[prios.index(p)] % qc, at[prios.index(p)] + 1
            if events is not None and pos >= 16:
                events["expired_at_16_up"] += expired
                events["qos0_at_16_up"] += not expired and msg[1] & 3 == 0
            out["refs"].append(msg[0])
            out["opts"].append(msg[1])
            out["classes"].append(prios.index(p))
            if expired:
                out["verdicts"].append(EXPIRED)
                out["pkt_ids"].append(0)
                cnt[2] += 1
            elif msg[1] & 3 == 0:
                out["verdicts"].append(W_SEND_QOS0)
                out["pkt_ids"].append(0)
                cnt[1] += 1
            else:
                out["verdicts"].append(W_SEND)
                out["pkt_ids"].append(pkt)
                pkt = 1 if pkt == 65535 else pkt + 1
                cnt[0] += 1
        if events is not None and budget and cnt[0] == budget and mq.last_prio is not None and mq.p_credit == 0:
            events["credit_zero_on_last_send"] += 1
        out["counts"].append(cnt)
        out["offsets"].append(len(out["refs"]))
        out["models"][sub] = (mq, t, dict(next_pkt_id=pkt, inflight=min(int(rec["inflight"]) + cnt[0], 0xFFFFFFFF)))
        for i in range(3):
            sums[1 + i] += cnt[i]
    items = len(out["refs"])
    if cap_out is not None and items > cap_out:
        flags |= F_OUTPUT_FULL
        out["full"] = True
    out["summary"] = [flags, sums[0], len(out["status"]), items, sums[1], sums[2], sums[3], sums[4]]
    return out


def check_tables(models, sessions, ring, heads, updated, before, keys):
    """The tables after a call against the models: per class the queue oldest first, the order, the
    credit, last_prio, and the record's fields ``keys`` maps; a session the call did not own, and every
    table when ``updated`` is false, is byte for byte what it was (the ring positions outside the live
    queues included)."""
    b_sessions, b_ring, b_heads = before
    qc = ring.shape[2]
    owned = set(models) if updated else set()
    for sub in range(sessions.size):
        if sub not in owned:
            assert heads[sub].tobytes() == b_heads[sub].tobytes(), sub
            assert sessions[sub].tobytes() == b_sessions[sub].tobytes(), sub
            continue
        mq, t, extra = models[sub]
        want = logical(mq, t)
        for c in range(ring.shape[1]):
            h, n = int(heads["head"][sub][c]), int(heads["len"][sub][c])
            assert h < qc and n <= qc
            got = [(int(ring[sub, c, (h + i) % qc]["ref"]), int(ring[sub, c, (h + i) % qc]["opts"])) for i in range(n)]
            assert got == want["queues"][c], (sub, c, got, want["queues"][c])
        nibs = [(int(heads["order"][sub]) >> (4 * p)) & 0xF for p in range(8)]
        assert nibs == want["order"] + [0xF] * (8 - len(want["order"])), (sub, nibs, want["order"])
        assert int(heads["credit"][sub]) == want["credit"] and int(heads["flags"][sub]) == want["last"], sub
        assert int(heads["table"][sub]) == int(b_heads["table"][sub]) and heads["rsv"][sub].tobytes() == b_heads["rsv"][sub].tobytes()
        assert int(sessions["mq_len"][sub]) == want["len"], sub
        for key, value in keys(extra).items():
            assert int(sessions[key][sub]) == value, (sub, key)
    return True


def all_events():
    return dict.fromkeys(EVENTS, 0)


def as_rows(entries, qc, head=0, dtype=None):
    """A class ring holding ``entries`` [(ref, opts)] from position ``head``."""
    row = np.zeros(qc, dtype=dtype)
    for i, (ref, opts) in enumerate(entries):
        row[(head + i) % qc] = (ref, opts, (0, 0, 0))
    return row
