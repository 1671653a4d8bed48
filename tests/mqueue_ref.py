"""A sequential restatement of the mqueue stage's contract (include/emqx_mqueue.h), written from the
reference's emqx_mqueue:in/2 and out/1 (without a priority table), emqx_session:dequeue/1,
dequeue/3, acc_cnt/2, deliver/3, deliver_msg/2, enqueue/2, batch_n/1, next_pkt_id/1 and
emqx_message:is_expired/1 the way they are written there: a session's queue is a ``deque``, ``in``
drops the oldest when the queue is at max_len, ``dequeue`` pops one message a step and counts down,
``deliver_msg`` asks ``is_full`` before every send.  It shares nothing with
emqx_amd/csrc/mqueue.h: no prefix count, no closed form, no plan.  The two check each other.

Messages are ``(ref, opts)`` pairs, records dicts of the window stage's fields, a ring table a list
of rows of ``[ref, opts]`` with a list of ``[head, len]`` headers next to it."""
from collections import deque

QOS_MASK = 0x03
PRESENT, PASS = 1, 8
A_OK, A_NO_SESSION, A_PASS = 1, 4, 5
W_SEND_QOS0, W_SEND, W_QUEUED, W_QUEUED_DROPPED, W_EVICTS, W_MASK = 1, 2, 3, 4, 0x80, 0x0F
MQ_EXPIRED = 10
NO_REF = 0xFFFFFFFF
NO_EXPIRY = 0xFFFFFFFFFFFFFFFF
DEFAULT_BATCH_N = 1000
F_INPUT_REFUSED, F_BAD_SUB, F_OUTPUT_FULL, F_BAD_REF, F_BAD_RING, F_ROW_FULL, F_LEN_MISMATCH = 2, 4, 8, 0x10, 0x20, 0x40, 0x80
U32 = 0xFFFFFFFF


# ---- emqx_mqueue ------------------------------------------------------------------------------

class MQ:
    """#mqueue{} without p_table: q, len (of the deque), max_len (0: infinity), store_qos0, dropped."""

    def __init__(self, max_len=1000, store_qos0=True, items=()):
        self.q = deque(items)
        self.max_len = max_len
        self.store_qos0 = store_qos0
        self.dropped = 0

    def __len__(self):
        return len(self.q)


def mq_in(msg, mq):
    """emqx_mqueue:in/2: the dropped message or None."""
    if msg[1] & QOS_MASK == 0 and not mq.store_qos0:
        return msg
    if mq.max_len != 0 and len(mq.q) == mq.max_len:
        dropped = mq.q.popleft()  # reached max length, drop the oldest message
        mq.q.append(msg)
        mq.dropped += 1
        return dropped
    mq.q.append(msg)
    return None


def mq_out(mq):
    """emqx_mqueue:out/1: None for `empty`."""
    if not mq.q:
        return None
    return mq.q.popleft()


# ---- emqx_session -----------------------------------------------------------------------------

def batch_n(inflight_max, inflight):
    """batch_n/1 (never below 0 here: the reference's dequeue/3 would not end)."""
    return DEFAULT_BATCH_N if inflight_max == 0 else max(inflight_max - inflight, 0)


def is_full(inflight, inflight_max):
    return inflight_max != 0 and inflight >= inflight_max


def next_pkt_id(i):
    return 1 if i == 0xFFFF else i + 1


def dequeue3(cnt, msgs, mq, expired_fn, on_expired):
    """dequeue/3: pops until Cnt is 0 or the queue is empty; an expired message costs nothing."""
    while True:
        if cnt == 0:
            return msgs
        msg = mq_out(mq)
        if msg is None:
            cnt = 0
            continue
        if expired_fn(msg):
            on_expired(msg)  # inc_expired_cnt(delivery)
            continue
        cnt = cnt if msg[1] & QOS_MASK == 0 else cnt - 1  # acc_cnt/2
        msgs.append(msg)


def deliver_msg(msg, sess, mq):
    """deliver_msg/2: the publish {PacketId | None, Msg} or None when the message was queued."""
    if msg[1] & QOS_MASK == 0:
        return (None, msg)
    if is_full(sess["inflight"], sess["inflight_max"]):
        mq_in(msg, mq)  # enqueue/2
        return None
    publish = (sess["next_pkt_id"], msg)
    sess["inflight"] = min(sess["inflight"] + 1, U32)  # await/3
    sess["next_pkt_id"] = next_pkt_id(sess["next_pkt_id"])
    return publish


def session_dequeue(sess, mq, expired_fn):
    """dequeue/1 of one session (``sess`` and ``mq`` change in place).  Returns what left the queue,
    in that order: (MQ_EXPIRED, 0, msg) for a message dequeue/3 dropped as expired, else deliver/3's
    publish as (W_SEND_QOS0, 0, msg) or (W_SEND, PacketId, msg)."""
    if not mq.q:  # emqx_mqueue:is_empty/1
        return []
    before = list(mq.q)
    gone = []
    msgs = dequeue3(batch_n(sess["inflight_max"], sess["inflight"]), [], mq, expired_fn, gone.append)
    pubs = []
    for msg in msgs:  # deliver/3
        p = deliver_msg(msg, sess, mq)
        assert p is not None, "deliver/3 re-queued a dequeued message"
        pubs.append(p)
    out, pi, gi = [], 0, 0
    for msg in before[:len(gone) + len(pubs)]:  # the two lists merged by their place in the queue
        if gi < len(gone) and gone[gi] is msg:
            gi += 1
            out.append((MQ_EXPIRED, 0, msg))
        else:
            pid, pmsg = pubs[pi]
            assert pmsg is msg
            pi += 1
            out.append((W_SEND_QOS0, 0, msg) if pid is None else (W_SEND, pid, msg))
    return out


# ---- the stage --------------------------------------------------------------------------------

def read_queue(row, head, q):
    """The deque of a row; whether its header was malformed."""
    h, n = int(head[0]), int(head[1])
    bad = h >= q or n > q
    h, n = h % q, min(n, q)
    return deque((int(row[(h + i) % q][0]), int(row[(h + i) % q][1])) for i in range(n)), h, bad


def put(inbox_subs, inbox_offsets, box_opts, verdicts, refs, ring, heads, q, sessions=None, sub_limit=None):
    """The put call: in/2 folded over the deliveries the window queued, one at a time; whether the
    queue was full is what the window's verdict says (EMQX_W_EVICTS).  ``ring`` and ``heads`` change
    in place.  Returns evicted (per position, [ref, opts]), unstored and the summary words."""
    sub_limit = len(ring) if sub_limit is None else sub_limit
    m = len(inbox_subs)
    total = int(inbox_offsets[m])
    evicted = [[NO_REF, 0] for _ in range(total)]
    unstored = []
    summary = [0, total, m, 0, 0, 0, 0, 0]
    for k in range(m):
        sub = int(inbox_subs[k])
        lo, hi = int(inbox_offsets[k]), int(inbox_offsets[k + 1])
        queued = [d for d in range(lo, hi) if int(verdicts[d]) & W_MASK in (W_QUEUED, W_QUEUED_DROPPED)]
        if sub >= sub_limit:
            n = sum(1 for d in queued if int(verdicts[d]) & W_MASK == W_QUEUED)
            unstored.append(n)
            summary[5] += n
            summary[0] |= F_BAD_SUB
            continue
        old, h, bad = read_queue(ring[sub], heads[sub], q)
        if bad:
            summary[0] |= F_BAD_RING
        # the queue holds ("old", entry) and ("new", position); in/2 pops the oldest when full
        dq = deque(("old", e) for e in old)
        gone_old = 0
        for d in queued:
            if int(verdicts[d]) & W_EVICTS:
                if dq:
                    kind, what = dq.popleft()
                    if kind == "old":
                        evicted[d] = [what[0], what[1]]
                        gone_old += 1
            dq.append(("new", d))
        survivors = [x for x in dq]
        keep = survivors[:q]
        over = len(survivors) - len(keep)
        new_head = (h + gone_old) % q
        for i, (kind, what) in enumerate(keep):
            if kind == "new":
                ring[sub][(new_head + i) % q] = [what if refs is None else int(refs[what]), int(box_opts[what])]
                summary[3] += 1
        heads[sub] = [new_head, len(keep)]
        unstored.append(over)
        summary[4] += gone_old
        summary[5] += over
        if over:
            summary[6] += 1
            summary[0] |= F_ROW_FULL
        if sessions is not None and sessions[sub]["mq_len"] != len(keep):
            summary[7] += 1
            summary[0] |= F_LEN_MISMATCH
    return {"evicted": evicted, "unstored": unstored, "summary": summary}


def is_expired(now, deadline):
    """emqx_message:is_expired/1 with deadline = CreatedAt + Interval * 1000 (NO_EXPIRY: no
    Message-Expiry-Interval): elapsed > interval."""
    return deadline != NO_EXPIRY and now > deadline


def take(subs, sessions, ring, heads, q, now=0, deadlines=None, cap_out=None, update_table=False, sub_limit=None):
    """The take call: dequeue/1 of every named session.  ``sessions``: a list of dicts; with
    ``update_table`` it and ``heads`` change in place."""
    sub_limit = len(ring) if sub_limit is None else sub_limit
    subs = list(range(sub_limit)) if subs is None else [int(s) for s in subs]
    m = len(subs)
    summary = [0, 0, m, 0, 0, 0, 0, 0]
    offsets, opts, verdicts, ids, refs, status, counts = [0], [], [], [], [], [], []
    updates = []
    for sub in subs:
        rec = sessions[sub] if sub < sub_limit else None
        if rec is None or not rec["flags"] & PRESENT or rec["flags"] & PASS:
            if rec is None:
                summary[0] |= F_BAD_SUB
            status.append(A_PASS if rec is not None and rec["flags"] & PRESENT else A_NO_SESSION)
            counts.append([0, 0, 0, 0])
            offsets.append(offsets[-1])
            continue
        status.append(A_OK)
        summary[1] += 1
        old, h, bad = read_queue(ring[sub], heads[sub], q)
        if bad:
            summary[0] |= F_BAD_RING
        if rec["mq_len"] != len(old):
            summary[7] += 1
            summary[0] |= F_LEN_MISMATCH
        mq = MQ(max_len=0, items=old)
        sess = dict(rec)
        bad_ref = []

        def expired_fn(msg):
            if deadlines is None:
                return False
            if msg[0] >= len(deadlines):
                bad_ref.append(msg)
                return False
            return is_expired(now, int(deadlines[msg[0]]))

        items = session_dequeue(sess, mq, expired_fn)
        n_out = len(items)
        c = [0, 0, 0, len(mq.q)]
        for v, pid, msg in items:
            c[0 if v == W_SEND else 1 if v == W_SEND_QOS0 else 2] += 1
            opts.append(msg[1])
            verdicts.append(v)
            ids.append(pid)
            refs.append(msg[0])
        if bad_ref:
            summary[0] |= F_BAD_REF
        counts.append(c)
        offsets.append(offsets[-1] + n_out)
        summary[4] += c[0]
        summary[5] += c[1]
        summary[6] += c[2]
        sess["mq_len"] = len(mq.q)
        updates.append((sub, sess, [(h + n_out) % q, len(mq.q)]))
    total = offsets[-1]
    summary[3] = total
    cap_out = total if cap_out is None else cap_out
    full = total > cap_out
    if full:
        summary[0] |= F_OUTPUT_FULL
        opts, verdicts, ids, refs = [], [], [], []
    elif update_table:
        for sub, sess, head in updates:
            sessions[sub] = sess
            heads[sub] = head
    return {"offsets": offsets, "opts": opts, "verdicts": verdicts, "pkt_ids": ids, "refs": refs, "status": status,
            "counts": counts, "summary": summary}
