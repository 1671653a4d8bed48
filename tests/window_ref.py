"""A plain sequential restatement of what a session does with the list emqx_channel:handle_deliver/2
hands it (reference: apps/emqx/src/emqx_channel.erl:791-814, emqx_session.erl:483-536 and :739-743,
emqx_inflight.erl:84-87, emqx_mqueue.erl:159-179), one delivery after the other: a real list as
the queue, ``is_full`` asked before every send, ``in/2`` evicting the head, ``next_pkt_id`` stepped
by one.  Deliberately none of the closed forms of include/emqx_window.h: the two check each other.
"""

QOS_MASK, DROP_NO_LOCAL, BAD_MESSAGE = 0x03, 0x10, 0x40
PRESENT, CONNECTED, STORE_QOS0, PASS = 1, 2, 4, 8
W_SEND_QOS0, W_SEND, W_QUEUED, W_QUEUED_DROPPED, W_DROP_QOS0 = 1, 2, 3, 4, 5
W_SKIP_NO_LOCAL, W_BAD_MESSAGE, W_NO_SESSION, W_PASS = 6, 7, 8, 9
W_EVICTS = 0x80
F_INPUT_REFUSED, F_BAD_SUB = 2, 4
FIELDS = ("inflight", "inflight_max", "mq_len", "mq_max", "next_pkt_id", "flags", "dropped")
U32 = 0xFFFFFFFF


def is_full(inflight, inflight_max):
    """emqx_inflight:is_full/1."""
    return inflight_max != 0 and inflight >= inflight_max


def next_pkt_id(i):
    """emqx_session:next_pkt_id/1."""
    return 1 if i == 0xFFFF else i + 1


def session_fold(rec, opts):
    """One inbox.  ``rec``: dict of FIELDS or None (no record).  Returns the verdicts, the ids,
    the record after the batch, the four counts, the drops and whether ids were reused."""
    n = len(opts)
    verdicts, ids = [0] * n, [0] * n
    if rec is None or not rec["flags"] & PRESENT or rec["flags"] & PASS:
        dead = W_NO_SESSION if rec is None or not rec["flags"] & PRESENT else W_PASS
        for d, o in enumerate(opts):
            verdicts[d] = W_SKIP_NO_LOCAL if o & DROP_NO_LOCAL else W_BAD_MESSAGE if o & BAD_MESSAGE else dead
        return verdicts, ids, dict(rec or dict.fromkeys(FIELDS, 0)), [0, 0, 0, 0], 0, False
    s = dict(rec)
    # the queue itself: the entries from before the batch (only their number matters: they leave
    # first), then the delivery positions as they come
    old_left, queue = s["mq_len"], []
    qlen = s["mq_len"]
    sends = sends0 = evicted_old = drops = 0
    handed = set()
    reused = False
    for d, o in enumerate(opts):
        if o & DROP_NO_LOCAL:
            verdicts[d] = W_SKIP_NO_LOCAL
            continue
        if o & BAD_MESSAGE:
            verdicts[d] = W_BAD_MESSAGE
            continue
        q = o & QOS_MASK
        if s["flags"] & CONNECTED:
            if q == 0:
                verdicts[d] = W_SEND_QOS0
                sends0 += 1
                continue
            if not is_full(s["inflight"], s["inflight_max"]):
                verdicts[d], ids[d] = W_SEND, s["next_pkt_id"]
                reused |= s["next_pkt_id"] in handed
                handed.add(s["next_pkt_id"])
                s["inflight"] = min(s["inflight"] + 1, U32)
                s["next_pkt_id"] = next_pkt_id(s["next_pkt_id"])
                sends += 1
                continue
        elif q == 0 and not s["flags"] & STORE_QOS0:
            verdicts[d] = W_DROP_QOS0  # emqx_mqueue:in/2, first clause: `dropped` is not counted
            drops += 1
            continue
        # emqx_mqueue:in/2
        if s["mq_max"] != 0 and qlen == s["mq_max"]:
            if old_left:
                old_left -= 1
                evicted_old += 1
            else:
                out = queue.pop(0)
                verdicts[out] = W_QUEUED_DROPPED | (verdicts[out] & W_EVICTS)
            queue.append(d)
            s["dropped"] += 1
            drops += 1
            verdicts[d] = W_QUEUED | W_EVICTS
        else:
            queue.append(d)
            qlen += 1
            verdicts[d] = W_QUEUED
    s["mq_len"] = min(qlen, U32)
    queued = sum(1 for v in verdicts if v & 0x0F == W_QUEUED)
    return verdicts, ids, s, [sends, sends0, queued, evicted_old], drops, reused


def run(inbox_subs, inbox_offsets, box_opts, sessions, cap_in=None, cap_boxes=None, update_table=False):
    """The stage over a batch.  ``sessions``: a list of FIELDS dicts indexed by subscriber id,
    replaced in place with ``update_table``.  Returns a dict of verdicts, pkt_ids, out_sessions,
    counts and the summary words."""
    m = len(inbox_subs)
    total = int(inbox_offsets[m]) if m < len(inbox_offsets) else 0
    cap_in = len(box_opts) if cap_in is None else cap_in
    cap_boxes = m if cap_boxes is None else cap_boxes
    if m > cap_boxes or total > cap_in or total > U32:
        return {"verdicts": [], "pkt_ids": [], "out_sessions": [], "counts": [],
                "summary": [F_INPUT_REFUSED, total if m <= cap_boxes else 0, m, 0, 0, 0, 0, 0]}
    verdicts, ids, recs, counts = [], [], [], []
    summary = [0, total, m, 0, 0, 0, 0, 0]
    for k in range(m):
        lo, hi = int(inbox_offsets[k]), int(inbox_offsets[k + 1])
        sub = int(inbox_subs[k])
        rec = sessions[sub] if sub < len(sessions) else None
        if rec is None:
            summary[0] |= F_BAD_SUB
        v, i, after, c, drops, reused = session_fold(rec, [int(o) for o in box_opts[lo:hi]])
        verdicts += v
        ids += i
        recs.append(after)
        counts.append(c)
        summary[3] += c[0]
        summary[4] += c[1]
        summary[5] += c[2]
        summary[6] += drops
        summary[7] += 1 if reused else 0
    if update_table:
        for k in range(m):
            sub = int(inbox_subs[k])
            if sub < len(sessions) and recs[k]["flags"] & PRESENT and not recs[k]["flags"] & PASS:
                sessions[sub] = dict(recs[k])
    return {"verdicts": verdicts, "pkt_ids": ids, "out_sessions": recs, "counts": counts, "summary": summary}
