"""A plain sequential restatement of what a session does with PUBACK, PUBREC and PUBCOMP
(reference: apps/emqx/src/emqx_session.erl:379-389 ``puback/2``, :404-414 ``pubrec/2``, :437-447
``pubcomp/2``, :783-787 ``batch_n/1``): the inflight window as a dict keyed by packet id, as
``emqx_inflight`` keeps a gb_tree, one ack after the other with ``lookup``, ``update`` and
``delete``.  Recording is "fill the lowest free slots".  Deliberately none of the closed forms of
include/emqx_ack.h or emqx_amd/csrc/ack.h: the two check each other.

A row is a list of ``[pkt_id, phase, qos, ref]``; a session record a dict with at least ``flags``,
``inflight`` and ``inflight_max``.
"""

EMPTY, MSG, PUBREL_AWAIT = 0, 1, 2
PUBACK, PUBREC, PUBCOMP = 1, 2, 3
A_OK, A_IN_USE, A_NOT_FOUND, A_NO_SESSION, A_PASS, A_BAD_KIND = 1, 2, 3, 4, 5, 6
PRESENT, PASS = 1, 8
W_SEND, W_VERDICT_MASK, QOS_MASK = 2, 0x0F, 0x03
F_INPUT_REFUSED, F_BAD_SUB, F_ROW_FULL = 2, 4, 8
NO_REF = 0xFFFFFFFF
DEFAULT_BATCH_N = 1000
MAX_ACKS = 1 << 31
U32 = 0xFFFFFFFF


def batch_n(inflight_max, inflight):
    """emqx_session:batch_n/1 (never below 0 here: the reference's dequeue/3 would not end)."""
    return DEFAULT_BATCH_N if inflight_max == 0 else max(inflight_max - inflight, 0)


def session_acks(row, rec, acks):
    """One session's list.  ``rec`` None: no record.  Rewrites ``row`` in place; returns the
    verdicts, the refs, the four counts and the inflight count after the list."""
    n = len(acks)
    if rec is None or not rec["flags"] & PRESENT:
        return [A_NO_SESSION] * n, [NO_REF] * n, [0, 0, 0, 0], None
    if rec["flags"] & PASS:
        return [A_PASS] * n, [NO_REF] * n, [0, 0, 0, 0], None
    inflight = {}  # packet id -> slot index; of an id held twice the lowest slot is the entry
    for w, s in enumerate(row):
        if s[1] != EMPTY and s[0] not in inflight:
            inflight[s[0]] = w
    verdicts, refs = [], []
    released = to_pubrel = errors = 0
    for a in acks:
        kind, pkt_id = a >> 16, a & 0xFFFF
        v, ref = A_BAD_KIND, NO_REF
        if kind in (PUBACK, PUBREC, PUBCOMP):
            w = inflight.get(pkt_id)  # emqx_inflight:lookup/2
            if w is None:
                v = A_NOT_FOUND
            else:
                is_msg, is_pubrel = row[w][1] == MSG, row[w][1] == PUBREL_AWAIT
                if kind == PUBACK and is_msg or kind == PUBCOMP and is_pubrel:
                    v, ref = A_OK, row[w][3]
                    del inflight[pkt_id]  # emqx_inflight:delete/2
                    row[w] = [0, EMPTY, 0, 0]
                    released += 1
                elif kind == PUBREC and is_msg:
                    v, ref = A_OK, row[w][3]
                    row[w][1] = PUBREL_AWAIT  # emqx_inflight:update/3
                    to_pubrel += 1
                else:
                    v = A_IN_USE
        errors += v != A_OK
        verdicts.append(v)
        refs.append(ref)
    after = max(rec["inflight"] - released, 0)
    return verdicts, refs, [released, to_pubrel, errors, batch_n(rec["inflight_max"], after)], after


def run(ack_subs, ack_offsets, acks, sessions, slots, cap_in=None, cap_boxes=None, update_table=False):
    """The run call over a batch.  ``sessions``: a list of dicts indexed by subscriber id;
    ``slots``: a list of rows; both changed in place (the sessions with ``update_table`` only).
    Returns a dict of verdicts, refs, counts and the summary words."""
    m = len(ack_subs)
    total = int(ack_offsets[m]) if m < len(ack_offsets) else 0
    cap_in = len(acks) if cap_in is None else cap_in
    cap_boxes = m if cap_boxes is None else cap_boxes
    if m > cap_boxes or total > cap_in or total >= MAX_ACKS:
        return {"verdicts": [], "refs": [], "counts": [],
                "summary": [F_INPUT_REFUSED, total if m <= cap_boxes else 0, m, 0, 0, 0, 0, 0]}
    verdicts, refs, counts = [], [], []
    summary = [0, total, m, 0, 0, 0, 0, 0]
    for k in range(m):
        lo, hi = int(ack_offsets[k]), int(ack_offsets[k + 1])
        sub = int(ack_subs[k])
        ok = sub < len(sessions)
        if not ok:
            summary[0] |= F_BAD_SUB
        v, r, c, after = session_acks(slots[sub] if ok else None, sessions[sub] if ok else None, [int(a) for a in acks[lo:hi]])
        verdicts += v
        refs += r
        counts.append(c)
        summary[3] += v.count(A_OK)
        summary[4] += c[0]
        summary[5] += v.count(A_IN_USE)
        summary[6] += v.count(A_NOT_FOUND)
        summary[7] += sum(1 for x in v if x in (A_NO_SESSION, A_PASS, A_BAD_KIND))
        if update_table and after is not None:
            sessions[sub]["inflight"] = after
    return {"verdicts": verdicts, "refs": refs, "counts": counts, "summary": summary}


def record(inbox_subs, inbox_offsets, box_opts, verdicts, pkt_ids, refs, slots, cap_in=None, cap_boxes=None):
    """The record call over a batch: every send of an inbox into the lowest slot that was free
    before the call.  ``slots`` changes in place.  Returns out_unrecorded and the summary words."""
    m = len(inbox_subs)
    total = int(inbox_offsets[m]) if m < len(inbox_offsets) else 0
    cap_in = len(verdicts) if cap_in is None else cap_in
    cap_boxes = m if cap_boxes is None else cap_boxes
    if m > cap_boxes or total > cap_in or total > U32:
        return {"unrecorded": [], "summary": [F_INPUT_REFUSED, total if m <= cap_boxes else 0, m, 0, 0, 0, 0, 0]}
    unrecorded = []
    summary = [0, total, m, 0, 0, 0, 0, 0]
    for k in range(m):
        sub = int(inbox_subs[k])
        ok = sub < len(slots)
        if not ok:
            summary[0] |= F_BAD_SUB
        free = [w for w, s in enumerate(slots[sub]) if s[1] == EMPTY] if ok else []
        missed = 0
        for d in range(int(inbox_offsets[k]), int(inbox_offsets[k + 1])):
            if int(verdicts[d]) & W_VERDICT_MASK != W_SEND:
                continue
            summary[3] += 1
            if not free:
                missed += 1
                continue
            slots[sub][free.pop(0)] = [int(pkt_ids[d]), MSG, int(box_opts[d]) & QOS_MASK, d if refs is None else int(refs[d])]
            summary[4] += 1
        unrecorded.append(missed)
        summary[5] += missed
        if ok and missed:
            summary[6] += 1
            summary[0] |= F_ROW_FULL
    return {"unrecorded": unrecorded, "summary": summary}
