"""The inbound QoS 2 half of emqx_session restated one event at a time, written from
apps/emqx/src/emqx_session.erl: publish/3 with is_awaiting_full/1 (:342-369), pubrel/2 (:420-428)
and expire(awaiting_rel, _) with expire_awaiting_rel/2 and age/2 (:657-674, :792), plus what the
channel does with the answers (apps/emqx/src/emqx_channel.erl:618-640 arms await_timer after an OK
QoS 2 publish; :1123-1125 a disconnected channel ignores the timer).  A session's awaiting_rel is a
dict here, keyed by the slot of the stage's row so that the restatement also says where an entry
lands: a publish takes the lowest empty slot, a pubrel frees the lowest slot that holds the id.
Plain Python on lists and dicts; independent of emqx_amd/csrc/rel.h."""

PUBLISH, PUBREL, DIRECT = 1, 2, 3
OK, IN_USE, NOT_FOUND, EXCEEDED, NO_SESSION, PASS, ROW_SMALL, BAD_KIND, IDLE = 1, 2, 3, 4, 5, 6, 7, 8, 9
F_INPUT_REFUSED, F_BAD_SUB, F_ROW_SMALL, F_BAD_TS = 2, 4, 8, 0x10
PRESENT, CONNECTED, PASSF = 1, 2, 8
NO_TIMEOUT = 0xFFFFFFFF
TS_LIMIT = 1 << 45
RC = {IN_USE: 0x91, NOT_FOUND: 0x92, EXCEEDED: 0x93}  # apps/emqx/include/emqx_mqtt.hrl:143-145


def entry(ts, pkt_id):
    return (ts << 17) | (1 << 16) | pkt_id


def awaiting_of(row):
    """The awaiting_rel map of a row: slot -> (pkt_id, ts) of every non-zero word."""
    return {s: (e & 0xFFFF, e >> 17) for s, e in enumerate(row) if e}


def row_of(awaiting, w):
    return [entry(awaiting[s][1], awaiting[s][0]) if s in awaiting else 0 for s in range(w)]


def _slot_of(awaiting, pkt_id):
    held = [s for s, (i, _) in awaiting.items() if i == pkt_id]
    return min(held) if held else None


def is_awaiting_full(awaiting, limit):
    """is_awaiting_full/1; `limit` 0 is infinity."""
    return limit != 0 and len(awaiting) >= limit


def publish(awaiting, limit, pkt_id, ts, w):
    """publish/3, first clause.  Returns the verdict."""
    if is_awaiting_full(awaiting, limit):  # the full check comes first
        return EXCEEDED
    if _slot_of(awaiting, pkt_id) is not None:  # maps:is_key
        return IN_USE
    awaiting[min(s for s in range(w) if s not in awaiting)] = (pkt_id, ts)  # maps:put
    return OK


def pubrel(awaiting, pkt_id):
    """pubrel/2: maps:take."""
    s = _slot_of(awaiting, pkt_id)
    if s is None:
        return NOT_FOUND
    del awaiting[s]
    return OK


def classify(sub, sub_limit, flags, limit, w):
    if sub >= sub_limit or not flags[sub] & PRESENT:
        return NO_SESSION
    if flags[sub] & PASSF:
        return PASS
    if limit == 0 or limit > w:
        return ROW_SMALL
    return 0


def run(subs, offsets, events, flags, rows, w, max_awaiting=100, maxes=None, now_ms=0, ts=None, src=None):
    """One run call.  `flags`: the flags word of every session record; `rows`: lists of w words,
    rewritten in place.  Returns verdicts, route, counts, arm and the eight summary words."""
    sub_limit = len(flags)
    m, total = len(subs), int(offsets[len(subs)])
    verdicts, route, counts, arm = [0] * total, [], [], []
    fl = routed = released = in_use = not_found = exceeded = 0
    for k in range(m):
        sub, lo, hi = int(subs[k]), int(offsets[k]), int(offsets[k + 1])
        if sub >= sub_limit:
            fl |= F_BAD_SUB
        limit = (int(maxes[sub]) if maxes is not None else max_awaiting) if sub < sub_limit else 0
        dead = classify(sub, sub_limit, flags, limit, w)
        if dead:
            if dead == ROW_SMALL:
                fl |= F_ROW_SMALL
            verdicts[lo:hi] = [dead] * (hi - lo)
            counts.append([0, 0, 0, 0])
            arm.append(0)
            continue
        awaiting = awaiting_of(rows[sub])
        c = [0, 0, 0, 0]
        armed = 0
        for d in range(lo, hi):
            kind, pkt_id = int(events[d]) >> 16, int(events[d]) & 0xFFFF
            if kind == DIRECT:  # publish/3, second clause
                v = OK
            elif kind == PUBLISH:
                stamp = int(ts[d]) if ts is not None else now_ms
                bad = stamp >= TS_LIMIT
                v = publish(awaiting, limit, pkt_id, min(stamp, TS_LIMIT - 1), w)
                if v == OK:
                    armed = 1  # ensure_timer(await_timer, _)
                    if bad:
                        fl |= F_BAD_TS
            elif kind == PUBREL:
                v = pubrel(awaiting, pkt_id)
                c[1] += v == OK
            else:
                v = BAD_KIND
            verdicts[d] = v
            if v == OK and kind != PUBREL:  # emqx_broker:publish(Msg)
                route.append(int(src[d]) if src is not None else d)
                c[0] += 1
            if v != OK:
                c[2] += 1
            in_use += v == IN_USE
            not_found += v == NOT_FOUND
            exceeded += v == EXCEEDED
        c[3] = len(awaiting)
        rows[sub][:] = row_of(awaiting, w)
        counts.append(c)
        arm.append(armed)
        routed += c[0]
        released += c[1]
    return {"verdicts": verdicts, "route": route, "counts": counts, "arm": arm,
            "summary": [fl, total, m, routed, released, in_use, not_found, exceeded]}


def expire(subs, m, flags, rows, w, now_ms, timeout_ms=300000, timeouts=None, channel_rule=False):
    """One expire call: expire_awaiting_rel(Now, Session) for the sessions `subs` names (None: 0 ..
    m - 1).  Returns status, counts and the eight summary words; `rows` is rewritten in place."""
    sub_limit = len(flags)
    status, counts = [], []
    fl = oks = expired = remaining = armed = 0
    for k in range(m):
        sub = int(subs[k]) if subs is not None else k
        if sub >= sub_limit:
            fl |= F_BAD_SUB
        if sub >= sub_limit or not flags[sub] & PRESENT:
            st = NO_SESSION
        elif flags[sub] & PASSF:
            st = PASS
        elif channel_rule and not flags[sub] & CONNECTED:
            st = IDLE
        else:
            st = OK
        status.append(st)
        if st != OK:
            counts.append([0, 0, 0, 0])
            continue
        timeout = int(timeouts[sub]) if timeouts is not None else timeout_ms
        awaiting = awaiting_of(rows[sub])
        # NotExpired = fun(_PacketId, Ts) -> age(Now, Ts) < Timeout end; Timeout infinity compares above every integer
        kept = {s: (i, t) for s, (i, t) in awaiting.items() if timeout == NO_TIMEOUT or now_ms - t < timeout}
        gone = len(awaiting) - len(kept)
        rows[sub][:] = row_of(kept, w)
        counts.append([gone, len(kept), 1 if kept else 0, 0])  # {ok, Timeout, NSession}: the full timeout again
        oks += 1
        expired += gone
        remaining += len(kept)
        armed += 1 if kept else 0
    return {"status": status, "counts": counts, "summary": [fl, oks, m, expired, remaining, armed, 0, 0]}
