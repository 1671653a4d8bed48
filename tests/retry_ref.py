"""A sequential restatement of the retry stage's contract (include/emqx_retry.h), written from the
reference's emqx_session:retry/1, retry_delivery/4,5, replay/1, with_ts/1 and
emqx_message:is_expired/1 the way they are written there: a session's inflight window is a dict
keyed by packet id, retry sorts its list by timestamp with a stable sort and walks it until the first
young entry, expiry is ``max(0, now - created) > interval_s * 1000``.  It shares nothing with
emqx_amd/csrc/retry.h: no per-slot predicate, no rank, no deadline word.  The two check each other.

Rows are lists of ``[pkt_id, phase, qos, ref]`` (tests/ack_cases.rows_of), stamps lists of ints,
records dicts of the window stage's fields.  A malformed row may hold one id twice; the dict is
therefore keyed by (pkt_id, slot), whose sorted order is gb_trees:to_list/1's."""

EMPTY, MSG, PUBREL_AWAIT = 0, 1, 2
A_OK, A_NO_SESSION, A_PASS = 1, 4, 5
PRESENT, PASS = 1, 8
MODE_RETRY, MODE_REPLAY = 0, 1
PUBLISH_DUP, PUBREL, EXPIRED = 1, 2, 3
NO_TIMER = 0xFFFFFFFF
F_INPUT_REFUSED, F_BAD_SUB, F_OUTPUT_FULL, F_BAD_REF, F_UNSTAMPED = 2, 4, 8, 0x10, 0x20
MAX_INTERVAL = 1 << 31


def make_stamp(ts, dup, phase, pkt_id):
    return (ts << 19) | (dup << 18) | ((phase & 3) << 16) | pkt_id


def read_stamp(s):
    return s >> 19, (s >> 18) & 1, (s >> 16) & 3, s & 0xFFFF


def owns(stamp, slot):
    """Whether the stamp is this slot's."""
    _, _, phase, pkt_id = read_stamp(stamp)
    return slot[1] != EMPTY and slot[1] == phase and slot[0] == pkt_id


def stamp(subs, rows, stamps, now, sub_limit=None):
    """The stamp call over ``rows`` and ``stamps`` (updated in place); its summary."""
    sub_limit = len(rows) if sub_limit is None else sub_limit
    subs = list(range(len(rows))) if subs is None else [int(s) for s in subs]
    flags = named = stamped = cleared = 0
    for sub in subs:
        if sub >= sub_limit:
            flags |= F_BAD_SUB
            continue
        named += 1
        for j, slot in enumerate(rows[sub]):
            old = stamps[sub][j]
            if slot[1] == EMPTY:
                new = 0
            elif owns(old, slot):
                new = old
            else:
                new = make_stamp(now, 0, slot[1], slot[0])
            if new != old:
                stamps[sub][j] = new
                stamped += new != 0
                cleared += new == 0
    return [flags, named, len(subs), stamped, cleared, 0, 0, 0]


def is_expired(now, created, interval_s):
    """emqx_message:is_expired/1 over elapsed/1; interval_s None: no Message-Expiry-Interval."""
    if interval_s is None:
        return False
    return max(0, now - created) > interval_s * 1000


def inflight_of(row, stamps, now):
    """The row as the session's window: {(pkt_id, slot): [phase, qos, ref, ts, dup, stamped]}."""
    window = {}
    for j, slot in enumerate(row):
        if slot[1] == EMPTY:
            continue
        stamped = stamps is not None and owns(stamps[j], slot)
        ts, dup = (read_stamp(stamps[j])[:2] if stamped else (now, 0))
        window[(slot[0], j)] = [slot[1], slot[2], slot[3], ts, dup, stamped]
    return window


def session_retry(window, now, interval, expiry):
    """retry/1 of one window (updated in place): the items, the timer, flags, unstamped entries.
    ``expiry``: None, or a list of (created, interval_s) by ref."""
    flags = 0
    unstamped = sum(1 for e in window.values() if not e[5])
    if unstamped:
        flags |= F_UNSTAMPED
    for e in window.values():  # an entry without a stamp is taken as entered now
        e[5] = True
    if not window:
        return [], NO_TIMER, flags, 0
    by_id = sorted(window.items())                       # emqx_inflight:to_list/1
    by_ts = sorted(by_id, key=lambda kv: kv[1][3])       # lists:sort(sort_fun(), ...), stable
    items, timer = [], interval
    for key, e in by_ts:
        age = now - e[3]
        if age < interval:
            timer = interval - max(0, age)
            break
        pkt_id = key[0]
        if e[0] == PUBREL_AWAIT:
            e[3], e[4] = now, 0  # {pubrel_await, Now}: the entry holds no message, so no dup flag
            items.append([pkt_id, PUBREL, e[1], e[2]])
            continue
        expired = False
        if expiry is not None:
            if e[2] >= len(expiry):
                flags |= F_BAD_REF
            else:
                expired = is_expired(now, *expiry[e[2]])
        if expired:
            del window[key]
            items.append([pkt_id, EXPIRED, e[1], e[2]])
        else:
            e[3], e[4] = now, 1
            items.append([pkt_id, PUBLISH_DUP, e[1], e[2]])
    return items, timer, flags, unstamped


def session_replay(window):
    return [[key[0], PUBREL if e[0] == PUBREL_AWAIT else PUBLISH_DUP, e[1], e[2]] for key, e in sorted(window.items())]


def write_back(window, row, stamps):
    """The window into the row and its stamps: a deleted entry leaves zeros."""
    for j, slot in enumerate(row):
        if slot[1] == EMPTY:
            continue
        e = window.get((slot[0], j))
        if e is None:
            row[j] = [0, 0, 0, 0]
            stamps[j] = 0
        else:
            stamps[j] = make_stamp(e[3], e[4], e[0], slot[0])


def sweep(subs, recs, rows, stamps, now, interval=0, intervals=None, expiry=None, mode=MODE_RETRY, cap_out=None,
          update_table=False, sub_limit=None, cap_boxes=None):
    """The sweep call; ``recs``, ``rows`` and ``stamps`` are updated in place unless it is full."""
    sub_limit = len(rows) if sub_limit is None else sub_limit
    m = sub_limit if subs is None else len(subs)
    if (cap_boxes is not None and m > cap_boxes) or (subs is None and m > sub_limit):
        return {"summary": [F_INPUT_REFUSED, 0, m, 0, 0, 0, 0, 0]}
    subs = list(range(m)) if subs is None else [int(s) for s in subs]
    flags = ok = unstamped = 0
    lists, status, counts, timers, after = [], [], [], [], []
    for sub in subs:
        if sub >= sub_limit:
            flags |= F_BAD_SUB
        if sub >= sub_limit or not recs[sub]["flags"] & PRESENT:
            st = A_NO_SESSION
        else:
            st = A_PASS if recs[sub]["flags"] & PASS else A_OK
        status.append(st)
        if st != A_OK:
            lists.append([])
            counts.append([0, 0, 0, 0])
            timers.append(NO_TIMER)
            after.append(None)
            continue
        ok += 1
        window = inflight_of(rows[sub], None if mode == MODE_REPLAY else stamps[sub], now)
        if mode == MODE_REPLAY:
            items, timer = session_replay(window), NO_TIMER
        else:
            iv = min(int(intervals[sub]) if intervals is not None else interval, MAX_INTERVAL)
            items, timer, f, u = session_retry(window, now, iv, expiry)
            flags |= f
            unstamped += u
        kinds = [it[1] for it in items]
        n_exp = kinds.count(EXPIRED)
        lists.append(items)
        counts.append([kinds.count(PUBLISH_DUP), kinds.count(PUBREL), n_exp, max(0, recs[sub]["inflight"] - n_exp)])
        timers.append(timer)
        after.append(window)
    offsets = [0]
    for items in lists:
        offsets.append(offsets[-1] + len(items))
    total = offsets[-1]
    full = cap_out is not None and total > cap_out
    if full:
        flags |= F_OUTPUT_FULL
    elif mode == MODE_RETRY:
        for sub, window, c in zip(subs, after, counts):
            if window is None:
                continue
            write_back(window, rows[sub], stamps[sub])
            if update_table:
                recs[sub]["inflight"] = c[3]
    col = lambda j: sum(c[j] for c in counts)  # noqa: E731
    return {"offsets": offsets, "items": [] if full else [it for items in lists for it in items], "status": status,
            "counts": counts, "timers": timers, "summary": [flags, ok, m, total, col(0), col(1), col(2), unstamped]}
