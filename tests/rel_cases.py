"""Cases of the rel stage shared by the CPU and the GPU tests: every branch of the table of
include/emqx_rel.h at every W, rows empty, with one free slot and full, every kind of limit, per
session event counts around the lanes of a group, session counts around a wave's and a block's
groups, event totals around the route passes' tile (emqx_amd/csrc/rel.h: RL_TILE), one session of
20,000 events that hovers at its limit, a randomised batch with ids from an alphabet of 6; and for
the expire call the ages around the timeout, infinity, mixed timeouts and the channel's rule.  A
case computes its reference (tests/rel_ref.py) once."""

import numpy as np

from emqx_amd import rel as T
from emqx_amd import window as W
from tests import rel_ref as R

TILE = T.TILE
PUB, REL, DIR = R.PUBLISH, R.PUBREL, R.DIRECT
LIVE = W.PRESENT | W.CONNECTED
NOW = 1_600_000_000_000
WIDTHS = T.WIDTHS
BLOCK = T.BLOCK


def lanes_of(w):
    return T.default_lanes(w)


def row(w, entries=(), at=None):
    """A row of w words holding `entries` ((pkt_id, ts)) at the slot indices `at` (default: the first)."""
    r = [0] * w
    for i, (pkt_id, ts) in enumerate(entries):
        r[i if at is None else at[i]] = R.entry(ts, pkt_id)
    return r


def filled(w, n, first_id=100, ts=NOW - 5, skip=()):
    """A row whose first slots, except `skip`, hold n entries with ids first_id, first_id + 1, ..."""
    at = [s for s in range(w) if s not in skip][:n]
    return row(w, [(first_id + i, ts + i) for i in range(n)], at=at)


def sess(events, row_=None, limit=None, flags=LIVE, bad_sub=False):
    """One session of a case: its events ((kind, pkt_id) or (kind, pkt_id, ts)), its row at entry,
    its max_awaiting_rel (None: the call's scalar) and its record's flags."""
    return dict(events=list(events), row=row_, limit=limit, flags=flags, bad_sub=bad_sub)


class RunCase:
    """Sessions no list names lie between the named ones in the tables; their rows must not change.
    `scalar`: the call's max_awaiting; any session with a limit of its own makes the case pass maxes[]."""

    def __init__(self, sessions, w=16, scalar=None, now_ms=NOW, src=False, spare=2):
        self.w = w
        self.max_awaiting = w if scalar is None else scalar
        self.now_ms = now_ms
        flags, rows, lims, subs, lens, flat, stamps, bad = [], [], [], [], [], [], [], 0
        any_ts = any(len(e) > 2 for s in sessions for e in s["events"])
        any_lim = any(s["limit"] is not None for s in sessions)
        for i, s in enumerate(sessions):
            lens.append(len(s["events"]))
            for e in s["events"]:
                flat.append((e[0] << 16) | e[1])
                stamps.append(e[2] if len(e) > 2 else now_ms)
            if s["bad_sub"]:
                subs.append(None)
                continue
            for j in range((i + 1) % (spare + 1)):  # sessions no list names
                flags.append(LIVE)
                rows.append(row(w, [(200 + j, NOW - 9), (7, NOW - 8)], at=[1, w - 1]))
                lims.append(self.max_awaiting)
            subs.append(len(flags))
            flags.append(s["flags"])
            rows.append(list(s["row"]) if s["row"] is not None else [0] * w)
            lims.append(self.max_awaiting if s["limit"] is None else s["limit"])
        flags.append(LIVE)
        rows.append(row(w, [(9, NOW - 1)]))
        lims.append(self.max_awaiting)
        for k, s in enumerate(subs):
            if s is None:
                subs[k] = len(flags) + 3 * bad  # the first of them is sub_limit itself
                bad += 1
        self.subs = np.asarray(subs, dtype=np.uint32)
        self.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.events = np.asarray(flat, dtype=np.uint32)
        self.ts = np.asarray(stamps, dtype=np.uint64) if any_ts else None
        self.m, self.total, self.sub_limit = len(sessions), len(flat), len(flags)
        self.src = (np.arange(self.total, dtype=np.uint32)[::-1] * 3 + 11).astype(np.uint32) if src else None
        self.maxes = np.asarray(lims, dtype=np.uint32) if any_lim else None
        self.table = W.pack_sessions(len(flags), flags=flags, inflight=3, next_pkt_id=77, mq_len=4, dropped=1 << 33)
        self.rel = np.asarray(rows, dtype=np.uint64).reshape(len(rows), w)
        self._ref = None

    def reference(self):
        if self._ref is None:
            rows = [[int(x) for x in r] for r in self.rel]
            r = R.run(self.subs, self.offsets, self.events, [int(f) for f in self.table["flags"]], rows, self.w,
                      max_awaiting=self.max_awaiting, maxes=self.maxes, now_ms=self.now_ms, ts=self.ts, src=self.src)
            self._ref = {"verdicts": np.asarray(r["verdicts"], dtype=np.uint8), "route": np.asarray(r["route"], dtype=np.uint32),
                         "counts": np.asarray(r["counts"], dtype=np.uint32).reshape(-1, 4), "arm": np.asarray(r["arm"], dtype=np.uint8),
                         "summary": r["summary"], "rel": np.asarray(rows, dtype=np.uint64).reshape(self.rel.shape)}
        return self._ref

    def host_args(self):
        """The arguments of Rel.run / Rel.run_host behind sessions and rel."""
        return dict(max_awaiting=self.max_awaiting, maxes=self.maxes, now_ms=self.now_ms, ts=self.ts, src=self.src)


def check_run(ref, got, rel=None):
    """``got``: an emqx_amd.rel.Ran; ``rel``: the awaiting table after the call."""
    assert [got.summary[k] for k in T.RUN_SUMMARY] == ref["summary"], (got.summary, ref["summary"])
    bad = np.flatnonzero(got.verdicts != ref["verdicts"])
    assert bad.size == 0, ("verdicts", bad[:8], got.verdicts[bad[:8]], ref["verdicts"][bad[:8]])
    assert got.verdicts.dtype == np.uint8 and got.route.dtype == np.uint32
    assert got.route.tobytes() == ref["route"].tobytes(), (got.route[:16], ref["route"][:16])
    assert got.counts.tobytes() == ref["counts"].tobytes(), (got.counts, ref["counts"])
    assert got.arm.tobytes() == ref["arm"].tobytes(), (got.arm, ref["arm"])
    if rel is not None:
        bad = np.flatnonzero((rel != ref["rel"]).any(axis=1))
        assert bad.size == 0, ("rows", bad[:4], rel[bad[:2]], ref["rel"][bad[:2]])


def same(x, y):
    assert x.summary == y.summary
    for a, b in zip(x[:-1], y[:-1]):
        assert a.tobytes() == b.tobytes()


# ---- the run call ------------------------------------------------------------------------------

def table_case(w, src=False):
    """Every branch of the table at one W, limits of every kind mixed in one batch through maxes[]."""
    half = max(w // 2, 2)
    full = filled(w, w)
    return RunCase([
        # an empty row, limit == W: publish, rel, publish of one id; a rel of an unknown id; DIRECT; bad kinds
        sess([(PUB, 1), (REL, 1), (PUB, 1), (REL, 9), (DIR, 0), (0, 1), (4, 1), (0xFFFF, 0xFFFF)], limit=w),
        # one free slot (slot 3): the publish takes it, the next one is EXCEEDED, and so is one of an id the row holds
        sess([(PUB, 5), (PUB, 6), (PUB, 100)], filled(w, w - 1, skip=(3,)), limit=w),
        # a full row: EXCEEDED wins over IN_USE; the rel of another id; a publish that now fits takes the freed slot; DIRECT
        sess([(PUB, 100), (DIR, 100), (REL, 100 + w // 2), (PUB, 4000), (PUB, 4001), (DIR, 4001)], full, limit=w),
        # limit < W: an id present at entry published again (IN_USE) and released, then published (OK)
        sess([(PUB, 100), (REL, 100), (PUB, 100), (PUB, 300), (PUB, 301)], filled(w, half - 1, skip=(0, 2)), limit=half),
        # limit 0 (infinity) and limit above W: ROW_SMALL, the rows untouched
        sess([(PUB, 1), (REL, 100), (DIR, 2)], filled(w, 2), limit=0),
        sess([(PUB, 1)], filled(w, 1), limit=w + 1),
        # no PRESENT flag; PASS; a subscriber at sub_limit and one above it
        sess([(PUB, 1), (DIR, 1)], filled(w, 1), limit=w, flags=0),
        sess([(PUB, 1), (REL, 100)], filled(w, 1), limit=w, flags=LIVE | W.PASS),
        sess([(PUB, 1)], bad_sub=True),
        sess([], limit=w),
        sess([(REL, 2), (DIR, 3)], bad_sub=True),
        # a malformed row that holds id 7 twice: two rels find both, the third finds none
        sess([(REL, 7), (PUB, 8), (REL, 7), (REL, 7)], row(w, [(7, 5), (6, 5), (7, 6)], at=[1, 2, w - 1]), limit=w),
        # ids 0 and 65535; a stamp in the future and one at 2^45 (stored as 2^45 - 1: BAD_TS); a stamp of 0
        sess([(PUB, 0, NOW + 10**6), (PUB, 65535, 1 << 45), (PUB, 2, 0), (REL, 0), (PUB, 3, (1 << 63) + 5)], limit=4),
        # a disconnected session takes events all the same
        sess([(PUB, 1), (REL, 1)], limit=1, flags=W.PRESENT),
    ], w=w, src=src)


def no_ts_case(w, now_ms=NOW, src=False):
    """ts NULL: the call's now_ms is every stamp; scalar limit, no maxes[]."""
    return RunCase([sess([(PUB, 1), (PUB, 2), (REL, 1), (PUB, 3)]), sess([(PUB, 1)], filled(w, w)),
                    sess([(DIR, 5), (REL, 100)], filled(w, 1))], w=w, now_ms=now_ms, src=src)


def lens_of(w):
    """Per-session event counts 0, 1, L - 1, L, L + 1 and 2 L + 1 for the L of this W and for the
    most lanes a session of this W can have (W / 2 capped at 64)."""
    out = [0, 1]
    for L in sorted({lanes_of(w), min(w // 2, 64)}):
        out += [n for n in (L - 1, L, L + 1, 2 * L + 1, L) if n > 1]
    return out


def lens_case(w):
    """Sessions of lens_of(w) events; limit 3."""
    out = []
    for i, n in enumerate(lens_of(w)):
        ev = [((PUB, REL, PUB, DIR, PUB)[(d + i) % 5], 1 + (d * 7 + i) % 5) for d in range(n)]
        out.append(sess(ev, filled(w, i % 3, first_id=1), limit=3))
    return RunCase(out, w=w)


def sessions_case(w, n):
    """n sessions of 0 .. 3 events: counts around the groups of a wave and of a block."""
    out = []
    for i in range(n):
        ev = [((PUB, PUB, REL, DIR)[(d + i) % 4], 1 + (d + i) % 3) for d in range(i % 4)]
        out.append(sess(ev, filled(w, i % 2, first_id=1), limit=2))
    return RunCase(out, w=w, spare=1)


def session_counts(w):
    L = lanes_of(w)
    gw, gb = 64 // L, BLOCK // L
    return sorted({max(gw - 1, 1), gw, gw + 1, gb - 1, gb, gb + 1, 2 * gb + 1})


def tile_case(total, routed, w=8):
    """`total` events over five sessions, all routed (DIRECT) or none (PUBREL of ids nobody holds)."""
    cut = [0, total // 7, total // 7, total // 2, total - 1, total]
    ev = (DIR, 3) if routed else (REL, 3)
    return RunCase([sess([ev] * (cut[i + 1] - cut[i]), limit=2) for i in range(5)], w=w, src=routed)


def hover_case(n=20000, w=16, limit=4):
    """One session of n events that hovers at its limit: publish of a fresh id (EXCEEDED at the
    limit), rel of the oldest, publish again (OK), ... next to two short sessions."""
    ev, held, fresh = [], [100 + i for i in range(limit - 1)], 1000
    while len(ev) < n:
        ev.append((PUB, fresh))
        held.append(fresh)        # OK: the row is at its limit now
        ev.append((PUB, fresh + 1))  # EXCEEDED
        ev.append((PUB, held[1]))    # EXCEEDED although the id is present
        ev.append((REL, held.pop(0)))
        ev.append((DIR, 5))
        fresh = 1000 + (fresh - 999) % 60000
    return RunCase([sess([(PUB, 1)], limit=1), sess(ev[:n], filled(w, limit - 1), limit=limit), sess([(REL, 1), (DIR, 2)], limit=2)], w=w)


RUNS = {}
for _w in WIDTHS:
    RUNS["table_w%d" % _w] = (lambda w=_w: table_case(w))
    RUNS["lens_w%d" % _w] = (lambda w=_w: lens_case(w))
RUNS["table_w16_src"] = lambda: table_case(16, src=True)
RUNS["no_ts_w8"] = lambda: no_ts_case(8)
RUNS["no_ts_w128_src_now_past_limit"] = lambda: no_ts_case(128, now_ms=(1 << 45) + 3, src=True)
for _w in (8, 32, 128):
    for _n in session_counts(_w):
        RUNS["sessions_w%d_%d" % (_w, _n)] = (lambda w=_w, n=_n: sessions_case(w, n))
for _t in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
    RUNS["tile_%d_all_routed" % _t] = (lambda t=_t: tile_case(t, True))
    RUNS["tile_%d_none_routed" % _t] = (lambda t=_t: tile_case(t, False))
RUNS["empty_batch"] = lambda: RunCase([], w=8)


def fuzz(seed=1, n_sessions=300, w=8):
    """Ids from an alphabet of 6 and limits of 2 to 4: collisions and the full check are common."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_sessions):
        kind_of = rng.random()
        limit = int(rng.integers(2, 5))
        n = int(rng.integers(0, 14))
        kinds = rng.choice([PUB, REL, DIR, 0, 7], size=n, p=[0.5, 0.3, 0.1, 0.05, 0.05])
        ids = rng.integers(1, 7, size=n)
        ev = [(int(k), int(p), NOW + int(rng.integers(-50, 50))) for k, p in zip(kinds, ids)]
        held = rng.choice(np.arange(1, 7), size=int(rng.integers(0, limit + 1)), replace=False)
        at = sorted(rng.choice(w, size=held.size, replace=False).tolist())
        r = row(w, [(int(p), NOW - 100) for p in held], at=at)
        if kind_of < 0.06:
            out.append(sess(ev, r, limit=limit, flags=0))
        elif kind_of < 0.12:
            out.append(sess(ev, r, limit=limit, flags=LIVE | W.PASS))
        elif kind_of < 0.18:
            out.append(sess(ev, r, limit=(0, w + 1 + i)[i % 2]))
        elif kind_of < 0.21:
            out.append(sess(ev, bad_sub=True))
        else:
            out.append(sess(ev, r, limit=limit))
    return RunCase(out, w=w, src=bool(seed % 2))


# ---- the expire call ---------------------------------------------------------------------------

class ExpireCase:
    """Sessions given as (flags, row, timeout or None); `listed`: subs[] names them in reverse
    order with one id at sub_limit, else subs is NULL and the call sweeps the table."""

    def __init__(self, sessions, w=16, now_ms=NOW, timeout_ms=300000, listed=False, channel_rule=False, m=None):
        self.w, self.now_ms, self.timeout_ms, self.channel_rule = w, now_ms, timeout_ms, channel_rule
        flags = [s[0] for s in sessions]
        self.table = W.pack_sessions(len(sessions), flags=flags, inflight=2, dropped=5)
        self.rel = np.asarray([s[1] for s in sessions], dtype=np.uint64).reshape(len(sessions), w)
        self.sub_limit = len(sessions)
        any_to = any(s[2] is not None for s in sessions)
        self.timeouts = np.asarray([timeout_ms if s[2] is None else s[2] for s in sessions], dtype=np.uint32) if any_to else None
        if listed:
            self.subs = np.asarray(list(range(len(sessions)))[::-2] + [len(sessions)], dtype=np.uint32)
            self.m = self.subs.size
        else:
            self.subs = None
            self.m = len(sessions) if m is None else m
        self._ref = None

    def reference(self):
        if self._ref is None:
            rows = [[int(x) for x in r] for r in self.rel]
            r = R.expire(self.subs, self.m, [int(f) for f in self.table["flags"]], rows, self.w, self.now_ms, timeout_ms=self.timeout_ms,
                         timeouts=self.timeouts, channel_rule=self.channel_rule)
            self._ref = {"status": np.asarray(r["status"], dtype=np.uint8), "counts": np.asarray(r["counts"], dtype=np.uint32).reshape(-1, 4),
                         "summary": r["summary"], "rel": np.asarray(rows, dtype=np.uint64).reshape(self.rel.shape)}
        return self._ref

    def host_args(self):
        return dict(now_ms=self.now_ms, timeout_ms=self.timeout_ms, timeouts=self.timeouts, subs=self.subs, m=self.m,
                    channel_rule=self.channel_rule)


def check_expire(ref, got, rel=None):
    assert [got.summary[k] for k in T.EXPIRE_SUMMARY] == ref["summary"], (got.summary, ref["summary"])
    assert got.status.tobytes() == ref["status"].tobytes(), (got.status, ref["status"])
    assert got.counts.tobytes() == ref["counts"].tobytes(), (got.counts, ref["counts"])
    if rel is not None:
        bad = np.flatnonzero((rel != ref["rel"]).any(axis=1))
        assert bad.size == 0, ("rows", bad[:4], rel[bad[:2]], ref["rel"][bad[:2]])


def expire_case(w, listed=False, channel_rule=False, timeout_ms=1000, mixed=False, n_extra=0):
    """Nothing due, everything due, age == timeout (expired) next to age == timeout - 1 (kept), a
    stamp in the future, an empty row, a full row of which every other entry is due; NO_SESSION,
    PASS and disconnected sessions; `mixed`: timeouts[] with infinity, 0 and 1 among them."""
    t = timeout_ms
    young, old = NOW - 5, NOW - 10 * t - 7
    every_other = row(w, [(i + 1, old if i % 2 else young) for i in range(w)])
    sessions = [
        (LIVE, row(w, [(1, young), (2, NOW - t + 1)], at=[0, w - 1]), None),                       # nothing due (age t - 1)
        (LIVE, row(w, [(1, old), (2, NOW - t), (3, 0)], at=[1, 2, w - 2]), None),                    # everything due (age == t)
        (LIVE, row(w, [(1, NOW - t), (2, NOW - t + 1), (3, NOW + 10**7)], at=[0, 1, 5]), None),      # the border, and the future
        (LIVE, [0] * w, None),
        (LIVE, every_other, None),
        (0, row(w, [(1, old)]), None),                                                               # NO_SESSION
        (LIVE | W.PASS, row(w, [(1, old)]), None),
        (W.PRESENT, row(w, [(1, old), (2, young)]), None),                                           # disconnected
        (LIVE, row(w, [(1, old), (2, young)], at=[w - 1, w - 2]), T.NO_TIMEOUT if mixed else None),
        (LIVE, row(w, [(1, NOW), (2, NOW + 1)]), 0 if mixed else None),                              # timeout 0: age 0 is due
        (LIVE, row(w, [(1, NOW), (2, NOW - 1)]), 1 if mixed else None),
    ]
    for i in range(n_extra):
        sessions.append((LIVE, row(w, [(i % 9 + 1, old if i % 3 else young), (50, young)], at=[i % w, (i + 3) % w]), None))
    return ExpireCase(sessions, w=w, timeout_ms=timeout_ms, listed=listed, channel_rule=channel_rule)


EXPIRES = {}
for _w in WIDTHS:
    EXPIRES["w%d" % _w] = (lambda w=_w: expire_case(w))
    EXPIRES["w%d_listed_mixed_channel_rule" % _w] = (lambda w=_w: expire_case(w, listed=True, channel_rule=True, mixed=True))
EXPIRES["w16_infinity"] = lambda: expire_case(16, timeout_ms=T.NO_TIMEOUT)
EXPIRES["w16_channel_rule"] = lambda: expire_case(16, channel_rule=True)
EXPIRES["w16_mixed"] = lambda: expire_case(16, mixed=True)
_g = BLOCK // (8 // 2)  # the sessions a block takes at W = 8 (at W = 128 it takes 4: every case above crosses that)
for _n in (_g - 1, _g, _g + 1, 2 * _g + 1):
    EXPIRES["w8_%d_sessions" % _n] = (lambda n=_n: expire_case(8, n_extra=n - 11))
EXPIRES["prefix_of_the_table"] = lambda: ExpireCase([(LIVE, row(8, [(1, 0)]), None)] * 5, w=8, m=3)
EXPIRES["no_sessions"] = lambda: ExpireCase([(LIVE, row(8, [(1, 0)]), None)], w=8, m=0)
