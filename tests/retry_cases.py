"""Cases of the retry stage shared by the CPU and the GPU tests: small tables written out slot by
slot, each with the sequential restatement's answer (tests/retry_ref.py) computed once on demand.

A session is ``S(entries, rec=..., interval=...)``; an entry is ``(slot, pkt_id, phase, qos, ref, ts,
dup)`` with ``ts`` None for a slot without a stamp.  ``rec`` None names a subscriber id at or above
sub_limit.  Between the named sessions lie rows no list names, filled with old entries: a sweep must
leave them alone."""

import numpy as np

from emqx_amd import ack as A
from emqx_amd import retry as RT
from emqx_amd import window as W
from tests import retry_ref as R
from tests.ack_cases import records_of, rows_of

NOW = 1_700_000_000_000
M, P = R.MSG, R.PUBREL_AWAIT
OKREC = dict(inflight=5, flags=W.PRESENT | W.CONNECTED)
WIDTHS = (8, 32, 64)


def rows_per_block(w):
    return 512 // w  # emqx_amd/csrc/retry.h: AK_BLOCK / (w / 2)


class S:
    def __init__(self, entries=(), rec=OKREC, interval=None):
        self.entries, self.rec, self.interval = list(entries), rec, interval


def full_row(w, ts, phase=M, first_id=1):
    return [(j, first_id + j, phase, 1, j, ts, 0) for j in range(w)]


class Case:
    def __init__(self, sessions, w=8, now=NOW, interval=100, expiry=None, mode=R.MODE_RETRY, cap_out=None, whole=False, spare=1,
                 reverse=True):
        self.w, self.now, self.interval, self.expiry, self.mode, self.cap_out = w, now, interval, expiry, mode, cap_out
        n = len(sessions)
        stride = 1 if whole else spare + 1
        self.sub_limit = max(n * stride, 1)
        self.table = W.pack_sessions(self.sub_limit, inflight=3)
        self.slots = A.empty_slots(self.sub_limit, w)
        self.stamps = RT.empty_stamps(self.sub_limit, w)
        for sub in range(self.sub_limit):  # what no list names: an old entry that would be due
            self.slots[sub, w - 1] = (9, M, 1, 0)
            self.stamps[sub, w - 1] = R.make_stamp(1, 0, M, 9)
        order = list(range(n))[::-1] if reverse and not whole else list(range(n))
        subs, bad = [], 0
        per = any(s.interval is not None for s in sessions)
        self.intervals = np.full(self.sub_limit, 7, dtype=np.uint32) if per else None
        for i, s in zip(order, sessions):
            if s.rec is None:
                subs.append(self.sub_limit + bad)
                bad += 1
                continue
            sub = i * stride
            subs.append(sub)
            self.table[sub] = W.pack_sessions(1, **s.rec)[0]
            self.slots[sub] = 0
            self.stamps[sub] = 0
            for slot, pkt_id, phase, qos, ref, ts, dup in s.entries:
                self.slots[sub, slot] = (pkt_id, phase, qos, ref)
                if ts is not None:
                    self.stamps[sub, slot] = R.make_stamp(ts, dup, phase, pkt_id)
            if per:
                self.intervals[sub] = interval if s.interval is None else s.interval
        self.subs = None if whole else np.array(subs, dtype=np.uint32)
        self.m = self.sub_limit if whole else n
        self.deadlines = None if expiry is None else np.array([RT.deadline(c, s) for c, s in expiry], dtype=np.uint64)
        self.ref_limit = 0 if expiry is None else len(expiry)
        self._ref = {}

    def reference(self, update_table=True, cap_out="case"):
        cap = self.cap_out if cap_out == "case" else cap_out
        key = (update_table, cap)
        if key not in self._ref:
            recs, rows, stamps = records_of(self.table), rows_of(self.slots), self.stamps.tolist()
            ref = R.sweep(None if self.subs is None else self.subs.tolist(), recs, rows, stamps, self.now, self.interval,
                          None if self.intervals is None else self.intervals.tolist(), self.expiry, self.mode, cap, update_table)
            ref["rows"], ref["stamps"], ref["inflight"] = rows, stamps, [r["inflight"] for r in recs]
            self._ref[key] = ref
        return self._ref[key]


def check(ref, got, slots, stamps, table):
    """A Swept and the tables after the call against the restatement's answer, every field exact."""
    assert [got.summary[k] for k in RT.SWEEP_SUMMARY] == ref["summary"]
    assert got.offsets.tolist() == ref["offsets"]
    assert [list(map(int, it)) for it in got.items.tolist()] == ref["items"]
    assert got.status.tolist() == ref["status"] and got.counts.tolist() == ref["counts"] and got.timers.tolist() == ref["timers"]
    assert rows_of(slots) == ref["rows"] and stamps.tolist() == ref["stamps"]
    assert table["inflight"].tolist() == ref["inflight"]


def same(x, y):
    """Two Swept byte for byte."""
    assert x.summary == y.summary
    for a, b in zip(x[:-1], y[:-1]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ages(w=8):
    iv = 100
    return Case([S([(0, 1, M, 1, 0, NOW - iv + 1, 0), (1, 2, M, 1, 1, NOW - iv, 0), (2, 3, M, 2, 2, NOW - iv - 1, 0),
                    (3, 4, P, 2, 3, NOW + 50, 0)])], w=w, interval=iv)


def _deadlines():
    # created + interval_s * 1000 = now - 1, now, now + 1; no expiry; a PUBREL_AWAIT slot on a past deadline
    expiry = [(NOW - 1001, 1), (NOW - 1000, 1), (NOW - 999, 1), (NOW - 5000, None), (NOW - 9000, 2)]
    return Case([S([(0, 10, M, 1, 0, NOW - 300, 0), (1, 11, M, 1, 1, NOW - 300, 0), (2, 12, M, 2, 2, NOW - 300, 0),
                    (3, 13, M, 1, 3, NOW - 300, 0), (4, 14, P, 2, 4, NOW - 300, 0), (5, 15, M, 1, 4, NOW - 10, 0)])], expiry=expiry)


def _rows(w, m, seed, **kw):
    rng = np.random.default_rng(seed)
    return Case([_random_session(rng, w, 100, 6) for _ in range(m)], w=w, expiry=_EXPIRY, spare=0, **kw)


_EXPIRY = [(NOW - 5000, 1), (NOW - 500, 1), (NOW - 100, None), (NOW + 20, 0), (NOW - 1000, 1), (NOW - 1001, 1)]


def _random_session(rng, w, interval, ref_limit, bad=False):
    roll = rng.integers(0, 40)
    if bad and roll == 0:
        return S(rec=None)
    flags = {1: 0, 2: W.PRESENT | W.PASS, 3: W.CONNECTED}.get(int(roll), W.PRESENT | W.CONNECTED)
    k = int(rng.choice([0, 1, w // 2, w])) if rng.integers(0, 3) == 0 else int(rng.integers(0, w + 1))
    slots = rng.permutation(w)[:k]
    ids = rng.permutation(np.arange(1, 4 * w))[:k]
    stamps = [NOW - 2 * interval, NOW - interval - 1, NOW - interval, NOW - interval + 1, NOW - 1, NOW, NOW + 7]
    tie = int(rng.integers(0, len(stamps)))
    entries = []
    for slot, pkt_id in zip(slots.tolist(), ids.tolist()):
        ts = stamps[tie if rng.integers(0, 2) else int(rng.integers(0, len(stamps)))]
        if rng.integers(0, 25) == 0:
            ts = None
        entries.append((slot, pkt_id, P if rng.integers(0, 4) == 0 else M, int(rng.integers(1, 3)),
                        int(rng.integers(0, ref_limit + (2 if bad else 0))), ts, int(rng.integers(0, 2))))
    return S(entries, rec=dict(inflight=int(rng.integers(0, w + 3)), flags=flags),
             interval=None if rng.integers(0, 3) else int(rng.choice([0, 1, interval, 2 * interval])))


def fuzz(seed=3, n_sessions=2500, w=16, mode=R.MODE_RETRY):
    rng = np.random.default_rng(seed)
    return Case([_random_session(rng, w, 100, len(_EXPIRY), bad=True) for _ in range(n_sessions)], w=w, expiry=_EXPIRY, mode=mode)


tie = NOW - 500
SWEEPS = {
    "empty_row": lambda: Case([S()]),
    "one_item": lambda: Case([S([(3, 7, M, 1, 40, NOW - 100, 0)])]),
    "ages_interval-1_interval_interval+1_future": _ages,
    "interval_0": lambda: Case([S([(0, 1, M, 1, 0, NOW, 0), (1, 2, M, 1, 1, NOW - 1, 0), (2, 3, M, 1, 2, NOW + 1, 0)])], interval=0),
    "tie_ids_1_and_65535": lambda: Case([S([(0, 65535, M, 1, 0, tie, 0), (1, 300, P, 2, 1, tie, 0), (5, 1, M, 2, 2, tie, 0),
                                            (6, 2, M, 1, 3, tie - 1, 0)])]),
    "intervals_override_the_call": lambda: Case([S([(0, 1, M, 1, 0, NOW - 50, 0)], interval=50), S([(0, 1, M, 1, 0, NOW - 50, 0)]),
                                                 S([(0, 1, M, 1, 0, NOW - 50, 0)], interval=51)], interval=1000),
    "deadlines_now-1_now_now+1_never_pubrel": _deadlines,
    "every_old_entry_expired": lambda: Case([S([(0, 1, M, 1, 0, NOW - 200, 0), (1, 2, M, 2, 0, NOW - 300, 1)],
                                               rec=dict(inflight=2, flags=3))], expiry=[(NOW - 5000, 1)]),
    "expired_below_inflight_0": lambda: Case([S([(0, 1, M, 1, 0, NOW - 200, 0)], rec=dict(inflight=0, flags=3))], expiry=[(0, 0)]),
    "not_present": lambda: Case([S(full_row(8, NOW - 900), rec=dict(flags=W.CONNECTED)), S([(0, 1, M, 1, 0, NOW - 900, 0)])]),
    "pass": lambda: Case([S(full_row(8, NOW - 900), rec=dict(flags=W.PRESENT | W.PASS)), S([(0, 1, M, 1, 0, NOW - 900, 0)])]),
    "sub_at_sub_limit": lambda: Case([S([(0, 1, M, 1, 0, NOW - 900, 0)]), S(rec=None), S([(1, 2, P, 2, 0, NOW - 900, 0)])]),
    "ref_at_ref_limit": lambda: Case([S([(0, 1, M, 1, 1, NOW - 900, 0), (1, 2, M, 1, 0, NOW - 900, 0), (2, 3, P, 2, 9, NOW - 900, 0),
                                         (3, 4, M, 1, 9, NOW - 1, 0)])], expiry=[(NOW - 5000, 1)]),
    "unstamped_slot": lambda: Case([S([(0, 1, M, 1, 0, None, 0), (1, 2, M, 1, 1, NOW - 100, 0)]),
                                    S([(0, 1, P, 2, 0, None, 0)], interval=0)]),
    "stamp_of_another_id_or_phase": lambda: _foreign(),
    "id_held_twice": lambda: Case([S([(0, 5, M, 1, 0, NOW - 200, 0), (3, 5, M, 2, 1, NOW - 200, 0), (4, 4, M, 1, 2, NOW - 200, 0),
                                      (6, 5, P, 2, 3, NOW - 300, 0)])]),
    "subs_null_whole_table": lambda: Case([S([(0, 1, M, 1, 0, NOW - 100, 0)]), S(), S(full_row(8, NOW - 5)),
                                           S([(2, 2, P, 2, 1, NOW - 400, 0)], rec=dict(flags=0))], whole=True),
    "replay": lambda: Case([S([(5, 2, P, 2, 1, NOW - 1, 0), (1, 65535, M, 1, 2, None, 0), (2, 1, M, 2, 3, NOW + 9, 1)]), S(),
                            S(full_row(8, NOW), rec=dict(flags=W.PRESENT | W.PASS))], mode=R.MODE_REPLAY, expiry=[(0, 0)] * 4),
    "scan_chunk_2_five_tiles_w64": lambda: _rows(64, 5 * rows_per_block(64) - 3, 11),
}
for _w in WIDTHS:
    SWEEPS["full_row_tie_w%d" % _w] = lambda w=_w: Case([S(full_row(w, NOW - 100)[::-1]), S(), S(full_row(w, NOW - 99))], w=w)
    SWEEPS["full_row_descending_ts_w%d" % _w] = lambda w=_w: Case(
        [S([(j, 1 + (j * 7) % w, P if j % 3 == 0 else M, 1, j, NOW - 100 - (w - j) // 2, 0) for j in range(w)])], w=w)
    for _d in (-1, 0, 1):
        SWEEPS["rows_per_block%+d_w%d" % (_d, _w)] = lambda w=_w, d=_d: _rows(w, rows_per_block(w) + d, 20 + w + d)


def _foreign():
    c = Case([S([(0, 1, M, 1, 0, NOW - 500, 0), (1, 2, P, 2, 1, NOW - 500, 0), (2, 3, M, 1, 2, NOW - 500, 1)])])
    sub = int(c.subs[0])
    c.stamps[sub, 0] = R.make_stamp(NOW - 500, 0, M, 8)  # another id
    c.stamps[sub, 1] = R.make_stamp(NOW - 500, 0, M, 2)  # the phase before the PUBREC
    c.stamps[sub, 5] = R.make_stamp(NOW - 500, 0, M, 6)  # an EMPTY slot's stale stamp: the stamp call's to clear
    return c


def overflow_case():
    """Five items in three sessions, an expiry among them."""
    return Case([S([(0, 1, M, 1, 0, NOW - 200, 0), (1, 2, M, 1, 1, NOW - 300, 0)]), S([(0, 1, P, 2, 0, NOW - 200, 0)]),
                 S([(4, 9, M, 1, 0, NOW - 100, 0), (5, 8, M, 2, 1, NOW - 100, 0), (6, 7, M, 2, 1, NOW, 0)])],
                expiry=[(NOW - 5000, 1), (NOW, 1)])


class StampCase:
    def __init__(self, sessions, w=8, now=NOW):
        base = Case(sessions, w=w, now=now)
        self.w, self.now, self.sub_limit, self.subs, self.m = w, now, base.sub_limit, base.subs, base.m
        self.slots, self.stamps = base.slots, base.stamps
        self._ref = None

    def reference(self):
        if self._ref is None:
            rows, stamps = rows_of(self.slots), self.stamps.tolist()
            summary = R.stamp(self.subs.tolist(), rows, stamps, self.now, self.sub_limit)
            self._ref = {"summary": summary, "stamps": stamps}
        return self._ref


def check_stamp(ref, got, stamps):
    assert [got.summary[k] for k in RT.STAMP_SUMMARY] == ref["summary"]
    assert stamps.tolist() == ref["stamps"]


def _stamp_mixed():
    """An insert, a PUBREC transition, an unchanged slot, a freed slot, a slot freed and refilled
    with another id, the same id refilled (keeps its stamp), next to a bad subscriber."""
    c = StampCase([S([(0, 1, M, 1, 0, None, 0), (1, 2, P, 2, 1, NOW - 40, 0), (2, 3, M, 1, 2, NOW - 40, 1), (4, 5, M, 1, 4, NOW - 40, 0),
                      (5, 6, M, 2, 5, NOW - 40, 1)]), S(rec=None), S([(7, 9, P, 2, 0, NOW - 7, 0)])])
    sub = int(c.subs[0])
    c.stamps[sub, 1] = R.make_stamp(NOW - 40, 0, M, 2)   # was MSG when it was stamped
    c.stamps[sub, 3] = R.make_stamp(NOW - 40, 0, M, 4)   # its slot was freed since
    c.stamps[sub, 4] = R.make_stamp(NOW - 40, 0, M, 44)  # freed and refilled with id 5
    return c


STAMPS = {"mixed": _stamp_mixed}
for _w in WIDTHS:
    STAMPS["rows_per_block+1_w%d" % _w] = lambda w=_w: _stamp_rows(w)


def _stamp_rows(w):
    rng = np.random.default_rng(w)
    c = StampCase([_random_session(rng, w, 100, 4, bad=True) for _ in range(rows_per_block(w) + 1)], w=w)
    for sub in range(c.sub_limit):  # stale stamps of every sort
        for j in range(w):
            if rng.integers(0, 4) == 0:
                c.stamps[sub, j] = R.make_stamp(NOW - 9, int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(1, 4 * w)))
    return c
