"""CPU-side checks of the rel stage (include/emqx_rel.h) on a host-only handle: the restatement
(tests/rel_ref.py) against the known answers of the reference's own suite
(tests/golden/rel_kats.json), emqx_rel_run_host and emqx_rel_expire_host byte for byte against the
restatement on every case, what the directed cases and the fuzz set reach, the exports, the
refusals and argument errors, and no batch call without a device."""

import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import rel_cases as C
from tests import rel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rel_kats.json")))
FUZZ_SEEDS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def T():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import rel
    return rel


def host(T):
    return T.Rel(T.HOST_ONLY)


def run(T, case, fn="run_host"):
    """The host evaluator on a copy of the case's rows; a bad subscriber's EINVAL carries the outputs."""
    from emqx_amd import _lib
    table, rel = case.table.copy(), case.rel.copy()
    try:
        got = getattr(host(T), fn)(case.subs, case.offsets, case.events, table, rel, **case.host_args())
        assert not case.reference()["summary"][0] & R.F_BAD_SUB
    except _lib.EngineError as e:
        assert e.code == EINVAL and e.summary["flags"] & R.F_BAD_SUB
        got = e.partial
    assert table.tobytes() == case.table.tobytes(), "the stage never writes sessions[]"
    return got, rel


def expire(T, case):
    from emqx_amd import _lib
    table, rel = case.table.copy(), case.rel.copy()
    try:
        got = host(T).expire_host(table, rel, **case.host_args())
        assert not case.reference()["summary"][0] & R.F_BAD_SUB
    except _lib.EngineError as e:
        assert e.code == EINVAL and e.summary["flags"] & R.F_BAD_SUB
        got = e.partial
    assert table.tobytes() == case.table.tobytes()
    return got, rel


# ---- the known answers --------------------------------------------------------------------------

def _stamp(ts, now):
    return now if ts == "now" else ts


def play(kat, publish, pubrel, cnt, full, awaiting, expire_):
    """One KAT through callbacks; answers are "ok" or an MQTT reason code."""
    now = kat["now"]
    for step in kat["steps"]:
        op = step[0]
        if op == "publish":
            assert publish(step[1]) == step[2], (kat["name"], step)
        elif op == "pubrel":
            assert pubrel(step[1]) == step[2], (kat["name"], step)
        elif op == "cnt":
            assert cnt() == step[1], (kat["name"], step)
        elif op == "full":
            assert full() == step[1], (kat["name"], step)
        elif op == "awaiting":
            assert awaiting() == sorted([p, _stamp(t, now)] for p, t in step[1]), (kat["name"], step)
        elif op == "expire":
            assert expire_() == step[1], (kat["name"], step)
        else:
            raise AssertionError(op)


def _answer(v):
    return "ok" if v == R.OK else R.RC[v]


@pytest.mark.parametrize("kat", GOLDEN["cases"], ids=[k["name"] for k in GOLDEN["cases"]])
def test_restatement_against_the_suite(kat):
    w, now, limit, timeout = 128, kat["now"], kat["max_awaiting_rel"], kat["await_rel_timeout"]
    state = {"a": {s: (p, _stamp(t, now)) for s, (p, t) in enumerate(kat["awaiting_rel"])}}

    def expire_():
        rows = [R.row_of(state["a"], w)]
        x = R.expire(None, 1, [R.PRESENT | R.CONNECTED], rows, w, now, timeout_ms=timeout)
        state["a"] = R.awaiting_of(rows[0])
        return timeout if x["counts"][0][2] else None
    play(kat, lambda p: _answer(R.publish(state["a"], limit, p, now, w)), lambda p: _answer(R.pubrel(state["a"], p)),
         lambda: len(state["a"]), lambda: R.is_awaiting_full(state["a"], limit),
         lambda: sorted([p, t] for p, t in state["a"].values()), expire_)


@pytest.mark.parametrize("kat", [k for k in GOLDEN["cases"] if k["max_awaiting_rel"]], ids=lambda k: k["name"])
def test_host_evaluator_against_the_suite(T, kat):
    """The same steps through emqx_rel_run_host and emqx_rel_expire_host, one call a step."""
    from emqx_amd import window
    w, now, limit, timeout = 128, kat["now"], kat["max_awaiting_rel"], kat["await_rel_timeout"]
    table = window.pack_sessions(1)
    rel = T.empty_rows(1, w)
    for s, (p, t) in enumerate(kat["awaiting_rel"]):
        rel[0, s] = T.pack_entry(_stamp(t, now), p)
    h = host(T)

    def event(kind, p):
        got = h.run_host([0], [0, 1], T.pack_events([kind], [p]), table, rel, max_awaiting=limit, now_ms=now)
        assert got.route.tolist() == ([0] if kind == R.PUBLISH and got.verdicts[0] == R.OK else [])
        return _answer(int(got.verdicts[0]))

    def expire_():
        x = h.expire_host(table, rel, now_ms=now, timeout_ms=timeout)
        return timeout if x.counts[0, 2] else None
    play(kat, lambda p: event(R.PUBLISH, p), lambda p: event(R.PUBREL, p), lambda: int(np.count_nonzero(rel)),
         lambda: int(np.count_nonzero(rel)) >= limit,
         lambda: sorted([int(T.entry_id(e)), int(T.entry_ts(e))] for e in rel[0] if e), expire_)


def test_defaults_and_reason_codes(T):
    d = GOLDEN["defaults"]
    assert (d["awaiting_rel_cnt"], d["awaiting_rel_max"], d["await_rel_timeout"]) == (0, T.DEFAULT_MAX_AWAITING, T.DEFAULT_TIMEOUT)
    assert T.MAX_W >= T.DEFAULT_MAX_AWAITING, "the widest row covers the default limit"
    rc = GOLDEN["reason_codes"]
    assert (R.RC[R.IN_USE], R.RC[R.NOT_FOUND], R.RC[R.EXCEEDED]) == (
        rc["packet_identifier_in_use"], rc["packet_identifier_not_found"], rc["receive_maximum_exceeded"]) == (0x91, 0x92, 0x93)
    # max_awaiting_rel infinity (t_is_awaiting_full_false) is what no row holds: ROW_SMALL, never a silent difference
    from emqx_amd import window
    got = host(T).run_host([0], [0, 1], T.pack_events([R.PUBLISH], [1]), window.pack_sessions(1), T.empty_rows(1, 128), max_awaiting=0)
    assert got.verdicts.tolist() == [R.ROW_SMALL] and got.summary["flags"] == R.F_ROW_SMALL and got.counts.tolist() == [[0, 0, 0, 0]]


# ---- the host evaluator against the restatement -------------------------------------------------

@pytest.mark.parametrize("name", list(C.RUNS))
def test_run_cases(T, name):
    case = C.RUNS[name]()
    got, rel = run(T, case)
    C.check_run(case.reference(), got, rel)


def test_hover_session_of_20000_events(T):
    case = C.hover_case()
    ref = case.reference()
    lo, hi = int(case.offsets[1]), int(case.offsets[2])
    assert hi - lo == 20000
    v = ref["verdicts"][lo:hi]
    assert v[:5].tolist() == [R.OK, R.EXCEEDED, R.EXCEEDED, R.OK, R.OK] and (v.reshape(-1, 5) == v[:5]).all()
    assert ref["counts"][1].tolist() == [8000, 4000, 8000, 3] and ref["arm"].tolist() == [1, 1, 0]
    got, rel = run(T, case)
    C.check_run(ref, got, rel)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(T, seed):
    case = C.fuzz(seed)
    got, rel = run(T, case)
    C.check_run(case.reference(), got, rel)


def test_fuzz_reaches_every_verdict():
    """The restatement alone: every verdict an event can get (OK through BAD_KIND) at least 20
    times over the fuzz set, and at least a quarter of the PUBLISH events of sessions with a limit
    EXCEEDED or IN_USE."""
    seen = np.zeros(16, dtype=np.int64)
    publishes = refused = 0
    for seed in FUZZ_SEEDS:
        case = C.fuzz(seed)
        v = case.reference()["verdicts"]
        seen += np.bincount(v, minlength=16)
        live = ~np.isin(v, (R.NO_SESSION, R.PASS, R.ROW_SMALL))
        pub = live & ((case.events >> 16) == R.PUBLISH)
        publishes += int(pub.sum())
        refused += int((pub & np.isin(v, (R.EXCEEDED, R.IN_USE))).sum())
    for verdict in (R.OK, R.IN_USE, R.NOT_FOUND, R.EXCEEDED, R.NO_SESSION, R.PASS, R.ROW_SMALL, R.BAD_KIND):
        assert seen[verdict] >= 20, (verdict, seen[:10])
    assert seen[0] == 0 and seen[R.IDLE:].sum() == 0
    assert 4 * refused >= publishes > 0, (refused, publishes)


def test_cases_mean_what_their_names_say():
    for w in C.WIDTHS:
        case = C.table_case(w)
        ref = case.reference()

        def box(k):
            lo, hi = int(case.offsets[k]), int(case.offsets[k + 1])
            return ref["verdicts"][lo:hi].tolist(), ref["counts"][k].tolist(), ref["rel"][case.subs[k]] if case.subs[k] < case.sub_limit else None
        v, cnt, row = box(0)
        assert v == [R.OK, R.OK, R.OK, R.NOT_FOUND, R.OK, R.BAD_KIND, R.BAD_KIND, R.BAD_KIND] and cnt == [3, 1, 4, 1]
        assert int(row[0]) == R.entry(C.NOW, 1) and not row[1:].any()
        v, cnt, row = box(1)
        assert v == [R.OK, R.EXCEEDED, R.EXCEEDED] and cnt == [1, 0, 2, w] and int(row[3]) == R.entry(C.NOW, 5)
        v, cnt, row = box(2)
        assert v == [R.EXCEEDED, R.OK, R.OK, R.OK, R.EXCEEDED, R.OK] and cnt == [3, 1, 2, w]
        assert int(row[w // 2]) & 0xFFFF == 4000, "the publish that now fits takes the freed slot"
        v, cnt, row = box(3)
        assert v == [R.IN_USE, R.OK, R.OK, R.OK, R.EXCEEDED] and int(row[0]) & 0xFFFF == 100 and int(row[1]) & 0xFFFF == 300
        assert box(4)[0] == [R.ROW_SMALL] * 3 and box(5)[0] == [R.ROW_SMALL] and box(4)[1] == [0, 0, 0, 0]
        assert box(6)[0] == [R.NO_SESSION] * 2 and box(7)[0] == [R.PASS] * 2 and box(8)[0] == [R.NO_SESSION] and box(10)[0] == [R.NO_SESSION] * 2
        v, cnt, row = box(11)
        assert v == [R.OK, R.OK, R.OK, R.NOT_FOUND] and cnt == [1, 2, 1, 2] and not row[1] and not row[w - 1] and int(row[0]) & 0xFFFF == 8
        v, cnt, row = box(12)
        assert v == [R.OK] * 5 and int(row[1]) >> 17 == (1 << 45) - 1 and int(row[0]) >> 17 == (1 << 45) - 1 and int(row[2]) >> 17 == 0
        assert ref["summary"][0] == R.F_BAD_SUB | R.F_ROW_SMALL | R.F_BAD_TS
        assert ref["arm"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]
        assert (ref["rel"][[s for s in range(case.sub_limit) if s not in set(case.subs.tolist())]] ==
                case.rel[[s for s in range(case.sub_limit) if s not in set(case.subs.tolist())]]).all()
    ref = C.RUNS["no_ts_w128_src_now_past_limit"]().reference()
    assert ref["summary"][0] == R.F_BAD_TS and ref["route"].tolist() == [11 + 3 * (6 - d) for d in (0, 1, 3, 5)]
    for t in (C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + 1):
        assert C.tile_case(t, True).reference()["summary"][3] == t and C.tile_case(t, False).reference()["summary"][3] == 0
        assert C.tile_case(t, False).reference()["summary"][6] == t
    for w in C.WIDTHS:
        lens = np.diff(C.lens_case(w).offsets.astype(np.int64)).tolist()
        assert lens == C.lens_of(w)
        for L in (C.lanes_of(w), min(w // 2, 64)):
            assert {0, 1, L - 1, L, L + 1, 2 * L + 1} <= set(lens), (w, L, lens)
    assert C.session_counts(8) == [15, 16, 17, 63, 64, 65, 129] and C.session_counts(128) == [7, 8, 9, 31, 32, 33, 65]


# ---- the expire call ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.EXPIRES))
def test_expire_cases(T, name):
    case = C.EXPIRES[name]()
    got, rel = expire(T, case)
    C.check_expire(case.reference(), got, rel)


def test_expire_cases_mean_what_their_names_say():
    for w in C.WIDTHS:
        ref = C.expire_case(w).reference()
        assert ref["status"].tolist() == [R.OK] * 5 + [R.NO_SESSION, R.PASS] + [R.OK] * 4
        assert ref["counts"][:5].tolist() == [[0, 2, 1, 0], [3, 0, 0, 0], [1, 2, 1, 0], [0, 0, 0, 0], [w // 2, w // 2, 1, 0]]
        assert ref["counts"][7].tolist() == [1, 1, 1, 0]
        case = C.expire_case(w, listed=True, channel_rule=True, mixed=True)
        ref = case.reference()
        assert case.subs.tolist() == [10, 8, 6, 4, 2, 0, 11] and ref["summary"][0] == R.F_BAD_SUB
        assert ref["status"].tolist() == [R.OK, R.OK, R.PASS, R.OK, R.OK, R.OK, R.NO_SESSION]
        assert ref["counts"][0].tolist() == [1, 1, 1, 0] and ref["counts"][1].tolist() == [0, 2, 1, 0], "timeout 1; infinity"
        assert (ref["rel"][[1, 3, 5, 7, 9]] == case.rel[[1, 3, 5, 7, 9]]).all(), "sessions the call does not name"
    ref = C.expire_case(16, channel_rule=True).reference()
    assert ref["status"][7] == R.IDLE and ref["counts"][7].tolist() == [0, 0, 0, 0]
    ref = C.expire_case(16, mixed=True).reference()
    assert ref["counts"][9].tolist() == [1, 1, 1, 0], "timeout 0: age 0 is due, a stamp in the future is not"
    ref = C.expire_case(16, timeout_ms=0xFFFFFFFF).reference()
    assert ref["summary"][3] == 0


# ---- the ABI ------------------------------------------------------------------------------------

def test_exports_every_rel_symbol(T):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_rel.h")
    assert len(declared) == 13
    assert sorted(_lib.REL_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(T):
    import emqx_amd
    assert emqx_amd.Rel is T.Rel


def test_constants_mirror_the_headers(T):
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "rel.h")).read()
    block = int(re.search(r"RL_BLOCK = (\d+);", src).group(1))
    rows = int(re.search(r"RL_ROWS = (\d+);", src).group(1))
    assert re.search(r"RL_TILE = RL_BLOCK \* RL_ROWS;", src)
    assert (T.BLOCK, T.ROWS, T.TILE) == (block, rows, block * rows)
    pub = open(os.path.join(ROOT, "include", "emqx_rel.h")).read()

    def define(name):
        return int(re.search(r"#define EMQX_REL_%s \(?(\w+?)(u|ull)?\b" % name, pub).group(1), 0)
    for name in ("PUBLISH", "PUBREL", "DIRECT", "OK", "IN_USE", "NOT_FOUND", "EXCEEDED", "NO_SESSION", "PASS", "ROW_SMALL", "BAD_KIND",
                 "IDLE", "F_INPUT_REFUSED", "F_BAD_SUB", "F_ROW_SMALL", "F_BAD_TS", "NO_TIMEOUT"):
        assert define(name) == getattr(T, name) == getattr(R, name), name
    assert define("DEFAULT_MAX_AWAITING") == T.DEFAULT_MAX_AWAITING and define("DEFAULT_TIMEOUT") == T.DEFAULT_TIMEOUT
    assert define("MAX_W") == T.MAX_W == max(T.WIDTHS)
    assert define("SUMMARY_WORDS") == T.SUMMARY_WORDS == len(T.RUN_SUMMARY) == len(T.EXPIRE_SUMMARY)
    assert re.search(r"#define EMQX_REL_TS_LIMIT \(1ull << 45\)", pub) and T.TS_LIMIT == R.TS_LIMIT == 1 << 45
    assert re.search(r"#define EMQX_REL_MAX_EVENTS \(1ull << 31\)", pub) and T.MAX_EVENTS == 1 << 31
    from emqx_amd import window
    assert (R.PRESENT, R.CONNECTED, R.PASSF) == (window.PRESENT, window.CONNECTED, window.PASS)
    assert int(T.pack_entry(5, 7)) == R.entry(5, 7) == (5 << 17) | (1 << 16) | 7
    assert int(T.entry_id(R.entry(5, 7))) == 7 and int(T.entry_ts(R.entry((1 << 45) - 1, 65535))) == (1 << 45) - 1
    assert [T.default_lanes(w) for w in T.WIDTHS] == [4, 4, 4, 4, 8]


def test_struct_sizes_and_stats_versioning(T):
    from emqx_amd import _lib
    assert ctypes.sizeof(_lib.RelRunArgs) == 20 * 8 and ctypes.sizeof(_lib.RelExpireArgs) == 14 * 8
    assert ctypes.sizeof(_lib.RelStats) == 64
    h = host(T)
    s = h.stats()
    assert set(s) == {"cap_in", "cap_boxes", "w", "scratch_bytes", "lanes", "calls", "last_call_ms"} and s["calls"] == 0
    short = _lib.RelStats()
    short.size = 16
    short.cap_boxes = 77
    assert _lib.lib().emqx_rel_stats_get(h._h, ctypes.byref(short)) == 0 and short.size == 16 and short.cap_boxes == 77
    short.size = 4
    assert _lib.lib().emqx_rel_stats_get(h._h, ctypes.byref(short)) == EINVAL
    big = (ctypes.c_uint64 * 16)(*([0x5A5A5A5A5A5A5A5A] * 16))
    big[0] = 128
    assert _lib.lib().emqx_rel_stats_get(h._h, ctypes.cast(big, ctypes.POINTER(_lib.RelStats))) == 0
    assert big[0] == 64 and big[8] == 0x5A5A5A5A5A5A5A5A, "no more than the library's struct is written"
    case = C.RUNS["no_ts_w8"]()
    h.run_host(case.subs, case.offsets, case.events, case.table.copy(), case.rel.copy(), **case.host_args())
    assert h.stats()["calls"] == 1


def test_tuning_keys(T):
    from emqx_amd import _lib
    h = host(T)
    for key, good, bad in (("lanes", (0, 4, 8, 16, 32, 64), (-1, 1, 2, 3, 12, 128)), ("max_blocks", (1, 4096), (0, 4097)),
                           ("scan_chunk", (1, 1024), (0, 1025))):
        for v in good:
            h.set_tuning(key, v)
        for v in bad:
            with pytest.raises(_lib.EngineError) as e:
                h.set_tuning(key, v)
            assert e.value.code == EINVAL, (key, v)
    assert h.stats()["lanes"] == 64
    for key in ("rematch", "path", ""):
        with pytest.raises(_lib.EngineError) as e:
            h.set_tuning(key, 1)
        assert e.value.code == ENOTFOUND


def _run_args(T, keep, **kw):
    b = T.Rel.run_args(keep["subs"].ctypes.data, keep["off"].ctypes.data, keep["ev"].ctypes.data, 1, 2, 1, keep["tab"].ctypes.data, 2,
                       keep["rel"].ctypes.data, keep["rel"].shape[1], keep["ver"].ctypes.data, keep["route"].ctypes.data,
                       keep["cnt"].ctypes.data, keep["arm"].ctypes.data, max_awaiting=4)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _keep(T, w=8):
    from emqx_amd import window
    return dict(subs=np.zeros(1, np.uint32), off=np.array([0, 2], np.uint64), ev=T.pack_events([1, 2], [3, 3]),
                tab=window.pack_sessions(2), rel=T.empty_rows(2, w), ver=np.zeros(2, np.uint8), route=np.zeros(2, np.uint32),
                cnt=np.zeros(4, np.uint32), arm=np.zeros(1, np.uint8), st=np.zeros(2, np.uint8), xcnt=np.zeros(8, np.uint32))


def test_argument_errors(T):
    from emqx_amd import _lib
    L, h = _lib.lib(), host(T)
    keep = _keep(T)
    summary = np.zeros(8, np.uint64)
    assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, keep)), summary.ctypes.data) == 0
    assert summary.tolist() == [0, 2, 1, 1, 1, 0, 0, 0] and keep["ver"].tolist() == [R.OK, R.OK]
    for w in (0, 4, 12, 24, 100, 256):  # W is one of 8, 16, 32, 64, 128
        assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, keep, w=w)), None) == EINVAL, w
        x = T.Rel.expire_args(1, 1, keep["tab"].ctypes.data, 2, keep["rel"].ctypes.data, w, 5, keep["st"].ctypes.data, keep["xcnt"].ctypes.data)
        assert L.emqx_rel_expire_host(h._h, ctypes.byref(x), None) == EINVAL, w
    for w in T.WIDTHS:
        k = _keep(T, w)
        assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, k)), None) == 0, w
    for field in ("ev_offsets", "ev_subs", "events", "sessions", "rel", "verdicts", "out_route", "out_counts", "out_arm"):
        assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, keep, **{field: None})), None) == EINVAL, field
    assert L.emqx_rel_run_host(None, ctypes.byref(_run_args(T, keep)), None) == EINVAL
    assert L.emqx_rel_run_host(h._h, None, None) == EINVAL
    assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, keep, m=2)), None) == EINVAL  # m > cap_boxes
    # refused: more events than cap_in; the summary alone is written
    keep["ver"][:] = 0x5A
    assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, keep, cap_in=1)), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [R.F_INPUT_REFUSED, 2, 1, 0, 0, 0, 0, 0] and keep["ver"].tolist() == [0x5A, 0x5A]
    bad = np.array([1, 0], np.uint64)  # offsets[0] != 0, decreasing
    assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, keep, ev_offsets=bad.ctypes.data)), None) == EINVAL
    count = np.array([2], np.uint64)  # the count behind n_boxes: 2 > cap_boxes
    assert L.emqx_rel_run_host(h._h, ctypes.byref(_run_args(T, keep, n_boxes=count.ctypes.data)), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [R.F_INPUT_REFUSED, 0, 2, 0, 0, 0, 0, 0]
    x = T.Rel.expire_args(3, 2, keep["tab"].ctypes.data, 2, keep["rel"].ctypes.data, 8, 5, keep["st"].ctypes.data, keep["xcnt"].ctypes.data)
    assert L.emqx_rel_expire_host(h._h, ctypes.byref(x), None) == EINVAL  # m > cap_boxes
    x.n_boxes, x.m = count.ctypes.data, 0
    count[0] = 3
    assert L.emqx_rel_expire_host(h._h, ctypes.byref(x), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [R.F_INPUT_REFUSED, 0, 3, 0, 0, 0, 0, 0]
    count[0] = 2
    keep["rel"][1, 2] = T.pack_entry(0, 9)
    assert L.emqx_rel_expire_host(h._h, ctypes.byref(x), summary.ctypes.data) == 0 and summary.tolist() == [0, 2, 2, 0, 1, 1, 0, 0]
    for field in ("sessions", "rel", "out_status", "out_counts"):
        y = T.Rel.expire_args(1, 1, keep["tab"].ctypes.data, 2, keep["rel"].ctypes.data, 8, 5, keep["st"].ctypes.data, keep["xcnt"].ctypes.data)
        setattr(y, field, None)
        assert L.emqx_rel_expire_host(h._h, ctypes.byref(y), None) == EINVAL, field
    h2 = ctypes.c_void_p()
    assert L.emqx_rel_create(-5, ctypes.byref(h2)) == EINVAL and L.emqx_rel_create(T.HOST_ONLY, None) == EINVAL
    assert L.emqx_rel_destroy(None) == EINVAL


def test_batch_calls_need_a_device(T):
    from emqx_amd import _lib
    h = host(T)
    case = C.RUNS["no_ts_w8"]()
    with pytest.raises(_lib.EngineError) as e:
        h.run(case.subs, case.offsets, case.events, case.table.copy(), case.rel.copy(), **case.host_args())
    assert e.value.code == EDEVICE
    xc = C.EXPIRES["w8"]()
    with pytest.raises(_lib.EngineError) as e:
        h.expire(xc.table.copy(), xc.rel.copy(), **xc.host_args())
    assert e.value.code == EDEVICE
    ra, xa = T.Rel.run_args(0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0, 0, 0), T.Rel.expire_args(0, 0, 0, 0, 0, 16, 0, 0, 0)
    for fn, args in ((h.run_device, ra), (h.expire_device, xa)):
        with pytest.raises(_lib.EngineError) as e:
            fn(args)
        assert e.value.code == EDEVICE
    for fn, args in ((h.run_device_async, ra), (h.expire_device_async, xa)):
        with pytest.raises(_lib.EngineError) as e:
            fn(args, 0)
        assert e.value.code == EDEVICE
    with pytest.raises(_lib.EngineError) as e:
        h.reserve(1000, 1000, 16)
    assert e.value.code == EDEVICE
