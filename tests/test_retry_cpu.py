"""CPU-side checks of the retry stage (include/emqx_retry.h) on a host-only handle: the restatement
(tests/retry_ref.py) against the known answers of the reference's own suite
(tests/golden/retry_kats.json), emqx_retry_sweep_host and emqx_retry_stamp_host against the
restatement on every case, the exports, the refusals and argument errors, and no batch call without a
device."""

import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import retry_cases as C
from tests import retry_ref as R
from tests.ack_cases import records_of, rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "retry_kats.json")))
KATS = GOLDEN["kats"]


@pytest.fixture(scope="module")
def T():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import retry
    return retry


def host(T):
    return T.Retry(T.HOST_ONLY)


def sweep(T, case, update_table=True, cap_out="case", h=None, fn="sweep_host"):
    """One sweep on copies of the case's tables; a bad subscriber's EINVAL and a full call's
    EOVERFLOW carry the outputs."""
    from emqx_amd import _lib
    table, slots, stamps = case.table.copy(), case.slots.copy(), case.stamps.copy()
    cap = case.cap_out if cap_out == "case" else cap_out
    want = case.reference(update_table, cap)["summary"][0]
    try:
        got = getattr(h or host(T), fn)(case.subs, table, slots, stamps, case.now, case.interval, intervals=case.intervals,
                                        deadlines=case.deadlines, mode=case.mode, cap_out=cap, update_table=update_table)
        assert not want & (R.F_BAD_SUB | R.F_OUTPUT_FULL)
    except _lib.EngineError as e:
        assert e.code == (EOVERFLOW if want & R.F_OUTPUT_FULL else EINVAL) and e.summary["flags"] == want
        got = e.partial
    return got, slots, stamps, table


# ---- the restatement against the reference's suite ----------------------------------------------

def play(kat, do_record, do_ack, do_stamp, do_sweep):
    """The steps of a known answer over one session of 8 slots; what the last sweep gave."""
    out = None
    for step in kat["steps"]:
        now = kat["t"] + step[1]
        if step[0] == "record":
            do_record(step[2])
            do_stamp(now)
        elif step[0] == "ack":
            do_ack(step[2])
            do_stamp(now)
        else:
            out = do_sweep(now, step[2])
    return out


def test_kats_cover_the_named_suite_tests():
    assert {k["source"] for k in KATS} == {"emqx_session_SUITE:t_retry", "emqx_session_SUITE:t_replay", "emqx_session:pubrec/2"}
    assert "by hand" in GOLDEN["comment"] and set(GOLDEN) == {"comment", "kats"}


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_ref_against_the_reference_suite(kat):
    from tests import ack_ref
    rows, stamps, recs = [[[0, 0, 0, 0] for _ in range(8)]], [[0] * 8], [dict(inflight=0, inflight_max=0, flags=3)]

    def record(msgs):
        for j, (pkt_id, qos, ref) in enumerate(msgs):
            rows[0][j] = [pkt_id, R.MSG, qos, ref]
        recs[0]["inflight"] += len(msgs)

    def ack(pairs):
        ack_ref.session_acks(rows[0], recs[0], [(k << 16) | i for k, i in pairs])

    out = play(kat, record, ack, lambda now: R.stamp([0], rows, stamps, now),
               lambda now, mode: R.sweep([0], recs, rows, stamps, now, kat["interval"], mode=mode, update_table=True))
    assert out["items"] == kat["items"] and out["timers"] == [kat["timer"]] and out["counts"][0][3] == kat["inflight"]
    assert out["status"] == [R.A_OK] and recs[0]["inflight"] == kat["inflight"]


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_host_against_the_reference_suite(T, kat):
    from emqx_amd import ack, window
    slots, stamps, table = ack.empty_slots(1, 8), T.empty_stamps(1, 8), window.pack_sessions(1, inflight=0, inflight_max=0)
    h, a = host(T), ack.Ack(ack.HOST_ONLY)

    def record(msgs):
        n = len(msgs)
        a.record_host([0], [0, n], [q for _, q, _ in msgs], [window.W_SEND] * n, [i for i, _, _ in msgs], slots, refs=[r for _, _, r in msgs])
        table["inflight"][0] += n

    def acks(pairs):
        a.run_host([0], [0, len(pairs)], ack.pack_acks([k for k, _ in pairs], [i for _, i in pairs]), table, slots, update_table=True)

    out = play(kat, record, acks, lambda now: h.stamp_host([0], slots, stamps, now),
               lambda now, mode: h.sweep_host([0], table, slots, stamps, now, kat["interval"], mode=mode, update_table=True))
    assert [list(map(int, it)) for it in out.items.tolist()] == kat["items"]
    assert out.timers.tolist() == [kat["timer"]] and int(out.counts[0, 3]) == kat["inflight"] == int(table["inflight"][0])


# ---- the ABI ------------------------------------------------------------------------------------

def test_exports_every_retry_symbol(T):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_retry.h")
    assert len(declared) == 13
    assert sorted(_lib.RETRY_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(T):
    import emqx_amd
    assert emqx_amd.Retry is T.Retry


def test_constants_mirror_the_headers(T):
    pub = open(os.path.join(ROOT, "include", "emqx_retry.h")).read()

    def define(name):
        return int(re.search(r"#define EMQX_RETRY_%s \(?(\w+?)(u|ull)?\b" % name, pub).group(1), 0)
    for name in ("MODE_RETRY", "MODE_REPLAY", "PUBLISH_DUP", "PUBREL", "EXPIRED", "NO_TIMER", "NO_EXPIRY", "F_INPUT_REFUSED", "F_BAD_SUB",
                 "F_OUTPUT_FULL", "F_BAD_REF", "F_UNSTAMPED", "SUMMARY_WORDS", "STAMP_TS_SHIFT", "STAMP_PHASE_SHIFT"):
        assert define(name) == getattr(T, name), name
        if hasattr(R, name):
            assert getattr(R, name) == getattr(T, name), name
    assert re.search(r"#define EMQX_RETRY_MAX_INTERVAL \(1ull << 31\)", pub) and T.MAX_INTERVAL == R.MAX_INTERVAL == 1 << 31
    assert re.search(r"#define EMQX_RETRY_MAX_NOW \(1ull << 45\)", pub) and T.MAX_NOW == 1 << 45
    assert re.search(r"#define EMQX_RETRY_STAMP_DUP \(1ull << 18\)", pub) and T.STAMP_DUP == 1 << 18
    assert len(T.SWEEP_SUMMARY) == len(T.STAMP_SUMMARY) == T.SUMMARY_WORDS
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "ack.h")).read()
    assert int(re.search(r"AK_BLOCK = (\d+);", src).group(1)) // (8 // 2) == C.rows_per_block(8)
    from emqx_amd import ack
    assert (R.A_OK, R.A_NO_SESSION, R.A_PASS, R.MSG, R.PUBREL_AWAIT) == (ack.A_OK, ack.A_NO_SESSION, ack.A_PASS, ack.MSG, ack.PUBREL_AWAIT)
    assert T.pack_stamp(5, 1, 2, 0x1234) == R.make_stamp(5, 1, 2, 0x1234) == (5 << 19) | (1 << 18) | (2 << 16) | 0x1234
    assert T.stamp_fields(T.pack_stamp(C.NOW, 0, 1, 65535)) == R.read_stamp(R.make_stamp(C.NOW, 0, 1, 65535)) == (C.NOW, 0, 1, 65535)
    it = np.zeros(1, dtype=T.ITEM)
    it[0] = (0x1234, 2, 1, 0xAABBCCDD)
    assert it.tobytes() == bytes([0x34, 0x12, 2, 1, 0xDD, 0xCC, 0xBB, 0xAA])
    assert T.deadline(1000, 2) == 3000 and T.deadline(1000, None) == T.NO_EXPIRY


def test_batch_calls_need_a_device(T):
    from emqx_amd import _lib
    h = host(T)
    case = C.SWEEPS["one_item"]()
    for call in (lambda: h.sweep(case.subs, case.table.copy(), case.slots.copy(), case.stamps.copy(), case.now, 100),
                 lambda: h.stamp(case.subs, case.slots, case.stamps.copy(), case.now),
                 lambda: h.stamp_device(T.Retry.stamp_args(0, 0, 0, 0, 0, 8, 0, 0)),
                 lambda: h.sweep_device(T.Retry.sweep_args(0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0, 0)),
                 lambda: h.stamp_device_async(T.Retry.stamp_args(0, 0, 0, 0, 0, 8, 0, 0), 0),
                 lambda: h.sweep_device_async(T.Retry.sweep_args(0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0, 0), 0),
                 lambda: h.reserve(1000, 16)):
        with pytest.raises(_lib.EngineError) as e:
            call()
        assert e.value.code == EDEVICE


# ---- the sweep's host evaluator against the restatement -----------------------------------------

@pytest.mark.parametrize("name", list(C.SWEEPS))
@pytest.mark.parametrize("update_table", [False, True], ids=["keep_table", "update_table"])
def test_sweep_cases(T, name, update_table):
    case = C.SWEEPS[name]()
    got, slots, stamps, table = sweep(T, case, update_table)
    C.check(case.reference(update_table), got, slots, stamps, table)
    if not update_table:
        assert table.tobytes() == case.table.tobytes()


def test_cases_mean_what_their_names_say():
    def one(name, k=0):
        case = C.SWEEPS[name]()
        ref = case.reference()
        lo, hi = ref["offsets"][k], ref["offsets"][k + 1]
        return ref["items"][lo:hi], ref["counts"][k], ref["timers"][k], ref, case
    assert one("empty_row")[:3] == ([], [0, 0, 0, 5], R.NO_TIMER)
    assert one("one_item")[:3] == ([[7, R.PUBLISH_DUP, 1, 40]], [1, 0, 0, 5], 100)
    items, counts, timer, _, _ = one("ages_interval-1_interval_interval+1_future")
    assert [it[0] for it in items] == [3, 2] and timer == 100 - 99, "age interval + 1 first, then interval; the youngest is 99 old"
    items, _, timer, _, _ = one("interval_0")
    assert [it[0] for it in items] == [2, 1] and timer == 0, "a future stamp is young"
    items, _, _, _, _ = one("tie_ids_1_and_65535")
    assert [it[0] for it in items] == [2, 1, 300, 65535] and items[2][1] == R.PUBREL
    ref = one("intervals_override_the_call")[3]
    assert ref["counts"] == [[1, 0, 0, 5], [0, 0, 0, 5], [0, 0, 0, 5]] and ref["timers"] == [50, 950, 1]
    items, counts, timer, ref, case = one("deadlines_now-1_now_now+1_never_pubrel")
    assert [(it[0], it[1]) for it in items] == [(10, 3), (11, 1), (12, 1), (13, 1), (14, 2)] and counts == [3, 1, 1, 4] and timer == 90
    assert case.deadlines.tolist()[:4] == [C.NOW - 1, C.NOW, C.NOW + 1, R.NO_TIMER << 32 | R.NO_TIMER]
    items, counts, timer, ref, case = one("every_old_entry_expired")
    assert counts == [0, 0, 2, 0] and timer == 100 and [it[0] for it in items] == [2, 1] and ref["inflight"][int(case.subs[0])] == 0
    assert one("expired_below_inflight_0")[1] == [0, 0, 1, 0]
    for name, st in (("not_present", R.A_NO_SESSION), ("pass", R.A_PASS)):
        items, counts, timer, ref, case = one(name)
        assert ref["status"] == [st, R.A_OK] and (items, counts, timer) == ([], [0, 0, 0, 0], R.NO_TIMER)
        assert ref["rows"] == C.rows_of(case.slots) or ref["summary"][3] == 1
    _, _, _, ref, case = one("sub_at_sub_limit")
    assert int(case.subs[1]) == case.sub_limit and ref["summary"][0] == R.F_BAD_SUB and ref["status"] == [1, R.A_NO_SESSION, 1]
    items, counts, _, ref, _ = one("ref_at_ref_limit")
    assert ref["summary"][0] == R.F_BAD_REF and [(it[0], it[1]) for it in items] == [(1, 1), (2, 3), (3, 2)]
    _, counts, timer, ref, case = one("unstamped_slot")
    assert ref["summary"][0] == R.F_UNSTAMPED and ref["summary"][7] == 2 and counts == [1, 0, 0, 5] and timer == 100
    assert ref["counts"][1] == [0, 1, 0, 5] and R.read_stamp(ref["stamps"][int(case.subs[0])][0]) == (C.NOW, 0, R.MSG, 1)
    _, counts, _, ref, case = one("stamp_of_another_id_or_phase")
    assert counts == [1, 0, 0, 5] and ref["summary"][7] == 2 and ref["stamps"][int(case.subs[0])][5] == int(case.stamps[int(case.subs[0]), 5])
    items, _, _, _, _ = one("id_held_twice")
    assert [(it[0], it[3]) for it in items] == [(5, 3), (4, 2), (5, 0), (5, 1)]
    _, _, _, ref, case = one("subs_null_whole_table")
    assert case.subs is None and ref["status"] == [1, 1, 1, R.A_NO_SESSION] and ref["timers"] == [100, R.NO_TIMER, 95, R.NO_TIMER]
    items, counts, timer, ref, case = one("replay")
    assert [(it[0], it[1]) for it in items] == [(1, 1), (2, 2), (65535, 1)] and timer == R.NO_TIMER and ref["summary"][0] == 0
    assert ref["rows"] == C.rows_of(case.slots) and ref["stamps"] == case.stamps.tolist()
    for w in C.WIDTHS:
        items, counts, timer, ref, _ = one("full_row_tie_w%d" % w)
        assert [it[0] for it in items] == list(range(1, w + 1)) and counts[0] == w and timer == 100
        assert ref["counts"][2][0] == 0 and ref["timers"][2] == 1
        items = one("full_row_descending_ts_w%d" % w)[0]
        assert len(items) == w and len({it[0] for it in items}) == w


def test_fuzz(T):
    case = C.fuzz()
    ref = case.reference(True)
    assert ref["summary"][0] == R.F_BAD_SUB | R.F_BAD_REF | R.F_UNSTAMPED and case.m == 2500 and min(ref["summary"][1:]) > 50
    got, slots, stamps, table = sweep(T, case, True)
    C.check(ref, got, slots, stamps, table)
    assert table.tobytes() != case.table.tobytes() and slots.tobytes() != case.slots.tobytes()
    replay = C.fuzz(mode=R.MODE_REPLAY, n_sessions=300)
    got, slots, stamps, table = sweep(T, replay, True)
    C.check(replay.reference(True), got, slots, stamps, table)
    assert (slots.tobytes(), stamps.tobytes(), table.tobytes()) == (replay.slots.tobytes(), replay.stamps.tobytes(), replay.table.tobytes())


def test_a_second_sweep_at_the_same_now_finds_nothing_due(T):
    case = C.fuzz(seed=5, n_sessions=200)
    h = host(T)
    _, slots, stamps, table = sweep(T, case, True)
    recs, rows, st = records_of(table), rows_of(slots), stamps.tolist()
    # interval 0 sessions aside, everything was restamped `now`
    second = R.sweep(case.subs.tolist(), recs, rows, st, case.now, case.interval, case.intervals.tolist(), case.expiry, update_table=True)
    from emqx_amd import _lib
    try:
        got = h.sweep_host(case.subs, table, slots, stamps, case.now, case.interval, intervals=case.intervals, deadlines=case.deadlines,
                           update_table=True)
    except _lib.EngineError as e:
        got = e.partial
    assert got.offsets.tolist() == second["offsets"] and got.timers.tolist() == second["timers"] and got.summary["unstamped"] == 0
    assert rows_of(slots) == rows and stamps.tolist() == st


def test_overflow_changes_nothing_and_the_repeat_succeeds(T):
    case = C.overflow_case()
    need = case.reference()["summary"][3]
    assert need == 5 and case.reference()["summary"][6] == 2  # ref 0 is past its deadline in two sessions
    ref = case.reference(True, need - 1)
    assert ref["summary"][0] == R.F_OUTPUT_FULL and ref["items"] == [] and ref["offsets"][-1] == need
    got, slots, stamps, table = sweep(T, case, True, cap_out=need - 1)
    C.check(ref, got, slots, stamps, table)
    assert (slots.tobytes(), stamps.tobytes(), table.tobytes()) == (case.slots.tobytes(), case.stamps.tobytes(), case.table.tobytes())
    assert got.summary["items"] == need and got.counts.tolist() == case.reference()["counts"]
    got, slots, stamps, table = sweep(T, case, True, cap_out=need)
    C.check(case.reference(True, need), got, slots, stamps, table)


# ---- the stamp call's host evaluator against the restatement ------------------------------------

def stamp(T, case, fn="stamp_host", h=None):
    from emqx_amd import _lib
    stamps = case.stamps.copy()
    try:
        got = getattr(h or host(T), fn)(case.subs, case.slots, stamps, case.now)
        assert not case.reference()["summary"][0]
    except _lib.EngineError as e:
        assert e.code == EINVAL and e.summary["flags"] == R.F_BAD_SUB
        got = e.partial
    return got, stamps


@pytest.mark.parametrize("name", list(C.STAMPS))
def test_stamp_cases(T, name):
    case = C.STAMPS[name]()
    got, stamps = stamp(T, case)
    C.check_stamp(case.reference(), got, stamps)


def test_stamp_case_means_what_its_name_says():
    case = C.STAMPS["mixed"]()
    ref = case.reference()
    sub = int(case.subs[0])
    after = [R.read_stamp(s) for s in ref["stamps"][sub]]
    assert after[0] == (C.NOW, 0, R.MSG, 1), "an insert"
    assert after[1] == (C.NOW, 0, R.PUBREL_AWAIT, 2), "the PUBREC's new stamp"
    assert after[2] == (C.NOW - 40, 1, R.MSG, 3), "unchanged, dup kept"
    assert ref["stamps"][sub][3] == 0 and case.stamps[sub, 3] != 0, "freed"
    assert after[4] == (C.NOW, 0, R.MSG, 5), "freed and refilled with another id"
    assert after[5] == (C.NOW - 40, 1, R.MSG, 6)
    assert ref["summary"] == [R.F_BAD_SUB, 2, 3, 3, 1, 0, 0, 0]
    other = int(case.subs[2])
    assert ref["stamps"][other] == case.stamps[other].tolist()
    # a slot freed and refilled with the same id and phase between two stamp calls keeps its stamp
    rows, stamps = [[[6, R.MSG, 1, 99]]], [[R.make_stamp(C.NOW - 40, 1, R.MSG, 6)]]
    assert R.stamp([0], rows, stamps, C.NOW)[3:5] == [0, 0] and R.read_stamp(stamps[0][0])[0] == C.NOW - 40


# ---- refusals and argument errors ---------------------------------------------------------------

def _sweep_args(T, case, **over):
    from emqx_amd import _lib
    keep = {"subs": case.subs.copy(), "table": case.table.copy(), "slots": case.slots.copy(), "stamps": case.stamps.copy(),
            "off": np.zeros(case.m + 2, dtype=np.uint64), "items": np.zeros(case.m * case.w + 1, dtype=T.ITEM),
            "status": np.zeros(case.m + 1, dtype=np.uint8), "cnt": np.zeros((case.m + 1, 4), dtype=np.uint32),
            "timers": np.zeros(case.m + 1, dtype=np.uint32)}
    p = lambda a: a.ctypes.data  # noqa: E731
    kw = dict(subs=p(keep["subs"]), n_boxes=None, m=case.m, cap_boxes=case.m, sessions=p(keep["table"]), sub_limit=case.sub_limit,
              update_table=1, slots=p(keep["slots"]), stamps=p(keep["stamps"]), w=case.w, now_ms=case.now, interval_ms=case.interval,
              intervals=None, deadlines=None, ref_limit=0, mode=0, cap_out=case.m * case.w, out_offsets=p(keep["off"]),
              out_items=p(keep["items"]), out_status=p(keep["status"]), out_counts=p(keep["cnt"]), out_timers=p(keep["timers"]))
    kw.update(over)
    return _lib.RetrySweepArgs(**kw), keep


SWEEP_ERRORS = {"no_sessions": dict(sessions=None), "no_slots": dict(slots=None), "no_stamps": dict(stamps=None),
                "no_out_offsets": dict(out_offsets=None), "no_out_items": dict(out_items=None), "no_out_status": dict(out_status=None),
                "no_out_counts": dict(out_counts=None), "no_out_timers": dict(out_timers=None), "m_over_cap_boxes": dict(cap_boxes=1),
                "cap_boxes_over": dict(cap_boxes=1 << 32), "sub_limit_over": dict(sub_limit=(1 << 32) + 1), "mode_2": dict(mode=2),
                "interval_over": dict(interval_ms=(1 << 31) + 1), "now_over": dict(now_ms=1 << 45),
                "w_0": dict(w=0), "w_12": dict(w=12), "w_4": dict(w=4), "w_128": dict(w=128)}


@pytest.mark.parametrize("what", list(SWEEP_ERRORS))
def test_sweep_argument_errors(T, what):
    from emqx_amd import _lib
    case = C.overflow_case()
    b, keep = _sweep_args(T, case, **SWEEP_ERRORS[what])
    summary = np.full(8, 77, dtype=np.uint64)
    assert _lib.lib().emqx_retry_sweep_host(host(T)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert not keep["status"].any() and not keep["cnt"].any() and not keep["off"].any() and (summary == 77).all()
    assert (keep["slots"].tobytes(), keep["stamps"].tobytes(), keep["table"].tobytes()) == (
        case.slots.tobytes(), case.stamps.tobytes(), case.table.tobytes())
    assert _lib.lib().emqx_retry_sweep_host(None, ctypes.byref(b), None) == EINVAL


def test_replay_takes_no_stamps_and_the_largest_interval_is_taken(T):
    from emqx_amd import _lib
    case = C.overflow_case()
    b, keep = _sweep_args(T, case, stamps=None, mode=1)
    assert _lib.lib().emqx_retry_sweep_host(host(T)._h, ctypes.byref(b), None) == 0 and keep["off"][case.m] == 6
    b, keep = _sweep_args(T, case, interval_ms=1 << 31)
    assert _lib.lib().emqx_retry_sweep_host(host(T)._h, ctypes.byref(b), None) == 0
    assert keep["off"][case.m] == 0 and keep["timers"][:case.m].tolist() == [(1 << 31) - 300, (1 << 31) - 200, (1 << 31) - 100]


def test_stamp_argument_errors(T):
    from emqx_amd import _lib
    case = C.STAMPS["mixed"]()
    p = lambda a: a.ctypes.data  # noqa: E731
    for over in (dict(slots=None), dict(stamps=None), dict(w=24), dict(now_ms=1 << 45), dict(cap_boxes=2)):
        stamps = case.stamps.copy()
        kw = dict(subs=p(case.subs), n_boxes=None, m=case.m, cap_boxes=case.m, slots=p(case.slots), stamps=p(stamps), w=case.w,
                  sub_limit=case.sub_limit, now_ms=case.now)
        kw.update(over)
        summary = np.full(8, 77, dtype=np.uint64)
        assert _lib.lib().emqx_retry_stamp_host(host(T)._h, ctypes.byref(_lib.RetryStampArgs(**kw)), summary.ctypes.data) == EINVAL
        assert stamps.tobytes() == case.stamps.tobytes() and (summary == 77).all()


def test_refused_input_writes_only_the_summary(T):
    from emqx_amd import _lib
    case = C.overflow_case()
    count = np.array([case.m + 1], dtype=np.uint64)
    b, keep = _sweep_args(T, case, n_boxes=count.ctypes.data, m=0)
    summary = np.zeros(8, dtype=np.uint64)
    assert _lib.lib().emqx_retry_sweep_host(host(T)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [R.F_INPUT_REFUSED, 0, case.m + 1, 0, 0, 0, 0, 0] and not keep["off"].any() and not keep["status"].any()
    assert keep["stamps"].tobytes() == case.stamps.tobytes()
    count[0] = case.m
    assert _lib.lib().emqx_retry_sweep_host(host(T)._h, ctypes.byref(b), summary.ctypes.data) == 0
    assert keep["off"][:case.m + 1].tolist() == case.reference()["offsets"] and keep["off"][case.m + 1] == 0
    # subs NULL names the sessions 0..m-1: more than sub_limit of them is refused
    b, keep = _sweep_args(T, case, subs=None, m=case.sub_limit + 1, cap_boxes=case.sub_limit + 1)
    assert _lib.lib().emqx_retry_sweep_host(host(T)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [R.F_INPUT_REFUSED, 0, case.sub_limit + 1, 0, 0, 0, 0, 0]
    assert R.sweep(None, [], [[]] * case.sub_limit, [], 0, cap_boxes=case.sub_limit - 1)["summary"][0] == R.F_INPUT_REFUSED


def test_tuning_keys(T):
    from emqx_amd import _lib
    from tests.test_ack_cpu import _grid_keys
    h = host(T)
    with pytest.raises(_lib.EngineError) as e:
        h.set_tuning("rematch", 1)
    assert e.value.code == ENOTFOUND
    case = C.overflow_case()
    before = sweep(T, case, h=h)
    _grid_keys(h, 4096)
    after = sweep(T, case, h=h)
    C.same(after[0], before[0])
    assert [x.tobytes() for x in after[1:]] == [x.tobytes() for x in before[1:]]


def test_stats_struct_is_versioned_by_size(T):
    from emqx_amd import _lib
    h = host(T)
    sweep(T, C.overflow_case(), h=h)
    s = _lib.RetryStats()
    s.size = 16
    s.w = 12345
    assert _lib.lib().emqx_retry_stats_get(h._h, ctypes.byref(s)) == 0
    assert s.size == 16 and s.cap_boxes == 0 and s.w == 12345  # nothing beyond 16 bytes written
    assert h.stats()["calls"] == 1
    s.size = 4
    assert _lib.lib().emqx_retry_stats_get(h._h, ctypes.byref(s)) == EINVAL
