"""CPU-side checks of the mqueue stage (include/emqx_mqueue.h) on a host-only handle: the restatement
(tests/mqueue_ref.py) against the known answers of the reference's own suites
(tests/golden/mqueue_kats.json), emqx_mqueue_put_host and emqx_mqueue_take_host against the
restatement on every case, the exports, the refusals and argument errors, and no batch call without a
device."""

import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mqueue_cases as C
from tests import mqueue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "mqueue_kats.json")))
PUT_CASES = C.put_cases()
TAKE_CASES = C.take_cases()


@pytest.fixture(scope="module")
def T():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import mqueue
    return mqueue


def host(T):
    return T.Mqueue(T.HOST_ONLY)


def put(T, case, h=None, fn="put_host"):
    """One put on copies of the case's tables; a bad subscriber's EINVAL carries the outputs."""
    from emqx_amd import _lib
    ring, heads = case.ring.copy(), case.heads.copy()
    sessions = None if case.sessions is None else case.sessions.copy()
    want = case.reference()[0]["summary"][0]
    try:
        got = getattr(h or host(T), fn)(case.subs, case.offsets, case.opts, case.verdicts, ring, heads, refs=case.refs, sessions=sessions)
        assert not want & R.F_BAD_SUB
    except _lib.EngineError as e:
        assert e.code == EINVAL and want & R.F_BAD_SUB and e.summary["flags"] == want
        got = e.partial
    if sessions is not None:
        assert sessions.tobytes() == case.sessions.tobytes()  # read only
    return got, ring, heads


def take(T, case, update_table=True, cap_out="case", h=None, fn="take_host"):
    """One take on copies of the case's tables; a bad subscriber's EINVAL and a full call's
    EOVERFLOW carry the outputs."""
    from emqx_amd import _lib
    sessions, ring, heads = case.sessions.copy(), case.ring.copy(), case.heads.copy()
    cap = case.cap_out if cap_out == "case" else cap_out
    want = case.reference(update_table, cap)[0]["summary"][0]
    try:
        got = getattr(h or host(T), fn)(case.subs, sessions, ring, heads, case.now, deadlines=case.deadlines, cap_out=cap,
                                        update_table=update_table)
        assert not want & (R.F_BAD_SUB | R.F_OUTPUT_FULL)
    except _lib.EngineError as e:
        assert e.code == (EOVERFLOW if want & R.F_OUTPUT_FULL else EINVAL) and e.summary["flags"] == want
        got = e.partial
    return got, sessions, heads, ring


# ---- the restatement against the reference's suites ---------------------------------------------

def test_kats_cover_the_named_suite_tests():
    assert {k["source"] for k in GOLDEN["mqueue"]} == {"emqx_mqueue_SUITE:" + t for t in (
        "t_in", "t_in_qos0", "t_out", "t_simple_mqueue", "t_infinity_simple_mqueue", "t_dropped")}
    assert {k["source"] for k in GOLDEN["session"]} == {"emqx_session_SUITE:" + t for t in (
        "t_dequeue", "t_puback_with_dequeue", "t_enqueue", "t_deliver_when_inflight_is_full")}
    assert "by hand" in GOLDEN["comment"] and set(GOLDEN) == {"comment", "mqueue", "session"}


@pytest.mark.parametrize("kat", GOLDEN["mqueue"], ids=[k["name"] for k in GOLDEN["mqueue"]])
def test_ref_queue_against_the_reference_suite(kat):
    mq = R.MQ(max_len=kat["max_len"], store_qos0=kat["store_qos0"])
    for step in kat["steps"]:
        if step[0] == "in":
            dropped = R.mq_in((step[2], step[1]), mq)
            if step[3] != "any":
                assert (None if dropped is None else dropped[0]) == step[3]
        elif step[0] == "in_seq":
            for ref in range(step[2], step[3] + 1):
                R.mq_in((ref, step[1]), mq)
        elif step[0] == "out":
            msg = R.mq_out(mq)
            assert (None if msg is None else msg[0]) == step[1]
        elif step[0] == "len":
            assert len(mq) == step[1]
        elif step[0] == "empty":
            assert (len(mq) == 0) == step[1]
        else:
            assert step[0] == "stats" and [len(mq), mq.max_len, mq.dropped] == step[1:]


def play_session(kat, enqueue, deliver, puback, dequeue, info):
    for step in kat["steps"]:
        if step[0] == "enqueue":
            enqueue(step[1])
        elif step[0] == "deliver":
            assert deliver(step[1]) == step[2]
        elif step[0] == "puback":
            puback(step[1])
        elif step[0] == "dequeue":
            got = dequeue()
            assert len(got) == len(step[1])
            for (pid, ref), (want_pid, want_ref) in zip(got, step[1]):
                assert ref == want_ref and (want_pid == "any" or pid == want_pid)
        else:
            assert step[0] == "info" and list(info()) == step[1:]


@pytest.mark.parametrize("kat", GOLDEN["session"], ids=[k["name"] for k in GOLDEN["session"]])
def test_ref_session_against_the_reference_suite(kat):
    mq = R.MQ(max_len=kat["max_len"], store_qos0=kat["store_qos0"])
    sess = dict(inflight=kat["inflight"], inflight_max=kat["inflight_max"], next_pkt_id=1)

    def enqueue(msgs):
        for qos, ref in msgs:
            R.mq_in((ref, qos), mq)

    def deliver(msgs):
        return sum(1 for qos, ref in msgs if R.deliver_msg((ref, qos), sess, mq) is not None)

    def puback(_pkt_id):
        sess["inflight"] -= 1

    def dequeue():
        return [(None if v == R.W_SEND_QOS0 else pid, msg[0]) for v, pid, msg in R.session_dequeue(sess, mq, lambda m: False)]

    play_session(kat, enqueue, deliver, puback, dequeue, lambda: (len(mq), sess["inflight"]))


@pytest.mark.parametrize("kat", GOLDEN["session"], ids=[k["name"] for k in GOLDEN["session"]])
def test_host_against_the_reference_suite(T, kat):
    """The same steps through the window stage's and this stage's host calls on one session."""
    from emqx_amd import window
    flags = window.PRESENT | (window.STORE_QOS0 if kat["store_qos0"] else 0)
    table = window.pack_sessions(1, inflight=kat["inflight"], inflight_max=kat["inflight_max"], mq_max=kat["max_len"], flags=flags)
    ring, heads = T.empty_ring(1, 1024), T.empty_heads(1)
    h, w = host(T), window.Window(window.HOST_ONLY)

    def admit(msgs, connected):
        table["flags"][0] = flags | (window.CONNECTED if connected else 0)
        opts = [qos for qos, _ in msgs]
        a = w.run_host([0], [0, len(msgs)], opts, table, update_table=True)
        h.put_host([0], [0, len(msgs)], opts, a.verdicts, ring, heads, refs=[ref for _, ref in msgs], sessions=table)
        return int(a.counts[0, 0])

    def dequeue():
        t = h.take_host([0], table, ring, heads, update_table=True)
        return [(None if v == window.W_SEND_QOS0 else int(p), int(r)) for v, p, r in zip(t.verdicts, t.pkt_ids, t.refs)]

    def puback(_pkt_id):
        table["inflight"][0] -= 1

    play_session(kat, lambda msgs: admit(msgs, False), lambda msgs: admit(msgs, True), puback, dequeue,
                 lambda: (int(heads["len"][0]), int(table["inflight"][0])))
    assert int(table["mq_len"][0]) == int(heads["len"][0])


# ---- the ABI ------------------------------------------------------------------------------------

def test_exports_every_mqueue_symbol(T):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_mqueue.h")
    assert len(declared) == 13
    assert sorted(_lib.MQUEUE_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(T):
    import emqx_amd
    assert emqx_amd.Mqueue is T.Mqueue


def test_struct_sizes_and_constants(T):
    from emqx_amd import _lib
    assert T.ENTRY.itemsize == 8 and T.RING.itemsize == 8 and T.ENTRY.fields["opts"][1] == 4
    assert ctypes.sizeof(_lib.MqueuePutArgs) == 16 * 8 and ctypes.sizeof(_lib.MqueueTakeArgs) == 21 * 8
    assert ctypes.sizeof(_lib.MqueueStats) == 48
    header = open(os.path.join(ROOT, "include", "emqx_mqueue.h")).read()
    for name, value in (("EMQX_MQ_EXPIRED", T.EXPIRED), ("EMQX_MQ_NO_REF", T.NO_REF), ("EMQX_MQ_MIN_Q", T.MIN_Q), ("EMQX_MQ_MAX_Q", T.MAX_Q),
                        ("EMQX_MQ_F_INPUT_REFUSED", T.F_INPUT_REFUSED), ("EMQX_MQ_F_BAD_SUB", T.F_BAD_SUB),
                        ("EMQX_MQ_F_OUTPUT_FULL", T.F_OUTPUT_FULL), ("EMQX_MQ_F_BAD_REF", T.F_BAD_REF),
                        ("EMQX_MQ_F_BAD_RING", T.F_BAD_RING), ("EMQX_MQ_F_ROW_FULL", T.F_ROW_FULL),
                        ("EMQX_MQ_F_LEN_MISMATCH", T.F_LEN_MISMATCH)):
        m = re.search(r"#define %s (\S+?)u\b" % name, header)
        assert m and int(m.group(1), 0) == value, name
    assert T.TILE == C.TILE
    s = host(T).stats()
    assert set(s) == {"cap_in", "cap_boxes", "scratch_bytes", "calls", "last_call_ms"} and s["calls"] == 0
    short = _lib.MqueueStats()
    short.size = 16
    h = host(T)
    assert _lib.lib().emqx_mqueue_stats_get(h._h, ctypes.byref(short)) == 0 and short.size == 16
    short.size = 4
    assert _lib.lib().emqx_mqueue_stats_get(h._h, ctypes.byref(short)) == EINVAL


def _put_args(T, q=8, **kw):
    from emqx_amd import _lib
    keep = dict(subs=np.zeros(1, np.uint32), off=np.array([0, 1], np.uint64), opts=np.ones(1, np.uint8),
                ver=np.full(1, 3, np.uint8), ring=T.empty_ring(2, 1024), heads=T.empty_heads(2), ev=np.zeros(1, T.ENTRY),
                un=np.zeros(1, np.uint32))
    b = _lib.MqueuePutArgs(inbox_subs=keep["subs"].ctypes.data, inbox_offsets=keep["off"].ctypes.data, box_opts=keep["opts"].ctypes.data,
                           n_boxes=None, m=1, cap_in=1, cap_boxes=1, verdicts=keep["ver"].ctypes.data, refs=None, sessions=None,
                           ring=keep["ring"].ctypes.data, heads=keep["heads"].ctypes.data, q=q, sub_limit=2,
                           out_evicted=keep["ev"].ctypes.data, out_unstored=keep["un"].ctypes.data)
    for k, v in kw.items():
        setattr(b, k, v)
    return b, keep


def _take_args(T, q=8, **kw):
    from emqx_amd import _lib, window
    keep = dict(subs=np.zeros(1, np.uint32), tab=window.pack_sessions(2), ring=T.empty_ring(2, 1024), heads=T.empty_heads(2),
                off=np.zeros(2, np.uint64), o=np.zeros(8, np.uint8), v=np.zeros(8, np.uint8), p=np.zeros(8, np.uint16),
                r=np.zeros(8, np.uint32), st=np.zeros(1, np.uint8), cnt=np.zeros(4, np.uint32))
    b = _lib.MqueueTakeArgs(subs=keep["subs"].ctypes.data, n_boxes=None, m=1, cap_boxes=1, sessions=keep["tab"].ctypes.data, sub_limit=2,
                            update_table=0, ring=keep["ring"].ctypes.data, heads=keep["heads"].ctypes.data, q=q, now_ms=5,
                            deadlines=None, ref_limit=0, cap_out=8, out_offsets=keep["off"].ctypes.data, out_opts=keep["o"].ctypes.data,
                            out_verdicts=keep["v"].ctypes.data, out_pkt_ids=keep["p"].ctypes.data, out_refs=keep["r"].ctypes.data,
                            out_status=keep["st"].ctypes.data, out_counts=keep["cnt"].ctypes.data)
    for k, v in kw.items():
        setattr(b, k, v)
    return b, keep


def test_argument_errors(T):
    from emqx_amd import _lib
    L, h = _lib.lib(), host(T)
    ok, keep = _put_args(T)
    assert L.emqx_mqueue_put_host(h._h, ctypes.byref(ok), None) == 0
    for q in (0, 4, 12, 2048, 7):
        b, keep = _put_args(T, q=q)
        assert L.emqx_mqueue_put_host(h._h, ctypes.byref(b), None) == EINVAL, q
        b, keep = _take_args(T, q=q)
        assert L.emqx_mqueue_take_host(h._h, ctypes.byref(b), None) == EINVAL, q
    for q in (8, 16, 64, 1024):
        b, keep = _take_args(T, q=q)
        assert L.emqx_mqueue_take_host(h._h, ctypes.byref(b), None) == 0, q
    for field in ("inbox_offsets", "inbox_subs", "verdicts", "box_opts", "ring", "heads", "out_evicted", "out_unstored"):
        b, keep = _put_args(T, **{field: None})
        assert L.emqx_mqueue_put_host(h._h, ctypes.byref(b), None) == EINVAL, field
    for field in ("sessions", "ring", "heads", "out_offsets", "out_opts", "out_verdicts", "out_pkt_ids", "out_refs", "out_status",
                  "out_counts"):
        b, keep = _take_args(T, **{field: None})
        assert L.emqx_mqueue_take_host(h._h, ctypes.byref(b), None) == EINVAL, field
    b, keep = _take_args(T, now_ms=1 << 45)
    assert L.emqx_mqueue_take_host(h._h, ctypes.byref(b), None) == EINVAL
    b, keep = _put_args(T, m=2)
    assert L.emqx_mqueue_put_host(h._h, ctypes.byref(b), None) == EINVAL  # m > cap_boxes
    assert L.emqx_mqueue_put_host(None, ctypes.byref(ok), None) == EINVAL and L.emqx_mqueue_put_host(h._h, None, None) == EINVAL
    # a refused input: the counts read from memory
    summary = np.zeros(8, np.uint64)
    n = np.array([3], np.uint64)
    b, keep = _put_args(T, n_boxes=n.ctypes.data)
    assert L.emqx_mqueue_put_host(h._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [T.F_INPUT_REFUSED, 0, 3, 0, 0, 0, 0, 0]
    b, keep = _put_args(T, cap_in=0)
    b.box_opts = keep["opts"].ctypes.data
    assert L.emqx_mqueue_put_host(h._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [T.F_INPUT_REFUSED, 1, 1, 0, 0, 0, 0, 0]
    b, keep = _take_args(T, subs=None, m=3, cap_boxes=3)
    assert L.emqx_mqueue_take_host(h._h, ctypes.byref(b), summary.ctypes.data) == EINVAL  # subs NULL and m > sub_limit
    assert summary.tolist() == [T.F_INPUT_REFUSED, 0, 3, 0, 0, 0, 0, 0]


def test_tuning_keys(T):
    h = host(T)
    from emqx_amd import _lib
    for key, hi in (("max_blocks", 4096), ("scan_chunk", 1024)):
        h.set_tuning(key, 1)
        h.set_tuning(key, hi)
        for bad in (0, hi + 1, -1):
            with pytest.raises(_lib.EngineError) as e:
                h.set_tuning(key, bad)
            assert e.value.code == EINVAL
    with pytest.raises(_lib.EngineError) as e:
        h.set_tuning("rematch", 1)
    assert e.value.code == ENOTFOUND


def test_host_only_handle_has_no_batch_calls(T):
    from emqx_amd import _lib
    L, h = _lib.lib(), host(T)
    p, keep = _put_args(T)
    t, keep2 = _take_args(T)
    s = np.zeros(8, np.uint64)
    assert L.emqx_mqueue_reserve(h._h, 10, 10) == EDEVICE
    for fn, b in ((L.emqx_mqueue_put_batch, p), (L.emqx_mqueue_take_batch, t)):
        assert fn(h._h, ctypes.byref(b), None) == EDEVICE
    for fn, b in ((L.emqx_mqueue_put_batch_device, p), (L.emqx_mqueue_put_batch_device_async, p),
                  (L.emqx_mqueue_take_batch_device, t), (L.emqx_mqueue_take_batch_device_async, t)):
        assert fn(h._h, ctypes.byref(b), s.ctypes.data, None) == EDEVICE


# ---- the host evaluator against the restatement --------------------------------------------------

@pytest.mark.parametrize("case", PUT_CASES, ids=[c.name for c in PUT_CASES])
def test_put_host_against_the_restatement(T, case):
    got, ring, heads = put(T, case)
    C.check_put(case.reference(), got, ring, heads)


def test_put_cases_reach_what_they_name():
    by = {c.name: c.reference()[0] for c in PUT_CASES}
    assert by["full_row_evicts"]["summary"][3:5] == [3, 3] and [e[0] for e in by["full_row_evicts"]["evicted"]] == [100, 101, 102]
    assert by["full_row_evicts_all"]["summary"][3:5] == [8, 8]
    assert by["more_than_max"]["summary"][3:5] == [4, 2] and by["more_than_max"]["evicted"][2:5] == [[100, 1], [101, 1], [R.NO_REF, 0]]
    # (the window counted 11 where the row holds 8: the record and the ring disagree from here on)
    assert by["beyond_max_row_full"]["summary"][0] == R.F_ROW_FULL | R.F_LEN_MISMATCH and by["beyond_max_row_full"]["unstored"] == [3]
    assert by["no_queued"]["summary"][3] == 0 and by["connected_window_full"]["summary"][3] > 0
    assert by["bad_sub"]["summary"][0] == R.F_BAD_SUB and by["bad_sub"]["unstored"] == [0, 2]
    assert by["bad_ring_header"]["summary"][0] == R.F_BAD_RING
    assert by["len_mismatch"]["summary"][0] == R.F_LEN_MISMATCH and by["len_mismatch"]["summary"][7] == 1
    assert by["one_inbox_has_all"]["summary"][1] > 2 * C.TILE and by["one_inbox_has_all"]["summary"][4] == 900
    for name in ("random_q8", "random_q64"):
        assert by[name]["summary"][3] > 100 and by[name]["summary"][4] > 20 and by[name]["summary"][0] & R.F_ROW_FULL


@pytest.mark.parametrize("update_table", [True, False])
@pytest.mark.parametrize("case", TAKE_CASES, ids=[c.name for c in TAKE_CASES])
def test_take_host_against_the_restatement(T, case, update_table):
    got, sessions, heads, ring = take(T, case, update_table)
    C.check_take(case.reference(update_table), got, sessions, heads, ring, case)


def test_take_cases_reach_what_they_name():
    by = {c.name: c.reference()[0] for c in TAKE_CASES}
    assert by["budget_zero_qos0_head"]["summary"][3] == 0
    assert by["budget_ends_at_last"]["counts"] == [[2, 1, 0, 0]]
    assert by["trailing_qos0_stays"]["counts"] == [[2, 0, 0, 2]]
    assert by["fewer_than_budget"]["counts"] == [[1, 2, 0, 0]]
    assert by["all_expired"]["counts"] == [[0, 0, 3, 0]]
    assert by["expired_between_counting"]["counts"] == [[3, 0, 2, 1]]
    assert by["expired_head_budget_zero"]["summary"][3] == 0
    assert by["unbounded_window"]["counts"][0][0] == 1000
    assert by["inflight_above_max"]["summary"][3] == 0
    assert by["ids_wrap"]["pkt_ids"] == [65534, 65535, 1, 2, 3]
    assert by["pass_absent_bad_sub"]["status"] == [R.A_PASS, R.A_NO_SESSION, R.A_NO_SESSION, R.A_OK]
    assert by["pass_absent_bad_sub"]["summary"][0] == R.F_BAD_SUB
    assert by["bad_ring_header"]["summary"][0] == R.F_BAD_RING and by["bad_ring_header"]["counts"][0][3] == 0
    assert by["bad_ref"]["summary"][0] == R.F_BAD_REF and by["bad_ref"]["counts"] == [[2, 0, 0, 2]]
    assert by["no_deadlines"]["counts"] == [[2, 0, 0, 0]]
    assert by["len_mismatch"]["summary"][0] == R.F_LEN_MISMATCH
    assert by["q256_trips"]["summary"][6] > 0 and by["q256_trips"]["counts"][1][0] == 150 and by["q256_trips"]["counts"][1][3] > 0


def test_take_output_full_then_repeated(T):
    case = C.overflow_case()
    got, sessions, heads, ring = take(T, case)
    C.check_take(case.reference(), got, sessions, heads, ring, case)
    assert got.summary["flags"] == R.F_OUTPUT_FULL and got.summary["items"] == 5 and got.opts.size == 0
    assert sessions.tobytes() == case.sessions.tobytes() and heads.tobytes() == case.heads.tobytes()  # untouched
    assert got.offsets.tolist() == [0, 3, 5] and got.counts.tolist() == [[2, 1, 0, 0], [2, 0, 0, 0]]
    again, sessions, heads, ring = take(T, case, cap_out=got.summary["items"])
    C.check_take(case.reference(cap_out=5), again, sessions, heads, ring, case)
    assert again.summary["flags"] == 0 and again.refs.tolist() == [1, 2, 3, 4, 5]


def test_put_then_take_round_trip(T):
    """What put stores is what take hands out, in order, through a wrapped head."""
    from emqx_amd import window
    h = host(T)
    table = window.pack_sessions(1, inflight=2, inflight_max=2, mq_max=8)
    ring, heads = T.empty_ring(1, 8), T.empty_heads(1)
    heads["head"][0] = 6
    w = window.Window(window.HOST_ONLY)
    opts = [1, 0, 2, 1]
    a = w.run_host([0], [0, 4], opts, table, update_table=True)
    assert a.verdicts.tolist() == [3, 1, 3, 3]
    p = h.put_host([0], [0, 4], opts, a.verdicts, ring, heads, refs=[10, 11, 12, 13], sessions=table)
    assert p.summary["stored"] == 3 and p.summary["flags"] == 0 and heads.tolist() == [(6, 3)]
    assert [int(e["ref"]) for e in T.queue_of(ring, heads, 0)] == [10, 12, 13]
    table["inflight"][0] = 0
    t = h.take_host([0], table, ring, heads, update_table=True)
    assert t.refs.tolist() == [10, 12] and t.pkt_ids.tolist() == [1, 2] and t.verdicts.tolist() == [2, 2]
    assert heads.tolist() == [(0, 1)] and int(table["mq_len"][0]) == 1 and int(table["inflight"][0]) == 2
