"""CPU-side checks of the ack stage (include/emqx_ack.h) on a host-only handle: the restatement
(tests/ack_ref.py) against the known answers of the reference's own suite
(tests/golden/ack_kats.json), emqx_ack_run_host and emqx_ack_record_host against the restatement
on every case, the exports, the refusals and argument errors, and no batch call without a device."""

import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ack_cases as C
from tests import ack_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ack_kats.json")))
KATS = GOLDEN["kats"]


@pytest.fixture(scope="module")
def A():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import ack
    return ack


def host(A):
    return A.Ack(A.HOST_ONLY)


def run(A, case, update_table=False):
    """The host evaluator on copies of the case's tables; a bad subscriber's EINVAL carries the outputs."""
    from emqx_amd import _lib
    table, slots = case.table.copy(), case.slots.copy()
    try:
        got = host(A).run_host(case.subs, case.offsets, case.acks, table, slots, update_table=update_table)
        assert not case.reference()["summary"][0]
    except _lib.EngineError as e:
        assert e.code == EINVAL and e.summary["flags"] == R.F_BAD_SUB
        got = e.partial
    return got, table, slots


def record(A, case, fn="record_host"):
    from emqx_amd import _lib
    slots = case.slots.copy()
    try:
        got = getattr(host(A), fn)(case.subs, case.offsets, case.opts, case.verdicts, case.pkt_ids, slots, refs=case.refs)
        assert not case.reference()["summary"][0] & R.F_BAD_SUB
    except _lib.EngineError as e:
        assert e.code == EINVAL and e.summary["flags"] & R.F_BAD_SUB
        got = e.partial
    return got, slots


# ---- the restatement against the reference's suite ----------------------------------------------

WANT = {"t_puback", "t_puback_with_dequeue", "t_puback_error_packet_id_in_use", "t_puback_error_packet_id_not_found", "t_pubrec",
        "t_pubrec_packet_id_in_use_error", "t_pubrec_packet_id_not_found_error", "t_pubcomp", "t_pubcomp_error_packetid_in_use",
        "t_pubcomp_error_packetid_not_found"}


def test_kats_cover_the_named_suite_tests():
    assert {k["source"] for k in KATS} == {"emqx_session_SUITE:" + t for t in WANT}
    assert "by hand" in GOLDEN["comment"] and set(GOLDEN) == {"comment", "kats", "batch_n"}


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_ref_against_the_reference_suite(kat):
    row = C.row(kat["row"], 8)
    verdicts, refs, counts, after = R.session_acks(row, kat["session"], C.acks(kat["acks"]))
    assert verdicts == kat["verdicts"] and refs == kat["refs"] and counts == kat["counts"]
    assert row == C.row(kat["row_after"], 8) and after == kat["session"]["inflight"] - counts[0]
    if kat["name"] == "puback_with_dequeue":
        assert counts[0] == 1 and counts[3] >= 1


def test_batch_n_against_the_reference():
    assert any(mx == 0 for mx, _, _ in GOLDEN["batch_n"])
    for mx, n, want in GOLDEN["batch_n"]:
        assert R.batch_n(mx, n) == want


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_host_against_the_reference_suite(A, kat):
    from emqx_amd import window
    slots = C.slots_of([C.row(kat["row"], 8)], 8)
    table = window.pack_sessions(1, **kat["session"])
    got = host(A).run_host([0], [0, len(kat["acks"])], C.acks(kat["acks"]), table, slots, update_table=True)
    assert got.verdicts.tolist() == kat["verdicts"] and got.refs.tolist() == kat["refs"]
    assert got.counts[0].tolist() == kat["counts"]
    assert C.rows_of(slots) == [C.row(kat["row_after"], 8)]
    assert int(table["inflight"][0]) == kat["session"]["inflight"] - kat["counts"][0]


def test_host_batch_n(A):
    from emqx_amd import window
    for mx, n, want in GOLDEN["batch_n"]:
        table = window.pack_sessions(1, inflight=n, inflight_max=mx)
        got = host(A).run_host([0], [0, 0], [], table, A.empty_slots(1, 8))
        assert got.counts[0].tolist() == [0, 0, 0, want]


# ---- the ABI ------------------------------------------------------------------------------------

def test_exports_every_ack_symbol(A):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_ack.h")
    assert len(declared) == 13
    assert sorted(_lib.ACK_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(A):
    import emqx_amd
    assert emqx_amd.Ack is A.Ack


def test_constants_mirror_the_headers(A):
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "ack.h")).read()
    block = int(re.search(r"AK_BLOCK = (\d+);", src).group(1))
    rows = int(re.search(r"AK_ROWS = (\d+);", src).group(1))
    assert re.search(r"AK_TILE = AK_BLOCK \* AK_ROWS;", src)
    assert (A.BLOCK, A.ROWS, A.TILE) == (block, rows, block * rows) and C.T == A.TILE
    pub = open(os.path.join(ROOT, "include", "emqx_ack.h")).read()

    def define(name):
        return int(re.search(r"#define EMQX_%s \(?(\w+?)(u|ull)?\b" % name, pub).group(1), 0)
    for name in ("A_OK", "A_IN_USE", "A_NOT_FOUND", "A_NO_SESSION", "A_PASS", "A_BAD_KIND"):
        assert define(name) == getattr(A, name) == getattr(R, name), name
    for name in ("EMPTY", "MSG", "PUBREL_AWAIT", "PUBACK", "PUBREC", "PUBCOMP", "F_INPUT_REFUSED", "F_BAD_SUB", "F_ROW_FULL", "NO_REF",
                 "DEFAULT_BATCH_N"):
        assert define("ACK_" + name) == getattr(A, name) == getattr(R, name), name
    assert define("ACK_SUMMARY_WORDS") == A.SUMMARY_WORDS == len(A.RUN_SUMMARY) == len(A.RECORD_SUMMARY)
    assert re.search(r"#define EMQX_ACK_MAX_ACKS \(1ull << 31\)", pub) and A.MAX_ACKS == R.MAX_ACKS == 1 << 31
    from emqx_amd import window
    assert (R.W_SEND, R.W_VERDICT_MASK, R.PRESENT, R.PASS) == (window.W_SEND, window.W_VERDICT_MASK, window.PRESENT, window.PASS)
    assert A.SLOT.itemsize == 8 and A.SLOT.names == ("pkt_id", "phase", "qos", "ref")
    s = np.zeros(1, dtype=A.SLOT)
    s[0] = (0x1234, 2, 1, 0xAABBCCDD)
    assert s.tobytes() == bytes([0x34, 0x12, 2, 1, 0xDD, 0xCC, 0xBB, 0xAA])


def test_batch_calls_need_a_device(A):
    from emqx_amd import _lib
    h = host(A)
    case = C.CELLS["puback_msg"]
    with pytest.raises(_lib.EngineError) as e:
        h.run(case.subs, case.offsets, case.acks, case.table.copy(), case.slots.copy())
    assert e.value.code == EDEVICE
    rc = C.RECORDS["free_0_2_5_takes_3"]()
    with pytest.raises(_lib.EngineError) as e:
        h.record(rc.subs, rc.offsets, rc.opts, rc.verdicts, rc.pkt_ids, rc.slots.copy())
    assert e.value.code == EDEVICE
    for fn, args in ((h.run_device, A.Ack.run_args(0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0, 0)),
                     (h.record_device, A.Ack.record_args(0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0))):
        with pytest.raises(_lib.EngineError) as e:
            fn(args)
        assert e.value.code == EDEVICE
    for fn, args in ((h.run_device_async, A.Ack.run_args(0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0, 0)),
                     (h.record_device_async, A.Ack.record_args(0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0))):
        with pytest.raises(_lib.EngineError) as e:
            fn(args, 0)
        assert e.value.code == EDEVICE
    with pytest.raises(_lib.EngineError) as e:
        h.reserve(1000, 1000, 16)
    assert e.value.code == EDEVICE


# ---- the run call's host evaluator against the restatement --------------------------------------

@pytest.mark.parametrize("name", list(C.RUNS))
@pytest.mark.parametrize("update_table", [False, True], ids=["keep_table", "update_table"])
def test_run_cases(A, name, update_table):
    case = C.RUNS[name]()
    got, table, slots = run(A, case, update_table)
    C.check_run(case.reference(update_table), got, slots, table)
    if not update_table:
        assert table.tobytes() == case.table.tobytes()


@pytest.mark.parametrize("name", list(C.CELLS))
def test_cells_mean_what_their_names_say(name):
    """Each cell of the table of include/emqx_ack.h, read off the restatement's answer."""
    case = C.CELLS[name]
    ref = case.reference()
    verdict, ref_out, phase, released, to_pubrel = C.CELL_ANSWERS[name]
    d = int(case.offsets[1])
    assert (int(ref["verdicts"][d]), int(ref["refs"][d])) == (verdict, ref_out)
    assert int(ref["slots"][case.subs[1], 0]["phase"]) == phase
    assert ref["counts"][1].tolist()[:3] == [released, to_pubrel, 0 if verdict == R.A_OK else 1]


def test_cases_mean_what_their_names_say():
    def box(name, update_table=False):
        case = C.RUNS[name]()
        ref = case.reference(update_table)
        lo, hi = int(case.offsets[1]), int(case.offsets[2])
        return ref["verdicts"][lo:hi].tolist(), ref["refs"][lo:hi].tolist(), ref["counts"][1].tolist(), case, ref
    assert box("pubrec_then_pubcomp")[0] == [1, 1] and box("pubrec_then_pubcomp")[2][:3] == [1, 1, 0]
    assert box("pubcomp_before_pubrec")[0] == [2, 1] and box("pubcomp_before_pubrec")[2][:3] == [0, 1, 1]
    assert box("puback_twice")[0] == [1, 3]
    assert box("pubrec_puback_pubcomp_pubcomp")[0] == [1, 2, 1, 3]
    assert box("pubrec_twice_then_pubcomp_twice")[0] == [1, 2, 1, 3, 3]
    assert box("ids_0_1_65535")[0] == [2, 1, 1, 1, 3] and box("ids_0_1_65535")[1] == [R.NO_REF, 1, 3, 2, R.NO_REF]
    assert box("kind_0_and_4")[0] == [6, 6, 6, 1] and box("kind_0_and_4")[2][:3] == [1, 0, 3]
    v, refs, _, case, ref = box("id_held_twice")
    assert v == [2, 1, 3, 3] and refs[1] == 40 and int(ref["slots"][case.subs[1], 8]["phase"]) == R.PUBREL_AWAIT
    assert box("unknown_phase")[0] == [2, 2, 2, 2]
    for w in (8, 32, 64):
        v, _, cnt, case, ref = box("full_row_reversed_w%d" % w)
        assert v == [1] * w and cnt == [w, 0, 0, w] and not ref["slots"][case.subs[1]]["phase"].any()
    v, _, cnt, _, _ = box("skew_2T+1")
    assert [i for i, x in enumerate(v) if x == 1] == [0, C.T, 2 * C.T] and cnt[:3] == [2, 1, 2 * C.T - 2]
    v, _, cnt, _, _ = box("same_id_T+1_times")
    assert v == [1] + [3] * C.T and cnt[:3] == [1, 0, C.T]
    assert set(box("not_present")[0]) == {R.A_NO_SESSION} and set(box("pass")[0]) == {R.A_PASS}
    assert box("not_present")[2] == box("pass")[2] == [0, 0, 0, 0]
    case = C.RUNS["sub_at_sub_limit"]()
    assert int(case.subs[1]) == case.sub_limit and case.reference()["summary"][0] == R.F_BAD_SUB
    _, _, cnt, case, ref = box("inflight_below_released", update_table=True)
    assert cnt == [2, 1, 0, 2] and int(ref["table"]["inflight"][case.subs[1]]) == 0
    assert box("inflight_max_0")[2] == [1, 0, 0, 1000] and box("inflight_over_max")[2] == [1, 0, 0, 0]
    case = C.RUNS["empty_lists_before_between_after"]()
    lens = np.diff(case.offsets.astype(np.int64)).tolist()
    assert lens[0] == lens[1] == lens[3] == lens[5] == 0 and lens[2] > 0 and lens[4] > 0


def test_fuzz(A):
    case = C.fuzz()
    ref = case.reference(True)
    assert ref["summary"][0] == R.F_BAD_SUB and case.m > 2000 and min(ref["summary"][3:]) > 50
    got, table, slots = run(A, case, True)
    C.check_run(ref, got, slots, table)
    assert table.tobytes() != case.table.tobytes() and slots.tobytes() != case.slots.tobytes()


def test_update_table_chains_two_batches(A):
    """The second batch sees the rows and the window the first one left."""
    case = C.fuzz(seed=4, n_sessions=300)
    recs, rows = C.records_of(case.table), C.rows_of(case.slots)
    R.run(case.subs, case.offsets, case.acks, recs, rows, update_table=True)
    second = R.run(case.subs, case.offsets, case.acks, recs, rows, update_table=True)
    _, table, slots = run(A, case, True)
    from emqx_amd import _lib
    try:
        got = host(A).run_host(case.subs, case.offsets, case.acks, table, slots, update_table=True)
    except _lib.EngineError as e:
        got = e.partial
    assert got.verdicts.tolist() == second["verdicts"] and got.counts.tolist() == second["counts"]
    assert C.rows_of(slots) == rows and table["inflight"].tolist() == [r["inflight"] for r in recs]


# ---- the record call's host evaluator against the restatement -----------------------------------

@pytest.mark.parametrize("name", list(C.RECORDS))
@pytest.mark.parametrize("refs", [False, True], ids=["refs_null", "refs"])
def test_record_cases(A, name, refs):
    case = C.RECORDS[name](refs)
    got, slots = record(A, case)
    C.check_rec(case.reference(), got, slots)


def test_record_cases_mean_what_their_names_say():
    for n, want in ((1, [0]), (3, [0, 2, 5]), (4, [0, 2, 5])):
        case = C.RECORDS["free_0_2_5_takes_%d" % n]()
        ref = case.reference()
        sub = int(case.subs[1])
        lo, hi = int(case.offsets[1]), int(case.offsets[2])
        sent = [d for d in range(lo, hi) if case.verdicts[d] == C.SEND]
        assert len(sent) == n and int(ref["unrecorded"][1]) == n - len(want)
        filled = [w for w in range(8) if case.slots[sub, w]["phase"] == R.EMPTY and ref["slots"][sub, w]["phase"] == R.MSG]
        assert filled == want[:n]
        for w, d in zip(filled, sent):
            assert ref["slots"][sub, w].tolist() == (int(case.pkt_ids[d]), R.MSG, int(case.opts[d]) & 3, d)
        assert bool(ref["summary"][0] & R.F_ROW_FULL) == (n == 4)
    case = C.RECORDS["sends_interleaved_across_a_tile_border"]()
    lo, hi = int(case.offsets[1]), int(case.offsets[2])
    assert lo < C.T < hi and {C.SEND, C.SEND0} <= set(case.verdicts[lo:hi].tolist()) and int(case.reference()["unrecorded"][1]) == 0
    case = C.RECORDS["one_inbox_over_3_tiles"]()
    assert case.reference()["unrecorded"].tolist()[1] == 20 and case.reference()["summary"][6] == 1
    case = C.RECORDS["bad_subscriber"]()
    ref = case.reference()
    assert ref["summary"][0] == R.F_BAD_SUB and ref["unrecorded"].tolist()[1] == 3 and int(case.subs[1]) == case.sub_limit
    assert C.RECORDS["free_0_2_5_takes_3"](True).refs is not None and C.RECORDS["free_0_2_5_takes_3"](False).refs is None


def test_record_fuzz(A):
    case = C.rec_fuzz()
    ref = case.reference()
    assert ref["summary"][0] == R.F_BAD_SUB | R.F_ROW_FULL and ref["summary"][4] > 3000 and ref["summary"][6] > 20
    got, slots = record(A, case)
    C.check_rec(ref, got, slots)


def test_record_then_run(A):
    """What record stores is what run finds: every recorded send acked once releases its slot."""
    from emqx_amd import window
    case = C.RECORDS["sends_interleaved_across_a_tile_border"]()
    _, slots = record(A, case)
    subs = case.subs
    lists = [[int(s["pkt_id"]) for s in slots[sub] if s["phase"] == R.MSG] for sub in subs]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    packed = A.pack_acks(R.PUBACK, [i for x in lists for i in x])
    table = window.pack_sessions(case.sub_limit, inflight=16, inflight_max=16)
    got = host(A).run_host(subs, offsets, packed, table, slots, update_table=True)
    assert set(got.verdicts.tolist()) == {R.A_OK} and got.summary["released"] == packed.size
    assert not slots[subs]["phase"].any() and table["inflight"][subs].tolist() == [16 - len(x) for x in lists]


# ---- refusals and argument errors ---------------------------------------------------------------

def _run_args(A, case, **over):
    from emqx_amd import _lib
    keep = {"subs": case.subs.copy(), "off": case.offsets.copy(), "acks": case.acks.copy(), "table": case.table.copy(),
            "slots": case.slots.copy(), "ver": np.zeros(case.total + 1, dtype=np.uint8), "refs": np.zeros(case.total + 1, dtype=np.uint32),
            "cnt": np.zeros((case.m + 1, 4), dtype=np.uint32)}
    p = lambda a: a.ctypes.data  # noqa: E731
    kw = dict(ack_subs=p(keep["subs"]), ack_offsets=p(keep["off"]), acks=p(keep["acks"]), n_boxes=None, m=case.m, cap_in=case.total,
              cap_boxes=case.m, sessions=p(keep["table"]), sub_limit=case.sub_limit, update_table=1, slots=p(keep["slots"]),
              w=case.w, verdicts=p(keep["ver"]), out_refs=p(keep["refs"]), out_counts=p(keep["cnt"]))
    kw.update(over)
    return _lib.AckRunArgs(**kw), keep


def _rec_args(A, case, **over):
    from emqx_amd import _lib
    keep = {"subs": case.subs.copy(), "off": case.offsets.copy(), "opts": case.opts.copy(), "ver": case.verdicts.copy(),
            "ids": case.pkt_ids.copy(), "slots": case.slots.copy(), "unrec": np.zeros(case.m + 1, dtype=np.uint32)}
    p = lambda a: a.ctypes.data  # noqa: E731
    kw = dict(inbox_subs=p(keep["subs"]), inbox_offsets=p(keep["off"]), box_opts=p(keep["opts"]), n_boxes=None, m=case.m,
              cap_in=case.total, cap_boxes=case.m, verdicts=p(keep["ver"]), pkt_ids=p(keep["ids"]), refs=None,
              slots=p(keep["slots"]), w=case.w, sub_limit=case.sub_limit, out_unrecorded=p(keep["unrec"]))
    kw.update(over)
    return _lib.AckRecordArgs(**kw), keep


RUN_ERRORS = {"no_acks": dict(acks=None), "no_offsets": dict(ack_offsets=None), "no_verdicts": dict(verdicts=None),
              "no_out_refs": dict(out_refs=None), "no_ack_subs": dict(ack_subs=None), "no_out_counts": dict(out_counts=None),
              "no_sessions": dict(sessions=None), "no_slots": dict(slots=None), "m_over_cap_boxes": dict(cap_boxes=2),
              "cap_in_over": dict(cap_in=1 << 32), "sub_limit_over": dict(sub_limit=(1 << 32) + 1),
              "w_0": dict(w=0), "w_12": dict(w=12), "w_4": dict(w=4), "w_128": dict(w=128)}


@pytest.mark.parametrize("what", list(RUN_ERRORS))
def test_run_argument_errors(A, what):
    from emqx_amd import _lib
    case = C.RUNS["pubrec_then_pubcomp"]()
    b, keep = _run_args(A, case, **RUN_ERRORS[what])
    summary = np.full(8, 77, dtype=np.uint64)
    assert _lib.lib().emqx_ack_run_host(host(A)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert not keep["ver"].any() and not keep["cnt"].any() and (summary == 77).all()
    assert keep["slots"].tobytes() == case.slots.tobytes() and keep["table"].tobytes() == case.table.tobytes()
    assert _lib.lib().emqx_ack_run_host(None, ctypes.byref(b), None) == EINVAL


REC_ERRORS = {"no_box_opts": dict(box_opts=None), "no_offsets": dict(inbox_offsets=None), "no_verdicts": dict(verdicts=None),
              "no_pkt_ids": dict(pkt_ids=None), "no_inbox_subs": dict(inbox_subs=None), "no_out_unrecorded": dict(out_unrecorded=None),
              "no_slots": dict(slots=None), "m_over_cap_boxes": dict(cap_boxes=2), "cap_in_over": dict(cap_in=1 << 32),
              "w_0": dict(w=0), "w_24": dict(w=24)}


@pytest.mark.parametrize("what", list(REC_ERRORS))
def test_record_argument_errors(A, what):
    from emqx_amd import _lib
    case = C.RECORDS["free_0_2_5_takes_3"]()
    b, keep = _rec_args(A, case, **REC_ERRORS[what])
    summary = np.full(8, 77, dtype=np.uint64)
    assert _lib.lib().emqx_ack_record_host(host(A)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert not keep["unrec"].any() and (summary == 77).all() and keep["slots"].tobytes() == case.slots.tobytes()
    assert _lib.lib().emqx_ack_record_host(None, ctypes.byref(b), None) == EINVAL


def test_refused_input_writes_only_the_summary(A):
    from emqx_amd import _lib
    case = C.RUNS["list_of_65"]()
    b, keep = _run_args(A, case, cap_in=case.total - 1)
    summary = np.zeros(8, dtype=np.uint64)
    assert _lib.lib().emqx_ack_run_host(host(A)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    want = [R.F_INPUT_REFUSED, case.total, case.m, 0, 0, 0, 0, 0]
    assert summary.tolist() == want == R.run(case.subs, case.offsets, case.acks, [], [], cap_in=case.total - 1)["summary"]
    assert not keep["ver"].any() and not keep["cnt"].any() and keep["slots"].tobytes() == case.slots.tobytes()
    # the count read through n_boxes: above cap_boxes it refuses the input
    count = np.array([case.m + 1], dtype=np.uint64)
    b, keep = _run_args(A, case, n_boxes=count.ctypes.data, m=0)
    assert _lib.lib().emqx_ack_run_host(host(A)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [R.F_INPUT_REFUSED, 0, case.m + 1, 0, 0, 0, 0, 0] and not keep["ver"].any()
    count[0] = case.m
    assert _lib.lib().emqx_ack_run_host(host(A)._h, ctypes.byref(b), summary.ctypes.data) == 0
    assert keep["ver"][:case.total].tobytes() == case.reference()["verdicts"].tobytes() and keep["ver"][case.total] == 0
    # the record call
    rc = C.RECORDS["free_0_2_5_takes_3"]()
    b, keep = _rec_args(A, rc, cap_in=rc.total - 1)
    assert _lib.lib().emqx_ack_record_host(host(A)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [R.F_INPUT_REFUSED, rc.total, rc.m, 0, 0, 0, 0, 0] and keep["slots"].tobytes() == rc.slots.tobytes()


def test_2_to_the_31_acks_are_refused(A):
    """A total of acks >= 2^31 is refused before anything is read: the offsets alone say so."""
    from emqx_amd import _lib
    case = C.RUNS["pubrec_then_pubcomp"]()
    for total in (1 << 31, (1 << 32) - 1):
        off = np.array([0, total], dtype=np.uint64)
        b, keep = _run_args(A, case, ack_offsets=off.ctypes.data, m=1, cap_in=(1 << 32) - 1)
        summary = np.zeros(8, dtype=np.uint64)
        assert _lib.lib().emqx_ack_run_host(host(A)._h, ctypes.byref(b), summary.ctypes.data) == EINVAL
        assert summary.tolist() == [R.F_INPUT_REFUSED, total, 1, 0, 0, 0, 0, 0]
        assert R.run([0], off, [], [], [], cap_in=1 << 40)["summary"] == summary.tolist()
        assert not keep["ver"].any() and keep["slots"].tobytes() == case.slots.tobytes()


def test_bad_offsets(A):
    from emqx_amd import _lib, window
    h = host(A)
    t, s = window.pack_sessions(4), A.empty_slots(4, 8)
    for off in ([0, 2, 1, 3], [1, 2, 3, 3]):
        with pytest.raises(_lib.EngineError) as e:
            h.run_host([0, 1, 2], off, A.pack_acks([1, 1, 1], [1, 2, 3]), t, s)
        assert e.value.code == EINVAL
        with pytest.raises(_lib.EngineError) as e:
            h.record_host([0, 1, 2], off, [1, 1, 1], [2, 2, 2], [1, 2, 3], s)
        assert e.value.code == EINVAL
    assert not s["phase"].any()


def test_tuning_keys(A):
    from emqx_amd import _lib
    h = host(A)
    with pytest.raises(_lib.EngineError) as e:
        h.set_tuning("no_such_key", 1)
    assert e.value.code == ENOTFOUND
    for v in (-1, 2):
        with pytest.raises(_lib.EngineError) as e:
            h.set_tuning("rematch", v)
        assert e.value.code == EINVAL
    h.set_tuning("rematch", 1)
    assert h.stats()["rematch"] == 1
    case, rec = C.RUNS["list_of_65"](), C.RECORDS["free_0_2_5_takes_3"]()

    def both():  # the host evaluator has no grid and no scan
        table, slots, rows = case.table.copy(), case.slots.copy(), rec.slots.copy()
        ran = h.run_host(case.subs, case.offsets, case.acks, table, slots, update_table=True)
        recorded = h.record_host(rec.subs, rec.offsets, rec.opts, rec.verdicts, rec.pkt_ids, rows, refs=rec.refs)
        C.check_run(case.reference(True), ran, slots, table)
        C.check_rec(rec.reference(), recorded, rows)
        return ran, recorded, table.tobytes(), slots.tobytes(), rows.tobytes()

    before = both()
    _grid_keys(h, 4096)
    after = both()
    C.same_run(after[0], before[0])
    assert after[1].summary == before[1].summary and after[1].unrecorded.tobytes() == before[1].unrecorded.tobytes()
    assert after[2:] == before[2:]


def _grid_keys(h, max_blocks):
    """"max_blocks" and "scan_chunk" on a host-only handle: accepted at 1 and at the maximum (it has
    no grid to cap), EINVAL at 0, below it and above the maximum."""
    from emqx_amd import _lib
    for key, top in (("max_blocks", max_blocks), ("scan_chunk", 1024)):
        for v in (1, top):
            h.set_tuning(key, v)
        for v in (0, -1, top + 1):
            with pytest.raises(_lib.EngineError) as e:
                h.set_tuning(key, v)
            assert e.value.code == EINVAL
    h.set_tuning("max_blocks", 1)
    h.set_tuning("scan_chunk", 1)


def test_stats_struct_is_versioned_by_size(A):
    from emqx_amd import _lib, window
    h = host(A)
    h.run_host([0], [0, 1], A.pack_acks([1], [1]), window.pack_sessions(1), A.empty_slots(1, 8))
    s = _lib.AckStats()
    s.size = 16
    s.cap_boxes = 12345
    assert _lib.lib().emqx_ack_stats_get(h._h, ctypes.byref(s)) == 0
    assert s.size == 16 and s.cap_in == 0 and s.cap_boxes == 12345  # nothing beyond 16 bytes written
    assert h.stats()["calls"] == 1
    s.size = 4
    assert _lib.lib().emqx_ack_stats_get(h._h, ctypes.byref(s)) == EINVAL
