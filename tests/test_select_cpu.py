"""CPU-side checks of the owner table and the select stage (include/emqx_select.h) on host-only
handles: the exports, the known answers (tests/golden/select_kats.json) through the restatement
(tests/select_ref.py) and through HookIndex, emqx_select_host against sets computed from the
contract and against the restatement, the rejected inputs, the overflow and refusal contracts,
and no batch call without a device."""

import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import select_cases as C
from tests import select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "select_kats.json")))["cases"]


@pytest.fixture(scope="module")
def S():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import select
    return select


def host(S):
    return S.OwnerTable(S.HOST_ONLY)


def test_exports_every_select_symbol(S):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_select.h")
    assert len(declared) == 12
    assert sorted(_lib.SELECT_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(S):
    import emqx_amd
    assert emqx_amd.OwnerTable is S.OwnerTable and emqx_amd.HookIndex is S.HookIndex


def test_batch_calls_need_a_device(S):
    from emqx_amd import _lib
    case = C.shape("e65")
    t = case.load(host(S))
    with pytest.raises(_lib.EngineError) as e:
        t.select_packed(*case.batch)
    assert e.value.code == EDEVICE
    b = S.OwnerTable.batch(0, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(_lib.EngineError) as e:
        t.select_device(b)
    assert e.value.code == EDEVICE
    with pytest.raises(_lib.EngineError) as e:
        t.select_device_async(b, 0)
    assert e.value.code == EDEVICE
    with pytest.raises(_lib.EngineError) as e:
        S.HookIndex(S.HOST_ONLY).select_device_async(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert e.value.code == EDEVICE


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(S, kat):
    """The restatement reproduces the transcribed answers, and so does the index."""
    assert [R.consumers(kat["world"], m) for m in kat["messages"]] == kat["expect"]
    index = R.load(kat["world"], S.HookIndex(S.HOST_ONLY))
    assert R.selected(index, kat["world"], kat["messages"]) == kat["expect"]


def test_reference_names(S):
    kat = next(k for k in KATS if k["name"] == "t_get_rules_for_topic_2")
    index = R.load(kat["world"], S.HookIndex(S.HOST_ONLY))
    assert index.get_rules_for_topic(b"simple/1") == ["rule-debug-1", "rule-debug-2", "rule-debug-4", "rule-debug-5"]
    assert index.get_rules_for_topics([b"simple/4", b"simple/1/1", b"other"]) == [
        ["rule-debug-1", "rule-debug-2", "rule-debug-5", "rule-debug-6"], ["rule-debug-1", "rule-debug-3"], []]
    index.set_bridge("mqtt:b", b"simple/+")
    assert index.get_matched_bridges(b"simple/1") == ["mqtt:b"] and index.get_rules_for_topic(b"x") == []
    index.delete_rule("rule-debug-1")
    index.delete_rule("no-such-rule")
    assert index.get_rules_for_topic(b"simple/1") == ["rule-debug-2", "rule-debug-4", "rule-debug-5"]


def test_shared_filter_leaves_with_its_last_owner(S):
    index = S.HookIndex(S.HOST_ONLY)
    index.insert_rule("a", [b"t/#", b"u"])
    index.insert_rule("b", [b"t/#"])
    index.set_exhook("h", [b"t/#"])
    assert index._filters[b"t/#"][1] == 3 and index.table is not None
    index.commit()
    assert index.table.stats()["n_filters"] == 2 and index.table.stats()["n_postings"] == 4
    index.delete_rule("a")
    index.insert_rule("b", [b"t/#"])  # replacing a rule by itself keeps the filter
    assert index._filters[b"t/#"][1] == 2 and b"u" not in index._filters
    index.delete_rule("b")
    index.delete_exhook("h")
    assert index._filters == {}
    assert index.on_message_publish([(b"t/1", False)]) == [[]]


@pytest.mark.parametrize("name, match_all, masked", C.SHAPE_CASES)
def test_shapes(S, name, match_all, masked):
    case = C.shape(name, match_all, masked)
    C.check(case, case.load(host(S)).select_host(*case.batch))


@pytest.mark.parametrize("start", [0, 3])
def test_straddle(S, start):
    case = C.straddle(start)
    C.check(case, case.load(host(S)).select_host(*case.batch))


def test_fuzz_against_the_restatement(S):
    """2 000 owners over 300 shared filters, lists of 0, 1, 2 and 65 filters, every mask of the
    three classes (0 included): the CSR of a brute-force match through emqx_select_host equals the
    restatement computed from the strings."""
    w = C.world(2000, 300, seed=3)
    assert {len(r["from"]) for r in w["rules"]} == {0, 1, 2, 65}
    assert any(h["topics"] == [] for h in w["exhooks"])
    index = R.load(w, S.HookIndex(S.HOST_ONLY))
    topics = [m["topic"] for m in C.messages(160, 60, seed=4)]
    masks = [i % 8 for i in range(len(topics))]
    got = index.select([t.encode() for t in topics], masks)
    want = [C.consumers_by_mask(w, t, m) for t, m in zip(topics, masks)]
    assert [sorted("%s:%s" % k for k in row) for row in got] == want
    assert sum(map(len, want)) > 2000 and sum(1 for x in want if not x) >= 20
    st = index.table.stats()
    assert st["n_owners"] == 2000 and st["n_match_all"] == 50 and st["max_list"] > 10


def test_fold_against_the_restatement(S):
    for ignore in (True, False):
        w = C.world(300, 80, seed=5, ignore_sys_message=ignore)
        index = R.load(w, S.HookIndex(S.HOST_ONLY))
        msgs = C.messages(400, 40, seed=6)
        assert any(m["sys"] for m in msgs)
        assert R.selected(index, w, msgs) == C.world_expected(w, msgs)


def one(t, filters, mask=None, **kw):
    return t.select_host([0, len(filters)], filters, None if mask is None else [mask], **kw)


def test_set_replaces_enable_and_remove_act_at_commit(S):
    t = host(S)
    t.set(4, 0, [7, 8, 7])
    t.set(5, 3, [8])
    t.set(6, 3, [], match_all=True)
    t.commit()
    assert one(t, [7, 8]).rows() == [[4, 5, 6]]
    assert t.stats()["n_postings"] == 3 and t.stats()["n_match_all"] == 1  # the duplicate 7 collapsed
    t.set(4, 0, [9])       # replaces the record
    t.enable([5, 99], False)  # 99 is unknown: ignored
    t.remove([6, 98])
    assert one(t, [7, 8]).rows() == [[4, 5, 6]]  # nothing changes before a commit
    t.commit()
    assert one(t, [7, 8, 9]).rows() == [[4]]
    t.enable([5], True)
    t.commit()
    got = one(t, [7, 8, 9], mask=1 << 3)
    assert got.rows() == [[5]]
    s = t.stats()
    assert s["n_owners"] == 2 and s["n_filters"] == 2 and s["max_list"] == 1 and s["epoch"] == 3


def test_no_filters_and_no_match_all_is_never_selected(S):
    t = host(S)
    t.set(1, 0, [])
    t.set(2, 0, [], match_all=True)
    t.set(3, 0, [5], enabled=False, match_all=True)  # disabled: not even as match-all
    t.commit()
    assert one(t, [5, 0]).rows() == [[2]]
    assert t.select_host([0, 0, 0], [], [1, 2]).rows() == [[2], []]


@pytest.mark.parametrize("what, args", [
    ("class", (9, 32, 1, [1])),
    ("flags", (9, 0, 4, [1])),
    ("filter", (9, 0, 1, [2, 1 << 30])),
    ("owner", (1 << 30, 0, 1, [1])),
])
def test_rejected_set_changes_nothing(S, what, args):
    from emqx_amd import _lib
    t = host(S)
    t.set(9, 0, [1])
    t.commit()
    with pytest.raises(_lib.EngineError) as e:
        t.set_flags(*args)
    assert e.value.code == EINVAL, what
    t.commit()
    assert one(t, [1, 2]).rows() == [[9]] and t.stats()["n_owners"] == 1
    t.set_flags(9, 31, 3, [(1 << 30) - 1])  # the bounds themselves are accepted
    t.set_flags((1 << 30) - 1, 0, 0, [])


def test_decreasing_offsets(S):
    from emqx_amd import _lib
    t = host(S)
    for off in ([0, 2, 1, 3], [1, 2, 3, 3], [0, 1, 2, 4]):
        with pytest.raises(_lib.EngineError) as e:
            t.select_host(off, [1, 2, 3], [1, 1, 1])
        assert e.value.code == EINVAL


@pytest.mark.parametrize("match_all", [True, False])
def test_cap_out_too_small(S, match_all):
    from emqx_amd import _lib
    case = C.shape("e257", match_all, True)
    t = case.load(host(S))
    ref = case.reference()
    need = ref["summary"][3]
    assert need > 100
    with pytest.raises(_lib.EngineError) as e:
        t.select_host(*case.batch, cap_out=need - 1)
    assert e.value.code == EOVERFLOW and e.value.needed == need
    assert e.value.out_offsets.tolist() == ref["offsets"]
    assert not e.value.out_owners.any(), "out_owners is untouched"
    assert [e.value.summary[k] for k in S.SUMMARY] == [1] + ref["summary"][1:]
    C.check(case, t.select_host(*case.batch, cap_out=need))


def test_tuning_keys(S):
    from emqx_amd import _lib
    t = host(S)
    t.set_tuning("max_blocks", 3)
    with pytest.raises(_lib.EngineError) as e:
        t.set_tuning("no_such_key", 1)
    assert e.value.code == ENOTFOUND
    for v in (0, 16385):
        with pytest.raises(_lib.EngineError) as e:
            t.set_tuning("max_blocks", v)
        assert e.value.code == EINVAL
    case = C.shape("e257")
    case.load(t)
    before = t.select_host(*case.batch)
    for v in (1, 1024):
        t.set_tuning("scan_chunk", v)
    for v in (0, -1, 1025):
        with pytest.raises(_lib.EngineError) as e:
            t.set_tuning("scan_chunk", v)
        assert e.value.code == EINVAL
    t.set_tuning("scan_chunk", 1)
    after = t.select_host(*case.batch)  # the host evaluator has no scan
    C.check(case, after)
    assert after.rows() == before.rows() and after.summary == before.summary


def test_stats_struct_is_versioned_by_size(S):
    from emqx_amd import _lib
    t = host(S)
    s = _lib.OwnTabStats()
    s.size = 16
    s.n_filters = 12345
    assert _lib.lib().emqx_owntab_stats_get(t._h, ctypes.byref(s)) == 0
    assert s.size == 16 and s.n_owners == 0 and s.n_filters == 12345  # nothing beyond 16 bytes written
    assert ctypes.sizeof(_lib.SelectBatch) == 64 and ctypes.sizeof(_lib.OwnTabStats) == 72


def test_expected_is_not_degenerate():
    """The shapes exercise what they claim: duplicates, unknown ids, disabled owners, masks."""
    s = C.shape("e10002").reference()["summary"]
    assert s[1] == 10002 and s[5] > 1000 and s[6] > 100 and s[3] > 1000 and s[7] > 100
    plain = C.shape("e257", False, False).reference()
    assert plain["summary"][4] < 5 and [] in plain["rows"]
    assert C.shape("e257", True, False).reference()["summary"][4] == 5  # match-all owners reach the empty messages
    assert np.asarray(C.shape("e0").reference()["offsets"]).tolist() == [0, 1, 4, 4]
