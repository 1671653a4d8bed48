"""CPU-side checks of the delivery-options table (include/emqx_deliver.h) on a host-only handle:
the exports, emqx_deliver_enrich_host against the restatement (tests/deliver_ref.py) byte for
byte, the key, the rejected inputs, and no batch call without a device."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import deliver_cases as C
from tests import deliver_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5


@pytest.fixture(scope="module")
def D():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import deliver
    return deliver


def host(D):
    return D.SubOpts(D.HOST_ONLY)


def test_exports_every_deliver_symbol(D):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_deliver.h")
    assert len(declared) == 12
    assert sorted(_lib.DELIVER_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(D):
    import emqx_amd
    assert emqx_amd.SubOpts is D.SubOpts


def test_batch_calls_need_a_device(D):
    from emqx_amd import _lib
    t = C.truth_table().load(host(D))
    with pytest.raises(_lib.EngineError) as e:
        t.enrich_packed(*C.truth_table().batch)
    assert e.value.code == EDEVICE
    b = D.SubOpts.batch(0, 0, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(_lib.EngineError) as e:
        t.enrich_device(b)
    assert e.value.code == EDEVICE
    with pytest.raises(_lib.EngineError) as e:
        t.enrich_device_async(b, 0)
    assert e.value.code == EDEVICE


def test_truth_table(D):
    """48 options words and the absent key, times 36 messages: exactly the restatement."""
    case = C.truth_table()
    t = case.load(host(D))
    for compact in (False, True):
        C.check(case, t.enrich_host(*case.batch, compact=compact), compact)
    ref = case.reference()
    assert len(ref["opts"]) == 49 * 36 and len(set(ref["opts"])) > 20
    assert ref["summary"][3] == 24 * 12  # nl = 1 words times the messages their subscriber published


def test_predicate_is_ignore_local_of_one_element():
    s = R.Sessions()
    s.set(7, 1, nl=1)
    s.set(8, 1, nl=0)
    sess = s.session(1)
    for topic, frm in itertools_cases():
        d = (topic, R.message(0, 0, frm))
        assert (R.ignore_local([d], 1, sess) == []) == R.no_local_hit(d, 1, sess)


def itertools_cases():
    return [(t, f) for t in (7, 8, 9) for f in (1, 2, None)]


def test_dropwhile_keeps_a_hit_behind_a_miss():
    """The reference's lists:dropwhile drops only the leading run: over [hit, miss, hit] the
    second hit survives.  The engine reports the predicate per delivery and its compacted form
    drops both (MQTT 5 section 3.8.3.1); the difference is on record here, on the restatement alone."""
    s = R.Sessions()
    s.set(7, 1, nl=1)
    s.set(8, 1, nl=0)
    sess = s.session(1)
    hit, miss = (7, R.message(0, 0, 1)), (8, R.message(0, 0, 1))
    assert [R.no_local_hit(d, 1, sess) for d in (hit, miss, hit)] == [True, False, True]
    assert R.ignore_local([hit, miss, hit], 1, sess) == [miss, hit]
    assert R.ignore_local([hit, hit, miss], 1, sess) == [miss]


def one(t, sub, word, qos=1, flags=0, frm=None, **kw):
    return t.enrich_host([0, 1], [sub], [word], [qos], [flags], None if frm is None else [frm], **kw)


def test_key_is_an_ordered_pair(D):
    t = host(D)
    t.set([3], [5], qos=2, nl=1, subid=9)
    t.commit()
    got = one(t, 5, 3, qos=2, frm=5)
    assert got.opts.tolist() == [2 | R.OUT_NL | R.OUT_DROP] and got.subids.tolist() == [9]
    got = one(t, 3, 5, qos=2, frm=3)
    assert got.opts.tolist() == [2 | R.OUT_NO_SUBOPTS] and got.subids.tolist() == [0]


def test_shared_and_retry_bits_do_not_change_the_key_and_pass_through(D):
    t = host(D)
    t.set([3], [5], qos=0, subid=4)
    t.commit()
    words = [3, 3 | R.SHARED_BIT, 3 | R.SHARED_BIT | R.RETRY_BIT]
    got = t.enrich_host([0, 3], [5, 5, 5], words, [1], [0], compact=True)
    assert got.opts.tolist() == [0, 0, 0] and got.subids.tolist() == [4, 4, 4]
    assert got.kept.filters.tolist() == words and got.kept.offsets.tolist() == [0, 3]


def test_set_twice_overwrites(D):
    t = host(D)
    t.set([3], [5], qos=0, subid=4)
    t.set([3], [5], qos=2, rap=1)
    t.commit()
    got = one(t, 5, 3, qos=2, flags=1)
    assert got.opts.tolist() == [2 | R.OUT_RETAIN] and got.subids.tolist() == [0]
    assert t.stats()["n_entries"] == 1


def test_remove_and_drop_take_effect_at_commit(D):
    t = host(D)
    t.set([1, 2, 3, 1], [5, 5, 6, 7], qos=2)
    t.commit()
    batch = ([0, 4], [5, 5, 6, 7], [1, 2, 3, 1], [2], [0])
    assert t.enrich_host(*batch).opts.tolist() == [2, 2, 2, 2]
    t.remove([1, 9], [5, 9])  # the second pair is absent: ignored
    t.drop_subscribers([6])
    assert t.enrich_host(*batch).opts.tolist() == [2, 2, 2, 2]
    t.commit()
    no = 2 | R.OUT_NO_SUBOPTS
    assert t.enrich_host(*batch).opts.tolist() == [no, 2, no, 2]
    s = t.stats()
    assert s["n_entries"] == 2 and s["epoch"] == 2 and s["n_slots"] > 2 and s["table_bytes"] == 16 * s["n_slots"]


@pytest.mark.parametrize("what, args", [
    ("filter", dict(filters=[1 << 30], words=[0])),
    ("qos3", dict(words=[3])),
    ("reserved", dict(words=[0x40])),
    ("subid0", dict(words=[0x20], subids=[0])),
    ("subid_2_28", dict(words=[0x20], subids=[1 << 28])),
    ("subid_missing", dict(words=[0x20])),
])
def test_rejected_set_changes_nothing(D, what, args):
    from emqx_amd import _lib
    t = host(D)
    t.set([3], [5], qos=1)
    t.commit()
    # one good pair in front of the bad one: nothing of the call is applied
    with pytest.raises(_lib.EngineError) as e:
        t.set_words([4] + args.get("filters", [3]), [5, 5], [2] + args["words"],
                    None if "subids" not in args else [0] + args["subids"])
    assert e.value.code == EINVAL, what
    t.commit()
    assert t.stats()["n_entries"] == 1
    assert one(t, 5, 3, qos=2).opts.tolist() == [1]
    assert one(t, 5, 4, qos=2).opts.tolist() == [2 | R.OUT_NO_SUBOPTS]


def test_subid_bounds_accepted(D):
    t = host(D)
    t.set([1, 2], [5, 5], subid=[1, 268435455])
    t.commit()
    assert t.enrich_host([0, 2], [5, 5], [1, 2], [0], [0]).subids.tolist() == [1, 268435455]


def test_decreasing_offsets(D):
    from emqx_amd import _lib
    t = host(D)
    for off in ([0, 2, 1, 3], [1, 2, 3, 3]):
        with pytest.raises(_lib.EngineError) as e:
            t.enrich_host(off, [1, 2, 3], [1, 2, 3], [0, 0, 0], [0, 0, 0])
        assert e.value.code == EINVAL


def test_cap_kept_too_small(D):
    from emqx_amd import _lib
    case = C.shape("257", "mixed")
    t = case.load(host(D))
    ref = case.reference()
    kept = ref["summary"][2]
    assert 0 < kept < 257
    with pytest.raises(_lib.EngineError) as e:
        t.enrich_host(*case.batch, compact=True, cap_kept=kept - 1)
    assert e.value.code == EOVERFLOW and e.value.needed == kept
    assert e.value.kept_offsets.tolist() == ref["kept"][0]
    assert e.value.summary["flags"] == 1
    C.check(case, t.enrich_host(*case.batch, compact=True, cap_kept=kept), True)


def test_bad_message_flags_only_its_own_deliveries(D):
    t = host(D)
    t.set([1], [5], qos=1, nl=1, subid=3)
    t.commit()
    got = t.enrich_host([0, 1, 3, 4, 5], [5] * 5, [1] * 5, [1, 3, 1, 1], [0, 0, 4, 1], [5, 5, 5, 9], compact=True)
    assert got.opts.tolist() == [1 | R.OUT_NL | R.OUT_DROP, 0x40, 0x40, 0x40, 1 | R.OUT_NL]
    assert got.subids.tolist() == [3, 0, 0, 0, 3]
    assert got.kept.offsets.tolist() == [0, 0, 2, 3, 4]  # a bad message's deliveries are kept
    assert got.summary == {"flags": 0, "deliveries": 5, "kept": 4, "dropped_no_local": 1, "no_subopts": 0,
                           "qos0": 0, "qos1": 1, "qos2": 0}


@pytest.mark.parametrize("name, mode", C.SHAPE_CASES)
def test_shapes(D, name, mode):
    case = C.shape(name, mode)
    t = case.load(host(D))
    C.check(case, t.enrich_host(*case.batch, compact=True), True)
    s = case.reference()["summary"]
    if mode == "all":
        assert s[2] == 0 and s[3] == s[1]
    if mode == "none":
        assert s[3] == 0
    if mode == "mixed" and s[1] >= 63:
        assert s[2] > 0 and s[3] > 0, "the shape mixes kept and dropped deliveries"


@pytest.mark.parametrize("pct", [50, 90])
def test_fuzz(D, pct):
    case = C.fuzz()
    t = host(D)
    t.set_tuning("max_load_pct", pct)
    case.load(t)
    for compact in (False, True):
        C.check(case, t.enrich_host(*case.batch, compact=compact), compact)
    s = t.stats()
    assert s["n_entries"] == C.FUZZ_ENTRIES and s["n_slots"] == -(-C.FUZZ_ENTRIES * 100 // pct)
    assert 1 <= s["max_probe"] < s["n_slots"]


def test_tuning_keys(D):
    from emqx_amd import _lib
    t = host(D)
    with pytest.raises(_lib.EngineError) as e:
        t.set_tuning("no_such_key", 1)
    assert e.value.code == ENOTFOUND
    for v in (9, 96):
        with pytest.raises(_lib.EngineError) as e:
            t.set_tuning("max_load_pct", v)
        assert e.value.code == EINVAL
    case = C.shape("257", "mixed")
    case.load(t)
    before = t.enrich_host(*case.batch, compact=True)
    _grid_keys(t, 16384)
    after = t.enrich_host(*case.batch, compact=True)  # the host evaluator has no grid and no scan
    C.check(case, after, True)
    assert after.opts.tobytes() == before.opts.tobytes() and after.summary == before.summary
    assert all(x.tobytes() == y.tobytes() for x, y in zip(after.kept, before.kept))


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


def test_stats_struct_is_versioned_by_size(D):
    from emqx_amd import _lib
    t = host(D)
    s = _lib.SubOptsStats()
    s.size = 16
    s.n_slots = 12345
    assert _lib.lib().emqx_subopts_stats_get(t._h, ctypes.byref(s)) == 0
    assert s.size == 16 and s.n_entries == 0 and s.n_slots == 12345  # nothing beyond 16 bytes written
