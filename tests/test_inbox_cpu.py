"""CPU-side checks of the inbox stage (include/emqx_inbox.h) on a host-only handle: the exports,
emqx_inbox_group_host against the restatement (tests/inbox_ref.py) on every named case, the
refusals and the argument errors, and no batch call without a device."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import inbox_cases as C
from tests import inbox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5


@pytest.fixture(scope="module")
def I():  # noqa: E743
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import inbox
    return inbox


def host(I):
    return I.Inbox(I.HOST_ONLY)


def run(I, case, **kw):
    a, k = case.args()
    return host(I).group_host(*a, **k, **kw)


def test_exports_every_inbox_symbol(I):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_inbox.h")
    assert len(declared) == 9
    assert sorted(_lib.INBOX_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(I):
    import emqx_amd
    assert emqx_amd.Inbox is I.Inbox


def test_constants_mirror_the_headers(I):
    src = open(os.path.join(ROOT, "emqx_amd", "csrc", "inbox.h")).read()
    block = int(re.search(r"IB_BLOCK = (\d+);", src).group(1))
    rows = int(re.search(r"IB_ROWS = (\d+);", src).group(1))
    assert re.search(r"IB_TILE = IB_BLOCK \* IB_ROWS;", src)
    assert (I.BLOCK, I.ROWS, I.TILE) == (block, rows, block * rows) and C.T == I.TILE
    pub = open(os.path.join(ROOT, "include", "emqx_inbox.h")).read()
    for name, value in (("F_BOX_OVERFLOW", I.F_BOX_OVERFLOW), ("F_INPUT_REFUSED", I.F_INPUT_REFUSED),
                        ("F_BAD_SUB", I.F_BAD_SUB), ("SUMMARY_WORDS", I.SUMMARY_WORDS)):
        assert int(re.search(r"#define EMQX_INBOX_%s (\w+?)u?\b" % name, pub).group(1), 0) == value
    assert (R.F_BOX_OVERFLOW, R.F_INPUT_REFUSED, R.F_BAD_SUB) == (1, 2, 4) and len(I.SUMMARY) == 8 == len(C.SUMMARY)


@pytest.mark.parametrize("limit, want", [(1, 1), (2, 1), (255, 1), (256, 1), (257, 2), (65536, 2), (65537, 3),
                                         (1 << 24, 3), ((1 << 24) + 1, 4), (1 << 32, 4)])
def test_passes(I, limit, want):
    assert I.passes(limit) == want
    h = host(I)
    h.group_host([0, 1], [0], [7], limit)
    assert h.stats()["last_passes"] == want


def test_batch_calls_need_a_device(I):
    from emqx_amd import _lib
    h = host(I)
    case = C.two_filters()
    a, k = case.args()
    with pytest.raises(_lib.EngineError) as e:
        h.group(*a, **k)
    assert e.value.code == EDEVICE
    b = I.Inbox.batch(0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0)
    with pytest.raises(_lib.EngineError) as e:
        h.group_device(b)
    assert e.value.code == EDEVICE
    with pytest.raises(_lib.EngineError) as e:
        h.group_device_async(b, 0)
    assert e.value.code == EDEVICE
    with pytest.raises(_lib.EngineError) as e:
        h.reserve(1000, 1000)
    assert e.value.code == EDEVICE


@pytest.mark.parametrize("name", C.TINY_CASES)
def test_tiny(I, name):
    case = C.tiny(name)
    got = run(I, case)
    C.check(case.reference(), got)
    assert got.inbox_offsets.tolist() == ([0] if case.total == 0 else [0, 1])


@pytest.mark.parametrize("total, mode", C.SHAPE_CASES)
def test_shapes(I, total, mode):
    case = C.shape(total, mode)
    ref = case.reference()
    got = run(I, case)
    C.check(ref, got)
    if mode == "one_sub":
        assert got.src.tolist() == list(range(total)) and ref["summary"][2:4] == [1, total]
    if mode == "distinct_desc":
        assert got.src.tolist() == list(range(total - 1, -1, -1)) and ref["summary"][2:4] == [total, 1]
    if mode == "alternating":
        assert got.inbox_subs.tolist() == [3, 0x10203] and got.src[:2].tolist() == [1, 3]


@pytest.mark.parametrize("sub_limit", C.SUB_LIMITS)
def test_digit_edges(I, sub_limit):
    case = C.digit_edge(sub_limit)
    got = run(I, case)
    C.check(case.reference(), got)
    assert got.inbox_subs[0] == 0 and got.inbox_subs[-1] == sub_limit - 1
    if sub_limit == 1 << 32:
        assert got.inbox_subs[-2] == 0xFFFFFFFE


def test_two_filters_of_one_message_keep_order_and_bits(I):
    case = C.two_filters()
    got = run(I, case)
    C.check(case.reference(), got)
    lo, hi = got.inbox_offsets[-2:].tolist()  # subscriber 9
    assert got.inbox_subs.tolist() == [4, 7, 9]
    assert got.msgs[lo:hi].tolist() == [0, 1, 1, 2]
    assert got.filters[lo:hi].tolist() == [11, 21 | R.SHARED_BIT | R.RETRY_BIT, 23, 31 | R.RETRY_BIT]


def test_empty_messages(I):
    case = C.empty_messages()
    got = run(I, case)
    C.check(case.reference(), got)
    assert sorted(set(got.msgs.tolist())) == [2, 6, 7, 9] and got.summary["messages"] == 4


def test_fuzz(I):
    case = C.fuzz()
    ref = case.reference()
    assert 4000 < ref["summary"][1] < 6000 and ref["summary"][3] > 300 and ref["summary"][2] > 200
    C.check(ref, run(I, case))


def test_fuzz_wide(I):
    case = C.fuzz_wide()
    assert I.passes(case.sub_limit) == 3 and case.total > 8 * C.T
    C.check(case.reference(), run(I, case))


@pytest.mark.parametrize("absent", ["opts", "subids", "src"])
def test_optional_outputs(I, absent):
    case = C.fuzz()
    want = {"opts": absent != "opts", "subids": absent != "subids"}
    a, k = case.args(**want)
    got = host(I).group_host(*a, **k, src=absent != "src")
    C.check(case.reference(**want), got, src=absent != "src", **want)


def test_offsets_over_cap_in_are_refused(I):
    from emqx_amd import _lib
    case = C.shape(65, "alternating")
    with pytest.raises(_lib.EngineError) as e:
        run(I, case, cap_in=64)
    assert e.value.code == EINVAL
    assert [e.value.summary[k] for k in C.SUMMARY] == [R.F_INPUT_REFUSED, 65, 0, 0, 0, 0, 0, 0]
    assert [e.value.summary[k] for k in C.SUMMARY] == case.reference(cap_in=64)["summary"]


def test_bad_subscriber(I):
    from emqx_amd import _lib
    case = C.shape(65, "alternating")
    a, k = case.args()
    with pytest.raises(_lib.EngineError) as e:
        host(I).group_host(a[0], a[1], a[2], 0x10203, **k)  # the larger id equals the limit
    assert e.value.code == EINVAL
    ref = R.group(a[0], a[1], a[2], 0x10203)
    assert [e.value.summary[k] for k in C.SUMMARY] == ref["summary"] and ref["summary"][0] == R.F_BAD_SUB
    assert ref["summary"][2] == 0 and ref["summary"][4] > 0
    C.check(R.group(a[0], a[1], a[2], 0x10204, case.opts, case.subids), host(I).group_host(a[0], a[1], a[2], 0x10204, **k))


@pytest.mark.parametrize("cap", ["m-1", 1, 0])
def test_box_overflow(I, cap):
    from emqx_amd import _lib
    case = C.fuzz()
    m = case.reference()["summary"][2]
    cap_boxes = m - 1 if cap == "m-1" else cap
    ref = case.reference(cap_boxes=cap_boxes)
    with pytest.raises(_lib.EngineError) as e:
        run(I, case, cap_boxes=cap_boxes)
    assert e.value.code == EOVERFLOW and e.value.needed == m
    assert ref["summary"][0] == R.F_BOX_OVERFLOW and len(ref["inbox_offsets"]) == cap_boxes + 1
    C.check(ref, e.value.partial)
    C.check(case.reference(cap_boxes=m), run(I, case, cap_boxes=m))


def test_bad_offsets(I):
    from emqx_amd import _lib
    h = host(I)
    for off in ([0, 2, 1, 3], [1, 2, 3, 3]):
        with pytest.raises(_lib.EngineError) as e:
            h.group_host(off, [1, 2, 3], [1, 2, 3], 16)
        assert e.value.code == EINVAL


@pytest.mark.parametrize("what", ["sub_limit0", "sub_limit_over", "no_offsets", "no_box_msgs", "opts_without_input",
                                  "subids_without_input", "no_inbox_offsets", "no_inbox_subs"])
def test_argument_errors(I, what):
    from emqx_amd import _lib
    h = host(I)
    off, subs, fils = (np.array(x, dtype=t) for x, t in (([0, 2], np.uint64), ([1, 2], np.uint32), ([5, 6], np.uint32)))
    out = [np.zeros(4, dtype=np.uint32) for _ in range(5)]
    o8, ioff = np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    kw = dict(offsets=p(off), subs=p(subs), filters=p(fils), n=1, cap_in=2, sub_limit=8, box_msgs=p(out[0]),
              box_filters=p(out[1]), inbox_subs=p(out[2]), inbox_offsets=p(ioff), cap_boxes=2)
    kw.update({"sub_limit0": dict(sub_limit=0), "sub_limit_over": dict(sub_limit=(1 << 32) + 1),
               "no_offsets": dict(offsets=None), "no_box_msgs": dict(box_msgs=None),
               "opts_without_input": dict(box_opts=p(o8)), "subids_without_input": dict(box_subids=p(out[3])),
               "no_inbox_offsets": dict(inbox_offsets=None), "no_inbox_subs": dict(inbox_subs=None)}[what])
    b = _lib.InboxBatch(**kw)
    assert _lib.lib().emqx_inbox_group_host(h._h, ctypes.byref(b), None, None) == EINVAL
    assert not out[0].any() and not ioff.any()
    assert _lib.lib().emqx_inbox_group_host(None, ctypes.byref(b), None, None) == EINVAL


def test_tuning_keys(I):
    from emqx_amd import _lib
    h = host(I)
    with pytest.raises(_lib.EngineError) as e:
        h.set_tuning("no_such_key", 1)
    assert e.value.code == ENOTFOUND
    for v in (-1, 2):
        with pytest.raises(_lib.EngineError) as e:
            h.set_tuning("path", v)
        assert e.value.code == EINVAL
    h.set_tuning("path", 1)
    assert h.stats()["path"] == 1
    case = C.fuzz()
    a, k = case.args()
    before = h.group_host(*a, **k)
    _grid_keys(h, 16384)
    after = h.group_host(*a, **k)  # the host evaluator has no grid and no scan
    C.check(case.reference(), after)
    C.same(after, before)


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


def test_stats_struct_is_versioned_by_size(I):
    from emqx_amd import _lib
    h = host(I)
    h.group_host([0, 1], [0], [7], 4)
    s = _lib.InboxStats()
    s.size = 16
    s.sub_limit = 12345
    assert _lib.lib().emqx_inbox_stats_get(h._h, ctypes.byref(s)) == 0
    assert s.size == 16 and s.cap_in == 0 and s.sub_limit == 12345  # nothing beyond 16 bytes written
    assert h.stats()["calls"] == 1
