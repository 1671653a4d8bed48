"""The route table's host side over the C ABI (include/emqx_route.h) on a HOST_ONLY handle: every
case of tests/route_cases.py through emqx_route_host, exact against tests/route_ref.py; add /
remove / purge sequences against the reference's bag; every refusal code; stats by size."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import route_cases as RC
from tests import route_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True, capture_output=True)
    from emqx_amd import _lib
    return _lib.lib()


def test_exports_every_route_symbol(L):
    from emqx_amd import _lib
    src = open(os.path.join(ROOT, "include", "emqx_route.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(emqx_[a-z_]+)\s*\(", src)))
    assert sorted(_lib.ROUTE_EXPORTS) == declared and len(declared) == 13
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, nm), name


@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_host_case(L, name):
    from emqx_amd.route import HOST_ONLY, RouteTable
    case = RC.BY_NAME[name]
    t = RouteTable(HOST_ONLY, case.local)
    RC.fill_table(t, case)
    got = t.route_host(case.offsets, case.filters)
    RC.check(case, got)
    again = t.route_host(case.offsets, case.filters)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:-1], again[:-1]))
    t.set_tuning("scan_chunk", 1)  # a host-only table accepts it; the host evaluator has no scan
    again = t.route_host(case.offsets, case.filters)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:-1], again[:-1])) and again.summary == got.summary
    t.close()


def test_host_capacity(L):
    """cap_fwd one below the forward count and exactly at it."""
    from emqx_amd.route import F_FWD_OVERFLOW, HOST_ONLY, EngineError, RouteTable
    case = RC.BY_NAME["fuzz_1"]
    exp = RC.expected(case.name)
    t = RouteTable(HOST_ONLY, case.local)
    RC.fill_table(t, case)
    need = exp.summary["forwards"]
    RC.check(case, t.route_host(case.offsets, case.filters, cap_fwd=need))
    with pytest.raises(EngineError) as ei:
        t.route_host(case.offsets, case.filters, cap_fwd=need - 1)
    e = ei.value
    assert e.code == -4 and e.needed == need and e.summary["flags"] == F_FWD_OVERFLOW
    r = e.result
    assert not r.fwd_msgs.any() and not r.fwd_filters.any()  # untouched
    full = t.route_host(case.offsets, case.filters)
    assert r.node_offsets.tolist() == full.node_offsets.tolist()  # complete
    assert r.msg_routes.tolist() == exp.msg_routes and r.entry_flags.tolist() == exp.entry_flags
    assert r.local_filters.tolist() == full.local_filters.tolist()
    assert {k: v for k, v in e.summary.items() if k != "flags"} == {k: v for k, v in exp.summary.items() if k != "flags"}


def test_add_remove_purge_against_ref(L):
    from emqx_amd.route import HOST_ONLY, NO_GROUP, EngineError, RouteTable
    rng = random.Random(9)
    t, ref = RouteTable(HOST_ONLY, 0), R.RouteTab(RC.node_name(0))
    ids = list(range(60))

    def dest(v, g):
        return RC.node_name(v) if g is None else (RC.group_name(g), RC.node_name(v))

    def same():
        for f in ids:
            exp = [r.dest for r in ref.lookup_routes(RC.filter_name(f))]
            got = [dest(v, None if g == NO_GROUP else g) for v, g in t.lookup(f)]
            assert got == exp, f  # insertion order

    for step in range(600):
        f, v = rng.choice(ids), rng.randrange(6)
        g = None if rng.random() < 0.6 else rng.randrange(3)
        if rng.random() < 0.75:
            t.add([f], [v], [NO_GROUP if g is None else g])
            ref.do_add_route(RC.filter_name(f), dest(v, g))
        else:
            t.remove([f], [v], [NO_GROUP if g is None else g])
            ref.do_delete_route(RC.filter_name(f), dest(v, g))
        if step % 97 == 0:
            same()
    same()
    # cleanup_routes/1: the filters left without a dest are reported; too small a room removes nothing
    before = {f for f in ids if ref.has_routes(RC.filter_name(f))}
    ref.cleanup_routes(RC.node_name(2))
    emptied = sorted(f for f in before if not ref.has_routes(RC.filter_name(f)))
    t.add([100, 101], [2, 2], [NO_GROUP, 4])  # two more that only node 2 holds
    emptied += [100, 101]
    with pytest.raises(EngineError) as ei:
        t.purge_node(2, cap=len(emptied) - 1)
    assert ei.value.code == -4 and ei.value.needed == len(emptied)
    assert t.lookup(100) == [(2, NO_GROUP)]  # nothing was removed
    assert t.purge_node(2).tolist() == emptied
    same()
    assert t.lookup(100) == [] and t.purge_node(2).tolist() == []
    # stats of the committed snapshot
    t.commit()
    s = t.stats()
    plain = sum(1 for r in ref.tab if isinstance(r.dest, str))
    assert s["n_filters"] == len(ref.topics()) and s["n_plain"] == plain and s["n_grouped"] == len(ref.tab) - plain
    assert s["epoch"] == 1 and s["n_nodes"] == len({r.dest if isinstance(r.dest, str) else r.dest[1] for r in ref.tab})
    assert s["last_build_ms"] >= 0.0


def test_changes_wait_for_commit(L):
    from emqx_amd.route import HOST_ONLY, LOCAL, REMOTE, RouteTable
    t = RouteTable(HOST_ONLY, 1)
    t.add([0, 0], [1, 2])
    assert t.route_host([0, 1], [0]).entry_flags.tolist() == [0]
    t.commit()
    assert t.route_host([0, 1], [0]).entry_flags.tolist() == [LOCAL | REMOTE]
    t.remove([0], [2])
    assert t.route_host([0, 1], [0]).entry_flags.tolist() == [LOCAL | REMOTE]
    t.commit()
    r = t.route_host([0, 1], [0])
    assert r.entry_flags.tolist() == [LOCAL] and r.msg_routes.tolist() == [1] and r.summary["forwards"] == 0


def test_refusals(L):
    from emqx_amd import _lib
    from emqx_amd._lib import RouteBatch
    from emqx_amd.route import HOST_ONLY, RouteTable
    h = ctypes.c_void_p()
    assert L.emqx_routetab_create(HOST_ONLY, 64, ctypes.byref(h)) == _lib.EMQX_EINVAL and not h.value
    assert L.emqx_routetab_create(-7, 0, ctypes.byref(h)) == _lib.EMQX_EINVAL
    assert L.emqx_routetab_create(HOST_ONLY, 0, None) == _lib.EMQX_EINVAL
    t = RouteTable(HOST_ONLY, 63)
    one = np.array([1], np.uint32)
    for f, v in (([1 << 30], [0]), ([0], [64]), ([0xFFFFFFFF], [0])):
        f, v = np.array(f, np.uint32), np.array(v, np.uint32)
        assert L.emqx_routetab_add(t._h, f.ctypes.data, v.ctypes.data, None, 1) == _lib.EMQX_EINVAL
        assert L.emqx_routetab_remove(t._h, f.ctypes.data, v.ctypes.data, None, 1) == _lib.EMQX_EINVAL
    # all of a call is checked before any of it is applied
    f, v = np.array([5, 6, 1 << 30], np.uint32), np.array([1, 1, 1], np.uint32)
    assert L.emqx_routetab_add(t._h, f.ctypes.data, v.ctypes.data, None, 3) == _lib.EMQX_EINVAL
    assert t.lookup(5) == []
    assert L.emqx_routetab_add(t._h, None, one.ctypes.data, None, 1) == _lib.EMQX_EINVAL
    assert L.emqx_routetab_add(None, one.ctypes.data, one.ctypes.data, None, 1) == _lib.EMQX_EINVAL
    assert L.emqx_routetab_purge_node(t._h, 64, None, 0, None) == _lib.EMQX_EINVAL
    assert L.emqx_routetab_set_tuning(t._h, b"nope", 1) == _lib.EMQX_ENOTFOUND
    assert L.emqx_routetab_set_tuning(t._h, b"max_blocks", 0) == _lib.EMQX_EINVAL
    assert L.emqx_routetab_set_tuning(t._h, b"path", 2) == _lib.EMQX_EINVAL
    assert L.emqx_routetab_set_tuning(t._h, b"stored_mask", 2) == _lib.EMQX_EINVAL
    assert L.emqx_routetab_set_tuning(t._h, b"stored_mask", 1) == _lib.EMQX_OK
    assert L.emqx_routetab_set_tuning(t._h, b"path", 1) == _lib.EMQX_OK
    assert L.emqx_routetab_set_tuning(t._h, b"max_blocks", 2) == _lib.EMQX_OK
    for v, rc in ((1, _lib.EMQX_OK), (1024, _lib.EMQX_OK), (0, _lib.EMQX_EINVAL), (-1, _lib.EMQX_EINVAL), (1025, _lib.EMQX_EINVAL)):
        assert L.emqx_routetab_set_tuning(t._h, b"scan_chunk", v) == rc
    t.add([1, 2], [0, 63])
    t.commit()

    fil = np.array([1, 2], np.uint32)
    routes, node_off = np.zeros(2, np.uint32), np.zeros(65, np.uint64)
    fm, ff = np.zeros(4, np.uint32), np.zeros(4, np.uint32)

    def call(offsets, fn=L.emqx_route_host, cap_in=2, **kw):
        off = np.array(offsets, np.uint64)
        args = dict(offsets=off.ctypes.data, filters=fil.ctypes.data, n=off.size - 1, cap_in=cap_in,
                    msg_routes=routes.ctypes.data, node_offsets=node_off.ctypes.data, fwd_msgs=fm.ctypes.data,
                    fwd_filters=ff.ctypes.data, cap_fwd=4)
        args.update(kw)
        return fn(t._h, ctypes.byref(RouteBatch(**args)), None, None)

    assert call([0, 1, 2]) == _lib.EMQX_OK and routes.tolist() == [1, 1] and int(node_off[64]) == 1
    assert call([1, 1, 2]) == _lib.EMQX_EINVAL      # offsets[0] != 0
    assert call([0, 2, 1]) == _lib.EMQX_EINVAL      # decreasing
    assert call([0, 1, 3]) == _lib.EMQX_EINVAL      # offsets[n] > cap_in
    assert call([0, 1, 2], node_offsets=None) == _lib.EMQX_EINVAL
    assert call([0, 1, 2], msg_routes=None) == _lib.EMQX_EINVAL
    assert call([0, 1, 2], fwd_msgs=None) == _lib.EMQX_EINVAL
    assert call([0, 1, 2], local_filters=fil.ctypes.data) == _lib.EMQX_EINVAL  # the pair, or neither
    assert L.emqx_route_host(t._h, None, None, None) == _lib.EMQX_EINVAL
    # a handle without a device never answers a batch call on the host silently
    assert call([0, 1, 2], fn=L.emqx_route_batch) == _lib.EMQX_EDEVICE
    b = RouteBatch()
    summary = np.zeros(8, np.uint64)
    assert L.emqx_route_batch_device(t._h, ctypes.byref(b), None, None, None) == _lib.EMQX_EDEVICE
    assert L.emqx_route_batch_device_async(t._h, ctypes.byref(b), summary.ctypes.data, None) == _lib.EMQX_EDEVICE


def test_stats_versioned_by_size(L):
    from emqx_amd import _lib
    from emqx_amd._lib import RouteTabStats
    from emqx_amd.route import HOST_ONLY, RouteTable
    t = RouteTable(HOST_ONLY, 0)
    t.add([3, 3, 4], [0, 1, 1], [0xFFFFFFFF, 0xFFFFFFFF, 2])
    t.commit()
    s = RouteTabStats()
    assert ctypes.sizeof(s) == 64
    assert L.emqx_routetab_stats_get(t._h, ctypes.byref(s)) == 0 and s.size == 64
    assert (s.n_filters, s.n_plain, s.n_grouped, s.n_nodes, s.epoch) == (2, 2, 1, 2, 1)
    old = RouteTabStats()  # a caller built against a shorter struct: only its bytes are written
    old.size = 24
    old.n_grouped = 777
    assert L.emqx_routetab_stats_get(t._h, ctypes.byref(old)) == 0
    assert old.size == 24 and old.n_filters == 2 and old.n_plain == 2 and old.n_grouped == 777
    new = (ctypes.c_uint64 * 16)()  # a caller built against a longer one
    new[0] = 128
    new[9] = 555
    assert L.emqx_routetab_stats_get(t._h, new) == 0 and new[0] == 64 and new[1] == 2 and new[9] == 555
    small = RouteTabStats()
    small.size = 4
    assert L.emqx_routetab_stats_get(t._h, ctypes.byref(small)) == _lib.EMQX_EINVAL
