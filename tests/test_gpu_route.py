"""The route stage on the device (include/emqx_route.h): every case of tests/route_cases.py
through emqx_route_batch, _device and _device_async on path 0 (with and without the stored
word) and path 1, with the grid at its default and capped at 2 blocks, exact against tests/route_ref.py and byte-identical to emqx_route_host;
capacity and refusal; snapshot lifetime across commit, remove and purge; two handles on two
streams; and the match -> route -> fan-out chain of ClusterRouter on one stream."""

import os
import subprocess

import numpy as np
import pytest

from tests import route_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S8, S32, S64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
TAIL = 64   # sentinel elements behind every output's capacity
SLACK = 100  # cap_in above the entry count


@pytest.fixture(scope="module")
def M():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True, capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import route
    return route


def dev(a, dtype, room=0):
    import torch
    view = {np.uint64: np.int64, np.uint32: np.int32}.get(dtype, dtype)
    a = np.concatenate((np.asarray(a, dtype=dtype).reshape(-1), np.zeros(max(room, 1), dtype=dtype)))
    return torch.from_numpy(a.view(view)).to(DEV)


def host(t, view):
    return t.cpu().numpy().view(view)


class DeviceBatch:
    """A case's batch in device memory: cap_in above the count, sentinel-filled outputs and a
    guard of TAIL sentinels behind each."""

    def __init__(self, M, case, cap_fwd, slack=SLACK):
        import torch
        self.n, self.total = len(case.offsets) - 1, len(case.filters)
        self.cap_in, self.cap_fwd = self.total + slack, cap_fwd
        self.off, self.fil = dev(case.offsets, np.uint64), dev(case.filters, np.uint32, slack)

        def full(count, fill, dtype):
            return torch.full((count + TAIL,), fill, dtype=dtype, device=DEV)

        self.flags = full(self.cap_in, S8, torch.uint8)
        self.routes = full(self.n, S32, torch.int32)
        self.node_off = full(65, S64, torch.int64)
        self.fm, self.ff = full(cap_fwd, S32, torch.int32), full(cap_fwd, S32, torch.int32)
        self.loff = full(self.n + 1, S64, torch.int64)
        self.lfil = full(self.cap_in, S32, torch.int32)
        self.summary = torch.full((8,), S64, dtype=torch.int64, device=DEV)
        self.args = M.RouteTable.batch(self.off.data_ptr(), self.fil.data_ptr(), self.n, self.cap_in,
                                       self.flags.data_ptr(), self.routes.data_ptr(), self.node_off.data_ptr(),
                                       self.fm.data_ptr(), self.ff.data_ptr(), cap_fwd, self.loff.data_ptr(),
                                       self.lfil.data_ptr())

    def outputs(self):
        return dict(flags=host(self.flags, np.uint8), routes=host(self.routes, np.uint32),
                    node_off=host(self.node_off, np.uint64), fm=host(self.fm, np.uint32), ff=host(self.ff, np.uint32),
                    loff=host(self.loff, np.uint64), lfil=host(self.lfil, np.uint32))

    def summary_dict(self, M):
        return dict(zip(M.SUMMARY, host(self.summary, np.uint64).tolist()))

    def result(self, M, summary=None, overflow=False):
        """The outputs as a Routed; everything behind what the call may write is still sentinel."""
        sm = self.summary_dict(M) if summary is None else summary
        o = self.outputs()
        fwd = 0 if overflow else sm["forwards"]
        assert (o["flags"][self.total:] == S8).all() and (o["routes"][self.n:] == S32).all()
        assert (o["node_off"][65:] == S64).all() and (o["loff"][self.n + 1:] == S64).all()
        assert (o["fm"][fwd:] == S32).all() and (o["ff"][fwd:] == S32).all()
        assert (o["lfil"][sm["kept"]:] == S32).all()
        return M.Routed(o["flags"][:self.total], o["routes"][:self.n], o["node_off"][:65], o["fm"][:fwd], o["ff"][:fwd],
                        o["loff"][:self.n + 1], o["lfil"][:sm["kept"]], sm)


def run_sync(M, t, case, cap_fwd):
    b = DeviceBatch(M, case, cap_fwd)
    return b.result(M, t.route_device(b.args))


def run_async(M, t, case, cap_fwd):
    import torch
    b = DeviceBatch(M, case, cap_fwd)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        t.route_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(M)


def same_bytes(a, b):
    return a.summary == b.summary and all(x.tobytes() == y.tobytes() for x, y in zip(a[:-1], b[:-1]))


def table_of(M, case, path=0, max_blocks=None, stored_mask=0):
    t = M.RouteTable(0, case.local)
    RC.fill_table(t, case)
    t.set_tuning("path", path)
    t.set_tuning("stored_mask", stored_mask)
    if max_blocks is not None:
        t.set_tuning("max_blocks", max_blocks)
    return t


# path 0 with the second pass gathering the records again or reading pass 1's per-entry word, and path 1
VARIANTS = [(0, 0), (0, 1), (1, 0)]


@pytest.mark.parametrize("max_blocks", [None, 2])
@pytest.mark.parametrize("path, stored_mask", VARIANTS)
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_case_every_form(M, name, path, stored_mask, max_blocks):
    case = RC.BY_NAME[name]
    t = table_of(M, case, path, max_blocks, stored_mask)
    ref = t.route_host(case.offsets, case.filters)
    RC.check(case, ref)
    need = ref.summary["forwards"]
    for got in (t.route_packed(case.offsets, case.filters), t.route_packed(case.offsets, case.filters, cap_fwd=need),
                run_sync(M, t, case, need), run_async(M, t, case, need + 3)):
        RC.check(case, got)
        assert same_bytes(got, ref)
    t.close()


@pytest.mark.parametrize("path, stored_mask", VARIANTS)
@pytest.mark.parametrize("form", ["host_buffers", "device", "async"])
def test_capacity_one_below(M, form, path, stored_mask):
    """cap_fwd one below the forward count: the flag, node_offsets and every other output
    complete, fwd_* untouched; exactly at it is covered by test_case_every_form."""
    import torch
    case = RC.BY_NAME["fuzz_2"]
    t = table_of(M, case, path, stored_mask=stored_mask)
    ref = t.route_host(case.offsets, case.filters)
    need = ref.summary["forwards"]
    want = dict(ref.summary, flags=M.F_FWD_OVERFLOW)
    if form == "host_buffers":
        with pytest.raises(M.EngineError) as ei:
            t.route_packed(case.offsets, case.filters, cap_fwd=need - 1)
        assert ei.value.code == -4 and ei.value.needed == need and ei.value.summary == want
        r = ei.value.result
        assert not r.fwd_msgs.any() and not r.fwd_filters.any()
    else:
        b = DeviceBatch(M, case, need - 1)
        if form == "device":
            with pytest.raises(M.EngineError) as ei:
                t.route_device(b.args)
            assert ei.value.code == -4 and ei.value.needed == need and ei.value.summary == want
        else:
            t.route_device_async(b.args, b.summary.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert b.summary_dict(M) == want
        r = b.result(M, want, overflow=True)
    assert r.node_offsets.tolist() == ref.node_offsets.tolist()
    assert r.msg_routes.tolist() == ref.msg_routes.tolist() and r.entry_flags.tolist() == ref.entry_flags.tolist()
    assert r.local_offsets.tolist() == ref.local_offsets.tolist() and r.local_filters.tolist() == ref.local_filters.tolist()
    t.close()


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("form", ["device", "async"])
def test_input_refused(M, form, path):
    """offsets[n] > cap_in: nothing read or written but the summary."""
    import torch
    case = RC.BY_NAME["total_2049_n_7"]
    t = table_of(M, case, path)
    b = DeviceBatch(M, case, 5000, slack=-1)  # cap_in one below the count
    assert b.cap_in == b.total - 1
    if form == "device":
        with pytest.raises(M.EngineError) as ei:
            t.route_device(b.args)
        assert ei.value.code == -1
        sm = ei.value.summary
    else:
        t.route_device_async(b.args, b.summary.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        sm = b.summary_dict(M)
    assert sm == dict(flags=M.F_INPUT_REFUSED, entries=b.total, forwards=0, dropped=0, forwarding_messages=0, kept=0,
                      unknown=0, forward_nodes=0)
    o = b.outputs()
    assert (o["flags"] == S8).all() and (o["routes"] == S32).all() and (o["node_off"] == S64).all()
    assert (o["fm"] == S32).all() and (o["ff"] == S32).all() and (o["loff"] == S64).all() and (o["lfil"] == S32).all()
    t.close()


@pytest.mark.parametrize("path, stored_mask", VARIANTS)
def test_wild_device_offsets_stay_in_bounds(M, path, stored_mask):
    """Offsets that are no CSR (decreasing, beyond the count) with offsets[n] within cap_in: the
    device forms do not check them; every access stays inside the buffers (the guards hold)."""
    case = RC.BY_NAME["total_2049_n_7"]
    off = case.offsets.copy()
    off[1], off[2], off[3], off[4] = 3000, 5, 1 << 40, 7
    wild = case._replace(offsets=off)
    t = table_of(M, case, path, stored_mask=stored_mask)
    b = DeviceBatch(M, wild, 3 * len(case.filters))
    sm = t.route_device(b.args)
    o = b.outputs()
    assert sm["entries"] == len(case.filters) and sm["flags"] == 0
    assert (o["flags"][b.total:] == S8).all() and (o["routes"][b.n:] == S32).all() and (o["loff"][b.n + 1:] == S64).all()
    assert (o["fm"][sm["forwards"]:] == S32).all() and (o["lfil"][sm["kept"]:] == S32).all()
    # what does not depend on the message boundaries is still right
    ref = t.route_host(case.offsets, case.filters)
    assert o["flags"][:b.total].tolist() == ref.entry_flags.tolist() and sm["forwards"] == ref.summary["forwards"]
    assert o["node_off"][:65].tolist() == ref.node_offsets.tolist()
    assert o["lfil"][:sm["kept"]].tolist() == ref.local_filters.tolist()
    t.close()


def test_optional_outputs_absent(M):
    """entry_flags and the local CSR are optional."""
    case = RC.BY_NAME["fuzz_3"]
    t = table_of(M, case)
    ref = t.route_host(case.offsets, case.filters)
    b = DeviceBatch(M, case, ref.summary["forwards"])
    b.args.entry_flags = None
    b.args.local_offsets = None
    b.args.local_filters = None
    sm = t.route_device(b.args)
    o = b.outputs()
    assert sm == ref.summary
    assert (o["flags"] == S8).all() and (o["loff"] == S64).all() and (o["lfil"] == S32).all()
    assert o["fm"][:sm["forwards"]].tolist() == ref.fwd_msgs.tolist()
    assert o["routes"][:b.n].tolist() == ref.msg_routes.tolist()
    t.close()


def test_async_call_keeps_its_snapshot_across_a_commit(M):
    import torch
    case = RC.BY_NAME["fuzz_1"]
    t = table_of(M, case)
    ref = t.route_host(case.offsets, case.filters)
    b = DeviceBatch(M, case, ref.summary["forwards"])
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        t.route_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    f, v, g = zip(*case.dests)  # everything goes; the call in flight reads the snapshot it started on
    t.remove(list(f), list(v), [RC.NO_GROUP if x is None else x for x in g])
    t.commit()
    stream.synchronize()
    assert same_bytes(b.result(M), ref)
    # the empty table, recommitted: nothing is known
    empty = t.route_packed(case.offsets, case.filters)
    assert empty.summary["unknown"] == len(case.filters) and empty.summary["forwards"] == 0
    assert empty.summary["dropped"] == len(case.offsets) - 1 and not empty.entry_flags.any()
    assert t.stats()["n_filters"] == 0 and t.stats()["epoch"] == 2
    RC.fill_table(t, case)
    assert same_bytes(t.route_packed(case.offsets, case.filters), ref)
    t.close()


@pytest.mark.parametrize("path", [0, 1])
def test_purge_then_batch(M, path):
    from tests import route_ref as R
    case = RC.BY_NAME["fuzz_2"]
    gone = (case.local + 1) % 9
    t = table_of(M, case, path)
    emptied = t.purge_node(gone)
    t.commit()
    tab, names = RC.ref_table(case)
    tab.cleanup_routes(RC.node_name(gone))
    assert sorted(emptied.tolist()) == sorted(f for f, to in names.items() if not tab.has_routes(to))
    exp = R.route_batch(tab, names, case.offsets.tolist(), case.filters.tolist())
    got = t.route_packed(case.offsets, case.filters)
    RC.check(case, got, exp)
    assert RC.node_name(gone) not in exp.forwards and same_bytes(got, t.route_host(case.offsets, case.filters))
    t.close()


def test_two_handles_on_two_streams(M):
    import torch
    cases = [RC.BY_NAME["fuzz_1"], RC.BY_NAME["64_nodes_local_31"]]
    tabs = [table_of(M, c, path, stored_mask=1 - path) for path, c in enumerate(cases)]
    refs = [t.route_host(c.offsets, c.filters) for t, c in zip(tabs, cases)]
    batches = [DeviceBatch(M, c, r.summary["forwards"]) for c, r in zip(cases, refs)]
    streams = [torch.cuda.Stream(device=DEV) for _ in cases]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    for _ in range(3):  # interleaved on both streams
        for t, b, s in zip(tabs, batches, streams):
            with torch.cuda.stream(s):
                t.route_device_async(b.args, b.summary.data_ptr(), stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    for c, b, r in zip(cases, batches, refs):
        got = b.result(M)
        RC.check(c, got)
        assert same_bytes(got, r)
    for t in tabs:
        t.close()


def test_cluster_router_chain(M):
    """ClusterRouter on a 200-filter table over 3 nodes: the reference's names, then match ->
    route on one stream, then the fan-out of the local CSR on the same stream.  Its deliveries
    equal the fan-out of the full match CSR: the local subscriber table has nothing for
    remote-only filters."""
    import torch
    from emqx_amd.fanout import SubTable
    from tests import route_ref as R
    rng = np.random.default_rng(4)
    nodes = ["a@h", "b@h", "c@h"]
    cr = M.ClusterRouter("b@h", nodes=nodes)
    ref = R.RouteTab("b@h")
    filters = [b"s/%d/+" % k for k in range(120)] + [b"s/%d/#" % k for k in range(40)] + \
              [b"s/%d/x" % k for k in range(39)] + [b"#"]
    for k, f in enumerate(filters):
        dests = [nodes[int(rng.integers(0, 3))]]
        if k % 5 == 0:
            dests.append(nodes[int(rng.integers(0, 3))])
        if k % 7 == 0:
            dests.append((b"g%d" % (k % 2), nodes[int(rng.integers(0, 3))]))
        if k % 14 == 0:
            dests.append((b"g%d" % (k % 2), nodes[int(rng.integers(0, 3))]))
        for d in dests:
            cr.add_route(f, d)
            cr.add_route(f, d)  # idempotent
            ref.do_add_route(f, d)
    cr.add_route(b"gone/+", "c@h")
    cr.delete_route(b"gone/+", "c@h")
    assert not cr.has_routes(b"gone/+") and cr.engine.lookup(b"gone/+") is None
    assert sorted(cr.topics()) == sorted(ref.topics())
    assert cr.lookup_routes(filters[0]) == [M.Route(*r) for r in ref.lookup_routes(filters[0])]
    assert cr.lookup_routes(filters[70]) == [M.Route(*r) for r in ref.lookup_routes(filters[70])]
    topics = [b"s/%d/x" % int(rng.integers(0, 130)) for _ in range(150)] + [b"other"]
    got = cr.match_routes(topics[0])
    exp = ref.match_routes([f for f in filters if _matches(topics[0], f)])
    assert sorted(got, key=repr) == sorted((M.Route(*r) for r in exp), key=repr) and len(got) >= 2

    # the local subscriber table: members for the plain local routes and for every group
    st = SubTable(0)
    fids, subs, groups = [], [], []
    for f in filters:
        fid = cr.engine.lookup(f)
        for r in ref.lookup_routes(f):
            if r.dest == "b@h":
                fids += [fid, fid]
                subs += [1000 + fid, 5000 + fid]
                groups += [0xFFFFFFFF] * 2
            elif isinstance(r.dest, tuple):
                fids += [fid, fid]
                subs += [9000 + fid, 9500 + fid]
                groups += [int(r.dest[0][1:])] * 2
    st.add(fids, subs, groups)
    st.commit()

    stream = torch.cuda.Stream(device=DEV)
    msg_routes, (l_off, l_fil), fwd = cr.route_batch(topics, stream=stream)
    names = {cr.engine.lookup(f): f for f in filters}
    last = cr.last
    m_off = last["match_offsets"].cpu().numpy().view(np.uint64)
    m_ids = last["match_ids"].cpu().numpy().view(np.uint32)[:int(m_off[-1])]
    exp = R.route_batch(ref, names, m_off.tolist(), m_ids.tolist())
    assert msg_routes.tolist() == exp.msg_routes and msg_routes[-1] == 1  # b"other" matches "#" only
    assert [l_fil[int(l_off[i]):int(l_off[i + 1])].tolist() for i in range(len(topics))] == exp.local
    assert {k: list(zip(m.tolist(), f.tolist())) for k, (m, f) in fwd.items()} == exp.forwards
    assert last["summary"] == exp.summary and exp.summary["forwards"] > 100 and exp.summary["kept"] > 100

    n, cap = last["n"], 1 << 16
    keys = torch.arange(7, 7 + n, dtype=torch.int32, device=DEV)

    def fanout(d_off, d_ids, match_cap):
        o = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        s, f = torch.zeros(cap, dtype=torch.int32, device=DEV), torch.zeros(cap, dtype=torch.int32, device=DEV)
        sm = torch.zeros(4, dtype=torch.int64, device=DEV)
        with torch.cuda.stream(stream):
            st.fanout_device_async("hash_clientid", d_off.data_ptr(), d_ids.data_ptr(), n, match_cap, keys.data_ptr(),
                                   o.data_ptr(), s.data_ptr(), f.data_ptr(), cap, sm.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        o, s, f = o.cpu().numpy(), s.cpu().numpy().view(np.uint32), f.cpu().numpy().view(np.uint32)
        assert int(sm.cpu()[0]) == 0
        return [sorted(zip(s[o[i]:o[i + 1]].tolist(), f[o[i]:o[i + 1]].tolist())) for i in range(n)]

    stream.wait_stream(torch.cuda.current_stream())
    local = fanout(last["local_offsets"], last["local_filters"], last["cap"])
    full = fanout(last["match_offsets"], last["match_ids"], last["cap"])
    assert local == full and sum(map(len, full)) > 100
    # a node goes down: its dests leave, filters only it held leave the engine
    cr.cleanup_routes("c@h")
    ref.cleanup_routes("c@h")
    assert sorted(cr.topics()) == sorted(ref.topics())
    _, _, fwd = cr.route_batch(topics, stream=stream)
    assert "c@h" not in fwd and set(fwd) == {"a@h"}
    st.close()
    cr.close()


def _matches(topic: bytes, filt: bytes) -> bool:
    from emqx_amd import topic as T
    return T.match(topic, filt)
