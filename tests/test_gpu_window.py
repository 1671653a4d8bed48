"""The window stage on the device (include/emqx_window.h): every case through the three device
entry points on both paths, every output byte and the summary exact against the sequential
restatement (tests/window_ref.py) and identical to the host evaluator; nothing written past the
defined extents; the refusals; two chained batches with the table written back on the stream; the
fan-out -> enrich -> inbox -> window chain on one stream."""

import os
import subprocess

import numpy as np
import pytest

from tests import window_cases as C
from tests import window_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S8, S16, S32, S64 = 0x5A, 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64  # sentinel elements behind every output buffer's capacity


@pytest.fixture(scope="module")
def W():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import window
    return window


@pytest.fixture(scope="module", params=[(0, None), (1, None), (0, 2), (1, 2)],
                ids=["tile_scan", "wave_per_inbox", "tile_scan-2_blocks", "wave_per_inbox-2_blocks"])
def handle(W, request):
    """One handle a path for the whole module: every test also reuses the scratch of the one
    before.  Capped at 2 blocks, a block takes several tiles and groups of inboxes of every case."""
    path, max_blocks = request.param
    h = W.Window(0)
    h.set_tuning("path", path)
    if max_blocks is not None:
        h.set_tuning("max_blocks", max_blocks)
    return h


def dev(a, dtype):
    import torch
    view = {np.uint64: np.int64, np.uint32: np.int32, np.uint16: np.int16}.get(dtype, dtype)
    a = np.array(a, dtype=dtype)  # a writable copy
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)
    return torch.from_numpy(a.view(view)).to(DEV)


def dev_table(table):
    import torch
    raw = np.frombuffer(table.tobytes() or bytes(32), dtype=np.int64).copy()
    return torch.from_numpy(raw).to(DEV)


def host_table(W, t, n):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=W.SESSION)[:n].copy()


class DeviceBatch:
    """A case's batch in device memory with sentinel-filled outputs and a guard behind each."""

    def __init__(self, W, case, table=None, cap_in=None, cap_boxes=None, update_table=False, count_on_device=False):
        import torch
        self.m, self.total, self.sub_limit = case.m, case.total, case.sub_limit
        self.cap_in = self.total if cap_in is None else cap_in
        self.cap_boxes = self.m if cap_boxes is None else cap_boxes
        self.subs, self.off, self.opts = dev(case.subs, np.uint32), dev(case.offsets, np.uint64), dev(case.opts, np.uint8)
        self.table = dev_table(case.table) if table is None else table
        self.count = dev([case.m], np.uint64) if count_on_device else None

        def filled(k, dtype):  # every byte 0x5A
            sent = {torch.uint8: S8, torch.int16: S16, torch.int32: S32, torch.int64: S64}[dtype]
            return torch.full((k + GUARD,), sent, dtype=dtype, device=DEV)

        self.ver, self.ids = filled(self.cap_in, torch.uint8), filled(self.cap_in, torch.int16)
        self.recs, self.cnt = filled(4 * self.cap_boxes, torch.int64), filled(4 * self.cap_boxes, torch.int32)
        self.summary = filled(8, torch.int64)
        self.args = W.Window.batch(self.subs.data_ptr(), self.off.data_ptr(), self.opts.data_ptr(),
                                   0 if count_on_device else self.m, self.cap_in, self.cap_boxes, self.table.data_ptr(),
                                   self.sub_limit, self.ver.data_ptr(), self.ids.data_ptr(), self.recs.data_ptr(),
                                   self.cnt.data_ptr(), update_table=update_table,
                                   d_n_boxes=self.count.data_ptr() if count_on_device else 0)

    def result(self, W, summary=None):
        """The outputs up to their defined extents, after checking that nothing behind them changed."""
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(W.SUMMARY, s[:8].tolist()))
        refused = summary["flags"] & R.F_INPUT_REFUSED
        total = 0 if refused else summary["deliveries"]
        m = 0 if refused else summary["inboxes"]
        ver, ids = self.ver.cpu().numpy(), self.ids.cpu().numpy().view(np.uint16)
        recs, cnt = self.recs.cpu().numpy().view(np.uint64), self.cnt.cpu().numpy().view(np.uint32)
        assert (ver[total:] == S8).all() and (ids[total:] == S16).all(), "a write past the defined extent"
        assert (recs[4 * m:] == S64).all() and (cnt[4 * m:] == S32).all(), "a write past the defined extent"
        return W.Admitted(ver[:total], ids[:total], np.frombuffer(recs[:4 * m].tobytes(), dtype=W.SESSION),
                          cnt[:4 * m].reshape(-1, 4), summary)


def run_host_buffers(W, h, case):
    from emqx_amd import _lib
    try:
        return h.run(case.subs, case.offsets, case.opts, case.table.copy())
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] == R.F_BAD_SUB
        return e.partial


def run_sync(W, h, case, **kw):
    from emqx_amd import _lib
    b = DeviceBatch(W, case, **kw)
    try:
        summary = h.run_device(b.args)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & (R.F_BAD_SUB | R.F_INPUT_REFUSED)
        summary = e.summary
    return b.result(W, summary)


def run_async(W, h, case, **kw):
    import torch
    b = DeviceBatch(W, case, **kw)
    h.reserve(b.cap_in, b.cap_boxes)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        h.run_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(W)


def all_forms(W, h, case):
    """Every device entry point: exact against the restatement, identical to the host evaluator."""
    from emqx_amd import _lib
    ref = case.reference()
    try:
        host = W.Window(W.HOST_ONLY).run_host(case.subs, case.offsets, case.opts, case.table.copy())
    except _lib.EngineError as e:
        host = e.partial
    C.check(ref, host)
    for got in (run_host_buffers(W, h, case), run_sync(W, h, case), run_async(W, h, case),
                run_async(W, h, case, count_on_device=True)):
        C.check(ref, got)
        C.same(got, host)
    return ref


@pytest.mark.parametrize("name", list(C.LAYOUTS))
def test_layouts(W, handle, name):
    """total = 0, one inbox holding everything, every inbox of length 1, totals of T - 1, T, T + 1
    and 3 T + 5, heads and ends at tile borders, one inbox over more than three tiles."""
    all_forms(W, handle, C.LAYOUTS[name]())


@pytest.mark.parametrize("name", list(C.EDGES))
def test_edges(W, handle, name):
    all_forms(W, handle, C.edge(name))


def test_edges_across_tile_borders(W, handle):
    ref = all_forms(W, handle, C.edges_across_borders())
    assert ref["summary"][0] == R.F_BAD_SUB


def test_more_than_65535_sends(W, handle):
    ref = all_forms(W, handle, C.more_than_65535_sends())
    assert ref["summary"][7] == 1


def test_fuzz(W, handle):
    case = C.fuzz()
    all_forms(W, handle, case)
    C.same(run_async(W, handle, case), run_async(W, handle, case))  # two runs are byte-identical


def test_count_is_read_on_the_device(W, handle):
    """cap_in and cap_boxes larger than the counts: the buffers are larger than what is written."""
    case = C.fuzz()
    ref = case.reference()
    for run in (run_sync, run_async):
        for on_device in (False, True):
            C.check(ref, run(W, handle, case, cap_in=case.total + 3 * C.T + 5, cap_boxes=case.m + 77, count_on_device=on_device))


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("what", ["cap_in", "cap_boxes"])
def test_refused_input_writes_only_the_summary(W, handle, form, what):
    """inbox_offsets[m] > cap_in (the stage in front overflowed), or a device-side inbox count
    above cap_boxes: the flag, nothing else written."""
    import torch
    from emqx_amd import _lib
    case = C.LAYOUTS["total_T+1"]()
    kw = dict(cap_in=C.T) if what == "cap_in" else dict(cap_boxes=case.m - 1, count_on_device=True)
    b = DeviceBatch(W, case, **kw)
    before = host_table(W, b.table, case.sub_limit)
    if form == "sync":
        with pytest.raises(_lib.EngineError) as e:
            handle.run_device(b.args)
        assert e.value.code == -1
        summary = e.value.summary
    else:
        handle.reserve(b.cap_in, b.cap_boxes)
        handle.run_device_async(b.args, b.summary.data_ptr())
        torch.cuda.synchronize()
        summary = dict(zip(W.SUMMARY, b.summary.cpu().numpy().view(np.uint64)[:8].tolist()))
    want = [R.F_INPUT_REFUSED, C.T + 1 if what == "cap_in" else 0, case.m, 0, 0, 0, 0, 0]
    assert [summary[k] for k in W.SUMMARY] == want
    got = b.result(W, summary)  # the sentinels are intact from the first element of every output
    assert got.verdicts.size == 0 and got.counts.size == 0
    assert host_table(W, b.table, case.sub_limit).tobytes() == before.tobytes()


def test_update_table_chains_two_batches_on_one_stream(W, handle):
    chain_two_batches(W, handle, *C.chained())


def chain_two_batches(W, handle, a, b):
    """Two asynchronous batches on one stream, the second reading the table the first wrote, no
    host read between them: equal to two sequential calls of the restatement."""
    import torch
    recs = C.records_of(a.table)
    ra = a.reference(update_table=True)
    R.run(a.subs, a.offsets, a.opts, recs, update_table=True)
    mid = C.table_of(recs)
    rb = b.reference(table=mid, update_table=True)
    R.run(b.subs, b.offsets, b.opts, recs, update_table=True)
    table = dev_table(a.table)
    da = DeviceBatch(W, a, table=table, update_table=True)
    db = DeviceBatch(W, b, table=table, update_table=True, count_on_device=True)
    handle.reserve(max(a.total, b.total), max(a.m, b.m))
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        handle.run_device_async(da.args, da.summary.data_ptr(), stream=stream.cuda_stream)
        handle.run_device_async(db.args, db.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    C.check(ra, da.result(W))
    C.check(rb, db.result(W))
    assert host_table(W, table, a.sub_limit).tobytes() == C.table_of(recs).tobytes() != a.table.tobytes()


def test_without_update_table_the_table_is_untouched(W, handle):
    case = C.edges_across_borders()
    for run in (run_sync, run_async):
        table = dev_table(case.table)
        C.check(case.reference(), run(W, handle, case, table=table))
        assert host_table(W, table, case.sub_limit).tobytes() == case.table.tobytes()


def test_scratch_reuse_on_one_handle(W):
    """A long batch, then an empty one, then short ones: no tile total, head prefix or counter of an
    earlier call shows in a later one."""
    h = W.Window(0)
    for name in ("one_inbox_holds_everything", "empty", "one_delivery", "total_3T+5", "inboxes_without_deliveries", "total_T"):
        case = C.LAYOUTS[name]()
        for run in (run_async, run_sync):
            C.check(case.reference(), run(W, h, case))
    assert h.stats()["cap_in"] == 3 * C.T + 5 and h.stats()["calls"] == 12


def test_async_needs_reserve(W):
    import torch
    from emqx_amd import _lib
    case = C.fuzz()
    h = W.Window(0)
    b = DeviceBatch(W, case)
    with pytest.raises(_lib.EngineError) as e:
        h.run_device_async(b.args, b.summary.data_ptr())
    assert e.value.code == _lib.EMQX_EOVERFLOW
    h.reserve(case.total, case.m - 1)  # one inbox short
    with pytest.raises(_lib.EngineError) as e:
        h.run_device_async(b.args, b.summary.data_ptr())
    assert e.value.code == _lib.EMQX_EOVERFLOW
    torch.cuda.synchronize()
    assert (b.summary.cpu().numpy().view(np.uint64) == S64).all(), "nothing was enqueued"
    assert h.stats()["calls"] == 0
    h.reserve(case.total, case.m)
    h.run_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    C.check(case.reference(), b.result(W))
    assert h.stats()["calls"] == 1 and h.stats()["scratch_bytes"] >= 8 * case.m


def test_misaligned_tables_are_refused(W, handle):
    from emqx_amd import _lib
    case = C.edge("pass")
    b = DeviceBatch(W, case)
    b.args.sessions += 8
    with pytest.raises(_lib.EngineError) as e:
        handle.run_device(b.args)
    assert e.value.code == -1


def test_chain_fanout_enrich_inbox_window_on_one_stream(W):
    """emqx_match_batch_device_async -> emqx_fanout_batch_device_async ->
    emqx_deliver_enrich_batch_device_async with compaction -> emqx_inbox_group_batch_device_async ->
    emqx_window_run_batch_device_async on one stream, no host read in between (the inbox count goes
    from the inbox stage's summary to the window stage on the device); against the host forms of
    the same chain and the restatement."""
    import torch
    from emqx_amd import deliver as D
    from emqx_amd import inbox as I
    from emqx_amd.engine import pack
    from tests.test_gpu_deliver import _broker_pair, _messages
    from tests import deliver_ref as DR
    b, _, _, _ = _broker_pair()
    b._sync()
    n = 1024
    msgs, keys = _messages(n)
    buf, offs = pack([m[0] for m in msgs])
    d_buf, d_off, d_keys = dev(buf, np.uint8), dev(offs, np.uint64), dev(keys, np.uint32)
    qos, flags = [m[1] for m in msgs], [1 if m[2] else 0 for m in msgs]
    frm = [DR.NO_SENDER if m[3] is None else b._sub_ids[m[3]] for m in msgs]
    d_qos, d_flags, d_from = dev(qos, np.uint8), dev(flags, np.uint8), dev(frm, np.uint32)
    cap = 64 * n
    sub_limit = len(b._subs_by_id)
    rng = np.random.default_rng(5)
    table = W.pack_sessions(sub_limit, inflight=rng.integers(0, 30, sub_limit), inflight_max=rng.choice([0, 8, 32], sub_limit),
                            mq_len=rng.integers(0, 5, sub_limit), mq_max=rng.choice([0, 4, 1000], sub_limit),
                            next_pkt_id=rng.integers(1, 65536, sub_limit),
                            flags=rng.choice([3, 3, 3, 1, 5, 0, 11], sub_limit))
    d_table = dev_table(table)
    e = b.router.engine
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    d_moff, d_mids, d_ms = z(n + 1, torch.int64), z(cap, torch.int32), z(e.SUMMARY_WORDS, torch.int64)
    d_doff, d_subs, d_fils, d_fs = z(n + 1, torch.int64), z(cap, torch.int32), z(cap, torch.int32), z(4, torch.int64)
    d_out, d_ids = z(cap, torch.uint8), z(cap, torch.int32)
    k_off, k_subs, k_fils, k_opts, k_ids = (z(n + 1, torch.int64), z(cap, torch.int32), z(cap, torch.int32),
                                            z(cap, torch.uint8), z(cap, torch.int32))
    d_sum, i_sum, w_sum = z(8, torch.int64), z(8, torch.int64), z(8, torch.int64)
    x_msgs, x_fils, x_opts = z(cap, torch.int32), z(cap, torch.int32), z(cap, torch.uint8)
    x_subs, x_off = z(sub_limit, torch.int32), z(sub_limit + 1, torch.int64)
    w_ver, w_ids, w_recs, w_cnt = z(cap, torch.uint8), z(cap, torch.int16), z(4 * sub_limit, torch.int64), z(4 * sub_limit, torch.int32)
    eargs = D.SubOpts.batch(d_doff.data_ptr(), d_subs.data_ptr(), d_fils.data_ptr(), n, cap, d_qos.data_ptr(),
                            d_flags.data_ptr(), d_from.data_ptr(), d_out.data_ptr(), d_ids.data_ptr(), k_off.data_ptr(),
                            k_subs.data_ptr(), k_fils.data_ptr(), k_opts.data_ptr(), k_ids.data_ptr(), cap)
    iargs = I.Inbox.batch(k_off.data_ptr(), k_subs.data_ptr(), k_fils.data_ptr(), n, cap, sub_limit, x_msgs.data_ptr(),
                          x_fils.data_ptr(), x_subs.data_ptr(), x_off.data_ptr(), sub_limit, d_opts=k_opts.data_ptr(),
                          d_box_opts=x_opts.data_ptr())
    wargs = W.Window.batch(x_subs.data_ptr(), x_off.data_ptr(), x_opts.data_ptr(), 0, cap, sub_limit, d_table.data_ptr(),
                           sub_limit, w_ver.data_ptr(), w_ids.data_ptr(), w_recs.data_ptr(), w_cnt.data_ptr(),
                           update_table=True, d_n_boxes=i_sum.data_ptr() + 16)
    box, win = I.Inbox(0), W.Window(0)
    box.reserve(cap, sub_limit)
    win.reserve(cap, sub_limit)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        e.match_device_async(d_buf.data_ptr(), d_off.data_ptr(), n, d_moff.data_ptr(), d_mids.data_ptr(), cap,
                             d_ms.data_ptr(), mode=0, stream=stream.cuda_stream)
        b.subs.fanout_device_async(b.strategy, d_moff.data_ptr(), d_mids.data_ptr(), n, cap, d_keys.data_ptr(),
                                   d_doff.data_ptr(), d_subs.data_ptr(), d_fils.data_ptr(), cap, d_fs.data_ptr(),
                                   stream=stream.cuda_stream)
        b.opts.enrich_device_async(eargs, d_sum.data_ptr(), stream=stream.cuda_stream)
        box.group_device_async(iargs, i_sum.data_ptr(), stream=stream.cuda_stream)
        win.run_device_async(wargs, w_sum.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert int(d_ms[0]) == 0 and int(d_fs[0]) == 0, "the match and the fan-out completed in one pass"
    # the host forms of the same chain, from the fan-out's CSR on
    total = int(d_fs[1])
    u32 = lambda t, k: t[:k].cpu().numpy().view(np.uint32)  # noqa: E731
    kept = b.opts.enrich_host(d_doff.cpu().numpy().view(np.uint64), u32(d_subs, total), u32(d_fils, total), qos, flags,
                              frm, compact=True).kept
    grouped = I.Inbox(I.HOST_ONLY).group_host(kept.offsets, kept.subs, kept.filters, sub_limit, opts=kept.opts)
    host_tab = table.copy()
    host = W.Window(W.HOST_ONLY).run_host(grouped.inbox_subs, grouped.inbox_offsets, grouped.opts, host_tab, update_table=True)
    s = w_sum.cpu().numpy().view(np.uint64).tolist()
    assert dict(zip(W.SUMMARY, s)) == host.summary and s[0] == 0 and s[1] > 1000 and s[2] > 10
    assert min(s[3:7]) > 0, "sends, QoS 0 sends, queued and drops all occur"
    t, m = s[1], s[2]
    got = W.Admitted(w_ver[:t].cpu().numpy(), w_ids[:t].cpu().numpy().view(np.uint16),
                     np.frombuffer(w_recs[:4 * m].cpu().numpy().tobytes(), dtype=W.SESSION),
                     w_cnt[:4 * m].cpu().numpy().view(np.uint32).reshape(-1, 4), host.summary)
    C.same(got, host)
    assert host_table(W, d_table, sub_limit).tobytes() == host_tab.tobytes() != table.tobytes()
    ref = R.run(grouped.inbox_subs, grouped.inbox_offsets, grouped.opts, C.records_of(table))
    assert got.verdicts.tolist() == ref["verdicts"] and got.pkt_ids.tolist() == ref["pkt_ids"] and s == ref["summary"]
