"""The inbox stage on the device (include/emqx_inbox.h): every named case through every entry
point and both paths, with the grid at its default and capped at 2 blocks, every output array and
the summary exact against the restatement (tests/inbox_ref.py) and byte-identical to the host
evaluator; nothing written past the defined extents; the refusals; scratch reuse on one handle; the match -> fan-out -> enrich -> inbox chain
on one stream."""

import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import inbox_cases as C
from tests import inbox_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S8, S32, S64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64  # sentinel elements behind every output buffer's capacity
PATHS = [0, 1]


@pytest.fixture(scope="module")
def I():  # noqa: E743
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import inbox
    return inbox


def make_handles(I, max_blocks=None):
    hs = {}
    for path in PATHS:
        hs[path] = I.Inbox(0)
        hs[path].set_tuning("path", path)
        if max_blocks is not None:
            hs[path].set_tuning("max_blocks", max_blocks)
    return hs


@pytest.fixture(scope="module")
def handles(I):
    """One handle a path for the whole module: every test also reuses the scratch of the one
    before.  The grid is at its default (TestCappedAt2Blocks: capped)."""
    return make_handles(I)


def dev(a, dtype):
    import torch
    view = {np.uint64: np.int64, np.uint32: np.int32}.get(dtype, dtype)
    a = np.array(a, dtype=dtype)  # a writable copy
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)
    return torch.from_numpy(a.view(view)).to(DEV)


class DeviceBatch:
    """A case's batch in device memory with sentinel-filled outputs and a guard behind each."""

    def __init__(self, I, case, opts=True, subids=True, src=True, cap_in=None, cap_boxes=None, sub_limit=None):
        import torch
        self.n, self.total = case.n, case.total
        self.cap_in = self.total if cap_in is None else cap_in
        self.sub_limit = case.sub_limit if sub_limit is None else sub_limit
        self.cap_boxes = min(self.cap_in, self.sub_limit) if cap_boxes is None else cap_boxes
        self.ins = [dev(case.offsets, np.uint64), dev(case.subs, np.uint32), dev(case.filters, np.uint32),
                    dev(case.opts, np.uint8) if opts else None, dev(case.subids, np.uint32) if subids else None]

        def filled(k, dtype):  # every byte 0x5A
            return torch.full((k + GUARD,), {torch.uint8: S8, torch.int32: S32, torch.int64: S64}[dtype], dtype=dtype,
                              device=DEV)

        c = self.cap_in
        self.msgs, self.fils = filled(c, torch.int32), filled(c, torch.int32)
        self.bopts = filled(c, torch.uint8) if opts else None
        self.bids = filled(c, torch.int32) if subids else None
        self.src = filled(c, torch.int32) if src else None
        self.isubs, self.ioff = filled(self.cap_boxes, torch.int32), filled(self.cap_boxes + 1, torch.int64)
        self.summary = filled(8, torch.int64)
        p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        i = self.ins
        self.args = I.Inbox.batch(p(i[0]), p(i[1]), p(i[2]), self.n, self.cap_in, self.sub_limit, p(self.msgs), p(self.fils),
                                  p(self.isubs), p(self.ioff), self.cap_boxes, d_opts=p(i[3]), d_subids=p(i[4]),
                                  d_box_opts=p(self.bopts), d_box_subids=p(self.bids), d_box_src=p(self.src))

    def host(self, t, dtype=np.uint32):
        return None if t is None else t.cpu().numpy().view(dtype)

    def result(self, I, summary=None):
        """The outputs up to their defined extents, after checking that nothing behind them changed."""
        if summary is None:
            s = self.host(self.summary, np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(I.SUMMARY, s[:8].tolist()))
        flags = summary["flags"]
        total = 0 if flags & (R.F_INPUT_REFUSED | R.F_BAD_SUB) else summary["deliveries"]
        boxes = min(summary["inboxes"], self.cap_boxes)
        offs = 0 if flags & (R.F_INPUT_REFUSED | R.F_BAD_SUB) else boxes + 1
        out = []
        for t, dtype, extent, sent in ((self.isubs, np.uint32, boxes, S32), (self.ioff, np.uint64, offs, S64),
                                       (self.msgs, np.uint32, total, S32), (self.fils, np.uint32, total, S32),
                                       (self.bopts, np.uint8, total, S8), (self.bids, np.uint32, total, S32),
                                       (self.src, np.uint32, total, S32)):
            a = self.host(t, dtype)
            if a is not None and not flags & R.F_BAD_SUB:  # (a bad subscriber leaves the outputs unspecified)
                assert (a[extent:] == sent).all(), "a write past the defined extent"
            out.append(None if a is None else a[:extent])
        return I.Grouped(*out, summary)

    def guards_intact(self):
        for t, dtype, cap, sent in ((self.isubs, np.uint32, self.cap_boxes, S32), (self.ioff, np.uint64, self.cap_boxes + 1, S64),
                                    (self.msgs, np.uint32, self.cap_in, S32), (self.fils, np.uint32, self.cap_in, S32),
                                    (self.bopts, np.uint8, self.cap_in, S8), (self.bids, np.uint32, self.cap_in, S32),
                                    (self.src, np.uint32, self.cap_in, S32)):
            if t is not None:
                assert (self.host(t, dtype)[cap:] == sent).all(), "a write past the buffer"


def run_sync(I, h, case, **kw):
    b = DeviceBatch(I, case, **kw)
    return b.result(I, h.group_device(b.args))


def run_async(I, h, case, **kw):
    import torch
    b = DeviceBatch(I, case, **kw)
    h.reserve(b.cap_in, b.sub_limit)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        h.group_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(I)


def all_forms(I, handles, case, opts=True, subids=True, src=True):
    """Every device entry point on both paths: exact against the restatement, identical to the host evaluator."""
    ref = case.reference(opts=opts, subids=subids)
    a, k = case.args(opts=opts, subids=subids)
    host = I.Inbox(I.HOST_ONLY).group_host(*a, **k, src=src)
    C.check(ref, host, opts, subids, src)
    for path in PATHS:
        h = handles[path]
        for got in (h.group(*a, **k, src=src), run_sync(I, h, case, opts=opts, subids=subids, src=src),
                    run_async(I, h, case, opts=opts, subids=subids, src=src)):
            C.check(ref, got, opts, subids, src)
            C.same(got, host)
    return ref


@pytest.mark.parametrize("name", C.TINY_CASES)
def test_tiny(I, handles, name):
    all_forms(I, handles, C.tiny(name))


@pytest.mark.parametrize("total, mode", C.SHAPE_CASES)
def test_shapes(I, handles, total, mode):
    """63 / 64 / 65 (the wave), T - 1 / T / T + 1 and 2 T + 1 (the tile): one subscriber (stability
    across waves, rows and tiles), all distinct in descending order, two alternating."""
    ref = all_forms(I, handles, C.shape(total, mode))
    assert ref["summary"][1] == total


@pytest.mark.parametrize("sub_limit", C.SUB_LIMITS)
def test_digit_edges(I, handles, sub_limit):
    case = C.digit_edge(sub_limit)
    ref = all_forms(I, handles, case)
    assert ref["inbox_subs"][0] == 0 and ref["inbox_subs"][-1] == sub_limit - 1
    assert handles[0].stats()["last_passes"] == I.passes(sub_limit)


def test_two_filters_of_one_message_keep_order_and_bits(I, handles):
    ref = all_forms(I, handles, C.two_filters())
    assert ref["filters"][-4:] == [11, 21 | R.SHARED_BIT | R.RETRY_BIT, 23, 31 | R.RETRY_BIT]


def test_empty_messages(I, handles):
    ref = all_forms(I, handles, C.empty_messages())
    assert sorted(set(ref["msgs"])) == [2, 6, 7, 9]


def test_fuzz(I, handles):
    ref = all_forms(I, handles, C.fuzz())
    assert ref["summary"][3] > 300


def test_fuzz_wide(I, handles):
    case = C.fuzz_wide()
    assert I.passes(case.sub_limit) == 3
    all_forms(I, handles, case)


@pytest.mark.parametrize("absent", ["opts", "subids", "src"])
def test_optional_outputs(I, handles, absent):
    all_forms(I, handles, C.fuzz(), opts=absent != "opts", subids=absent != "subids", src=absent != "src")


@pytest.mark.parametrize("path", PATHS)
def test_two_runs_are_byte_identical(I, handles, path):
    case = C.fuzz_wide()
    C.same(run_async(I, handles[path], case), run_async(I, handles[path], case))


def _summary_of(I, h, b, form):
    """The summary of a call that the synchronous form answers with an error."""
    import torch
    from emqx_amd import _lib
    if form == "sync":
        with pytest.raises(_lib.EngineError) as e:
            h.group_device(b.args)
        return e.value.code, e.value.summary
    h.reserve(b.cap_in, b.sub_limit)
    h.group_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    return None, dict(zip(I.SUMMARY, b.host(b.summary, np.uint64)[:8].tolist()))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", ["sync", "async"])
def test_input_refused(I, handles, form, path):
    """offsets[n] > cap_in (the stage in front overflowed): the flag, nothing else written."""
    case = C.shape(C.T + 1, "alternating")
    b = DeviceBatch(I, case, cap_in=C.T)
    code, summary = _summary_of(I, handles[path], b, form)
    assert code in (None, -1)
    assert [summary[k] for k in I.SUMMARY] == [R.F_INPUT_REFUSED, C.T + 1, 0, 0, 0, 0, 0, 0]
    got = b.result(I, summary)
    assert all(x is None or x.size == 0 for x in got[:-1])  # the sentinels are intact from the first element


@pytest.mark.parametrize("path", PATHS)
def test_count_is_read_on_the_device(I, handles, path):
    """cap_in larger than the count, the buffers larger than the deliveries."""
    case = C.fuzz()
    ref = case.reference()
    for run in (run_sync, run_async):
        got = run(I, handles[path], case, cap_in=case.total + 3 * C.T + 5, cap_boxes=case.sub_limit)
        C.check(ref, got)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", ["sync", "async"])
def test_bad_subscriber(I, handles, form, path):
    """A subscriber at sub_limit: BAD_SUB, no inboxes reported, nothing outside the buffers touched."""
    case = C.shape(2 * C.T + 1, "alternating")
    b = DeviceBatch(I, case, sub_limit=0x10203)
    code, summary = _summary_of(I, handles[path], b, form)
    assert code in (None, -1)
    ref = R.group(case.offsets, case.subs, case.filters, 0x10203)
    assert [summary[k] for k in I.SUMMARY] == ref["summary"] and summary["flags"] == R.F_BAD_SUB and summary["inboxes"] == 0
    b.guards_intact()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cap", ["m-1", 1, 0])
def test_box_overflow(I, handles, cap, path):
    from emqx_amd import _lib
    case = C.fuzz()
    m = case.reference()["summary"][2]
    cap_boxes = m - 1 if cap == "m-1" else cap
    ref = case.reference(cap_boxes=cap_boxes)
    assert ref["summary"][0] == R.F_BOX_OVERFLOW and ref["summary"][2] == m
    h = handles[path]
    a, k = case.args()
    with pytest.raises(_lib.EngineError) as e:
        h.group(*a, **k, cap_boxes=cap_boxes)
    assert e.value.code == _lib.EMQX_EOVERFLOW and e.value.needed == m
    C.check(ref, e.value.partial)
    for form in ("sync", "async"):
        b = DeviceBatch(I, case, cap_boxes=cap_boxes)
        code, summary = _summary_of(I, h, b, form)
        assert code in (None, _lib.EMQX_EOVERFLOW)
        C.check(ref, b.result(I, summary))


class TestCappedAt2Blocks:
    """Every test above that takes `handles`, again with the grid capped at 2 blocks: a block
    takes several tiles of every case with more than 2 T deliveries and several rows of the
    longest pass, the heads and path 1's prep and gather beyond 512.  The tests above keep their
    ids."""

    @pytest.fixture(scope="class")
    def handles(self, I):
        return make_handles(I, max_blocks=2)


for _name, _test in list(globals().items()):
    if _name.startswith("test_") and "handles" in inspect.signature(_test).parameters:
        setattr(TestCappedAt2Blocks, _name, staticmethod(_test))


def test_scratch_reuse_on_one_handle(I):
    """2 T + 1 deliveries to one subscriber, then one delivery, then the three-pass fuzz: no
    histogram, tile count or boundary of an earlier call shows in a later one."""
    for path in PATHS:
        h = I.Inbox(0)
        h.set_tuning("path", path)
        for case in (C.shape(2 * C.T + 1, "one_sub"), C.tiny("one"), C.fuzz_wide(), C.tiny("n3_total0"), C.fuzz()):
            for run in (run_async, run_sync):
                C.check(case.reference(), run(I, h, case))
        assert h.stats()["cap_in"] == C.fuzz_wide().total


def test_async_needs_reserve(I):
    import torch
    from emqx_amd import _lib
    case = C.fuzz()
    h = I.Inbox(0)
    b = DeviceBatch(I, case)
    with pytest.raises(_lib.EngineError) as e:
        h.group_device_async(b.args, b.summary.data_ptr())
    assert e.value.code == _lib.EMQX_EOVERFLOW
    h.reserve(case.total - 1, case.sub_limit)  # one delivery short
    with pytest.raises(_lib.EngineError) as e:
        h.group_device_async(b.args, b.summary.data_ptr())
    assert e.value.code == _lib.EMQX_EOVERFLOW
    torch.cuda.synchronize()
    assert (b.host(b.summary, np.uint64) == S64).all(), "nothing was enqueued"
    assert b.result(I, dict(zip(I.SUMMARY, [R.F_INPUT_REFUSED] + [0] * 7))).msgs.size == 0
    assert h.stats()["calls"] == 0
    h.reserve(case.total, case.sub_limit)
    h.group_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    C.check(case.reference(), b.result(I))
    assert h.stats()["calls"] == 1 and h.stats()["scratch_bytes"] > 20 * case.total


def test_chain_match_fanout_enrich_inbox_on_one_stream(I):
    """emqx_match_batch_device_async -> emqx_fanout_batch_device_async ->
    emqx_deliver_enrich_batch_device_async with compaction -> emqx_inbox_group_batch_device_async
    on one stream, no host read in between; against the restatement applied to the host path's
    kept CSR."""
    import torch
    from emqx_amd import deliver as D
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
    e = b.router.engine
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    d_moff, d_mids, d_ms = z(n + 1, torch.int64), z(cap, torch.int32), z(e.SUMMARY_WORDS, torch.int64)
    d_doff, d_subs, d_fils, d_fs = z(n + 1, torch.int64), z(cap, torch.int32), z(cap, torch.int32), z(4, torch.int64)
    d_out, d_ids = z(cap, torch.uint8), z(cap, torch.int32)
    k_off, k_subs, k_fils, k_opts, k_ids = (z(n + 1, torch.int64), z(cap, torch.int32), z(cap, torch.int32),
                                            z(cap, torch.uint8), z(cap, torch.int32))
    d_sum, i_sum = z(8, torch.int64), z(8, torch.int64)
    x_msgs, x_fils, x_opts, x_ids, x_src = (z(cap, torch.int32), z(cap, torch.int32), z(cap, torch.uint8),
                                            z(cap, torch.int32), z(cap, torch.int32))
    x_subs, x_off = z(sub_limit, torch.int32), z(sub_limit + 1, torch.int64)
    eargs = D.SubOpts.batch(d_doff.data_ptr(), d_subs.data_ptr(), d_fils.data_ptr(), n, cap, d_qos.data_ptr(),
                            d_flags.data_ptr(), d_from.data_ptr(), d_out.data_ptr(), d_ids.data_ptr(), k_off.data_ptr(),
                            k_subs.data_ptr(), k_fils.data_ptr(), k_opts.data_ptr(), k_ids.data_ptr(), cap)
    iargs = I.Inbox.batch(k_off.data_ptr(), k_subs.data_ptr(), k_fils.data_ptr(), n, cap, sub_limit, x_msgs.data_ptr(),
                          x_fils.data_ptr(), x_subs.data_ptr(), x_off.data_ptr(), sub_limit, d_opts=k_opts.data_ptr(),
                          d_subids=k_ids.data_ptr(), d_box_opts=x_opts.data_ptr(), d_box_subids=x_ids.data_ptr(),
                          d_box_src=x_src.data_ptr())
    box = I.Inbox(0)
    box.reserve(cap, sub_limit)
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
    stream.synchronize()
    assert int(d_ms[0]) == 0 and int(d_fs[0]) == 0, "the match and the fan-out completed in one pass"
    es = d_sum.cpu().numpy().view(np.uint64).tolist()
    assert es[0] == 0 and es[3] > 0, "No Local dropped something: the inbox stage reads the compacted CSR"
    # the host path: the fan-out's CSR enriched and compacted on the CPU, then the restatement
    total = int(d_fs[1])
    u32 = lambda t, k: t[:k].cpu().numpy().view(np.uint32)  # noqa: E731
    host = b.opts.enrich_host(d_doff.cpu().numpy().view(np.uint64), u32(d_subs, total), u32(d_fils, total), qos, flags,
                              frm, compact=True)
    kept = host.kept
    assert kept.subs.size == es[2] and kept.subs.size > 1000
    ref = R.group(kept.offsets, kept.subs, kept.filters, sub_limit, kept.opts, kept.subids, cap_in=cap)
    s = i_sum.cpu().numpy().view(np.uint64).tolist()
    assert s == ref["summary"] and s[0] == 0 and s[2] > 10
    t, m = s[1], s[2]
    got = I.Grouped(u32(x_subs, m), x_off[:m + 1].cpu().numpy().view(np.uint64), u32(x_msgs, t), u32(x_fils, t),
                    x_opts[:t].cpu().numpy(), u32(x_ids, t), u32(x_src, t), dict(zip(I.SUMMARY, s)))
    C.check(ref, got)
