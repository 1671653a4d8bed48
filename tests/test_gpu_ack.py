"""The ack stage on the device (include/emqx_ack.h): every case of both calls through the three
device entry points, with the grid at its default and capped at 2 blocks, every output byte, the rows, the table and the summary exact against the
sequential restatement (tests/ack_ref.py) and identical to the host evaluator; nothing written past
the defined extents; the refusals; scratch reuse; the chain window -> record -> inbox-stage
grouping of raw acks -> ack -> window on one stream with no host read."""

import os
import subprocess

import numpy as np
import pytest

from tests import ack_cases as C
from tests import ack_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S8, S32, S64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64  # sentinel elements behind every output buffer's capacity


@pytest.fixture(scope="module")
def A():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import ack
    return ack


@pytest.fixture(scope="module", params=[(0, None), (1, None), (0, 2), (1, 2)],
                ids=["carry_slot", "rematch", "carry_slot-2_blocks", "rematch-2_blocks"])
def handle(A, request):
    """One handle a setting for the whole module: every test also reuses the scratch of the one
    before.  Capped at 2 blocks, a block takes several tiles and groups of rows of every case."""
    rematch, max_blocks = request.param
    h = A.Ack(0)
    h.set_tuning("rematch", rematch)
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


def dev_raw(table, guard=0):
    """A structured table as int64 words, `guard` sentinel words behind it."""
    import torch
    raw = np.frombuffer(table.tobytes() or bytes(32), dtype=np.int64)
    return torch.from_numpy(np.concatenate([raw, np.full(guard, S64, dtype=np.int64)])).to(DEV)


def filled(k, dtype):  # every byte 0x5A
    import torch
    sent = {torch.uint8: S8, torch.int32: S32, torch.int64: S64}[dtype]
    return torch.full((k + GUARD,), sent, dtype=dtype, device=DEV)


def host_slots(A, t, case):
    raw = t.cpu().numpy()
    n = case.sub_limit * case.w
    assert (raw[n:] == S64).all(), "a write past the slot table"
    return np.frombuffer(raw[:n].tobytes(), dtype=A.SLOT).reshape(case.sub_limit, case.w).copy()


def host_table(t, case):
    from emqx_amd import window
    raw = t.cpu().numpy()
    assert (raw[4 * case.sub_limit:] == S64).all(), "a write past the session table"
    return np.frombuffer(raw[:4 * case.sub_limit].tobytes(), dtype=window.SESSION).copy()


class RunBatch:
    """A run case in device memory with sentinel-filled outputs and a guard behind each."""

    def __init__(self, A, case, cap_in=None, cap_boxes=None, update_table=False, count_on_device=False):
        import torch
        self.case = case
        self.cap_in = case.total if cap_in is None else cap_in
        self.cap_boxes = case.m if cap_boxes is None else cap_boxes
        self.subs, self.off, self.acks = dev(case.subs, np.uint32), dev(case.offsets, np.uint64), dev(case.acks, np.uint32)
        self.table, self.slots = dev_raw(case.table, GUARD), dev_raw(case.slots, GUARD)
        self.count = dev([case.m], np.uint64) if count_on_device else None
        self.ver, self.refs = filled(self.cap_in, torch.uint8), filled(self.cap_in, torch.int32)
        self.cnt, self.summary = filled(4 * self.cap_boxes, torch.int32), filled(8, torch.int64)
        self.args = A.Ack.run_args(self.subs.data_ptr(), self.off.data_ptr(), self.acks.data_ptr(), 0 if count_on_device else case.m,
                                   self.cap_in, self.cap_boxes, self.table.data_ptr(), case.sub_limit, self.slots.data_ptr(), case.w,
                                   self.ver.data_ptr(), self.refs.data_ptr(), self.cnt.data_ptr(), update_table=update_table,
                                   d_n_boxes=self.count.data_ptr() if count_on_device else 0)

    def result(self, A, summary=None):
        """The outputs up to their defined extents, after checking that nothing behind them changed."""
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(A.RUN_SUMMARY, s[:8].tolist()))
        refused = summary["flags"] & R.F_INPUT_REFUSED
        total = 0 if refused else summary["acks"]
        m = 0 if refused else summary["sessions"]
        ver, refs = self.ver.cpu().numpy(), self.refs.cpu().numpy().view(np.uint32)
        cnt = self.cnt.cpu().numpy().view(np.uint32)
        assert (ver[total:] == S8).all() and (refs[total:] == S32).all(), "a write past the defined extent"
        assert (cnt[4 * m:] == S32).all(), "a write past the defined extent"
        return (A.Acked(ver[:total], refs[:total], cnt[:4 * m].reshape(-1, 4), summary), host_slots(A, self.slots, self.case),
                host_table(self.table, self.case))


def run_host_buffers(A, h, case, update_table):
    from emqx_amd import _lib
    table, slots = case.table.copy(), case.slots.copy()
    try:
        got = h.run(case.subs, case.offsets, case.acks, table, slots, update_table=update_table)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] == R.F_BAD_SUB
        got = e.partial
    return got, slots, table


def run_sync(A, h, case, **kw):
    from emqx_amd import _lib
    b = RunBatch(A, case, **kw)
    try:
        summary = h.run_device(b.args)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & (R.F_BAD_SUB | R.F_INPUT_REFUSED)
        summary = e.summary
    return b.result(A, summary)


def run_async(A, h, case, **kw):
    import torch
    b = RunBatch(A, case, **kw)
    h.reserve(b.cap_in, b.cap_boxes, case.w)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        h.run_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(A)


def host_answer(A, case, update_table):
    from emqx_amd import _lib
    table, slots = case.table.copy(), case.slots.copy()
    try:
        got = A.Ack(A.HOST_ONLY).run_host(case.subs, case.offsets, case.acks, table, slots, update_table=update_table)
    except _lib.EngineError as e:
        got = e.partial
    return got, slots, table


def all_forms(A, h, case, update_table=True):
    """Every device entry point: exact against the restatement, identical to the host evaluator."""
    ref = case.reference(update_table)
    host, host_rows, host_tab = host_answer(A, case, update_table)
    C.check_run(ref, host, host_rows, host_tab)
    for got, slots, table in (run_host_buffers(A, h, case, update_table), run_sync(A, h, case, update_table=update_table),
                              run_async(A, h, case, update_table=update_table),
                              run_async(A, h, case, update_table=update_table, count_on_device=True)):
        C.check_run(ref, got, slots, table)
        C.same_run(got, host)
        assert slots.tobytes() == host_rows.tobytes() and table.tobytes() == host_tab.tobytes()
    return ref


@pytest.mark.parametrize("name", list(C.RUNS))
def test_run_cases(A, handle, name):
    """The nine cells, the orders of one id, ids 0, 1 and 65535, bad kinds, W of 8, 32 and 64, lists
    of 0 .. T + 1 acks, the skewed list, sessions that take no acks, empty lists around."""
    all_forms(A, handle, C.RUNS[name]())


@pytest.mark.parametrize("name", ["inflight_below_released", "list_of_65", "sub_at_sub_limit"])
def test_without_update_table_the_table_is_untouched(A, handle, name):
    case = C.RUNS[name]()
    all_forms(A, handle, case, update_table=False)
    for run in (run_sync, run_async):
        _, _, table = run(A, handle, case)
        assert table.tobytes() == case.table.tobytes()


def test_fuzz(A, handle):
    case = C.fuzz()
    all_forms(A, handle, case)
    x, y = run_async(A, handle, case), run_async(A, handle, case)  # two runs are byte-identical
    C.same_run(x[0], y[0])
    assert x[1].tobytes() == y[1].tobytes()


def test_count_is_read_on_the_device(A, handle):
    """cap_in and cap_boxes larger than the counts: the buffers are larger than what is written."""
    case = C.fuzz(seed=6, n_sessions=400)
    ref = case.reference(True)
    for run in (run_sync, run_async):
        for on_device in (False, True):
            got, slots, table = run(A, handle, case, cap_in=case.total + 3 * C.T + 5, cap_boxes=case.m + 77, update_table=True,
                                    count_on_device=on_device)
            C.check_run(ref, got, slots, table)


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("what", ["cap_in", "cap_boxes"])
def test_refused_input_writes_only_the_summary(A, handle, form, what):
    import torch
    from emqx_amd import _lib
    case = C.RUNS["list_of_%d" % (C.T + 1)]()
    kw = dict(cap_in=case.total - 1) if what == "cap_in" else dict(cap_boxes=case.m - 1, count_on_device=True)
    b = RunBatch(A, case, update_table=True, **kw)
    if form == "sync":
        with pytest.raises(_lib.EngineError) as e:
            handle.run_device(b.args)
        assert e.value.code == -1
        summary = e.value.summary
    else:
        handle.reserve(b.cap_in, b.cap_boxes, case.w)
        handle.run_device_async(b.args, b.summary.data_ptr())
        torch.cuda.synchronize()
        summary = dict(zip(A.RUN_SUMMARY, b.summary.cpu().numpy().view(np.uint64)[:8].tolist()))
    want = [R.F_INPUT_REFUSED, case.total if what == "cap_in" else 0, case.m, 0, 0, 0, 0, 0]
    assert [summary[k] for k in A.RUN_SUMMARY] == want
    got, slots, table = b.result(A, summary)  # the sentinels are intact from the first element of every output
    assert got.verdicts.size == 0 and got.counts.size == 0
    assert slots.tobytes() == case.slots.tobytes() and table.tobytes() == case.table.tobytes()


def test_scratch_reuse_on_one_handle(A):
    """The 2 T + 1 list, then one ack, then the fuzz: no minimum or counter of an earlier call shows
    in a later one."""
    h = A.Ack(0)
    for case in (C.RUNS["skew_2T+1"](), C.RUNS["puback_msg"](), C.fuzz()):
        for run in (run_async, run_sync):
            got, slots, table = run(A, h, case, update_table=True)
            C.check_run(case.reference(True), got, slots, table)
    assert h.stats()["calls"] == 6 and h.stats()["scratch_bytes"] >= 8 * C.fuzz().m * 16


def test_async_needs_reserve(A):
    import torch
    from emqx_amd import _lib
    case = C.RUNS["list_of_65"]()
    h = A.Ack(0)
    b = RunBatch(A, case)
    rc = C.RECORDS["free_0_2_5_takes_3"]()
    rb = RecBatch(A, rc)
    for short in (None, (case.total - 1, case.m, case.w), (case.total, case.m - 1, case.w), (case.total, case.m, 8)):
        if short:
            h = A.Ack(0)
            h.reserve(*short)
        with pytest.raises(_lib.EngineError) as e:
            h.run_device_async(b.args, b.summary.data_ptr())
        assert e.value.code == _lib.EMQX_EOVERFLOW
    with pytest.raises(_lib.EngineError) as e:
        A.Ack(0).record_device_async(rb.args, rb.summary.data_ptr())
    assert e.value.code == _lib.EMQX_EOVERFLOW
    torch.cuda.synchronize()
    assert (b.summary.cpu().numpy().view(np.uint64) == S64).all(), "nothing was enqueued"
    assert (rb.summary.cpu().numpy().view(np.uint64) == S64).all() and h.stats()["calls"] == 0
    h.reserve(case.total, case.m, case.w)
    h.run_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    got, slots, table = b.result(A)
    C.check_run(case.reference(), got, slots, table)
    assert h.stats()["calls"] == 1 and h.stats()["scratch_bytes"] >= 8 * case.m * case.w


def test_misaligned_tables_and_bad_widths_are_refused(A, handle):
    from emqx_amd import _lib
    case = C.RUNS["puback_msg"]()
    for change in (dict(slots=8), dict(sessions=8), dict(out_counts=4), dict(w=-4), dict(w=-16)):
        b = RunBatch(A, case)
        for k, v in change.items():
            setattr(b.args, k, getattr(b.args, k) + v)
        with pytest.raises(_lib.EngineError) as e:
            handle.run_device(b.args)
        assert e.value.code == -1
        assert b.result(A, dict(dict.fromkeys(A.RUN_SUMMARY, 0), flags=R.F_INPUT_REFUSED))[1].tobytes() == case.slots.tobytes()


# ---- the record call ---------------------------------------------------------------------------

class RecBatch:
    def __init__(self, A, case, cap_in=None, cap_boxes=None, count_on_device=False):
        import torch
        self.case = case
        self.cap_in = case.total if cap_in is None else cap_in
        self.cap_boxes = case.m if cap_boxes is None else cap_boxes
        self.subs, self.off = dev(case.subs, np.uint32), dev(case.offsets, np.uint64)
        self.opts, self.ver, self.ids = dev(case.opts, np.uint8), dev(case.verdicts, np.uint8), dev(case.pkt_ids, np.uint16)
        self.refs = None if case.refs is None else dev(case.refs, np.uint32)
        self.slots = dev_raw(case.slots, GUARD)
        self.count = dev([case.m], np.uint64) if count_on_device else None
        self.unrec, self.summary = filled(self.cap_boxes, torch.int32), filled(8, torch.int64)
        self.args = A.Ack.record_args(self.subs.data_ptr(), self.off.data_ptr(), self.opts.data_ptr(), 0 if count_on_device else case.m,
                                      self.cap_in, self.cap_boxes, self.ver.data_ptr(), self.ids.data_ptr(), self.slots.data_ptr(),
                                      case.w, case.sub_limit, self.unrec.data_ptr(),
                                      d_refs=0 if self.refs is None else self.refs.data_ptr(),
                                      d_n_boxes=self.count.data_ptr() if count_on_device else 0)

    def result(self, A, summary=None):
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(A.RECORD_SUMMARY, s[:8].tolist()))
        m = 0 if summary["flags"] & R.F_INPUT_REFUSED else summary["inboxes"]
        unrec = self.unrec.cpu().numpy().view(np.uint32)
        assert (unrec[m:] == S32).all(), "a write past the defined extent"
        return A.Recorded(unrec[:m], summary), host_slots(A, self.slots, self.case)


def rec_sync(A, h, case, **kw):
    from emqx_amd import _lib
    b = RecBatch(A, case, **kw)
    try:
        summary = h.record_device(b.args)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & (R.F_BAD_SUB | R.F_INPUT_REFUSED)
        summary = e.summary
    return b.result(A, summary)


def rec_async(A, h, case, **kw):
    import torch
    b = RecBatch(A, case, **kw)
    h.reserve(b.cap_in, b.cap_boxes, case.w)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        h.record_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(A)


def rec_host_buffers(A, h, case):
    from emqx_amd import _lib
    slots = case.slots.copy()
    try:
        got = h.record(case.subs, case.offsets, case.opts, case.verdicts, case.pkt_ids, slots, refs=case.refs)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & R.F_BAD_SUB
        got = e.partial
    return got, slots


def rec_all_forms(A, h, case):
    from emqx_amd import _lib
    ref = case.reference()
    host_rows = case.slots.copy()
    try:
        host = A.Ack(A.HOST_ONLY).record_host(case.subs, case.offsets, case.opts, case.verdicts, case.pkt_ids, host_rows, refs=case.refs)
    except _lib.EngineError as e:
        host = e.partial
    C.check_rec(ref, host, host_rows)
    for got, slots in (rec_host_buffers(A, h, case), rec_sync(A, h, case), rec_async(A, h, case),
                       rec_async(A, h, case, count_on_device=True)):
        C.check_rec(ref, got, slots)
        assert got.summary == host.summary and got.unrecorded.tobytes() == host.unrecorded.tobytes()
        assert slots.tobytes() == host_rows.tobytes()


@pytest.mark.parametrize("name", list(C.RECORDS))
@pytest.mark.parametrize("refs", [False, True], ids=["refs_null", "refs"])
def test_record_cases(A, handle, name, refs):
    """Free slots {0, 2, 5} taking 1, 3 and 4 sends; sends interleaved with QoS 0 and queued verdicts
    across a tile border; one inbox over three tiles; a bad subscriber; a full row of 64."""
    rec_all_forms(A, handle, C.RECORDS[name](refs))


def test_record_fuzz(A, handle):
    case = C.rec_fuzz()
    rec_all_forms(A, handle, case)
    ref = case.reference()
    for run in (rec_sync, rec_async):  # buffers larger than what is written
        got, slots = run(A, handle, case, cap_in=case.total + 2 * C.T + 3, cap_boxes=case.m + 9, count_on_device=True)
        C.check_rec(ref, got, slots)


def test_record_refused_input_writes_only_the_summary(A, handle):
    import torch
    case = C.RECORDS["total_T"]()
    b = RecBatch(A, case, cap_in=case.total - 1)
    handle.reserve(b.cap_in, b.cap_boxes, case.w)
    handle.record_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    got, slots = b.result(A)
    assert [got.summary[k] for k in A.RECORD_SUMMARY] == [R.F_INPUT_REFUSED, case.total, case.m, 0, 0, 0, 0, 0]
    assert got.unrecorded.size == 0 and slots.tobytes() == case.slots.tobytes()


# ---- the chain ---------------------------------------------------------------------------------

def test_chain_window_record_group_ack_window_on_one_stream(A):
    """emqx_window_run_batch_device_async (a session with inflight_max 2 and four QoS 1 deliveries:
    two SEND, two QUEUED) -> emqx_ack_record_batch_device_async -> emqx_inbox_group_batch_device_async
    over the raw acks -> emqx_ack_run_batch_device_async of id 1 with update_table ->
    emqx_window_run_batch_device_async with one more QoS 1 delivery, which is EMQX_W_SEND with id 3.
    One stream, no host read in between; all of it against the restatements."""
    import torch
    from emqx_amd import inbox as I
    from emqx_amd import window as W
    from tests import window_ref as WR
    sub_limit, w, sub = 5, 8, 3
    table = W.pack_sessions(sub_limit, inflight_max=2)
    rows = A.empty_slots(sub_limit, w)
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    d_table, d_rows = dev_raw(table), dev_raw(rows)
    # batch 1: four QoS 1 deliveries to the session
    subs1, off1, opts1 = dev([sub], np.uint32), dev([0, 4], np.uint64), dev([1, 1, 1, 1], np.uint8)
    ver1, ids1, recs1, cnt1, sum1 = z(4, torch.uint8), z(4, torch.int16), z(4, torch.int64), z(4, torch.int32), z(8, torch.int64)
    refs1 = dev([70, 71, 72, 73], np.uint32)
    unrec, rsum = z(1, torch.int32), z(8, torch.int64)
    # the raw acks as they arrive: (session, packed ack), one "message" each
    raw_subs, raw_acks = dev([sub, 1], np.uint32), dev(A.pack_acks([R.PUBACK, R.PUBACK], [1, 9]), np.uint32)
    raw_off = dev([0, 1, 2], np.uint64)
    box_msgs, box_acks, ack_subs, ack_off, isum = z(2, torch.int32), z(2, torch.int32), z(2, torch.int32), z(3, torch.int64), z(8, torch.int64)
    aver, arefs, acnt, asum = z(2, torch.uint8), z(2, torch.int32), z(8, torch.int32), z(8, torch.int64)
    # batch 2: one more QoS 1 delivery
    off2, opts2 = dev([0, 1], np.uint64), dev([1], np.uint8)
    ver2, ids2, recs2, cnt2, sum2 = z(1, torch.uint8), z(1, torch.int16), z(4, torch.int64), z(4, torch.int32), z(8, torch.int64)
    win, ack, box = W.Window(0), A.Ack(0), I.Inbox(0)
    win.reserve(4, 1)
    ack.reserve(4, 2, w)
    box.reserve(2, sub_limit)
    w1 = W.Window.batch(subs1.data_ptr(), off1.data_ptr(), opts1.data_ptr(), 1, 4, 1, d_table.data_ptr(), sub_limit, ver1.data_ptr(),
                        ids1.data_ptr(), recs1.data_ptr(), cnt1.data_ptr(), update_table=True)
    r1 = A.Ack.record_args(subs1.data_ptr(), off1.data_ptr(), opts1.data_ptr(), 1, 4, 1, ver1.data_ptr(), ids1.data_ptr(),
                           d_rows.data_ptr(), w, sub_limit, unrec.data_ptr(), d_refs=refs1.data_ptr())
    g1 = I.Inbox.batch(raw_off.data_ptr(), raw_subs.data_ptr(), raw_acks.data_ptr(), 2, 2, sub_limit, box_msgs.data_ptr(),
                       box_acks.data_ptr(), ack_subs.data_ptr(), ack_off.data_ptr(), 2)
    a1 = A.Ack.run_args(ack_subs.data_ptr(), ack_off.data_ptr(), box_acks.data_ptr(), 0, 2, 2, d_table.data_ptr(), sub_limit,
                        d_rows.data_ptr(), w, aver.data_ptr(), arefs.data_ptr(), acnt.data_ptr(), update_table=True,
                        d_n_boxes=isum.data_ptr() + 16)
    w2 = W.Window.batch(subs1.data_ptr(), off2.data_ptr(), opts2.data_ptr(), 1, 1, 1, d_table.data_ptr(), sub_limit, ver2.data_ptr(),
                        ids2.data_ptr(), recs2.data_ptr(), cnt2.data_ptr(), update_table=True)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        win.run_device_async(w1, sum1.data_ptr(), stream=stream.cuda_stream)
        ack.record_device_async(r1, rsum.data_ptr(), stream=stream.cuda_stream)
        box.group_device_async(g1, isum.data_ptr(), stream=stream.cuda_stream)
        ack.run_device_async(a1, asum.data_ptr(), stream=stream.cuda_stream)
        win.run_device_async(w2, sum2.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    # the restatements, step by step
    recs = [{f: int(table[f][i]) for f in WR.FIELDS} for i in range(sub_limit)]
    x1 = WR.run([sub], [0, 4], [1, 1, 1, 1], recs, update_table=True)
    assert x1["verdicts"] == [W.W_SEND, W.W_SEND, W.W_QUEUED, W.W_QUEUED] and x1["pkt_ids"] == [1, 2, 0, 0]
    assert ver1.cpu().numpy().tolist() == x1["verdicts"] and ids1.cpu().numpy().view(np.uint16).tolist() == x1["pkt_ids"]
    ref_rows = C.rows_of(rows)
    xr = R.record([sub], [0, 4], [1, 1, 1, 1], x1["verdicts"], x1["pkt_ids"], [70, 71, 72, 73], ref_rows)
    assert rsum.cpu().numpy().view(np.uint64).tolist() == xr["summary"] == [0, 4, 1, 2, 2, 0, 0, 0] and int(unrec[0]) == 0
    # the grouping: session 1 first (ascending subscriber id), then session 3
    assert isum.cpu().numpy().view(np.uint64)[:3].tolist() == [0, 2, 2]
    assert ack_subs.cpu().numpy().view(np.uint32).tolist() == [1, sub] and ack_off.cpu().numpy().tolist() == [0, 1, 2]
    grouped = box_acks.cpu().numpy().view(np.uint32)
    assert grouped.tolist() == [(R.PUBACK << 16) | 9, (R.PUBACK << 16) | 1]
    xa = R.run([1, sub], [0, 1, 2], grouped, recs, ref_rows, update_table=True)
    assert xa["verdicts"] == [R.A_NOT_FOUND, R.A_OK] and xa["refs"] == [R.NO_REF, 70] and xa["counts"][1] == [1, 0, 0, 1]
    assert aver.cpu().numpy().tolist() == xa["verdicts"] and arefs.cpu().numpy().view(np.uint32).tolist() == xa["refs"]
    assert acnt.cpu().numpy().view(np.uint32).reshape(-1, 4).tolist() == xa["counts"]
    assert asum.cpu().numpy().view(np.uint64).tolist() == xa["summary"]
    got_rows = np.frombuffer(d_rows.cpu().numpy().tobytes(), dtype=A.SLOT).reshape(sub_limit, w)
    assert C.rows_of(got_rows) == ref_rows and ref_rows[sub][:2] == [[0, 0, 0, 0], [2, R.MSG, 1, 71]]
    x2 = WR.run([sub], [0, 1], [1], recs, update_table=True)
    assert x2["verdicts"] == [W.W_SEND] and x2["pkt_ids"] == [3], "the window reopened"
    assert ver2.cpu().numpy().tolist() == x2["verdicts"] and ids2.cpu().numpy().view(np.uint16).tolist() == x2["pkt_ids"]
    got_table = np.frombuffer(d_table.cpu().numpy().tobytes(), dtype=W.SESSION)
    assert [{f: int(got_table[f][i]) for f in WR.FIELDS} for i in range(sub_limit)] == recs
    assert int(got_table["inflight"][sub]) == 2 and int(got_table["mq_len"][sub]) == 2 and int(got_table["next_pkt_id"][sub]) == 4
