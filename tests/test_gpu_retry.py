"""The retry stage on the device (include/emqx_retry.h): every case of both calls through the three
device entry points, with the grid at its default, capped at 1 block and capped at 2 blocks with a
scan that carries every 2 tiles; every output byte, the rows, the stamps, the table and the summary
exact against the sequential restatement (tests/retry_ref.py) and identical to the host evaluator;
nothing written past the defined extents; overflow and its repeat; scratch reuse; the chain window ->
record -> stamp -> sweep -> ack -> stamp -> sweep -> sweep -> window on one stream with no host
read."""

import os
import subprocess

import numpy as np
import pytest

from tests import retry_cases as C
from tests import retry_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S8, S32, S64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64  # sentinel elements behind every output buffer's capacity


@pytest.fixture(scope="module")
def T():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import retry
    return retry


@pytest.fixture(scope="module", params=[(None, None), (1, None), (2, 2)], ids=["default", "1_block", "2_blocks-scan_chunk_2"])
def handle(T, request):
    """One handle a setting for the whole module: every test also reuses the scratch of the one
    before.  Capped, a block takes several groups of rows of every case with more than one."""
    max_blocks, scan_chunk = request.param
    h = T.Retry(0)
    if max_blocks is not None:
        h.set_tuning("max_blocks", max_blocks)
    if scan_chunk is not None:
        h.set_tuning("scan_chunk", scan_chunk)
    return h


def dev(a, dtype):
    import torch
    view = {np.uint64: np.int64, np.uint32: np.int32, np.uint16: np.int16}.get(dtype, dtype)
    a = np.array(a, dtype=dtype)  # a writable copy
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)
    return torch.from_numpy(a.view(view)).to(DEV)


def dev_raw(table, guard=0):
    """A table as int64 words, `guard` sentinel words behind it."""
    import torch
    raw = np.frombuffer(table.tobytes() or bytes(32), dtype=np.int64)
    return torch.from_numpy(np.concatenate([raw, np.full(guard, S64, dtype=np.int64)])).to(DEV)


def filled(k, dtype):  # every byte 0x5A
    import torch
    sent = {torch.uint8: S8, torch.int32: S32, torch.int64: S64}[dtype]
    return torch.full((k + GUARD,), sent, dtype=dtype, device=DEV)


def back(t, n, dtype, shape, what):
    """The first n int64 words of a guarded device table as a host array."""
    raw = t.cpu().numpy()
    assert (raw[n:] == S64).all(), "a write past " + what
    return np.frombuffer(raw[:n].tobytes(), dtype=dtype).reshape(shape).copy()


class SweepBatch:
    """A sweep case in device memory with sentinel-filled outputs and a guard behind each."""

    def __init__(self, T, case, cap_out="case", cap_boxes=None, update_table=True, count_on_device=False):
        import torch
        self.case = case
        cap = case.cap_out if cap_out == "case" else cap_out
        self.cap_out = case.m * case.w if cap is None else cap
        self.cap_boxes = case.m if cap_boxes is None else cap_boxes
        self.subs = None if case.subs is None else dev(case.subs, np.uint32)
        self.table, self.slots, self.stamps = dev_raw(case.table, GUARD), dev_raw(case.slots, GUARD), dev_raw(case.stamps, GUARD)
        self.intervals = None if case.intervals is None else dev(case.intervals, np.uint32)
        self.deadlines = None if case.deadlines is None else dev(case.deadlines, np.uint64)
        self.count = dev([case.m], np.uint64) if count_on_device else None
        self.off, self.items = filled(self.cap_boxes + 1, torch.int64), filled(self.cap_out, torch.int64)
        self.status, self.cnt = filled(self.cap_boxes, torch.uint8), filled(4 * self.cap_boxes, torch.int32)
        self.timers, self.summary = filled(self.cap_boxes, torch.int32), filled(8, torch.int64)
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        self.args = T.Retry.sweep_args(ptr(self.subs), 0 if count_on_device else case.m, self.cap_boxes, self.table.data_ptr(),
                                       case.sub_limit, self.slots.data_ptr(), self.stamps.data_ptr(), case.w, case.now, case.interval,
                                       self.cap_out, self.off.data_ptr(), self.items.data_ptr(), self.status.data_ptr(),
                                       self.cnt.data_ptr(), self.timers.data_ptr(), d_intervals=ptr(self.intervals),
                                       d_deadlines=ptr(self.deadlines), ref_limit=case.ref_limit, mode=case.mode,
                                       update_table=update_table, d_n_boxes=ptr(self.count))

    def result(self, T, summary=None):
        """The outputs up to their defined extents, after checking that nothing behind them changed."""
        from emqx_amd import ack, window
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.SWEEP_SUMMARY, s[:8].tolist()))
        refused = summary["flags"] & R.F_INPUT_REFUSED
        full = summary["flags"] & R.F_OUTPUT_FULL
        m = 0 if refused else summary["sessions"]
        n_items = 0 if refused or full else summary["items"]
        off, items = self.off.cpu().numpy().view(np.uint64), self.items.cpu().numpy()
        status, cnt, timers = self.status.cpu().numpy(), self.cnt.cpu().numpy().view(np.uint32), self.timers.cpu().numpy().view(np.uint32)
        assert (off[(0 if refused else m + 1):] == S64).all() and (items[n_items:] == S64).all(), "a write past the defined extent"
        assert (status[m:] == S8).all() and (cnt[4 * m:] == S32).all() and (timers[m:] == S32).all(), "a write past the defined extent"
        c = self.case
        got = T.Swept(off[:0 if refused else m + 1], np.frombuffer(items[:n_items].tobytes(), dtype=T.ITEM), status[:m],
                      cnt[:4 * m].reshape(-1, 4), timers[:m], summary)
        return (got, back(self.slots, c.sub_limit * c.w, ack.SLOT, (c.sub_limit, c.w), "the slot table"),
                back(self.stamps, c.sub_limit * c.w, np.uint64, (c.sub_limit, c.w), "the stamp table"),
                back(self.table, 4 * c.sub_limit, window.SESSION, (c.sub_limit,), "the session table"))


def sweep_host_buffers(T, h, case, **kw):
    from tests.test_retry_cpu import sweep
    return sweep(T, case, h=h, fn="sweep", **kw)


def sweep_sync(T, h, case, **kw):
    from emqx_amd import _lib
    b = SweepBatch(T, case, **kw)
    try:
        summary = h.sweep_device(b.args)
    except _lib.EngineError as e:
        assert e.code == (-4 if e.summary["flags"] & R.F_OUTPUT_FULL and not e.summary["flags"] & R.F_INPUT_REFUSED else -1)
        assert e.summary["flags"] & (R.F_BAD_SUB | R.F_INPUT_REFUSED | R.F_OUTPUT_FULL)
        summary = e.summary
    return b.result(T, summary)


def sweep_async(T, h, case, **kw):
    import torch
    b = SweepBatch(T, case, **kw)
    h.reserve(b.cap_boxes, case.w)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        h.sweep_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(T)


def all_forms(T, h, case, update_table=True, cap_out="case"):
    """Every device entry point: exact against the restatement, identical to the host evaluator."""
    from tests.test_retry_cpu import sweep
    cap = case.cap_out if cap_out == "case" else cap_out
    ref = case.reference(update_table, cap)
    host = sweep(T, case, update_table, cap_out)
    C.check(ref, *host)
    kw = dict(update_table=update_table, cap_out=cap_out)
    for got in (sweep_host_buffers(T, h, case, **kw), sweep_sync(T, h, case, **kw), sweep_async(T, h, case, **kw),
                sweep_async(T, h, case, count_on_device=True, **kw)):
        C.check(ref, *got)
        C.same(got[0], host[0])
        assert [x.tobytes() for x in got[1:]] == [x.tobytes() for x in host[1:]]
    return ref


@pytest.mark.parametrize("name", list(C.SWEEPS))
def test_sweep_cases(T, handle, name):
    """Rows of 8, 32 and 64 slots with 0, 1 and W items, ties, the age and deadline boundaries,
    sessions that are not swept, unstamped and malformed rows, the whole-table sweep, replay, row
    counts around a block's rows, five tiles."""
    all_forms(T, handle, C.SWEEPS[name]())


@pytest.mark.parametrize("name", ["every_old_entry_expired", "deadlines_now-1_now_now+1_never_pubrel"])
def test_without_update_table_the_table_is_untouched(T, handle, name):
    case = C.SWEEPS[name]()
    all_forms(T, handle, case, update_table=False)
    for run in (sweep_sync, sweep_async):
        assert run(T, handle, case, update_table=False)[3].tobytes() == case.table.tobytes()


def test_fuzz(T, handle):
    case = C.fuzz()
    all_forms(T, handle, case)
    x, y = sweep_async(T, handle, case), sweep_async(T, handle, case)  # two runs are byte-identical
    C.same(x[0], y[0])
    assert [a.tobytes() for a in x[1:]] == [a.tobytes() for a in y[1:]]
    all_forms(T, handle, C.fuzz(mode=R.MODE_REPLAY, n_sessions=300))


def test_count_is_read_on_the_device(T, handle):
    """cap_boxes and cap_out larger than the counts: the buffers are larger than what is written."""
    case = C.fuzz(seed=6, n_sessions=400)
    ref = case.reference(True)
    for run in (sweep_sync, sweep_async):
        for on_device in (False, True):
            got = run(T, handle, case, cap_boxes=case.m + 77, cap_out=ref["summary"][3] + 9, count_on_device=on_device)
            C.check(ref, *got)


def test_overflow_changes_nothing_and_the_repeat_succeeds(T, handle):
    case = C.overflow_case()
    need = case.reference()["summary"][3]
    ref = all_forms(T, handle, case, cap_out=need - 1)
    assert ref["summary"][0] == R.F_OUTPUT_FULL and ref["summary"][3] == need
    # on one set of device buffers: the full call, then the same call with room
    import torch
    b = SweepBatch(T, case, cap_out=need - 1)
    handle.reserve(b.cap_boxes, case.w)
    handle.sweep_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    got, slots, stamps, table = b.result(T)
    assert got.summary["flags"] == R.F_OUTPUT_FULL and got.summary["items"] == need and got.items.size == 0
    assert (slots.tobytes(), stamps.tobytes(), table.tobytes()) == (case.slots.tobytes(), case.stamps.tobytes(), case.table.tobytes())
    room = filled(need, torch.int64)
    b.args.out_items, b.args.cap_out, b.items = room.data_ptr(), need, room
    handle.sweep_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    C.check(case.reference(True, need), *b.result(T))


@pytest.mark.parametrize("form", ["sync", "async"])
def test_refused_input_writes_only_the_summary(T, handle, form):
    import torch
    from emqx_amd import _lib
    case = C.overflow_case()
    b = SweepBatch(T, case, cap_boxes=case.m - 1, count_on_device=True)
    if form == "sync":
        with pytest.raises(_lib.EngineError) as e:
            handle.sweep_device(b.args)
        assert e.value.code == -1
        summary = e.value.summary
    else:
        handle.reserve(b.cap_boxes, case.w)
        handle.sweep_device_async(b.args, b.summary.data_ptr())
        torch.cuda.synchronize()
        summary = dict(zip(T.SWEEP_SUMMARY, b.summary.cpu().numpy().view(np.uint64)[:8].tolist()))
    assert [summary[k] for k in T.SWEEP_SUMMARY] == [R.F_INPUT_REFUSED, 0, case.m, 0, 0, 0, 0, 0]
    got, slots, stamps, table = b.result(T, summary)  # the sentinels are intact from the first element of every output
    assert got.offsets.size == 0 and got.status.size == 0
    assert (slots.tobytes(), stamps.tobytes(), table.tobytes()) == (case.slots.tobytes(), case.stamps.tobytes(), case.table.tobytes())


def test_scratch_reuse_on_one_handle(T):
    """Five tiles, then one row, then the fuzz: no total or counter of an earlier call shows in a
    later one."""
    h = T.Retry(0)
    for case in (C.SWEEPS["scan_chunk_2_five_tiles_w64"](), C.SWEEPS["one_item"](), C.fuzz()):
        for run in (sweep_async, sweep_sync):
            C.check(case.reference(True), *run(T, h, case))
    assert h.stats()["calls"] == 6 and h.stats()["cap_boxes"] == C.fuzz().m and h.stats()["w"] == 64


def test_async_needs_reserve(T):
    import torch
    from emqx_amd import _lib
    case = C.SWEEPS["full_row_tie_w32"]()
    b = SweepBatch(T, case)
    h = T.Retry(0)
    for short in (None, (case.m - 1, case.w), (case.m, 8)):
        if short:
            h = T.Retry(0)
            h.reserve(*short)
        with pytest.raises(_lib.EngineError) as e:
            h.sweep_device_async(b.args, b.summary.data_ptr())
        assert e.value.code == _lib.EMQX_EOVERFLOW
    torch.cuda.synchronize()
    assert (b.summary.cpu().numpy().view(np.uint64) == S64).all() and h.stats()["calls"] == 0, "nothing was enqueued"
    h.reserve(case.m, case.w)
    h.sweep_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    C.check(case.reference(True), *b.result(T))


def test_misaligned_tables_and_bad_widths_are_refused(T, handle):
    from emqx_amd import _lib
    case = C.SWEEPS["one_item"]()
    for change in (dict(slots=8), dict(stamps=8), dict(sessions=8), dict(out_counts=4), dict(w=-4), dict(mode=2)):
        b = SweepBatch(T, case)
        for k, v in change.items():
            setattr(b.args, k, getattr(b.args, k) + v)
        with pytest.raises(_lib.EngineError) as e:
            handle.sweep_device(b.args)
        assert e.value.code == -1
        assert b.result(T, dict(dict.fromkeys(T.SWEEP_SUMMARY, 0), flags=R.F_INPUT_REFUSED))[2].tobytes() == case.stamps.tobytes()


# ---- the stamp call ----------------------------------------------------------------------------

class StampBatch:
    def __init__(self, T, case, cap_boxes=None, count_on_device=False):
        import torch
        self.case = case
        self.cap_boxes = case.m if cap_boxes is None else cap_boxes
        self.subs, self.slots, self.stamps = dev(case.subs, np.uint32), dev_raw(case.slots), dev_raw(case.stamps, GUARD)
        self.count = dev([case.m], np.uint64) if count_on_device else None
        self.summary = filled(8, torch.int64)
        self.args = T.Retry.stamp_args(self.subs.data_ptr(), 0 if count_on_device else case.m, self.cap_boxes, self.slots.data_ptr(),
                                       self.stamps.data_ptr(), case.w, case.sub_limit, case.now,
                                       d_n_boxes=self.count.data_ptr() if count_on_device else 0)

    def result(self, T, summary=None):
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.STAMP_SUMMARY, s[:8].tolist()))
        c = self.case
        return T.Stamped(summary), back(self.stamps, c.sub_limit * c.w, np.uint64, (c.sub_limit, c.w), "the stamp table")


def stamp_sync(T, h, case, **kw):
    from emqx_amd import _lib
    b = StampBatch(T, case, **kw)
    try:
        summary = h.stamp_device(b.args)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & R.F_BAD_SUB
        summary = e.summary
    return b.result(T, summary)


def stamp_async(T, h, case, **kw):
    import torch
    b = StampBatch(T, case, **kw)
    h.reserve(b.cap_boxes, case.w)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        h.stamp_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(T)


@pytest.mark.parametrize("name", list(C.STAMPS))
def test_stamp_cases(T, handle, name):
    """An insert, a PUBREC transition, an unchanged slot, a freed slot, a slot refilled with another
    id, a bad subscriber; rows per block + 1 at each width over stale stamps of every sort."""
    from tests.test_retry_cpu import stamp
    case = C.STAMPS[name]()
    ref = case.reference()
    host = stamp(T, case)
    C.check_stamp(ref, *host)
    for got in (stamp(T, case, fn="stamp", h=handle), stamp_sync(T, handle, case), stamp_async(T, handle, case),
                stamp_async(T, handle, case, cap_boxes=case.m + 9, count_on_device=True)):
        C.check_stamp(ref, *got)
        assert got[0].summary == host[0].summary and got[1].tobytes() == host[1].tobytes()


# ---- the chain ---------------------------------------------------------------------------------

def test_chain_window_record_stamp_sweep_ack_stamp_sweep_sweep_window_on_one_stream(T):
    """A session with inflight_max 3 takes three deliveries at t (ids 1, 2, 3; refs 70, 71, 72; ref 70
    expires at t + 100).  Record and stamp at t; a sweep at t + 40 with interval 100 finds nothing due
    and says 60; a PUBREC of id 2 and the stamp at t + 50; the sweep at t + 120 deletes id 1 as expired,
    sends id 3 again and says 30 (the PUBREL entry is 70 old); the same sweep again finds nothing due;
    the window then has room for one more delivery, id 4.  One stream, no host read in between."""
    import torch
    from emqx_amd import ack as A
    from emqx_amd import window as W
    from tests import ack_ref as AR
    from tests import window_ref as WR
    from tests.ack_cases import rows_of
    sub_limit, w, sub, t, iv = 5, 8, 3, C.NOW, 100
    table = W.pack_sessions(sub_limit, inflight_max=3)
    rows, stamps = A.empty_slots(sub_limit, w), T.empty_stamps(sub_limit, w)
    expiry = [(0, 0)] * 70 + [(t - 900, 1), (t, None), (t, 50)]
    deadlines = np.array([T.deadline(c, s) for c, s in expiry], dtype=np.uint64)
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    d_table, d_rows, d_stamps, d_dead = dev_raw(table), dev_raw(rows), dev_raw(stamps), dev(deadlines, np.uint64)
    subs1, off1, opts1, refs1 = dev([sub], np.uint32), dev([0, 3], np.uint64), dev([1, 2, 1], np.uint8), dev([70, 71, 72], np.uint32)
    ver1, ids1, recs1, cnt1, sum1 = z(3, torch.uint8), z(3, torch.int16), z(4, torch.int64), z(4, torch.int32), z(8, torch.int64)
    unrec, rsum = z(1, torch.int32), z(8, torch.int64)
    acks, aoff = dev(A.pack_acks([AR.PUBREC], [2]), np.uint32), dev([0, 1], np.uint64)
    aver, arefs, acnt, asum = z(1, torch.uint8), z(1, torch.int32), z(4, torch.int32), z(8, torch.int64)
    off2, opts2 = dev([0, 1], np.uint64), dev([1], np.uint8)
    ver2, ids2, recs2, cnt2, sum2 = z(1, torch.uint8), z(1, torch.int16), z(4, torch.int64), z(4, torch.int32), z(8, torch.int64)
    tsum = [z(8, torch.int64) for _ in range(2)]
    sw = [dict(off=z(2, torch.int64), items=z(w, torch.int64), status=z(1, torch.uint8), cnt=z(4, torch.int32), timers=z(1, torch.int32),
               summary=z(8, torch.int64)) for _ in range(3)]
    win, ack, rt = W.Window(0), A.Ack(0), T.Retry(0)
    win.reserve(3, 1)
    ack.reserve(3, 1, w)
    rt.reserve(1, w)
    w1 = W.Window.batch(subs1.data_ptr(), off1.data_ptr(), opts1.data_ptr(), 1, 3, 1, d_table.data_ptr(), sub_limit, ver1.data_ptr(),
                        ids1.data_ptr(), recs1.data_ptr(), cnt1.data_ptr(), update_table=True)
    r1 = A.Ack.record_args(subs1.data_ptr(), off1.data_ptr(), opts1.data_ptr(), 1, 3, 1, ver1.data_ptr(), ids1.data_ptr(),
                           d_rows.data_ptr(), w, sub_limit, unrec.data_ptr(), d_refs=refs1.data_ptr())
    a1 = A.Ack.run_args(subs1.data_ptr(), aoff.data_ptr(), acks.data_ptr(), 1, 1, 1, d_table.data_ptr(), sub_limit, d_rows.data_ptr(), w,
                        aver.data_ptr(), arefs.data_ptr(), acnt.data_ptr(), update_table=True)
    w2 = W.Window.batch(subs1.data_ptr(), off2.data_ptr(), opts2.data_ptr(), 1, 1, 1, d_table.data_ptr(), sub_limit, ver2.data_ptr(),
                        ids2.data_ptr(), recs2.data_ptr(), cnt2.data_ptr(), update_table=True)

    def stamp_at(now):
        return T.Retry.stamp_args(subs1.data_ptr(), 1, 1, d_rows.data_ptr(), d_stamps.data_ptr(), w, sub_limit, now)

    def sweep_at(now, o):
        return T.Retry.sweep_args(subs1.data_ptr(), 1, 1, d_table.data_ptr(), sub_limit, d_rows.data_ptr(), d_stamps.data_ptr(), w, now, iv,
                                  w, o["off"].data_ptr(), o["items"].data_ptr(), o["status"].data_ptr(), o["cnt"].data_ptr(),
                                  o["timers"].data_ptr(), d_deadlines=d_dead.data_ptr(), ref_limit=len(expiry), update_table=True)

    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        win.run_device_async(w1, sum1.data_ptr(), stream=s)
        ack.record_device_async(r1, rsum.data_ptr(), stream=s)
        rt.stamp_device_async(stamp_at(t), tsum[0].data_ptr(), stream=s)
        rt.sweep_device_async(sweep_at(t + 40, sw[0]), sw[0]["summary"].data_ptr(), stream=s)
        ack.run_device_async(a1, asum.data_ptr(), stream=s)
        rt.stamp_device_async(stamp_at(t + 50), tsum[1].data_ptr(), stream=s)
        rt.sweep_device_async(sweep_at(t + 120, sw[1]), sw[1]["summary"].data_ptr(), stream=s)
        rt.sweep_device_async(sweep_at(t + 120, sw[2]), sw[2]["summary"].data_ptr(), stream=s)
        win.run_device_async(w2, sum2.data_ptr(), stream=s)
    stream.synchronize()
    # the restatements, step by step
    u64 = lambda x: x.cpu().numpy().view(np.uint64).tolist()  # noqa: E731
    recs = [{f: int(table[f][i]) for f in WR.FIELDS} for i in range(sub_limit)]
    x1 = WR.run([sub], [0, 3], [1, 2, 1], recs, update_table=True)
    assert x1["verdicts"] == [W.W_SEND] * 3 and x1["pkt_ids"] == [1, 2, 3] and ids1.cpu().numpy().view(np.uint16).tolist() == [1, 2, 3]
    ref_rows, ref_stamps = rows_of(rows), stamps.tolist()
    assert u64(rsum) == AR.record([sub], [0, 3], [1, 2, 1], x1["verdicts"], x1["pkt_ids"], [70, 71, 72], ref_rows)["summary"]
    assert u64(tsum[0]) == R.stamp([sub], ref_rows, ref_stamps, t) == [0, 1, 1, 3, 0, 0, 0, 0]

    def swept(o, ref):
        n = ref["offsets"][-1]
        assert u64(o["summary"]) == ref["summary"] and u64(o["off"]) == ref["offsets"]
        items = np.frombuffer(o["items"].cpu().numpy()[:n].tobytes(), dtype=T.ITEM).tolist()
        assert [list(map(int, it)) for it in items] == ref["items"]
        assert o["status"].cpu().numpy().tolist() == ref["status"] and o["cnt"].cpu().numpy().view(np.uint32).tolist() == ref["counts"][0]
        assert o["timers"].cpu().numpy().view(np.uint32).tolist() == ref["timers"]
        return ref

    x = swept(sw[0], R.sweep([sub], recs, ref_rows, ref_stamps, t + 40, iv, expiry=expiry, update_table=True))
    assert x["items"] == [] and x["timers"] == [iv - 40] and x["counts"] == [[0, 0, 0, 3]], "nothing due: interval - elapsed"
    xa = AR.run([sub], [0, 1], A.pack_acks([AR.PUBREC], [2]), recs, ref_rows, update_table=True)
    assert xa["verdicts"] == [AR.A_OK] and u64(asum) == xa["summary"] and aver.cpu().numpy().tolist() == [AR.A_OK]
    assert u64(tsum[1]) == R.stamp([sub], ref_rows, ref_stamps, t + 50) == [0, 1, 1, 1, 0, 0, 0, 0]
    x = swept(sw[1], R.sweep([sub], recs, ref_rows, ref_stamps, t + 120, iv, expiry=expiry, update_table=True))
    assert x["items"] == [[1, R.EXPIRED, 1, 70], [3, R.PUBLISH_DUP, 1, 72]] and x["timers"] == [30] and x["counts"] == [[1, 0, 1, 2]]
    x = swept(sw[2], R.sweep([sub], recs, ref_rows, ref_stamps, t + 120, iv, expiry=expiry, update_table=True))
    assert x["items"] == [] and x["timers"] == [30] and x["counts"] == [[0, 0, 0, 2]], "the second sweep at the same now"
    x2 = WR.run([sub], [0, 1], [1], recs, update_table=True)
    assert x2["verdicts"] == [W.W_SEND] and x2["pkt_ids"] == [4], "the expiry reopened the window"
    assert ver2.cpu().numpy().tolist() == x2["verdicts"] and ids2.cpu().numpy().view(np.uint16).tolist() == x2["pkt_ids"]
    got_rows = np.frombuffer(d_rows.cpu().numpy().tobytes(), dtype=A.SLOT).reshape(sub_limit, w)
    assert rows_of(got_rows) == ref_rows and ref_rows[sub][:3] == [[0, 0, 0, 0], [2, AR.PUBREL_AWAIT, 2, 71], [3, AR.MSG, 1, 72]]
    assert d_stamps.cpu().numpy().view(np.uint64).reshape(sub_limit, w).tolist() == ref_stamps
    assert [R.read_stamp(v) for v in ref_stamps[sub][:3]] == [(0, 0, 0, 0), (t + 50, 0, 2, 2), (t + 120, 1, 1, 3)]
    got_table = np.frombuffer(d_table.cpu().numpy().tobytes(), dtype=W.SESSION)
    assert [{f: int(got_table[f][i]) for f in WR.FIELDS} for i in range(sub_limit)] == recs
    assert int(got_table["inflight"][sub]) == 3 and int(got_table["next_pkt_id"][sub]) == 5
