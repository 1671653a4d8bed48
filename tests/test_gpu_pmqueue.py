"""The priority mqueue stage (include/emqx_pmqueue.h) on the device: every case of tests/pmqueue_cases.py
through emqx_pmqueue_*_batch, _batch_device and _batch_device_async, exact against the literal restatement and
byte for byte what the host evaluator leaves (outputs, rings, heads, records), with sentinels behind
every output; on a default handle and on one whose single block strides and whose scan carries at every
total; every group width; the lattice of tests/pmqueue_cases.py (C x Qc x group width) from uploaded tables and with the tables
kept on the device; the count read on the device; the cycle window -> record -> stamp -> put -> ack run -> stamp
-> take -> record -> stamp on one stream with no host read, against the restatements of all four stages."""

import os
import random

import numpy as np
import pytest

from tests import pmqueue_cases as C
from tests import pmqueue_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S8, S16, S32, S64 = 0x5A, 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64  # sentinel elements behind every output buffer's capacity
PUT_CASES = C.put_cases()
TAKE_CASES = C.take_cases()


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import pmqueue
    return pmqueue


@pytest.fixture(scope="module", params=[(None, None), (1, 1)], ids=["default", "1_block-scan_chunk_1"])
def handle(T, request):
    max_blocks, scan_chunk = request.param
    h = T.Pmqueue(0)
    if max_blocks is not None:
        h.set_tuning("max_blocks", max_blocks)
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
    raw = np.frombuffer(table.tobytes() or bytes(64), dtype=np.int64)
    return torch.from_numpy(np.concatenate([raw, np.full(guard, S64, dtype=np.int64)])).to(DEV)


def filled(k, dtype):  # every byte 0x5A
    import torch
    sent = {torch.uint8: S8, torch.int16: S16, torch.int32: S32, torch.int64: S64}[dtype]
    return torch.full((k + GUARD,), sent, dtype=dtype, device=DEV)


def back(t, table, what):
    """A guarded device table as a host array of the shape and type of `table`."""
    raw = t.cpu().numpy()
    n = table.nbytes // 8
    assert (raw[n:] == S64).all(), "a write past " + what
    return np.frombuffer(raw[:n].tobytes(), dtype=table.dtype).reshape(table.shape).copy()


def ptr(t):
    return 0 if t is None else t.data_ptr()


class State:
    """The tables of a case in device memory, a guard behind each."""

    def __init__(self, case):
        self.case = case
        self.tables = dev_raw(case.tables)
        self.sessions, self.ring, self.heads = dev_raw(case.sessions, GUARD), dev_raw(case.ring, GUARD), dev_raw(case.heads, GUARD)

    def result(self):
        c = self.case
        return back(self.sessions, c.sessions, "the records"), back(self.ring, c.ring, "the rings"), back(self.heads, c.heads, "the heads")


class PutBatch(State):
    def __init__(self, T, case, update_table=True, count_on_device=False, slack=0):
        import torch
        super().__init__(case)
        self.m, self.total = case.subs.size, int(case.offsets[-1])
        self.cap_in, self.cap_boxes = self.total + slack, self.m + slack
        pad = lambda a, n, dt: np.concatenate([np.asarray(a, dtype=dt), np.zeros(n - len(a), dtype=dt)])  # noqa: E731
        self.subs, self.off = dev(pad(case.subs, self.cap_boxes, np.uint32), np.uint32), dev(pad(case.offsets, self.cap_boxes + 1, np.uint64), np.uint64)
        self.opts, self.ver = dev(pad(case.opts, self.cap_in, np.uint8), np.uint8), dev(pad(case.verdicts, self.cap_in, np.uint8), np.uint8)
        self.src = dev(pad(case.src, self.cap_in, np.uint32), np.uint32)
        self.refs = None if case.refs is None else dev(pad(case.refs, self.cap_in, np.uint32), np.uint32)
        self.mc = dev(case.msg_class.reshape(-1), np.uint8)
        self.count = dev([self.m], np.uint64) if count_on_device else None
        self.o_ver, self.o_cls, self.ev = filled(self.cap_in, torch.uint8), filled(self.cap_in, torch.uint8), filled(self.cap_in, torch.int64)
        self.cnt, self.summary = filled(8 * self.cap_boxes, torch.int32), filled(8, torch.int64)
        self.args = T.Pmqueue.put_args(
            inbox_subs=ptr(self.subs), inbox_offsets=ptr(self.off), box_opts=ptr(self.opts), n_boxes=ptr(self.count),
            m=0 if count_on_device else self.m, cap_in=self.cap_in, cap_boxes=self.cap_boxes, verdicts=ptr(self.ver), refs=ptr(self.refs),
            box_src=ptr(self.src), msg_class=ptr(self.mc), n_msgs=case.msg_class.shape[0], tables=ptr(self.tables),
            n_tables=case.tables.size, sessions=ptr(self.sessions), sub_limit=case.sessions.size, update_table=1 if update_table else 0,
            ring=ptr(self.ring), heads=ptr(self.heads), c=case.ring.shape[1], qc=case.ring.shape[2], out_verdicts=ptr(self.o_ver),
            out_class=ptr(self.o_cls), out_evicted=ptr(self.ev), out_counts=ptr(self.cnt))

    def outputs(self, T, summary=None):
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.PUT_SUMMARY, s[:8].tolist()))
        ver, cls, ev = self.o_ver.cpu().numpy(), self.o_cls.cpu().numpy(), self.ev.cpu().numpy()
        cnt = self.cnt.cpu().numpy().view(np.uint32)
        assert (ver[self.total:] == S8).all() and (cls[self.total:] == S8).all() and (ev[self.total:] == S64).all()
        assert (cnt[8 * self.m:] == S32).all(), "a write past the defined extent"
        return T.Put(ver[:self.total], cls[:self.total], np.frombuffer(ev[:self.total].tobytes(), dtype=T.ENTRY),
                     cnt[:8 * self.m].reshape(-1, 8), summary)


def put_device(T, h, case, mode, **kw):
    import torch
    from emqx_amd import _lib
    b = PutBatch(T, case, **kw)
    if mode == "sync":
        try:
            summary = h.put_device(b.args)
        except _lib.EngineError as e:
            assert e.code == -1 and e.summary["flags"] & R.F_BAD_SUB
            summary = e.summary
        return (b.outputs(T, summary),) + b.result()
    h.reserve(b.cap_in, b.cap_boxes)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        h.put_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return (b.outputs(T),) + b.result()


def same(x, y):
    assert x.summary == y.summary
    for a, b in zip(x[:-1], y[:-1]):
        assert a.tobytes() == b.tobytes()


def check_put_everywhere(T, h, case, update_table=True, **kw):
    from tests.test_pmqueue_cpu import put
    want, sessions, ring, heads = put(T, case, update_table)
    for mode in ("sync", "async"):
        got, d_sessions, d_ring, d_heads = put_device(T, h, case, mode, update_table=update_table, **kw)
        C.check_put(case.reference(), got, case, d_sessions, d_ring, d_heads, update_table)
        same(got, want)
        assert d_sessions.tobytes() == sessions.tobytes() and d_ring.tobytes() == ring.tobytes() and d_heads.tobytes() == heads.tobytes()
    if not kw:  # host buffers to the device: the rows the call names travel
        got, b_sessions, b_ring, b_heads = put(T, case, update_table, h=h, fn="put")
        same(got, want)
        assert b_sessions.tobytes() == sessions.tobytes() and b_ring.tobytes() == ring.tobytes() and b_heads.tobytes() == heads.tobytes()


@pytest.mark.parametrize("case", PUT_CASES, ids=[c.name for c in PUT_CASES])
def test_put_cases(T, handle, case):
    check_put_everywhere(T, handle, case)


@pytest.mark.parametrize("name", ["many_inboxes", "malformed_heads", "c3_q8_full_e5"])
def test_put_without_update_table_leaves_heads_and_records(T, handle, name):
    check_put_everywhere(T, handle, next(c for c in PUT_CASES if c.name == name), update_table=False)


# ---- take ---------------------------------------------------------------------------------------

class TakeBatch(State):
    def __init__(self, T, case, update_table=True, cap_out="case", count_on_device=False, slack=0):
        import torch
        super().__init__(case)
        n, c, qc = case.ring.shape
        self.m = n if case.subs is None else case.subs.size
        self.cap_boxes = self.m + slack
        cap = case.cap_out if cap_out == "case" else cap_out
        self.cap_out = self.m * c * qc if cap is None else cap
        self.subs = None if case.subs is None else dev(np.concatenate([case.subs, np.zeros(slack, np.uint32)]), np.uint32)
        self.deadlines = None if case.deadlines is None else dev(case.deadlines, np.uint64)
        self.count = dev([self.m], np.uint64) if count_on_device else None
        self.off = filled(self.cap_boxes + 1, torch.int64)
        self.opts, self.ver, self.cls = (filled(self.cap_out, torch.uint8) for _ in range(3))
        self.ids, self.refs = filled(self.cap_out, torch.int16), filled(self.cap_out, torch.int32)
        self.status, self.cnt, self.summary = filled(self.cap_boxes, torch.uint8), filled(4 * self.cap_boxes, torch.int32), filled(8, torch.int64)
        self.args = T.Pmqueue.take_args(
            subs=ptr(self.subs), n_boxes=ptr(self.count), m=0 if count_on_device else self.m, cap_boxes=self.cap_boxes,
            sessions=ptr(self.sessions), sub_limit=n, update_table=1 if update_table else 0, tables=ptr(self.tables),
            n_tables=case.tables.size, ring=ptr(self.ring), heads=ptr(self.heads), c=c, qc=qc, now_ms=case.now,
            deadlines=ptr(self.deadlines), ref_limit=0 if case.deadlines is None else case.deadlines.size, cap_out=self.cap_out,
            out_offsets=ptr(self.off), out_opts=ptr(self.opts), out_verdicts=ptr(self.ver), out_pkt_ids=ptr(self.ids),
            out_refs=ptr(self.refs), out_class=ptr(self.cls), out_status=ptr(self.status), out_counts=ptr(self.cnt))

    def outputs(self, T, summary=None):
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.TAKE_SUMMARY, s[:8].tolist()))
        full = summary["flags"] & R.F_OUTPUT_FULL
        k = 0 if full else min(summary["items"], self.cap_out)
        off = self.off.cpu().numpy().view(np.uint64)
        opts, ver, cls = self.opts.cpu().numpy(), self.ver.cpu().numpy(), self.cls.cpu().numpy()
        ids, refs = self.ids.cpu().numpy().view(np.uint16), self.refs.cpu().numpy().view(np.uint32)
        status, cnt = self.status.cpu().numpy(), self.cnt.cpu().numpy().view(np.uint32)
        assert (off[self.m + 1:] == S64).all() and (status[self.m:] == S8).all() and (cnt[4 * self.m:] == S32).all()
        assert (opts[k:] == S8).all() and (ver[k:] == S8).all() and (cls[k:] == S8).all() and (ids[k:] == S16).all() and (refs[k:] == S32).all()
        return T.Taken(off[:self.m + 1], opts[:k], ver[:k], ids[:k], refs[:k], cls[:k], status[:self.m], cnt[:4 * self.m].reshape(-1, 4), summary)


def take_device(T, h, case, mode, **kw):
    import torch
    from emqx_amd import _lib
    b = TakeBatch(T, case, **kw)
    if mode == "sync":
        try:
            summary = h.take_device(b.args)
        except _lib.EngineError as e:
            assert e.code in (-1, -4) and e.summary["flags"] & (R.F_BAD_SUB | R.F_OUTPUT_FULL)
            summary = e.summary
        return (b.outputs(T, summary),) + b.result()
    h.reserve(0, b.cap_boxes)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        h.take_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return (b.outputs(T),) + b.result()


def check_take_everywhere(T, h, case, update_table=True, cap_out="case", **kw):
    from tests.test_pmqueue_cpu import take
    want, sessions, ring, heads = take(T, case, update_table, cap_out)
    for mode in ("sync", "async"):
        got, d_sessions, d_ring, d_heads = take_device(T, h, case, mode, update_table=update_table, cap_out=cap_out, **kw)
        C.check_take(case.reference(cap_out), got, case, d_sessions, d_ring, d_heads, update_table)
        same(got, want)
        assert d_sessions.tobytes() == sessions.tobytes() and d_ring.tobytes() == ring.tobytes() and d_heads.tobytes() == heads.tobytes()
    if not kw:
        got, b_sessions, b_ring, b_heads = take(T, case, update_table, cap_out, h=h, fn="take")
        same(got, want)
        assert b_sessions.tobytes() == sessions.tobytes() and b_ring.tobytes() == ring.tobytes() and b_heads.tobytes() == heads.tobytes()
    return want


@pytest.mark.parametrize("case", TAKE_CASES, ids=[c.name for c in TAKE_CASES])
def test_take_cases(T, handle, case):
    check_take_everywhere(T, handle, case)


@pytest.mark.parametrize("name", ["many_sessions", "malformed_heads", "full_row_budget_1000"])
def test_take_without_update_table_nothing_is_touched(T, handle, name):
    check_take_everywhere(T, handle, next(c for c in TAKE_CASES if c.name == name), update_table=False)


def test_overflow_changes_nothing_and_the_repeat_succeeds(T, handle):
    case = C.overflow_case()
    first = check_take_everywhere(T, handle, case)
    assert first.summary["flags"] == R.F_OUTPUT_FULL and first.summary["items"] == 5
    again = check_take_everywhere(T, handle, case, cap_out=5)
    assert again.summary["flags"] == 0 and sorted(again.refs.tolist()) == [1, 2, 3, 4, 5]


# ---- the group width, the count on the device, the scratch ---------------------------------------

@pytest.mark.parametrize("group", [4, 8, 16, 32, 64])
def test_every_group_width_gives_the_same_bytes(T, group):
    """256 / G inboxes or sessions a block: 300 of them span more than one block at every width but 4,
    where many_* still fills the second block's first groups; an inbox of 2 349 takes 37 to 588 trips."""
    h = T.Pmqueue(0)
    h.set_tuning("group", group)
    assert h.stats()["group"] == group
    for name in ("many_inboxes", "inbox_2349", "inbox_1024", "c8_q64_full_e6", "row_full", "unfit_tables", "q128_full_bytes",
                 "one_group_last_tile"):
        check_put_everywhere(T, h, next(c for c in PUT_CASES if c.name == name))
    for name in ("many_sessions", "full_row_budget_1000", "full_row_budget_4", "expired_and_qos0", "statuses", "subs_null",
                 "q128_full_bytes", "q32_bits_word1", "one_group_last_tile"):
        check_take_everywhere(T, h, next(c for c in TAKE_CASES if c.name == name))


def test_the_count_is_read_on_the_device(T, handle):
    """n_boxes names device memory; the capacities exceed the counts and nothing behind them is written."""
    check_put_everywhere(T, handle, next(c for c in PUT_CASES if c.name == "many_inboxes"), count_on_device=True, slack=37)
    check_take_everywhere(T, handle, next(c for c in TAKE_CASES if c.name == "many_sessions"), count_on_device=True, slack=37)


def test_a_refused_count_writes_the_summary_alone(T, handle):
    import torch
    case = next(c for c in PUT_CASES if c.name == "many_inboxes")
    b = PutBatch(T, case, count_on_device=True)
    b.count.fill_(b.cap_boxes + 1)
    handle.reserve(b.cap_in, b.cap_boxes)
    handle.put_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    assert b.summary.cpu().numpy().view(np.uint64)[:8].tolist() == [T.F_INPUT_REFUSED, 0, b.cap_boxes + 1, 0, 0, 0, 0, 0]
    assert (b.o_ver.cpu().numpy() == S8).all() and (b.cnt.cpu().numpy() == S32).all()
    sessions, ring, heads = b.result()
    assert ring.tobytes() == case.ring.tobytes() and heads.tobytes() == case.heads.tobytes() and sessions.tobytes() == case.sessions.tobytes()


def test_async_needs_the_scratch_reserved(T):
    from emqx_amd import _lib
    h = T.Pmqueue(0)
    b = TakeBatch(T, next(c for c in TAKE_CASES if c.name == "statuses"))
    with pytest.raises(_lib.EngineError) as e:
        h.take_device_async(b.args, b.summary.data_ptr())
    assert e.value.code == -4
    assert (b.summary.cpu().numpy() == S64).all()  # nothing was enqueued
    h.reserve(0, b.cap_boxes)
    h.take_device_async(b.args, b.summary.data_ptr())
    import torch
    torch.cuda.synchronize()
    assert b.outputs(T).summary["sessions"] == b.m and h.stats()["calls"] == 1 and h.stats()["cap_boxes"] == b.cap_boxes


def test_misaligned_tables_are_refused(T, handle):
    """One pointer at a time is off by half of what the device forms require of it (ring 8, heads 64,
    sessions 16, out_counts 16, out_offsets 8): EMQX_EINVAL, nothing is enqueued, every byte stays."""
    from emqx_amd import _lib
    put = next(c for c in PUT_CASES if c.name == "no_refs")
    take = next(c for c in TAKE_CASES if c.name == "rotated_list")
    for case, batch, call, fields in (
            (put, PutBatch, handle.put_device, (("ring", 4), ("heads", 32), ("sessions", 8), ("out_counts", 8))),
            (take, TakeBatch, handle.take_device, (("ring", 4), ("heads", 32), ("sessions", 8), ("out_counts", 8), ("out_offsets", 4)))):
        for field, by in fields:
            b = batch(T, case)
            assert getattr(b.args, field)
            setattr(b.args, field, getattr(b.args, field) + by)
            with pytest.raises(_lib.EngineError) as e:
                call(b.args)
            assert e.value.code == -1
            assert (b.cnt.cpu().numpy().view(np.uint32) == S32).all()
            if batch is TakeBatch:
                assert (b.off.cpu().numpy() == S64).all() and (b.status.cpu().numpy() == S8).all()
            else:
                assert (b.o_ver.cpu().numpy() == S8).all() and (b.ev.cpu().numpy() == S64).all()
            sessions, ring, heads = b.result()
            assert ring.tobytes() == case.ring.tobytes() and heads.tobytes() == case.heads.tobytes() and sessions.tobytes() == case.sessions.tobytes()


# ---- the lattice: C x Qc x group width ------------------------------------------------------------

def run_lattice(T, h, c, qc, g):
    """The rounds of tests/pmqueue_cases.py's lattice at one shape, sized around the group width g: every
    call through all three device forms against the restatement and the host's bytes; the host's tables
    carry the world on."""
    from tests.test_pmqueue_cpu import put, take
    lat = C.Lattice(c, qc)
    for kind, case in lat.rounds(g):
        if kind == "put":
            check_put_everywhere(T, h, case)
            lat.advance(kind, case, *put(T, case)[1:])
            continue
        for cap in ("case", case.room)[case.cap_out == case.room:]:  # the short round is repeated with room
            check_take_everywhere(T, h, case, cap_out=cap)
            lat.advance(kind, case, *take(T, case, True, cap)[1:], cap)
    assert lat.flags["take"] & R.F_OUTPUT_FULL and lat.events["evictions"] > 0
    return lat


@pytest.mark.parametrize("group", [4, 16, 64])
@pytest.mark.parametrize("c,qc", C.LATTICE_SHAPES, ids=["c%d_q%d" % s for s in C.LATTICE_SHAPES])
def test_lattice(T, c, qc, group):
    """129 sessions (a last tile of one group at every width), inboxes of 0, 1, G - 1, G, G + 1, 2 G + 1 and
    3 Qc deliveries, tables of fewer classes than rings, max_len up to Qc, mult with base, heads at Qc - 1,
    expired and QoS 0 entries in every ring word."""
    h = T.Pmqueue(0)
    h.set_tuning("group", group)
    run_lattice(T, h, c, qc, group)


@pytest.mark.parametrize("group", [8, 32])
@pytest.mark.parametrize("c,qc", [(1, 128), (8, 128), (5, 8)], ids=["c1_q128", "c8_q128", "c5_q8"])
def test_lattice_one_block_scan_chunk_1(T, c, qc, group):
    """One block strides every tile, the take's scan carries at every total."""
    h = T.Pmqueue(0)
    for key, value in (("max_blocks", 1), ("scan_chunk", 1), ("group", group)):
        h.set_tuning(key, value)
    run_lattice(T, h, c, qc, group)


def test_lattice_state_stays_on_the_device(T):
    """C 8, Qc 128, G 4: the six rounds (and the repeat of the short take) are enqueued on one stream; records,
    rings and heads are uploaded once and never read or written by the host in between, only the inflight
    column is stored from the host before a take (the acks).  Outputs and a device-to-device copy of the
    tables are kept per call and read at the end: a head or a ring entry the device writes in a form its
    own next call reads differently shows here, and not where every call starts from uploaded tables."""
    import torch
    from tests.test_pmqueue_cpu import put, take
    c, qc, g = 8, 128, 4
    lat = C.Lattice(c, qc)
    w, n = lat.world, lat.n
    d_tables = dev_raw(w.tables)
    d_sessions, d_ring, d_heads = (dev_raw(x, GUARD) for x in (w.sessions, w.ring, w.heads))
    d_inflight = d_sessions[:n * 4].view(torch.int32).view(n, 8)[:, 0]
    h = T.Pmqueue(0)
    h.set_tuning("group", g)
    h.reserve(C.REF_BASE, n + 1)
    stream = torch.cuda.Stream(device=DEV)
    calls = []
    for kind, case in lat.rounds(g):
        for cap in ("case",) if kind == "put" else ("case", case.room)[case.cap_out == case.room:]:
            b = PutBatch(T, case) if kind == "put" else TakeBatch(T, case, cap_out=cap)
            for name, t in (("tables", d_tables), ("sessions", d_sessions), ("ring", d_ring), ("heads", d_heads)):
                setattr(b.args, name, t.data_ptr())
            inflight = dev(case.sessions["inflight"], np.uint32)
            stream.wait_stream(torch.cuda.current_stream())  # the inputs were filled there
            with torch.cuda.stream(stream):
                if kind == "put":
                    h.put_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
                else:
                    d_inflight.copy_(inflight)
                    h.take_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
                after = [x.clone() for x in (d_sessions, d_ring, d_heads)]  # device to device, on the stream
            want = put(T, case) if kind == "put" else take(T, case, True, cap)
            calls.append((kind, case, cap, b, inflight, after, want))
            lat.advance(kind, case, *want[1:], *(() if kind == "put" else (cap,)))
    stream.synchronize()
    # ---- only now the host reads
    fulls = 0
    for kind, case, cap, b, _, after, (want, sessions, ring, heads) in calls:
        got = b.outputs(T)
        d_s, d_r, d_h = back(after[0], w.sessions, "the records"), back(after[1], w.ring, "the rings"), back(after[2], w.heads, "the heads")
        if kind == "put":
            C.check_put(case.reference(), got, case, d_s, d_r, d_h)
        else:
            C.check_take(case.reference(cap), got, case, d_s, d_r, d_h)
            fulls += bool(got.summary["flags"] & R.F_OUTPUT_FULL)
        same(got, want)
        assert d_s.tobytes() == sessions.tobytes() and d_r.tobytes() == ring.tobytes() and d_h.tobytes() == heads.tobytes(), case.name
    assert len(calls) == 7 and fulls == 1


# ---- the cycle ----------------------------------------------------------------------------------

def test_cycle_three_rounds_on_one_stream_with_no_host_read(T):
    """300 sessions of three tables with windows of 2 to 4, mixed QoS, mq_max 0 in every record.  A round is
    window (update_table) -> ack record -> retry stamp -> PUT, then ack run (update_table) -> stamp -> TAKE
    (update_table) -> ack record fed with the take's outputs as they are -> stamp.  All three rounds are
    enqueued on one stream before anything is read; the tables after each round are copied aside on the
    stream.  The sequential model runs the restatements of the four stages in the same order (the literal
    list model of tests/pmqueue_ref.py for this one, a model a session kept across the calls); it also
    chooses the acks (packet ids that are inflight in the model)."""
    import types

    import torch
    from emqx_amd import ack as A
    from emqx_amd import retry as RT
    from emqx_amd import window as W
    from tests import ack_ref as AR
    from tests import mqueue_cases as MC
    from tests import retry_ref as RR
    from tests import window_ref as WR
    from tests.ack_cases import rows_of
    rng = np.random.default_rng(11)
    n, w, c, qc, rounds, t0 = 300, 8, 4, 8, 3, MC.NOW
    flags = rng.choice([MC.CONN, MC.CONN, MC.CONN, MC.CONN, MC.PRESENT | MC.STORE_QOS0, MC.PRESENT, MC.CONN | MC.PASS, 0], size=n)
    table = W.pack_sessions(n, inflight_max=rng.integers(2, 5, size=n), mq_max=0, flags=flags)
    world = C.World([C.T_TWO, C.T_THREE, C.T_NEG], n, c, qc, table=np.arange(n) % 3)
    tables, ring, heads = world.tables, world.ring, world.heads
    slots, stamps = A.empty_slots(n, w), RT.empty_stamps(n, w)
    ref_limit = 8192
    deadlines = np.where(rng.random(ref_limit) < 0.15, t0 + rng.integers(0, 60, size=ref_limit), 0xFFFFFFFFFFFFFFFF).astype(np.uint64)
    # the model's state
    recs = [{f: int(table[f][i]) for f in WR.FIELDS} for i in range(n)]
    m_rows, m_stamps = rows_of(slots), stamps.tolist()
    models = {}
    # the device's state and handles
    d_table, d_slots, d_stamps, d_ring, d_heads = (dev_raw(x) for x in (table, slots, stamps, ring, heads))
    d_tables, d_dead = dev_raw(tables), dev(deadlines, np.uint64)
    win, ack, rt, pq = W.Window(0), A.Ack(0), RT.Retry(0), T.Pmqueue(0)
    cap_in = 8 * n
    win.reserve(cap_in, n)
    ack.reserve(max(cap_in, (n // 2) * c * qc), n, w)  # (the second record call takes the take's capacity)
    rt.reserve(n, w)
    pq.reserve(cap_in, n)
    z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=DEV)  # noqa: E731
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    s = stream.cuda_stream
    expect, outs, keep, next_ref = [], [], [], 0
    for r in range(rounds):
        now = t0 + 20 * r
        subs = [int(x) for x in rng.permutation(n)[: n * 2 // 3]]
        sizes = rng.choice([0, 1, 2, 4, 7], size=len(subs), p=[0.1, 0.25, 0.3, 0.25, 0.1])
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        total = int(off[-1])
        opts = rng.choice([0, 1, 2, 0x11, 0x42], size=total, p=[0.25, 0.4, 0.25, 0.05, 0.05]).astype(np.uint8)
        refs = (next_ref + np.arange(total)).astype(np.uint32)
        next_ref += total
        cls = rng.integers(0, 5, size=(max(total, 1), 3)).astype(np.uint8)
        x_win = WR.run(subs, off, opts, recs, update_table=True)
        x_rec = AR.record(subs, off, opts, x_win["verdicts"], x_win["pkt_ids"], refs, m_rows)
        x_st1 = RR.stamp(subs, m_rows, m_stamps, now)
        x_put = R.put_reference(types.SimpleNamespace(
            subs=np.array(subs, np.uint32), offsets=off, opts=opts, verdicts=np.array(x_win["verdicts"], np.uint8), refs=refs,
            src=np.arange(total, dtype=np.uint32), msg_class=cls[:total], tables=tables, sessions=MC.np_sessions(recs), ring=ring, heads=heads),
            models=models)
        for sub, (mq, _, after) in x_put["models"].items():
            models[sub] = mq
            recs[sub]["mq_len"], recs[sub]["dropped"] = mq.len, after
        # the acks: of every second session, the entries that are inflight in the model
        a_subs, a_off, kinds, ids = [], [0], [], []
        for sub in (int(x) for x in rng.permutation(n)[: n // 2]):
            mine = [(e[0], e[1], e[2]) for e in m_rows[sub] if e[1] != AR.EMPTY and rng.random() < 0.7]
            for pkt_id, phase, qos in mine:
                kinds.append(AR.PUBCOMP if phase == AR.PUBREL_AWAIT else AR.PUBREC if qos == 2 and rng.random() < 0.5 else AR.PUBACK)
                ids.append(pkt_id)
            a_subs.append(sub)
            a_off.append(len(ids))
        acks = A.pack_acks(kinds, ids)
        ma = len(a_subs)
        x_run = AR.run(a_subs, a_off, acks, recs, m_rows, update_table=True)
        x_st2 = RR.stamp(a_subs, m_rows, m_stamps, now + 5)
        x_take = R.take_reference(types.SimpleNamespace(subs=np.array(a_subs, np.uint32), tables=tables, sessions=MC.np_sessions(recs), ring=ring,
                                                        heads=heads, now=now + 5, deadlines=deadlines), ma * c * qc, models=models)
        for sub, (mq, _, extra) in x_take["models"].items():
            models[sub] = mq
            recs[sub].update(extra)
            recs[sub]["mq_len"] = mq.len
        x_rec2 = AR.record(a_subs, x_take["offsets"], x_take["opts"], x_take["verdicts"], x_take["pkt_ids"], x_take["refs"], m_rows)
        x_st3 = RR.stamp(a_subs, m_rows, m_stamps, now + 5)
        expect.append(dict(win=x_win, rec=x_rec, st1=x_st1, put=x_put, run=x_run, st2=x_st2, take=x_take, rec2=x_rec2, st3=x_st3,
                           recs=[dict(x) for x in recs], rows=[[list(e) for e in row] for row in m_rows],
                           stamps=[list(x) for x in m_stamps], queues={sub: R.logical(mq, tables[sub % 3]) for sub, mq in models.items()},
                           total=total, m=len(subs), ma=ma))
        cap_t = ma * c * qc
        b = dict(subs=dev(subs, np.uint32), off=dev(off, np.uint64), opts=dev(opts, np.uint8), refs=dev(refs, np.uint32),
                 src=dev(np.arange(total), np.uint32), cls=dev(cls.reshape(-1), np.uint8),
                 ver=z(total, torch.uint8), ids=z(total, torch.int16), orecs=z(4 * len(subs), torch.int64), wcnt=z(4 * len(subs), torch.int32),
                 unrec=z(len(subs), torch.int32), o_ver=z(total, torch.uint8), o_cls=z(total, torch.uint8), ev=z(total, torch.int64),
                 cnt=z(8 * len(subs), torch.int32),
                 a_subs=dev(a_subs, np.uint32), a_off=dev(a_off, np.uint64), acks=dev(acks, np.uint32), aver=z(len(ids), torch.uint8),
                 arefs=z(len(ids), torch.int32), acnt=z(4 * ma, torch.int32),
                 t_off=z(ma + 1, torch.int64), t_opts=z(cap_t, torch.uint8), t_ver=z(cap_t, torch.uint8), t_cls=z(cap_t, torch.uint8),
                 t_ids=z(cap_t, torch.int16), t_refs=z(cap_t, torch.int32), t_status=z(ma, torch.uint8), t_cnt=z(4 * ma, torch.int32),
                 unrec2=z(ma, torch.int32), sums=[z(8, torch.int64) for _ in range(9)])
        keep.append(b)
        m = len(subs)
        P = lambda name: b[name].data_ptr()  # noqa: E731
        sm = [t.data_ptr() for t in b["sums"]]
        with torch.cuda.stream(stream):
            win.run_device_async(W.Window.batch(P("subs"), P("off"), P("opts"), m, total, m, d_table.data_ptr(), n, P("ver"), P("ids"),
                                                P("orecs"), P("wcnt"), update_table=True), sm[0], stream=s)
            ack.record_device_async(A.Ack.record_args(P("subs"), P("off"), P("opts"), m, total, m, P("ver"), P("ids"), d_slots.data_ptr(),
                                                      w, n, P("unrec"), d_refs=P("refs")), sm[1], stream=s)
            rt.stamp_device_async(RT.Retry.stamp_args(P("subs"), m, m, d_slots.data_ptr(), d_stamps.data_ptr(), w, n, now), sm[2], stream=s)
            pq.put_device_async(T.Pmqueue.put_args(
                inbox_subs=P("subs"), inbox_offsets=P("off"), box_opts=P("opts"), n_boxes=0, m=m, cap_in=total, cap_boxes=m, verdicts=P("ver"),
                refs=P("refs"), box_src=P("src"), msg_class=P("cls"), n_msgs=total, tables=d_tables.data_ptr(), n_tables=3,
                sessions=d_table.data_ptr(), sub_limit=n, update_table=1, ring=d_ring.data_ptr(), heads=d_heads.data_ptr(), c=c, qc=qc,
                out_verdicts=P("o_ver"), out_class=P("o_cls"), out_evicted=P("ev"), out_counts=P("cnt")), sm[3], stream=s)
            ack.run_device_async(A.Ack.run_args(P("a_subs"), P("a_off"), P("acks"), ma, len(ids), ma, d_table.data_ptr(), n,
                                                d_slots.data_ptr(), w, P("aver"), P("arefs"), P("acnt"), update_table=True), sm[4], stream=s)
            rt.stamp_device_async(RT.Retry.stamp_args(P("a_subs"), ma, ma, d_slots.data_ptr(), d_stamps.data_ptr(), w, n, now + 5), sm[5],
                                  stream=s)
            pq.take_device_async(T.Pmqueue.take_args(
                subs=P("a_subs"), n_boxes=0, m=ma, cap_boxes=ma, sessions=d_table.data_ptr(), sub_limit=n, update_table=1,
                tables=d_tables.data_ptr(), n_tables=3, ring=d_ring.data_ptr(), heads=d_heads.data_ptr(), c=c, qc=qc, now_ms=now + 5,
                deadlines=d_dead.data_ptr(), ref_limit=ref_limit, cap_out=cap_t, out_offsets=P("t_off"), out_opts=P("t_opts"),
                out_verdicts=P("t_ver"), out_pkt_ids=P("t_ids"), out_refs=P("t_refs"), out_class=P("t_cls"), out_status=P("t_status"),
                out_counts=P("t_cnt")), sm[6], stream=s)
            # the take's outputs as they are: offsets, opts, verdicts, ids and refs of a record call
            ack.record_device_async(A.Ack.record_args(P("a_subs"), P("t_off"), P("t_opts"), ma, cap_t, ma, P("t_ver"), P("t_ids"),
                                                      d_slots.data_ptr(), w, n, P("unrec2"), d_refs=P("t_refs")), sm[7], stream=s)
            rt.stamp_device_async(RT.Retry.stamp_args(P("a_subs"), ma, ma, d_slots.data_ptr(), d_stamps.data_ptr(), w, n, now + 5), sm[8],
                                  stream=s)
            outs.append([x.clone() for x in (d_table, d_slots, d_stamps, d_ring, d_heads)])  # device to device, on the stream
    stream.synchronize()
    # ---- only now the host reads
    u64 = lambda x: x.cpu().numpy().view(np.uint64).tolist()  # noqa: E731
    took = evicted = 0
    for r in range(rounds):
        e, b = expect[r], keep[r]
        sums = [u64(x) for x in b["sums"]]
        total, m, ma = e["total"], e["m"], e["ma"]
        assert sums[0] == e["win"]["summary"] and b["ver"].cpu().numpy()[:total].tolist() == e["win"]["verdicts"]
        assert b["ids"].cpu().numpy().view(np.uint16)[:total].tolist() == e["win"]["pkt_ids"]
        assert sums[1] == e["rec"]["summary"] and b["unrec"].cpu().numpy()[:m].tolist() == e["rec"]["unrecorded"]
        assert sums[2] == e["st1"] and sums[5] == e["st2"] and sums[8] == e["st3"]
        x = e["put"]
        evicted += x["summary"][4]
        assert sums[3] == x["summary"] and b["o_ver"].cpu().numpy()[:total].tolist() == x["verdicts"]
        assert b["o_cls"].cpu().numpy()[:total].tolist() == x["classes"]
        ev = np.frombuffer(b["ev"].cpu().numpy()[:total].tobytes(), dtype=T.ENTRY)
        assert [[int(v["ref"]), int(v["opts"])] for v in ev] == x["evicted"]
        assert b["cnt"].cpu().numpy().view(np.uint32)[:8 * m].reshape(-1, 8).tolist() == x["counts"]
        assert sums[4] == e["run"]["summary"] and b["aver"].cpu().numpy()[:len(e["run"]["verdicts"])].tolist() == e["run"]["verdicts"]
        assert b["acnt"].cpu().numpy().view(np.uint32)[:4 * ma].reshape(-1, 4).tolist() == e["run"]["counts"]
        x = e["take"]
        k = x["offsets"][-1]
        took += k
        assert sums[6] == x["summary"] and u64(b["t_off"])[:ma + 1] == x["offsets"]
        assert b["t_opts"].cpu().numpy()[:k].tolist() == x["opts"] and b["t_ver"].cpu().numpy()[:k].tolist() == x["verdicts"]
        assert b["t_ids"].cpu().numpy().view(np.uint16)[:k].tolist() == x["pkt_ids"] and b["t_cls"].cpu().numpy()[:k].tolist() == x["classes"]
        assert b["t_refs"].cpu().numpy().view(np.uint32)[:k].tolist() == x["refs"]
        assert b["t_status"].cpu().numpy()[:ma].tolist() == x["status"]
        assert b["t_cnt"].cpu().numpy().view(np.uint32)[:4 * ma].reshape(-1, 4).tolist() == x["counts"]
        assert sums[7] == e["rec2"]["summary"] and b["unrec2"].cpu().numpy()[:ma].tolist() == e["rec2"]["unrecorded"]
        assert not x["summary"][0] & R.F_OUTPUT_FULL and e["rec2"]["summary"][5] == 0, "the loop is closed: every send found its slot"
        g_table, g_slots, g_stamps, g_ring, g_heads = outs[r]
        got_table = np.frombuffer(g_table.cpu().numpy().tobytes(), dtype=W.SESSION)
        assert [{f: int(got_table[f][i]) for f in WR.FIELDS} for i in range(n)] == e["recs"]
        assert rows_of(np.frombuffer(g_slots.cpu().numpy().tobytes(), dtype=A.SLOT).reshape(n, w)) == e["rows"]
        assert g_stamps.cpu().numpy().view(np.uint64).reshape(n, w).tolist() == e["stamps"]
        got_ring, got_heads = back(g_ring, ring, "the rings"), back(g_heads, heads, "the heads")
        for sub in range(n):
            want = e["queues"].get(sub)
            if want is None:
                assert got_heads[sub].tobytes() == heads[sub].tobytes() and got_ring[sub].tobytes() == ring[sub].tobytes(), sub
                continue
            assert T.order_of(got_heads, sub) == want["order"] and int(got_heads["credit"][sub]) == want["credit"], sub
            assert int(got_heads["flags"][sub]) == want["last"], sub
            for k in range(c):
                assert [(int(v["ref"]), int(v["opts"])) for v in T.queue_of(got_ring, got_heads, sub, k)] == want["queues"][k], (sub, k)
    # the rounds are not idle: items are handed out, old entries are evicted, messages expire
    assert took > 0 and evicted > 0 and sum(e["take"]["summary"][6] for e in expect) > 0
