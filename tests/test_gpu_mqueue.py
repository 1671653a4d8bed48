"""The mqueue stage on the device (include/emqx_mqueue.h): every case of both calls through the three
device entry points, with the grid at its default and capped at 1 block with a scan that carries
every tile; every output byte, the ring, the headers, the table and the summary exact against the
sequential restatement (tests/mqueue_ref.py) and identical to the host evaluator; nothing written
past the defined extents; the count read on the device; overflow and its repeat; and the cycle
window -> record -> stamp -> put -> run -> stamp -> take -> record -> stamp, three rounds on one
stream with no host read, against the restatements of all four stages."""

import os
import subprocess

import numpy as np
import pytest

from tests import mqueue_cases as C
from tests import mqueue_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S8, S16, S32, S64 = 0x5A, 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64  # sentinel elements behind every output buffer's capacity
PUT_CASES = C.put_cases()
TAKE_CASES = C.take_cases()


@pytest.fixture(scope="module")
def T():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import mqueue
    return mqueue


@pytest.fixture(scope="module", params=[(None, None), (1, 1)], ids=["default", "1_block-scan_chunk_1"])
def handle(T, request):
    """One handle a setting for the whole module: every test also reuses the scratch of the one
    before.  Capped, the one block strides over every tile and the scans carry at every total."""
    max_blocks, scan_chunk = request.param
    h = T.Mqueue(0)
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
    raw = np.frombuffer(table.tobytes() or bytes(32), dtype=np.int64)
    return torch.from_numpy(np.concatenate([raw, np.full(guard, S64, dtype=np.int64)])).to(DEV)


def filled(k, dtype):  # every byte 0x5A
    import torch
    sent = {torch.uint8: S8, torch.int16: S16, torch.int32: S32, torch.int64: S64}[dtype]
    return torch.full((k + GUARD,), sent, dtype=dtype, device=DEV)


def back(t, n, dtype, shape, what):
    """The first n int64 words of a guarded device table as a host array."""
    raw = t.cpu().numpy()
    assert (raw[n:] == S64).all(), "a write past " + what
    return np.frombuffer(raw[:n].tobytes(), dtype=dtype).reshape(shape).copy()


def ptr(t):
    return 0 if t is None else t.data_ptr()


# ---- put ----------------------------------------------------------------------------------------

class PutBatch:
    """A put case in device memory with sentinel-filled outputs and a guard behind each."""

    def __init__(self, T, case, cap_in=None, cap_boxes=None, count_on_device=False):
        import torch
        self.case = case
        self.m, self.total = case.subs.size, int(case.offsets[-1])
        self.cap_in = self.total if cap_in is None else cap_in
        self.cap_boxes = self.m if cap_boxes is None else cap_boxes
        pad = lambda a, n, dt: np.concatenate([np.asarray(a, dtype=dt), np.zeros(n - len(a), dtype=dt)])  # noqa: E731
        self.subs, self.off = dev(pad(case.subs, self.cap_boxes, np.uint32), np.uint32), dev(pad(case.offsets, self.cap_boxes + 1, np.uint64), np.uint64)
        self.opts, self.ver = dev(pad(case.opts, self.cap_in, np.uint8), np.uint8), dev(pad(case.verdicts, self.cap_in, np.uint8), np.uint8)
        self.refs = None if case.refs is None else dev(pad(case.refs, self.cap_in, np.uint32), np.uint32)
        self.sessions = None if case.sessions is None else dev_raw(case.sessions, GUARD)
        self.ring, self.heads = dev_raw(case.ring, GUARD), dev_raw(case.heads, GUARD)
        self.count = dev([self.m], np.uint64) if count_on_device else None
        self.ev, self.un, self.summary = filled(self.cap_in, torch.int64), filled(self.cap_boxes, torch.int32), filled(8, torch.int64)
        self.args = T.Mqueue.put_args(self.subs.data_ptr(), self.off.data_ptr(), self.opts.data_ptr(), 0 if count_on_device else self.m,
                                      self.cap_in, self.cap_boxes, self.ver.data_ptr(), self.ring.data_ptr(), self.heads.data_ptr(), case.q,
                                      case.ring.shape[0], self.ev.data_ptr(), self.un.data_ptr(), d_refs=ptr(self.refs),
                                      d_sessions=ptr(self.sessions), d_n_boxes=ptr(self.count))

    def result(self, T, summary=None):
        c = self.case
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.PUT_SUMMARY, s[:8].tolist()))
        ev, un = self.ev.cpu().numpy(), self.un.cpu().numpy().view(np.uint32)
        assert (ev[self.total:] == S64).all() and (un[self.m:] == S32).all(), "a write past the defined extent"
        if self.sessions is not None:
            assert back(self.sessions, 4 * c.sessions.size, C.SESSION, c.sessions.shape, "the table").tobytes() == c.sessions.tobytes()
        got = T.Put(np.frombuffer(ev[:self.total].tobytes(), dtype=T.ENTRY), un[:self.m], summary)
        n = c.ring.shape[0]
        return got, back(self.ring, n * c.q, T.ENTRY, (n, c.q), "the ring"), back(self.heads, n, T.RING, (n,), "the headers")


def put_sync(T, h, case, **kw):
    from emqx_amd import _lib
    b = PutBatch(T, case, **kw)
    try:
        summary = h.put_device(b.args)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & R.F_BAD_SUB
        summary = e.summary
    return b.result(T, summary)


def put_async(T, h, case, **kw):
    import torch
    b = PutBatch(T, case, **kw)
    h.reserve(b.cap_in, b.cap_boxes)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        h.put_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(T)


@pytest.mark.parametrize("case", PUT_CASES, ids=[c.name for c in PUT_CASES])
def test_put_cases(T, handle, case):
    """Every device entry point: exact against the restatement, identical to the host evaluator."""
    from tests.test_mqueue_cpu import put
    ref = case.reference()
    host = put(T, case)
    C.check_put(ref, *host)
    for got in (put(T, case, h=handle, fn="put"), put_sync(T, handle, case), put_async(T, handle, case),
                put_async(T, handle, case, cap_in=int(case.offsets[-1]) + 9, cap_boxes=case.subs.size + 5, count_on_device=True)):
        C.check_put(ref, *got)
        assert got[0].summary == host[0].summary and got[0].evicted.tobytes() == host[0].evicted.tobytes()
        assert [x.tobytes() for x in got[1:]] == [x.tobytes() for x in host[1:]]


# ---- take ---------------------------------------------------------------------------------------

class TakeBatch:
    def __init__(self, T, case, cap_out="case", cap_boxes=None, update_table=True, count_on_device=False):
        import torch
        self.case = case
        n = case.ring.shape[0]
        self.m = n if case.subs is None else len(case.subs)
        cap = case.cap_out if cap_out == "case" else cap_out
        self.cap_out = self.m * case.q if cap is None else cap
        self.cap_boxes = self.m if cap_boxes is None else cap_boxes
        self.subs = None if case.subs is None else dev(list(case.subs) + [0] * (self.cap_boxes - self.m), np.uint32)
        self.table, self.ring, self.heads = dev_raw(case.sessions, GUARD), dev_raw(case.ring, GUARD), dev_raw(case.heads, GUARD)
        self.deadlines = None if case.deadlines is None else dev(case.deadlines, np.uint64)
        self.count = dev([self.m], np.uint64) if count_on_device else None
        self.off, self.opts, self.ver = filled(self.cap_boxes + 1, torch.int64), filled(self.cap_out, torch.uint8), filled(self.cap_out, torch.uint8)
        self.ids, self.refs = filled(self.cap_out, torch.int16), filled(self.cap_out, torch.int32)
        self.status, self.cnt, self.summary = filled(self.cap_boxes, torch.uint8), filled(4 * self.cap_boxes, torch.int32), filled(8, torch.int64)
        self.args = T.Mqueue.take_args(ptr(self.subs), 0 if count_on_device else self.m, self.cap_boxes, self.table.data_ptr(), n,
                                       self.ring.data_ptr(), self.heads.data_ptr(), case.q, case.now, self.cap_out, self.off.data_ptr(),
                                       self.opts.data_ptr(), self.ver.data_ptr(), self.ids.data_ptr(), self.refs.data_ptr(),
                                       self.status.data_ptr(), self.cnt.data_ptr(), d_deadlines=ptr(self.deadlines),
                                       ref_limit=0 if case.deadlines is None else case.deadlines.size, update_table=update_table,
                                       d_n_boxes=ptr(self.count))

    def result(self, T, summary=None):
        c = self.case
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.TAKE_SUMMARY, s[:8].tolist()))
        refused = summary["flags"] & R.F_INPUT_REFUSED
        full = summary["flags"] & R.F_OUTPUT_FULL
        m = 0 if refused else summary["sessions"]
        k = 0 if refused or full else summary["items"]
        off, status, cnt = self.off.cpu().numpy().view(np.uint64), self.status.cpu().numpy(), self.cnt.cpu().numpy().view(np.uint32)
        opts, ver = self.opts.cpu().numpy(), self.ver.cpu().numpy()
        ids, refs = self.ids.cpu().numpy().view(np.uint16), self.refs.cpu().numpy().view(np.uint32)
        assert (off[(0 if refused else m + 1):] == S64).all() and (status[m:] == S8).all() and (cnt[4 * m:] == S32).all()
        assert (opts[k:] == S8).all() and (ver[k:] == S8).all() and (ids[k:] == S16).all() and (refs[k:] == S32).all()
        got = T.Taken(off[:0 if refused else m + 1], opts[:k], ver[:k], ids[:k], refs[:k], status[:m], cnt[:4 * m].reshape(-1, 4), summary)
        n = c.ring.shape[0]
        return (got, back(self.table, 4 * n, C.SESSION, (n,), "the table"), back(self.heads, n, T.RING, (n,), "the headers"),
                back(self.ring, n * c.q, T.ENTRY, (n, c.q), "the ring"))


def take_sync(T, h, case, **kw):
    from emqx_amd import _lib
    b = TakeBatch(T, case, **kw)
    try:
        summary = h.take_device(b.args)
    except _lib.EngineError as e:
        assert e.code == (-4 if e.summary["flags"] & R.F_OUTPUT_FULL else -1)
        assert e.summary["flags"] & (R.F_BAD_SUB | R.F_OUTPUT_FULL)
        summary = e.summary
    return b.result(T, summary)


def take_async(T, h, case, **kw):
    import torch
    b = TakeBatch(T, case, **kw)
    h.reserve(0, b.cap_boxes)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        h.take_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(T)


def same_taken(x, y):
    assert x.summary == y.summary
    for a, b in zip(x[:-1], y[:-1]):
        assert a.tobytes() == b.tobytes()


def all_take_forms(T, h, case, update_table=True, cap_out="case"):
    from tests.test_mqueue_cpu import take
    cap = case.cap_out if cap_out == "case" else cap_out
    ref = case.reference(update_table, cap)
    host = take(T, case, update_table, cap_out)
    C.check_take(ref, *host, case)
    kw = dict(update_table=update_table, cap_out=cap_out)
    m = case.ring.shape[0] if case.subs is None else len(case.subs)
    more = dict(kw, cap_out=(m * case.q if cap is None else cap))
    for got in (take(T, case, update_table, cap_out, h=h, fn="take"), take_sync(T, h, case, **kw), take_async(T, h, case, **kw),
                take_async(T, h, case, cap_boxes=m + 7, count_on_device=True, **more)):
        C.check_take(ref, *got, case)
        same_taken(got[0], host[0])
        assert [x.tobytes() for x in got[1:]] == [x.tobytes() for x in host[1:]]
    return ref


@pytest.mark.parametrize("case", TAKE_CASES, ids=[c.name for c in TAKE_CASES])
def test_take_cases(T, handle, case):
    if case.subs is None:  # (the whole table: the count on the device may not exceed sub_limit, so no spare boxes)
        from tests.test_mqueue_cpu import take
        ref, host = case.reference(), take(T, case)
        for got in (take(T, case, h=handle, fn="take"), take_sync(T, handle, case), take_async(T, handle, case),
                    take_async(T, handle, case, count_on_device=True)):
            C.check_take(ref, *got, case)
            same_taken(got[0], host[0])
        return
    all_take_forms(T, handle, case)


@pytest.mark.parametrize("name", ["expired_between_counting", "random_q64"])
def test_without_update_table_nothing_is_touched(T, handle, name):
    case = next(c for c in TAKE_CASES if c.name == name)
    all_take_forms(T, handle, case, update_table=False)
    for run in (take_sync, take_async):
        got = run(T, handle, case, update_table=False)
        assert got[1].tobytes() == case.sessions.tobytes() and got[2].tobytes() == case.heads.tobytes()


def test_overflow_changes_nothing_and_the_repeat_succeeds(T, handle):
    import torch
    case = C.overflow_case()
    ref = all_take_forms(T, handle, case)
    assert ref[0]["summary"][0] == R.F_OUTPUT_FULL and ref[0]["summary"][3] == 5
    b = TakeBatch(T, case)
    handle.reserve(0, b.cap_boxes)
    handle.take_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    got, table, heads, ring = b.result(T)
    assert got.summary["flags"] == R.F_OUTPUT_FULL and got.summary["items"] == 5 and got.opts.size == 0
    assert (table.tobytes(), heads.tobytes()) == (case.sessions.tobytes(), case.heads.tobytes())
    room = [filled(5, dt) for dt in (torch.uint8, torch.uint8, torch.int16, torch.int32)]
    b.opts, b.ver, b.ids, b.refs = room
    b.args.out_opts, b.args.out_verdicts, b.args.out_pkt_ids, b.args.out_refs = [t.data_ptr() for t in room]
    b.args.cap_out = b.cap_out = 5
    handle.take_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    C.check_take(case.reference(True, 5), *b.result(T), case)


def test_async_needs_the_scratch_reserved(T):
    from emqx_amd import _lib
    h = T.Mqueue(0)
    p, t = PutBatch(T, PUT_CASES[0]), TakeBatch(T, TAKE_CASES[0])
    for call, b in ((h.put_device_async, p), (h.take_device_async, t)):
        with pytest.raises(_lib.EngineError) as e:
            call(b.args, b.summary.data_ptr())
        assert e.value.code == -4  # EMQX_EOVERFLOW, nothing enqueued
    import torch
    torch.cuda.synchronize()
    assert (p.summary.cpu().numpy() == S64).all() and (t.summary.cpu().numpy() == S64).all()
    assert h.stats()["scratch_bytes"] == 0
    h.reserve(10, 10)
    assert h.stats()["scratch_bytes"] > 0 and h.stats()["cap_in"] == 10


def test_misaligned_tables_are_refused(T, handle):
    """One pointer at a time is off by half of what the device forms require of it (ring 16, heads 8,
    sessions 16, out_counts 16, out_offsets 8): EMQX_EINVAL, nothing is enqueued, every byte stays."""
    from emqx_amd import _lib
    put = next(c for c in PUT_CASES if c.name == "head_wraps")
    take = next(c for c in TAKE_CASES if c.name == "budget_ends_at_last")
    n = put.ring.shape[0]
    for field, by in (("ring", 8), ("heads", 4), ("sessions", 8)):
        b = PutBatch(T, put)
        assert getattr(b.args, field)
        setattr(b.args, field, getattr(b.args, field) + by)
        with pytest.raises(_lib.EngineError) as e:
            handle.put_device(b.args)
        assert e.value.code == -1
        assert (b.ev.cpu().numpy() == S64).all() and (b.un.cpu().numpy().view(np.uint32) == S32).all()
        assert back(b.ring, n * put.q, T.ENTRY, (n, put.q), "the ring").tobytes() == put.ring.tobytes()
        assert back(b.heads, n, T.RING, (n,), "the headers").tobytes() == put.heads.tobytes()
        assert back(b.sessions, 4 * put.sessions.size, C.SESSION, put.sessions.shape, "the table").tobytes() == put.sessions.tobytes()
    n = take.ring.shape[0]
    for field, by in (("ring", 8), ("heads", 4), ("sessions", 8), ("out_counts", 8), ("out_offsets", 4)):
        b = TakeBatch(T, take)
        assert getattr(b.args, field)
        setattr(b.args, field, getattr(b.args, field) + by)
        with pytest.raises(_lib.EngineError) as e:
            handle.take_device(b.args)
        assert e.value.code == -1
        assert (b.off.cpu().numpy() == S64).all() and (b.cnt.cpu().numpy().view(np.uint32) == S32).all() and (b.status.cpu().numpy() == S8).all()
        assert back(b.ring, n * take.q, T.ENTRY, (n, take.q), "the ring").tobytes() == take.ring.tobytes()
        assert back(b.heads, n, T.RING, (n,), "the headers").tobytes() == take.heads.tobytes()
        assert back(b.table, 4 * n, C.SESSION, (n,), "the table").tobytes() == take.sessions.tobytes()


# ---- the cycle ----------------------------------------------------------------------------------

def test_cycle_three_rounds_on_one_stream_with_no_host_read(T):
    """About 300 sessions with windows of 2 to 4 and queues of 4 to 8, mixed QoS.  A round is
    window (update_table) -> ack record -> retry stamp -> mqueue put, then ack run (update_table) ->
    stamp -> TAKE (update_table) -> ack record fed with the take's outputs -> stamp.  All three
    rounds are enqueued on one stream before anything is read; the tables after each round are
    copied aside on the stream.  The sequential model runs the restatements of the four stages in
    the same order; it also chooses the acks (packet ids that are inflight in the model)."""
    import torch
    from emqx_amd import ack as A
    from emqx_amd import retry as RT
    from emqx_amd import window as W
    from tests import ack_ref as AR
    from tests import retry_ref as RR
    from tests import window_ref as WR
    from tests.ack_cases import rows_of
    rng = np.random.default_rng(11)
    n, w, q, rounds, t0 = 300, 8, 8, 3, C.NOW
    flags = rng.choice([C.CONN, C.CONN, C.CONN, C.CONN, C.PRESENT | C.STORE_QOS0, C.PRESENT, C.CONN | C.PASS, 0], size=n)
    table = W.pack_sessions(n, inflight_max=rng.integers(2, 5, size=n), mq_max=rng.integers(4, 9, size=n), flags=flags)
    slots, stamps, ring, heads = A.empty_slots(n, w), RT.empty_stamps(n, w), T.empty_ring(n, q), T.empty_heads(n)
    ref_limit = 8192
    deadlines = np.where(rng.random(ref_limit) < 0.15, t0 + rng.integers(0, 60, size=ref_limit), R.NO_EXPIRY).astype(np.uint64)
    # the model's state
    recs = [{f: int(table[f][i]) for f in WR.FIELDS} for i in range(n)]
    m_rows, m_stamps = rows_of(slots), stamps.tolist()
    m_ring, m_heads = C.lists_of(ring, heads)
    # the device's state and handles
    d_table, d_slots, d_stamps, d_ring, d_heads = (dev_raw(x) for x in (table, slots, stamps, ring, heads))
    d_dead = dev(deadlines, np.uint64)
    win, ack, rt, mq = W.Window(0), A.Ack(0), RT.Retry(0), T.Mqueue(0)
    cap_in = 8 * n
    win.reserve(cap_in, n)
    ack.reserve(cap_in, n, w)
    rt.reserve(n, w)
    mq.reserve(cap_in, n)
    z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=DEV)  # noqa: E731
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    s = stream.cuda_stream
    expect, outs, keep, next_ref = [], [], [], 0
    for r in range(rounds):
        now = t0 + 20 * r
        # ---- the inputs of the round's first half, and the model through it
        subs = [int(x) for x in rng.permutation(n)[: n * 2 // 3]]
        sizes = rng.choice([0, 1, 2, 4, 7], size=len(subs), p=[0.1, 0.25, 0.3, 0.25, 0.1])
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        total = int(off[-1])
        opts = rng.choice([0, 1, 2, 0x11, 0x42], size=total, p=[0.25, 0.4, 0.25, 0.05, 0.05]).astype(np.uint8)
        refs = (next_ref + np.arange(total)).astype(np.uint32)
        next_ref += total
        x_win = WR.run(subs, off, opts, recs, update_table=True)
        x_rec = AR.record(subs, off, opts, x_win["verdicts"], x_win["pkt_ids"], refs, m_rows)
        x_st1 = RR.stamp(subs, m_rows, m_stamps, now)
        x_put = R.put(subs, off, opts, x_win["verdicts"], refs, m_ring, m_heads, q, sessions=recs)
        # the acks: of every third session, the entries that are inflight in the model
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
        x_take = R.take(a_subs, recs, m_ring, m_heads, q, now=now + 5, deadlines=deadlines, cap_out=ma * q, update_table=True)
        x_rec2 = AR.record(a_subs, x_take["offsets"], x_take["opts"], x_take["verdicts"], x_take["pkt_ids"], x_take["refs"], m_rows)
        x_st3 = RR.stamp(a_subs, m_rows, m_stamps, now + 5)
        expect.append(dict(win=x_win, rec=x_rec, st1=x_st1, put=x_put, run=x_run, st2=x_st2, take=x_take, rec2=x_rec2, st3=x_st3,
                           recs=[dict(x) for x in recs], rows=[[list(e) for e in row] for row in m_rows],
                           stamps=[list(x) for x in m_stamps], ring=[[list(e) for e in row] for row in m_ring],
                           heads=[list(x) for x in m_heads], total=total, m=len(subs), ma=ma))
        # ---- the same on the device: buffers, argument blocks, nine calls
        b = dict(subs=dev(subs, np.uint32), off=dev(off, np.uint64), opts=dev(opts, np.uint8), refs=dev(refs, np.uint32),
                 ver=z(total, torch.uint8), ids=z(total, torch.int16), orecs=z(4 * len(subs), torch.int64), wcnt=z(4 * len(subs), torch.int32),
                 unrec=z(len(subs), torch.int32), ev=z(total, torch.int64), unst=z(len(subs), torch.int32),
                 a_subs=dev(a_subs, np.uint32), a_off=dev(a_off, np.uint64), acks=dev(acks, np.uint32), aver=z(len(ids), torch.uint8),
                 arefs=z(len(ids), torch.int32), acnt=z(4 * ma, torch.int32),
                 t_off=z(ma + 1, torch.int64), t_opts=z(ma * q, torch.uint8), t_ver=z(ma * q, torch.uint8), t_ids=z(ma * q, torch.int16),
                 t_refs=z(ma * q, torch.int32), t_status=z(ma, torch.uint8), t_cnt=z(4 * ma, torch.int32), unrec2=z(ma, torch.int32),
                 sums=[z(8, torch.int64) for _ in range(9)])
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
            mq.put_device_async(T.Mqueue.put_args(P("subs"), P("off"), P("opts"), m, total, m, P("ver"), d_ring.data_ptr(),
                                                  d_heads.data_ptr(), q, n, P("ev"), P("unst"), d_refs=P("refs"),
                                                  d_sessions=d_table.data_ptr()), sm[3], stream=s)
            ack.run_device_async(A.Ack.run_args(P("a_subs"), P("a_off"), P("acks"), ma, len(ids), ma, d_table.data_ptr(), n,
                                                d_slots.data_ptr(), w, P("aver"), P("arefs"), P("acnt"), update_table=True), sm[4], stream=s)
            rt.stamp_device_async(RT.Retry.stamp_args(P("a_subs"), ma, ma, d_slots.data_ptr(), d_stamps.data_ptr(), w, n, now + 5), sm[5],
                                  stream=s)
            mq.take_device_async(T.Mqueue.take_args(P("a_subs"), ma, ma, d_table.data_ptr(), n, d_ring.data_ptr(), d_heads.data_ptr(), q,
                                                    now + 5, ma * q, P("t_off"), P("t_opts"), P("t_ver"), P("t_ids"), P("t_refs"),
                                                    P("t_status"), P("t_cnt"), d_deadlines=d_dead.data_ptr(), ref_limit=ref_limit,
                                                    update_table=True), sm[6], stream=s)
            # the take's outputs as they are: offsets, opts, verdicts, ids and refs of a record call
            ack.record_device_async(A.Ack.record_args(P("a_subs"), P("t_off"), P("t_opts"), ma, ma * q, ma, P("t_ver"), P("t_ids"),
                                                      d_slots.data_ptr(), w, n, P("unrec2"), d_refs=P("t_refs")), sm[7], stream=s)
            rt.stamp_device_async(RT.Retry.stamp_args(P("a_subs"), ma, ma, d_slots.data_ptr(), d_stamps.data_ptr(), w, n, now + 5), sm[8],
                                  stream=s)
            outs.append([x.clone() for x in (d_table, d_slots, d_stamps, d_ring, d_heads)])  # device to device, on the stream
    stream.synchronize()
    # ---- only now the host reads
    u64 = lambda x: x.cpu().numpy().view(np.uint64).tolist()  # noqa: E731
    took = 0
    for r in range(rounds):
        e, b = expect[r], keep[r]
        sums = [u64(x) for x in b["sums"]]
        total, m, ma = e["total"], e["m"], e["ma"]
        assert sums[0] == e["win"]["summary"] and b["ver"].cpu().numpy()[:total].tolist() == e["win"]["verdicts"]
        assert b["ids"].cpu().numpy().view(np.uint16)[:total].tolist() == e["win"]["pkt_ids"]
        assert sums[1] == e["rec"]["summary"] and b["unrec"].cpu().numpy()[:m].tolist() == e["rec"]["unrecorded"]
        assert sums[2] == e["st1"] and sums[5] == e["st2"] and sums[8] == e["st3"]
        assert sums[3] == e["put"]["summary"] and b["unst"].cpu().numpy()[:m].tolist() == e["put"]["unstored"]
        ev = np.frombuffer(b["ev"].cpu().numpy()[:total].tobytes(), dtype=T.ENTRY)
        assert [[int(x["ref"]), int(x["opts"])] for x in ev] == e["put"]["evicted"]
        assert sums[4] == e["run"]["summary"] and b["aver"].cpu().numpy()[:len(e["run"]["verdicts"])].tolist() == e["run"]["verdicts"]
        assert b["acnt"].cpu().numpy().view(np.uint32)[:4 * ma].reshape(-1, 4).tolist() == e["run"]["counts"]
        x = e["take"]
        k = x["offsets"][-1]
        took += k
        assert sums[6] == x["summary"] and u64(b["t_off"])[:ma + 1] == x["offsets"]
        assert b["t_opts"].cpu().numpy()[:k].tolist() == x["opts"] and b["t_ver"].cpu().numpy()[:k].tolist() == x["verdicts"]
        assert b["t_ids"].cpu().numpy().view(np.uint16)[:k].tolist() == x["pkt_ids"]
        assert b["t_refs"].cpu().numpy().view(np.uint32)[:k].tolist() == x["refs"]
        assert b["t_status"].cpu().numpy()[:ma].tolist() == x["status"]
        assert b["t_cnt"].cpu().numpy().view(np.uint32)[:4 * ma].reshape(-1, 4).tolist() == x["counts"]
        assert sums[7] == e["rec2"]["summary"] and b["unrec2"].cpu().numpy()[:ma].tolist() == e["rec2"]["unrecorded"]
        assert not x["summary"][0] & (R.F_LEN_MISMATCH | R.F_OUTPUT_FULL) and e["rec2"]["summary"][5] == 0, "the loop is closed"
        g_table, g_slots, g_stamps, g_ring, g_heads = outs[r]
        got_table = np.frombuffer(g_table.cpu().numpy().tobytes(), dtype=W.SESSION)
        assert [{f: int(got_table[f][i]) for f in WR.FIELDS} for i in range(n)] == e["recs"]
        assert rows_of(np.frombuffer(g_slots.cpu().numpy().tobytes(), dtype=A.SLOT).reshape(n, w)) == e["rows"]
        assert g_stamps.cpu().numpy().view(np.uint64).reshape(n, w).tolist() == e["stamps"]
        got_ring = np.frombuffer(g_ring.cpu().numpy().tobytes(), dtype=T.ENTRY).reshape(n, q)
        got_heads = np.frombuffer(g_heads.cpu().numpy().tobytes(), dtype=T.RING)
        assert C.lists_of(got_ring, got_heads) == (e["ring"], e["heads"])
        # every connected session's window and queue agree with its record
        for i in range(n):
            if e["recs"][i]["flags"] & 1 and not e["recs"][i]["flags"] & 8:
                assert e["recs"][i]["mq_len"] == e["heads"][i][1]
                assert e["recs"][i]["inflight"] == sum(1 for slot in e["rows"][i] if slot[1] != AR.EMPTY)
    assert took > 100 and any(e["take"]["summary"][6] for e in expect) and any(e["put"]["summary"][4] for e in expect)
