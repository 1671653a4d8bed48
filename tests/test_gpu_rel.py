"""The rel stage on the device (include/emqx_rel.h): every case of both calls through the three
device entry points on two handles (the defaults; max_blocks 1 and scan_chunk 1, where one block
strides over every tile and group and the scan carries at every tile), every output byte, the rows
and the summary exact against the sequential restatement (tests/rel_ref.py) and identical to the
host evaluator; sessions[] unchanged; nothing written past the defined extents; the "lanes"
override at every legal value; the refusals; the chain inbox-stage grouping of raw events -> rel ->
gather -> match on one stream with no host read, three rounds with an expire call between."""

import os
import subprocess

import numpy as np
import pytest

from tests import rel_cases as C
from tests import rel_ref as R

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
    from emqx_amd import rel
    return rel


@pytest.fixture(scope="module", params=[None, (1, 1)], ids=["defaults", "1_block-scan_chunk_1"])
def handle(T, request):
    """One handle a setting for the whole module: every test also reuses the scratch of the one
    before.  With max_blocks 1 one block takes every tile and every group of sessions of a case,
    with scan_chunk 1 the scan of the tile totals carries at every tile."""
    h = T.Rel(0)
    if request.param is not None:
        h.set_tuning("max_blocks", request.param[0])
        h.set_tuning("scan_chunk", request.param[1])
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


def host_rel(t, case):
    raw = t.cpu().numpy()
    n = case.sub_limit * case.w
    assert (raw[n:] == S64).all(), "a write past the awaiting table"
    return raw[:n].view(np.uint64).reshape(case.sub_limit, case.w).copy()


def table_unchanged(t, case):
    raw = t.cpu().numpy()
    assert raw.tobytes() == dev_raw(case.table, GUARD).cpu().numpy().tobytes(), "the stage never writes sessions[]"


class RunBatch:
    """A run case in device memory with sentinel-filled outputs and a guard behind each."""

    def __init__(self, T, case, cap_in=None, cap_boxes=None, count_on_device=False):
        import torch
        self.case = case
        self.cap_in = case.total if cap_in is None else cap_in
        self.cap_boxes = case.m if cap_boxes is None else cap_boxes
        self.subs, self.off, self.ev = dev(case.subs, np.uint32), dev(case.offsets, np.uint64), dev(case.events, np.uint32)
        self.ts = None if case.ts is None else dev(case.ts, np.uint64)
        self.src = None if case.src is None else dev(case.src, np.uint32)
        self.maxes = None if case.maxes is None else dev(case.maxes, np.uint32)
        self.table, self.rel = dev_raw(case.table, GUARD), dev_raw(case.rel, GUARD)
        self.count = dev([case.m], np.uint64) if count_on_device else None
        self.ver, self.route = filled(self.cap_in, torch.uint8), filled(self.cap_in, torch.int32)
        self.cnt, self.arm = filled(4 * self.cap_boxes, torch.int32), filled(self.cap_boxes, torch.uint8)
        self.summary = filled(8, torch.int64)
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        self.args = T.Rel.run_args(self.subs.data_ptr(), self.off.data_ptr(), self.ev.data_ptr(), 0 if count_on_device else case.m,
                                   self.cap_in, self.cap_boxes, self.table.data_ptr(), case.sub_limit, self.rel.data_ptr(), case.w,
                                   self.ver.data_ptr(), self.route.data_ptr(), self.cnt.data_ptr(), self.arm.data_ptr(),
                                   max_awaiting=case.max_awaiting, d_maxes=ptr(self.maxes), now_ms=case.now_ms, d_ts=ptr(self.ts),
                                   d_src=ptr(self.src), d_n_boxes=ptr(self.count))

    def result(self, T, summary=None):
        """The outputs up to their defined extents, after checking that nothing behind them changed."""
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.RUN_SUMMARY, s[:8].tolist()))
        refused = summary["flags"] & R.F_INPUT_REFUSED
        total = 0 if refused else summary["events"]
        routed = 0 if refused else summary["routed"]
        m = 0 if refused else summary["sessions"]
        ver, route = self.ver.cpu().numpy(), self.route.cpu().numpy().view(np.uint32)
        cnt, arm = self.cnt.cpu().numpy().view(np.uint32), self.arm.cpu().numpy()
        assert (ver[total:] == S8).all() and (route[routed:] == S32).all(), "a write past the defined extent"
        assert (cnt[4 * m:] == S32).all() and (arm[m:] == S8).all(), "a write past the defined extent"
        table_unchanged(self.table, self.case)
        return T.Ran(ver[:total], route[:routed], cnt[:4 * m].reshape(-1, 4), arm[:m], summary), host_rel(self.rel, self.case)


def run_host_buffers(T, h, case):
    from emqx_amd import _lib
    table, rel = case.table.copy(), case.rel.copy()
    try:
        got = h.run(case.subs, case.offsets, case.events, table, rel, **case.host_args())
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & R.F_BAD_SUB
        got = e.partial
    assert table.tobytes() == case.table.tobytes()
    return got, rel


def run_sync(T, h, case, **kw):
    from emqx_amd import _lib
    b = RunBatch(T, case, **kw)
    try:
        summary = h.run_device(b.args)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & (R.F_BAD_SUB | R.F_INPUT_REFUSED)
        summary = e.summary
    return b.result(T, summary)


def run_async(T, h, case, **kw):
    import torch
    b = RunBatch(T, case, **kw)
    h.reserve(b.cap_in, b.cap_boxes, case.w)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        h.run_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(T)


def host_answer(T, case):
    from emqx_amd import _lib
    rel = case.rel.copy()
    try:
        got = T.Rel(T.HOST_ONLY).run_host(case.subs, case.offsets, case.events, case.table.copy(), rel, **case.host_args())
    except _lib.EngineError as e:
        got = e.partial
    return got, rel


def all_forms(T, h, case):
    """Every device entry point: exact against the restatement, identical to the host evaluator."""
    ref = case.reference()
    host, host_rows = host_answer(T, case)
    C.check_run(ref, host, host_rows)
    for got, rel in (run_host_buffers(T, h, case), run_sync(T, h, case), run_async(T, h, case),
                     run_async(T, h, case, count_on_device=True)):
        C.check_run(ref, got, rel)
        C.same(got, host)
        assert rel.tobytes() == host_rows.tobytes()
    return ref


@pytest.mark.parametrize("name", list(C.RUNS))
def test_run_cases(T, handle, name):
    """Every branch of the table at every W, lists of 0 .. 2 L + 1 events, session counts around a
    wave's and a block's groups, event totals around the tile with all and with none routed."""
    all_forms(T, handle, C.RUNS[name]())


def test_hover_session_of_20000_events(T, handle):
    all_forms(T, handle, C.hover_case())


def test_fuzz(T, handle):
    case = C.fuzz()
    all_forms(T, handle, case)
    x, y = run_async(T, handle, case), run_async(T, handle, case)  # two runs are byte-identical
    C.same(x[0], y[0])
    assert x[1].tobytes() == y[1].tobytes()


@pytest.mark.parametrize("w", C.WIDTHS)
def test_lanes_override_gives_the_same_bytes(T, w):
    """Every legal number of lanes a session for this W (and one above W / 2, which is lowered)."""
    h = T.Rel(0)
    cases = [C.table_case(w, src=True), C.lens_case(w), C.fuzz(seed=3, n_sessions=90, w=w)]
    for lanes in [v for v in T.LANES if v <= w // 2] + [64, 0]:
        h.set_tuning("lanes", lanes)
        assert h.stats()["lanes"] == lanes
        for case in cases:
            for got, rel in (run_sync(T, h, case), run_async(T, h, case, count_on_device=True)):
                C.check_run(case.reference(), got, rel)


def test_count_is_read_on_the_device(T, handle):
    """cap_in and cap_boxes larger than the counts: the buffers are larger than what is written."""
    case = C.fuzz(seed=6, n_sessions=400)
    ref = case.reference()
    for run in (run_sync, run_async):
        for on_device in (False, True):
            got, rel = run(T, handle, case, cap_in=case.total + 3 * C.TILE + 5, cap_boxes=case.m + 77, count_on_device=on_device)
            C.check_run(ref, got, rel)


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("what", ["cap_in", "cap_boxes"])
def test_refused_input_writes_only_the_summary(T, handle, form, what):
    import torch
    from emqx_amd import _lib
    case = C.RUNS["tile_%d_all_routed" % (C.TILE + 1)]()
    kw = dict(cap_in=case.total - 1) if what == "cap_in" else dict(cap_boxes=case.m - 1, count_on_device=True)
    b = RunBatch(T, case, **kw)
    if form == "sync":
        with pytest.raises(_lib.EngineError) as e:
            handle.run_device(b.args)
        assert e.value.code == -1
        summary = e.value.summary
    else:
        handle.reserve(b.cap_in, b.cap_boxes, case.w)
        handle.run_device_async(b.args, b.summary.data_ptr())
        torch.cuda.synchronize()
        summary = dict(zip(T.RUN_SUMMARY, b.summary.cpu().numpy().view(np.uint64)[:8].tolist()))
    want = [R.F_INPUT_REFUSED, case.total if what == "cap_in" else 0, case.m, 0, 0, 0, 0, 0]
    assert [summary[k] for k in T.RUN_SUMMARY] == want
    got, rel = b.result(T, summary)  # the sentinels are intact from the first element of every output
    assert got.verdicts.size == 0 and got.counts.size == 0 and rel.tobytes() == case.rel.tobytes()


def test_scratch_reuse_on_one_handle(T):
    """The 2 T + 1 batch, then three events, then the fuzz: no tile total or counter of an earlier
    call shows in a later one."""
    h = T.Rel(0)
    for case in (C.RUNS["tile_%d_all_routed" % (2 * C.TILE + 1)](), C.RUNS["no_ts_w8"](), C.fuzz()):
        for run in (run_async, run_sync):
            got, rel = run(T, h, case)
            C.check_run(case.reference(), got, rel)
    assert h.stats()["calls"] == 6 and h.stats()["cap_in"] >= 2 * C.TILE + 1 and h.stats()["scratch_bytes"] > 0


def test_async_needs_reserve(T):
    import torch
    from emqx_amd import _lib
    case = C.lens_case(16)
    h = T.Rel(0)
    b = RunBatch(T, case)
    xc = C.EXPIRES["w16"]()
    xb = ExpireBatch(T, xc)
    for short in (None, (case.total - 1, case.m, case.w), (case.total, case.m - 1, case.w), (case.total, case.m, 8)):
        if short:
            h = T.Rel(0)
            h.reserve(*short)
        with pytest.raises(_lib.EngineError) as e:
            h.run_device_async(b.args, b.summary.data_ptr())
        assert e.value.code == _lib.EMQX_EOVERFLOW
    with pytest.raises(_lib.EngineError) as e:
        T.Rel(0).expire_device_async(xb.args, xb.summary.data_ptr())
    assert e.value.code == _lib.EMQX_EOVERFLOW
    torch.cuda.synchronize()
    assert (b.summary.cpu().numpy().view(np.uint64) == S64).all(), "nothing was enqueued"
    assert (xb.summary.cpu().numpy().view(np.uint64) == S64).all() and h.stats()["calls"] == 0
    h.reserve(case.total, case.m, case.w)
    h.run_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    got, rel = b.result(T)
    C.check_run(case.reference(), got, rel)
    assert h.stats()["calls"] == 1


def test_misaligned_tables_and_bad_widths_are_refused(T, handle):
    from emqx_amd import _lib
    case = C.RUNS["no_ts_w8"]()
    for change in (dict(rel=8), dict(sessions=8), dict(out_counts=4), dict(w=-4), dict(w=4)):
        b = RunBatch(T, case)
        for k, v in change.items():
            setattr(b.args, k, getattr(b.args, k) + v)
        with pytest.raises(_lib.EngineError) as e:
            handle.run_device(b.args)
        assert e.value.code == -1
        assert b.result(T, dict(dict.fromkeys(T.RUN_SUMMARY, 0), flags=R.F_INPUT_REFUSED))[1].tobytes() == case.rel.tobytes()


# ---- the expire call ---------------------------------------------------------------------------

class ExpireBatch:
    def __init__(self, T, case, cap_boxes=None, count_on_device=False):
        import torch
        self.case = case
        self.cap_boxes = case.m if cap_boxes is None else cap_boxes
        self.subs = None if case.subs is None else dev(case.subs, np.uint32)
        self.timeouts = None if case.timeouts is None else dev(case.timeouts, np.uint32)
        self.table, self.rel = dev_raw(case.table, GUARD), dev_raw(case.rel, GUARD)
        self.count = dev([case.m], np.uint64) if count_on_device else None
        self.status, self.cnt = filled(self.cap_boxes, torch.uint8), filled(4 * self.cap_boxes, torch.int32)
        self.summary = filled(8, torch.int64)
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        self.args = T.Rel.expire_args(0 if count_on_device else case.m, self.cap_boxes, self.table.data_ptr(), case.sub_limit,
                                      self.rel.data_ptr(), case.w, case.now_ms, self.status.data_ptr(), self.cnt.data_ptr(),
                                      timeout_ms=case.timeout_ms, d_timeouts=ptr(self.timeouts), d_subs=ptr(self.subs),
                                      channel_rule=case.channel_rule, d_n_boxes=ptr(self.count))

    def result(self, T, summary=None):
        if summary is None:
            s = self.summary.cpu().numpy().view(np.uint64)
            assert (s[8:] == S64).all()
            summary = dict(zip(T.EXPIRE_SUMMARY, s[:8].tolist()))
        m = 0 if summary["flags"] & R.F_INPUT_REFUSED else summary["sessions"]
        status, cnt = self.status.cpu().numpy(), self.cnt.cpu().numpy().view(np.uint32)
        assert (status[m:] == S8).all() and (cnt[4 * m:] == S32).all(), "a write past the defined extent"
        table_unchanged(self.table, self.case)
        return T.Expired(status[:m], cnt[:4 * m].reshape(-1, 4), summary), host_rel(self.rel, self.case)


def expire_sync(T, h, case, **kw):
    from emqx_amd import _lib
    b = ExpireBatch(T, case, **kw)
    try:
        summary = h.expire_device(b.args)
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & (R.F_BAD_SUB | R.F_INPUT_REFUSED)
        summary = e.summary
    return b.result(T, summary)


def expire_async(T, h, case, **kw):
    import torch
    b = ExpireBatch(T, case, **kw)
    h.reserve(0, b.cap_boxes, case.w)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        h.expire_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(T)


def expire_host_buffers(T, h, case):
    from emqx_amd import _lib
    table, rel = case.table.copy(), case.rel.copy()
    try:
        got = h.expire(table, rel, **case.host_args())
    except _lib.EngineError as e:
        assert e.code == -1 and e.summary["flags"] & R.F_BAD_SUB
        got = e.partial
    assert table.tobytes() == case.table.tobytes()
    return got, rel


@pytest.mark.parametrize("name", list(C.EXPIRES))
def test_expire_cases(T, handle, name):
    """Nothing due, everything due, age == timeout and timeout - 1, infinity, timeouts[] mixed, the
    channel's rule, subs NULL and listed, at every W and around a block's sessions."""
    from emqx_amd import _lib
    case = C.EXPIRES[name]()
    ref = case.reference()
    host_rows = case.rel.copy()
    try:
        host = T.Rel(T.HOST_ONLY).expire_host(case.table.copy(), host_rows, **case.host_args())
    except _lib.EngineError as e:
        host = e.partial
    C.check_expire(ref, host, host_rows)
    for got, rel in (expire_host_buffers(T, handle, case), expire_sync(T, handle, case), expire_async(T, handle, case),
                     expire_async(T, handle, case, count_on_device=True),
                     expire_sync(T, handle, case, cap_boxes=case.m + 9, count_on_device=True)):
        C.check_expire(ref, got, rel)
        C.same(got, host)
        assert rel.tobytes() == host_rows.tobytes()


def test_expire_refused_input_writes_only_the_summary(T, handle):
    import torch
    case = C.EXPIRES["w8_65_sessions"]()
    b = ExpireBatch(T, case, cap_boxes=case.m - 1, count_on_device=True)
    handle.reserve(0, b.cap_boxes, case.w)
    handle.expire_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    got, rel = b.result(T)
    assert [got.summary[k] for k in T.EXPIRE_SUMMARY] == [R.F_INPUT_REFUSED, 0, case.m, 0, 0, 0, 0, 0]
    assert got.status.size == 0 and rel.tobytes() == case.rel.tobytes()


# ---- the chain ---------------------------------------------------------------------------------

def test_chain_group_rel_gather_match_on_one_stream(T):
    """Three rounds of raw inbound events on one stream with no host read: each round is
    emqx_inbox_group_batch_device_async over the raw events (one "message" each) ->
    emqx_rel_run_batch_device_async on its box_filters, inbox_subs, inbox_offsets, box_src and summary
    word 2 -> a gather of the topics out_route names -> emqx_match_batch_device_async; an
    emqx_rel_expire_batch_device_async sits between rounds 2 and 3 and drops what round 1 stored.
    All of it against the restatements, and the matched sets against the oracle for exactly the
    routed messages."""
    import torch
    from emqx_amd import inbox as I
    from emqx_amd import window as W
    from emqx_amd.engine import Engine
    from oracle import emqx_ref as O
    sub_limit, w, limit, n, width = 6, 8, 2, 10, 8
    filters = [b"sens/+", b"sens/001", b"sens/005", b"#", b"other/#", b"sens/00+", b"+/007"]
    e = Engine(0)
    e.insert(filters)
    e.commit()
    table = W.pack_sessions(sub_limit)
    table["flags"][4] = W.PRESENT | W.CONNECTED | W.PASS
    rows = T.empty_rows(sub_limit, w)
    rows[2, 5] = T.pack_entry(900, 7)  # session 2 awaits id 7 from before
    P, L, D_ = R.PUBLISH, R.PUBREL, R.DIRECT
    rounds = [  # (now_ms, [(session, kind, pkt_id)] in arrival order); message i of round r has topic sens/%03d of 10 r + i
        (1000, [(2, P, 7), (0, P, 1), (2, P, 8), (0, P, 2), (1, D_, 0), (0, P, 3), (2, P, 9), (4, P, 1), (5, L, 4), (1, P, 1)]),
        (5000, [(0, L, 1), (0, P, 3), (0, P, 1), (2, L, 7), (2, P, 9), (1, P, 1), (1, L, 1), (1, P, 2), (3, D_, 9), (3, P, 5)]),
        (7000, [(0, P, 1), (0, P, 2), (0, P, 3), (2, P, 7), (2, P, 8), (1, P, 1), (1, P, 2), (1, P, 3), (3, P, 5), (3, P, 6)]),
    ]
    expire_now, timeout = 6000, 3000  # what round 1 stored (and the entry from before) is due, round 2's is not
    topics = [[b"sens/%03d" % (10 * r + i) for i in range(n)] for r in range(3)]
    assert all(len(t) == width for ts_ in topics for t in ts_)
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    d_table, d_rows = dev_raw(table), dev_raw(rows)
    d_raw_off, d_topic_off = dev(np.arange(n + 1), np.uint64), dev(np.arange(n + 1) * width, np.uint64)
    cap = n * len(filters)
    box, rel = I.Inbox(0), T.Rel(0)
    box.reserve(n, sub_limit)
    rel.reserve(n, sub_limit, w)
    bufs = []
    for r, (now, evs) in enumerate(rounds):
        b = dict(raw_subs=dev([s for s, _, _ in evs], np.uint32), raw_ev=dev(T.pack_events([k for _, k, _ in evs], [p for _, _, p in evs]), np.uint32),
                 topic_bytes=dev(np.frombuffer(b"".join(topics[r]), dtype=np.uint8).reshape(n, width), np.uint8),
                 box_msgs=z(n, torch.int32), box_ev=z(n, torch.int32), box_src=z(n, torch.int32), subs=z(sub_limit, torch.int32),
                 off=z(sub_limit + 1, torch.int64), isum=z(8, torch.int64), ver=z(n, torch.uint8), route=z(n, torch.int32),
                 cnt=z(4 * sub_limit, torch.int32), arm=z(sub_limit, torch.uint8), rsum=z(8, torch.int64), moff=z(n + 1, torch.int64),
                 mids=z(cap, torch.int32), msum=z(e.SUMMARY_WORDS, torch.int64))
        b["g"] = I.Inbox.batch(d_raw_off.data_ptr(), b["raw_subs"].data_ptr(), b["raw_ev"].data_ptr(), n, n, sub_limit, b["box_msgs"].data_ptr(),
                               b["box_ev"].data_ptr(), b["subs"].data_ptr(), b["off"].data_ptr(), sub_limit, d_box_src=b["box_src"].data_ptr())
        b["a"] = T.Rel.run_args(b["subs"].data_ptr(), b["off"].data_ptr(), b["box_ev"].data_ptr(), 0, n, sub_limit, d_table.data_ptr(),
                                sub_limit, d_rows.data_ptr(), w, b["ver"].data_ptr(), b["route"].data_ptr(), b["cnt"].data_ptr(),
                                b["arm"].data_ptr(), max_awaiting=limit, now_ms=now, d_src=b["box_src"].data_ptr(),
                                d_n_boxes=b["isum"].data_ptr() + 16)
        bufs.append(b)
    x_status, x_cnt, x_sum = z(sub_limit, torch.uint8), z(4 * sub_limit, torch.int32), z(8, torch.int64)
    xargs = T.Rel.expire_args(sub_limit, sub_limit, d_table.data_ptr(), sub_limit, d_rows.data_ptr(), w, expire_now, x_status.data_ptr(),
                              x_cnt.data_ptr(), timeout_ms=timeout)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for r, b in enumerate(bufs):
            if r == 2:
                rel.expire_device_async(xargs, x_sum.data_ptr(), stream=stream.cuda_stream)
            box.group_device_async(b["g"], b["isum"].data_ptr(), stream=stream.cuda_stream)
            rel.run_device_async(b["a"], b["rsum"].data_ptr(), stream=stream.cuda_stream)
            # the topics of out_route, in its order; the entries behind its count name message 0 (the buffer starts zeroed)
            b["gathered"] = b["topic_bytes"].index_select(0, b["route"].to(torch.int64).clamp_(0, n - 1)).contiguous()
            e.match_device_async(b["gathered"].data_ptr(), d_topic_off.data_ptr(), n, b["moff"].data_ptr(), b["mids"].data_ptr(), cap,
                                 b["msum"].data_ptr(), mode=0, stream=stream.cuda_stream)
    stream.synchronize()
    # the restatements, step by step
    flags = [int(f) for f in table["flags"]]
    ref_rows = [[int(x) for x in row] for row in rows]
    routed_per_round = []
    for r, (now, evs) in enumerate(rounds):
        b = bufs[r]
        if r == 2:
            x = R.expire(None, sub_limit, flags, ref_rows, w, expire_now, timeout_ms=timeout)
            assert x_sum.cpu().numpy().view(np.uint64).tolist() == x["summary"] and x["summary"][3:6] == [2, 4, 4]
            assert x_status.cpu().numpy().tolist() == x["status"] and x_cnt.cpu().numpy().view(np.uint32).reshape(-1, 4).tolist() == x["counts"]
        g = I.Inbox(I.HOST_ONLY).group_host(np.arange(n + 1), [s for s, _, _ in evs], T.pack_events([k for _, k, _ in evs], [p for _, _, p in evs]),
                                            sub_limit)
        m = g.inbox_subs.size
        assert b["isum"].cpu().numpy().view(np.uint64)[:3].tolist() == [0, n, m]
        assert b["subs"].cpu().numpy().view(np.uint32)[:m].tolist() == g.inbox_subs.tolist()
        assert b["box_ev"].cpu().numpy().view(np.uint32).tolist() == g.filters.tolist()
        assert b["box_src"].cpu().numpy().view(np.uint32).tolist() == g.src.tolist()
        x = R.run(g.inbox_subs, g.inbox_offsets, g.filters, flags, ref_rows, w, max_awaiting=limit, now_ms=now, src=g.src)
        assert b["rsum"].cpu().numpy().view(np.uint64).tolist() == x["summary"]
        assert b["ver"].cpu().numpy().tolist() == x["verdicts"]
        k = len(x["route"])
        assert b["route"].cpu().numpy().view(np.uint32)[:k].tolist() == x["route"]
        assert b["cnt"].cpu().numpy().view(np.uint32)[:4 * m].reshape(-1, 4).tolist() == x["counts"]
        assert b["arm"].cpu().numpy()[:m].tolist() == x["arm"]
        # the match of exactly the routed messages against the oracle
        assert int(b["msum"][0]) == 0, "the match completed in one pass"
        moff, mids = b["moff"].cpu().numpy(), b["mids"].cpu().numpy().view(np.uint32)
        for i, msg in enumerate(x["route"]):
            got = sorted(mids[moff[i]:moff[i + 1]].tolist())
            want = O.brute_force_routes(filters, topics[r][msg])
            assert got == sorted(want), (r, i, msg, got, want)
        routed_per_round.append(x["route"])
    got_rows = d_rows.cpu().numpy().view(np.uint64).reshape(sub_limit, w)
    assert got_rows.tolist() == ref_rows
    assert d_table.cpu().numpy().tobytes() == dev_raw(table).cpu().numpy().tobytes()
    # what the rounds mean: round 1 fills sessions 0 and 2 to their limit; round 3's publishes land only because the expire made room
    assert routed_per_round[0] == [1, 3, 4, 9, 2] and routed_per_round[2] == [0, 5, 3, 9]

