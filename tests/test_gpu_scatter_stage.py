"""The CSR scatter's two paths (GPU): ids stored straight to their final positions, or staged
through an LDS window and stored as whole 16-byte vectors (match_kernels.hip
scatter_tile_staged; emqx_set_tuning "scatter_stage" 0 / 1).

Both paths give every id the same position, so every case runs both on one engine and one
input and wants the offsets and the ids bit-identical, guard words in front of the ids buffer
and behind the last id untouched, and each topic's sorted ids equal to the brute-force oracle.
Tables are families of '#' filters that all match one topic, so a tile's id total is chosen
exactly: 63 topics of a family of K filters and one topic of a family of r filters hold
63 K + r ids.  The totals sit around the window (W ids) and the window count a tile may take
(P; one id more goes the direct way); tile 0's total and the buffer's address move the spans
to every 4-byte alignment within a 16-byte block."""

import os
import re

import numpy as np
import pytest

from oracle import emqx_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "emqx_amd", "csrc", "kernels.h")) as _f:
    _H = _f.read()
W = int(re.search(r"SCATTER_STAGE_W = (\d+);", _H).group(1))  # ids per window
P = int(re.search(r"SCATTER_STAGE_P = (\d+);", _H).group(1))  # windows a staged tile may take
SIZES = (W - 1, W, W + 1, 2 * W + 1, P * W + 1)
SMALL = (0, 5, 6, 7, 40)  # tile 0's totals (odd, 2 mod 4, 3 mod 4), an empty tile, a filler
GUARD = -1515870811  # 0xA5A5A5A5 as int32
FRONT = 4            # guard words in front of the ids (one 16-byte block)
CAP = 1 << 15
TAIL = b"/a" * 7
DEEP = b"D/" + b"/".join([b"a"] * 85)  # more than 80 levels: the deep path takes it
SUM_F_OVERFLOW = 2


def family(name, k):
    """k filters that all match name/a/a/a/a/a/a/a (and nothing of another family)."""
    out = []
    for n in range(8):
        for m in range(1 << n):
            if len(out) == k:
                return out
            out.append(b"/".join([name] + [b"+" if (m >> i) & 1 else b"a" for i in range(n)] + [b"#"]))
    assert len(out) == k, (name, k)
    return out


def tile(total):
    """64 topics holding exactly `total` ids in modes 0 and 1."""
    return [b"F%d" % total + TAIL] * 63 + [b"R%d" % total + TAIL]


def table():
    f = []
    for t in SIZES + SMALL:
        f += family(b"F%d" % t, t // 63) + family(b"R%d" % t, t % 63)
    f += [b"D/#", b"D/+/#", b"X/#", b"X" + TAIL, b"X/a"]  # X: an exact filter too (mode 2 differs)
    return f


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (shares the HIP runtime with the engine)
    from emqx_amd.engine import Engine as E
    from emqx_amd import _lib
    _lib.lib()
    return E


def make_engine(Engine, filters, ext=None):
    from emqx_amd.engine import pack
    e = Engine()
    ext = list(range(len(filters))) if ext is None else ext
    ids = e.insert_packed_ext(*pack(list(filters)), np.asarray(ext, dtype=np.uint32))
    assert list(ids) == list(range(len(filters)))
    e.commit()
    e.set_tuning("small_batch", 0)  # the batched kernels are the subject
    return e


class Oracle:
    """Brute-force rows per distinct topic, computed once and shared by every test."""

    def __init__(self, filters):
        self.filters = filters
        self.wild = [f if R.wildcard(f) else b"\x00never" for f in filters]
        self.memo = {}

    def row(self, topic, mode):
        k = (topic, mode)
        if k not in self.memo:
            if mode == 0:
                r = R.brute_force_routes(self.filters, topic)
            else:
                r = R.brute_force_trie(self.filters if mode == 1 else self.wild, topic)
            self.memo[k] = sorted(int(i) for i in r)
        return self.memo[k]

    def rows(self, topics, mode, ext=None):
        rows = [self.row(t, mode) for t in topics]
        return rows if ext is None else [sorted(ext[i] for i in r) for r in rows]


@pytest.fixture(scope="module")
def shared(Engine):
    f = table()
    return make_engine(Engine, f), Oracle(f)


class Out:
    def __init__(self, off, ids, flags, total):
        self.off, self.ids, self.flags, self.total = off, ids, flags, total

    def rows(self):
        return [sorted(self.ids[self.off[i]:self.off[i + 1]].tolist()) for i in range(len(self.off) - 1)]


class Call:
    """One call's device buffers: the ids buffer starts 4 * mis bytes past a 16-byte boundary,
    with guard words in front of it and all through it."""

    def __init__(self, topics, mis=0):
        import torch
        from emqx_amd.engine import pack
        dev = torch.device("cuda:0")
        tb, to = pack(list(topics))
        self.n = len(topics)
        self.tb = torch.from_numpy(np.array(tb)).to(dev)
        self.to = torch.from_numpy(to.view(np.int64)).to(dev)
        self.off = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.buf = torch.full((FRONT + mis + CAP + 8,), GUARD, dtype=torch.int32, device=dev)
        self.ids = self.buf[FRONT + mis:FRONT + mis + CAP]
        assert self.ids.data_ptr() % 16 == 4 * mis
        self.summ = torch.zeros(8, dtype=torch.int64, device=dev)
        self.mis = mis

    def enqueue(self, e, mode, cap, stream):
        e.match_device_async(self.tb.data_ptr(), self.to.data_ptr(), self.n, self.off.data_ptr(), self.ids.data_ptr(),
                             cap, self.summ.data_ptr(), mode=mode, stream=stream)

    def sync_call(self, e, mode, stream):
        return e.match_device(self.tb.data_ptr(), self.to.data_ptr(), self.n, self.off.data_ptr(), self.ids.data_ptr(),
                              CAP, mode=mode, stream=stream)

    def result(self, cap=CAP, total=None, flags=0):
        """The CSR, after checking that no word outside ids[0, min(total, cap)) was written."""
        if total is None:
            s = self.summ.cpu().numpy().view(np.uint64)
            flags, total = int(s[0]), int(s[1])
        off = self.off.cpu().numpy().view(np.uint64)
        assert int(off[-1]) == total
        buf = self.buf.cpu().numpy()
        lo, written = FRONT + self.mis, min(total, cap)
        assert (buf[:lo] == GUARD).all(), "a word in front of out_ids was written"
        assert (buf[lo + written:] == GUARD).all(), "a word at or past min(total, out_cap) was written"
        return Out(off, buf[lo:lo + written].view(np.uint32).copy(), flags, total)


def run(e, topics, stage, mode=0, mis=0, cap=None, order=None):
    """One call with scatter_stage = stage: synchronous (reruns in place), or, with an out_cap,
    through the async entry point, whose summary carries the overflow flag."""
    import torch
    c = Call(topics, mis)
    s = torch.cuda.current_stream().cuda_stream
    e.set_tuning("scatter_stage", stage)
    if order is not None:
        e.set_tuning("order", order)
    try:
        if cap is None:
            return c.result(total=c.sync_call(e, mode, s))
        c.enqueue(e, mode, cap, s)
        torch.cuda.synchronize()
        return c.result(cap=cap)
    finally:
        e.set_tuning("scatter_stage", -1)
        if order is not None:
            e.set_tuning("order", -1)


def both(e, oracle, topics, modes=(0,), mis=0, ext=None):
    """Both paths on the same engine and input: bit-identical CSRs that equal the oracle."""
    for mode in modes:
        d = run(e, topics, 0, mode=mode, mis=mis)
        s = run(e, topics, 1, mode=mode, mis=mis)
        assert d.flags == 0 and s.flags == 0
        assert np.array_equal(d.off, s.off), mode
        assert np.array_equal(d.ids, s.ids), mode
        assert s.rows() == oracle.rows(topics, mode, ext), mode
    return s


def test_tile_totals_are_what_the_cases_assume(shared):
    _, oracle = shared
    for t in SIZES + SMALL:
        assert sum(map(len, oracle.rows(tile(t), 0))) == t
    assert len(oracle.row(b"X" + TAIL, 0)) == 2 and len(oracle.row(b"X" + TAIL, 2)) == 1


@pytest.mark.parametrize("n", [1, 65, 100, 192])
def test_batch_sizes(shared, n):
    """One topic; a second tile of one topic; a batch that is no multiple of 64; whole tiles."""
    e, oracle = shared
    topics = (tile(W + 1) + [b"X" + TAIL, b"nope", b"X/a"] * 12 + tile(2 * W + 1)[:28] + tile(40))[:n]
    assert len(topics) == n
    both(e, oracle, topics, modes=(0, 1, 2))


def test_tile_without_ids(shared):
    e, oracle = shared
    s = both(e, oracle, tile(W + 1) + tile(0) + tile(7), modes=(0, 1, 2))
    assert s.off[64] == s.off[128] == W + 1 and s.total == W + 8


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
@pytest.mark.parametrize("first", [5, 6, 7])
@pytest.mark.parametrize("total", SIZES)
def test_tile_totals_bases_and_buffer_alignment(shared, total, first, mis):
    """A tile of W - 1, W, W + 1, 2 W + 1 and P W + 1 ids (the last is scattered directly) whose
    span starts 1, 2 or 3 entries past a multiple of 4, in a buffer 0, 4, 8 or 12 bytes past a
    16-byte boundary, with a tile behind it."""
    e, oracle = shared
    s = both(e, oracle, tile(first) + tile(total) + tile(40), mis=mis)
    assert s.off[64] == first and s.total == first + total + 40


@pytest.mark.parametrize("total", [W + 1, P * W + 1])
def test_every_mode_on_staged_and_direct_tiles(shared, total):
    e, oracle = shared
    both(e, oracle, tile(6) + tile(total) + [b"X" + TAIL] * 64, modes=(0, 1, 2), mis=3)


@pytest.mark.parametrize("where", ["mid-tile", "tile-boundary", "first-tile"])
@pytest.mark.parametrize("mis", [0, 1])
def test_out_cap_cuts_the_csr(shared, where, mis):
    """out_cap in the middle of a tile, exactly at a tile's end, and inside tile 0: the call is
    flagged, nothing at or past out_cap is written (Call.result), and the ids below it are the
    direct path's — and the uncapped call's."""
    e, oracle = shared
    topics = tile(W + 1) + tile(2 * W + 1) + tile(40)
    full = both(e, oracle, topics, mis=mis)
    cap = {"mid-tile": W + 1 + W + 3, "tile-boundary": W + 1 + 2 * W + 1, "first-tile": W - 2}[where]
    d = run(e, topics, 0, mis=mis, cap=cap)
    s = run(e, topics, 1, mis=mis, cap=cap)
    for r in (d, s):
        assert r.flags == SUM_F_OVERFLOW and r.total == full.total and len(r.ids) == cap
        assert np.array_equal(r.off, full.off)
    assert np.array_equal(d.ids, s.ids)
    assert np.array_equal(s.ids, full.ids[:cap])


def test_deferred_topic_beside_ordinary_ones(shared):
    """One topic of tile 1 goes to the deep path, which fills its range itself: that tile takes
    the direct path, its neighbours the staged one, and all three are exact.  (The deep path
    ranks a topic's ids with atomics, so only that topic's range may differ in order.)"""
    e, oracle = shared
    mid = tile(W + 1)
    mid[17] = DEEP
    topics = tile(W + 1) + mid + tile(2 * W + 1)
    d, s = run(e, topics, 0), run(e, topics, 1)
    exp = oracle.rows(topics, 0)
    assert len(exp[64 + 17]) == 2
    assert np.array_equal(d.off, s.off) and d.rows() == exp and s.rows() == exp
    a, b = int(s.off[64 + 17]), int(s.off[64 + 18])
    assert np.array_equal(d.ids[:a], s.ids[:a]) and np.array_equal(d.ids[b:], s.ids[b:])


def test_slab_grown_by_the_first_call(Engine, shared):
    """Fresh engines, whose first call overflows the tile slab and is rerun with the learnt size
    (the flagged pass scatters the overflowed tile directly whatever the switch says)."""
    _, oracle = shared
    topics = tile(5) + tile(2 * W + 1) + tile(W)
    outs = []
    for stage in (0, 1):
        e = make_engine(Engine, oracle.filters)
        outs.append(run(e, topics, stage))
        assert e.stats()["last_evals"] > 0
    assert np.array_equal(outs[0].off, outs[1].off) and np.array_equal(outs[0].ids, outs[1].ids)
    assert outs[1].rows() == oracle.rows(topics, 0)


def test_wide_entries(Engine, shared):
    """The 8-byte slab entry (one reported id of 2^26 or more forces it) through both paths."""
    _, oracle = shared
    f = oracle.filters
    ext = list(range(len(f)))
    big = (1 << 26) + 5
    ext[f.index(b"F%d/#" % (W + 1))] = big
    e = make_engine(Engine, f, ext)
    for mis in (0, 1):
        s = both(e, oracle, tile(6) + tile(W + 1) + tile(2 * W + 1) + tile(P * W + 1), modes=(0, 2), mis=mis, ext=ext)
        assert big in s.rows()[64] and big in s.rows()[126]


def test_walk_order_ignores_the_switch(shared):
    """A reordered batch's tiles have no contiguous span: with the walk order forced on, the
    switch changes nothing and the CSR is the batch-order call's."""
    e, oracle = shared
    topics = tile(7) + tile(W + 1) + [b"X" + TAIL, b"nope"] * 32 + tile(2 * W + 1)[:30]
    ref = both(e, oracle, topics)
    for stage in (0, 1):
        r = run(e, topics, stage, order=1)
        assert np.array_equal(r.off, ref.off) and r.rows() == ref.rows()


def test_async_calls_on_two_streams(shared):
    """Two calls in flight on two streams, each with its own buffers: both CSRs are exact and
    bit-identical to the direct path's."""
    import torch
    e, oracle = shared
    batches = [tile(5) + tile(2 * W + 1) + tile(W - 1), tile(6) + tile(W) + tile(P * W + 1) + tile(40)[:9]]
    refs = [run(e, b, 0, mis=m) for b, m in zip(batches, (1, 2))]
    calls = [Call(b, m) for b, m in zip(batches, (1, 2))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    e.set_tuning("scatter_stage", 1)
    try:
        for _ in range(2):  # the second round reuses both workspaces
            for c, st in zip(calls, streams):
                c.enqueue(e, 0, CAP, st.cuda_stream)
        torch.cuda.synchronize()
    finally:
        e.set_tuning("scatter_stage", -1)
    for c, ref, b in zip(calls, refs, batches):
        r = c.result()
        assert r.flags == 0
        assert np.array_equal(r.off, ref.off) and np.array_equal(r.ids, ref.ids)
        assert r.rows() == oracle.rows(b, 0)
