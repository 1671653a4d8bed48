"""The sharded step (emqx_amd/csrc/shard_step.hip) driven through its C API in one process: one
step handle per rank, the two exchanges done in place (rank r is handed the address of chunk r
inside each source's buffer, as dist.py EmulatedWorld does), a synthetic matcher (shard_ref.synth_csr)
in place of the engines.  The same driver runs the step's host mode (device -1, numpy memory) and
its kernels (device 0, torch tensors); only allocation and read-back differ.  Every output buffer
is allocated larger than needed over a sentinel and compared whole against the restatement
(tests/shard_ref.py).

The cases sit on the thresholds of the launch code (kSortTile = 512 requests a tile: 256 topics
with two keys a topic, 512 with one; N = (3 world + 1) * tiles table entries, one block up to
kOneBlockScan = 8192, else segments of kScanSeg = 2048; recv and answer grids capped at
1024 / world blocks):

  one_block_full  world 64, 10,752 topics: 42 tiles, N = 8,106, the largest one-block table
  seg_first       world 64, 10,753 topics: 43 tiles, N = 8,299, 5 segments (the last 107 entries)
  seg_exact       world 5, 163,840 topics: 640 tiles x 16 buckets = 5 full segments
  skew            world 64, two sources of 10,753 topics k/l/m/%d: one A and one B bucket with
                  > 10 K requests from each of two sources (second trips of unpack_part and
                  answer_source at the 16-block cap, byte gather)
  tile_edges      world 3, n around the row (256 requests) and tile (512) bounds
  one_key         one request a topic: world 1, and world 3 with space P replicated
  split_plan      world 8, hot keys split over ranks (the plan staged in LDS), space P replicated
                  (the plan shard_plan chooses) and sharded
  lengths         world 3, every topic length 0-80 and 255, 256, 1,000, 4,099
  large           world 64, 1,100,000 topics: N = 829,321, 405 segments (per = 2 in
                  shard_seg_scan_kernel), 2.2 M requests (> 2,097,152: shard_gather_kernel's
                  second trip), n > 524,288 (shard_merge_kernel's)
  fixed3, fixed64 world 3 (1,500 topics a source) and 64 (300 a source) in the fixed form (FIXED_CASES:
                  exact capacities, one capacity too small, a bad summary, and capacities with padding
                  topics behind the requests: 0, 1, 17 and more than a pass of the recv grid,
                  without ids and with marked ids of their own, pad_extras)
  fixed3_sparse   world 3, 8 topics from two sources: slots no source asks, with padding only
"""

import ctypes
import functools

import numpy as np

from tests import shard_ref as R

E, HW, MW = R.E, R.HW, R.MW
TAIL = 256  # bytes allocated past every output, checked to still hold the sentinel
EMPTY_PLAN = np.zeros((0, 2), np.uint32)


# ---- topics ------------------------------------------------------------------------------------

def pack(items):
    lens = np.fromiter((len(s) for s in items), dtype=np.int64, count=len(items))
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), offs


def empty_batch():
    return np.zeros(0, np.uint8), np.zeros(1, np.uint64)


EXTRA = [b"$SYS/brokers", b"$SYS/x/y/z", b"$SYS", b"a/+/c", b"+/b1/c", b"#", b"a7/#", b"+", b"+/+/c3"]


def random_topics(n, seed):
    """n topics a%d/b%d/c%d (every 97th one-level), the last few '$SYS/...' and wildcard names."""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.integers(0, hi, n).tolist() for hi in (1000, 1000, 50))
    items = [b"a%d/b%d/c%d" % t for t in zip(a, b, c)]
    for i in range(0, n, 97):
        items[i] = b"a%d" % a[i]
    k = min(len(EXTRA), n // 4)
    if k:
        items[n - k:] = EXTRA[:k]
    return pack(items)


def numbered_topics(n, fmt):
    return pack([fmt % i for i in range(n)])


def length_topics(seed):
    """'x/y/' + tail at every total length 0-80 and 255, 256, 1,000, 4,099, shuffled."""
    items = []
    for i, L in enumerate(list(range(81)) + [255, 256, 1000, 4099]):
        items.append((b"x/y/" + bytes(97 + (i * 7 + j * 3) % 26 for j in range(L)))[:L])
    order = np.random.default_rng(seed).permutation(len(items))
    return pack([items[i] for i in order])


class Case:
    def __init__(self, name, world, plan, batches):
        self.name, self.world, self.plan = name, world, plan
        self.batches = [b if b is not None else empty_batch() for b in batches]
        self._ref = None

    @property
    def ref(self):  # computed once, shared by every test of the case
        if self._ref is None:
            self._ref = R.Ref(self.world, self.plan, self.batches)
        return self._ref


def _sources(world, given):
    return [given.get(s) for s in range(world)]


TILE_EDGE_N = (0, 1, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1500)
ONE_KEY_N = (1, 511, 512, 513, 700)
ONE_KEY_FILTERS = [b"#", b"+/#", b"a1/#", b"a2/b2/c2", b"+/b1/c1", b"+/b2/#", b"a3/+/c3", b"$SYS/#", b"+/b3", b"a4/b4"]


@functools.lru_cache(maxsize=None)
def replicated_plan(world):
    from emqx_amd import dist as D
    plan = D.shard_plan(pack(ONE_KEY_FILTERS), world, p_space="replicated")
    assert D.plan_p_replicated(plan)
    return plan


@functools.lru_cache(maxsize=None)
def split_plan_workload():
    """Config B's filters with keys split at 5 % of a rank's share: the plan as shard_plan chooses it
    (space P replicated for this table: one key a topic) and with space P sharded (two keys)."""
    from emqx_amd import dist as D
    from emqx_amd import workloads as W
    wl = W.config_b(n_filters=20_000, n_topics=3000, seed=3, vocab_scale=4, extra_topic_seeds=(1003, 1007))
    plans = (D.shard_plan(wl.filters, 8, max_piece_pm=50),
             D.shard_plan(wl.filters, 8, max_piece_pm=50, p_space="sharded"))
    for plan in plans:  # split keys, few enough to be staged in LDS (kLdsSplits = 2048)
        assert ((plan[:, 1] >> 16) > 1).any() and len(plan) <= 2048
    assert not D.plan_p_replicated(plans[1])
    return plans, [wl.topics] + list(wl.extra_topics)


@functools.lru_cache(maxsize=None)
def case(name):  # noqa: C901
    """The named case; a tuple of cases for the names that sweep n."""
    rt = random_topics
    if name == "one_block_full":
        return Case(name, 64, EMPTY_PLAN, _sources(64, {0: rt(10_752, 1), 1: rt(300, 2), 63: rt(300, 3)}))
    if name == "seg_first":
        return Case(name, 64, EMPTY_PLAN, _sources(64, {0: rt(10_753, 1), 1: rt(300, 2), 63: rt(300, 3)}))
    if name == "seg_first_again":  # other topics in the same shape (the second step on the same handles)
        return Case(name, 64, EMPTY_PLAN, _sources(64, {0: rt(10_753, 4), 1: rt(300, 5), 63: rt(300, 6)}))
    if name == "seg_exact":
        return Case(name, 5, EMPTY_PLAN, _sources(5, {0: rt(163_840, 7), 3: rt(300, 8)}))
    if name == "skew":
        return Case(name, 64, EMPTY_PLAN, _sources(64, {0: numbered_topics(10_753, b"k/l/m/%d"),
                                                        1: numbered_topics(10_753, b"k/l/m/%d"), 63: rt(300, 9)}))
    if name == "tile_edges":
        return tuple(Case("%s_%d" % (name, n), 3, EMPTY_PLAN, _sources(3, {0: rt(n, 10 + n), 2: rt(40, 11)}))
                     for n in TILE_EDGE_N)
    if name == "one_key":
        return tuple(Case("%s_w1_%d" % (name, n), 1, EMPTY_PLAN, [rt(n, 20 + n)]) for n in ONE_KEY_N) + \
            tuple(Case("%s_w3_%d" % (name, n), 3, replicated_plan(3), _sources(3, {0: rt(n, 30 + n), 2: rt(40, 12)}))
                  for n in ONE_KEY_N)
    if name == "split_plan":
        plans, tops = split_plan_workload()
        return tuple(Case("%s_%d" % (name, i), 8, plan, _sources(8, {0: tops[0], 3: tops[1], 7: tops[2]}))
                     for i, plan in enumerate(plans))
    if name == "lengths":
        return Case(name, 3, EMPTY_PLAN, _sources(3, {0: length_topics(1), 1: length_topics(2)}))
    if name == "large":
        return Case(name, 64, EMPTY_PLAN, _sources(64, {0: rt(1_100_000, 13), 1: rt(300, 14)}))
    if name == "fixed3":
        return Case(name, 3, EMPTY_PLAN, [rt(1500, 40 + s) for s in range(3)])
    if name == "fixed64":
        return Case(name, 64, EMPTY_PLAN, [rt(300, 50 + s) for s in range(64)])
    if name == "fixed3_sparse":  # a small batch after a large one: slots with capacity and no request
        return Case(name, 3, EMPTY_PLAN, _sources(3, {0: numbered_topics(7, b"zz%d/y"), 2: pack([b"solo"])}))
    raise KeyError(name)


SMALL_CASES = ("one_block_full", "seg_first", "seg_exact", "skew", "tile_edges", "one_key", "split_plan", "lengths")


def cases_of(name):
    c = case(name)
    return c if isinstance(c, tuple) else (c,)


def scan_shape(c):
    """(tiles, table entries N, segments; 0 = the one-block scan) of source 0's send."""
    m = c.ref.sends[0].m
    tiles = (m + 511) // 512
    N = (E * c.world + 1) * tiles
    return tiles, N, 0 if N <= 8192 else (N + 2047) // 2048


# ---- memory: numpy (host mode) or torch tensors (the device) ---------------------------------------

class Buf:
    """nbytes of output memory over the sentinel, TAIL bytes more than asked for."""

    def __init__(self, device, nbytes, fill=R.SENTINEL, data=None):
        self.device = device
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            if len(data) % 16:
                data = np.concatenate([data, np.zeros(16 - len(data) % 16, np.uint8)])
            if not len(data):
                data = np.zeros(16, np.uint8)
            nbytes = len(data)
        else:
            nbytes = R.al16(int(nbytes)) + TAIL
        self.nbytes = nbytes
        if device < 0:
            self.a = data.copy() if data is not None else np.full(nbytes, fill, np.uint8)
            self.ptr = self.a.ctypes.data
        else:
            import torch
            if data is not None:
                self.a = torch.from_numpy(data).to("cuda:%d" % device)
            else:
                self.a = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda:%d" % device)
            self.ptr = self.a.data_ptr()

    def read(self, dtype=np.uint8):
        if self.device < 0:
            return self.a.view(dtype)
        import torch
        torch.cuda.synchronize(self.device)
        return self.a.cpu().numpy().view(dtype)


def _ptrs(addrs):
    return (ctypes.c_void_p * len(addrs))(*[a if a else None for a in addrs])


def assert_sentinel(arr, used, what):
    """Everything past the first `used` elements of a buffer read back still holds the sentinel."""
    assert (arr[used:].view(np.uint8) == R.SENTINEL).all(), "%s: written past element %d" % (what, used)


class Result:
    """What one step left behind, read back: per source the send buffer and meta, per rank the
    answer buffer (and meta, classic form), per source the CSR; fixed form: every rank's flag."""

    def __init__(self):
        self.send, self.meta, self.answer, self.ans_meta, self.csr, self.flags = [], [], [], [], [], []


class World:
    """One step handle per rank of a world on `device` (-1: host mode)."""

    def __init__(self, world, plan, device):
        from emqx_amd import _lib
        self.L, self._lib = _lib.lib(), _lib
        self.G, self.device = world, device
        pl = np.ascontiguousarray(plan, dtype=np.uint32) if len(plan) else np.zeros((1, 2), np.uint32)
        self.h = []
        for _ in range(world):
            h = ctypes.c_void_p()
            _lib.check(self.L.emqx_shard_step_create(device, world, pl.ctypes.data, len(plan), ctypes.byref(h)),
                       "emqx_shard_step_create")
            self.h.append(h)

    def close(self):
        for h in self.h:
            self.L.emqx_shard_step_destroy(h)
        self.h = []

    def buf(self, nbytes=0, data=None):
        return Buf(self.device, nbytes, data=data)

    def step(self, batches, ref, fixed=None):  # noqa: C901
        """One step of every rank over `batches`, checked against `ref` (shard_ref.Ref) as it goes:
        the meta words before any address is derived from them, the slot batches before they are
        answered.  fixed: None (the classic calls) or a dict chunk_bytes, capq[r][e], capy[r][e],
        chunk_words, bad (ranks given a nonzero summary word)."""
        L, G, chk = self.L, self.G, self._lib.check
        res = Result()
        cb = fixed["chunk_bytes"] if fixed else 0
        # 1. send on every rank
        sends = []
        for s in range(G):
            tb, to = batches[s]
            n = len(to) - 1
            dtb = self.buf(data=tb)
            dto = self.buf(data=np.asarray(to).astype(np.uint64))
            cap = G * cb if fixed else int(L.emqx_shard_send_cap(n, len(tb), G))
            send, meta = self.buf(cap), self.buf(8 * MW * G)
            if fixed:
                chk(L.emqx_shard_step_send_fixed(self.h[s], dtb.ptr, dto.ptr, n, send.ptr, cb, meta.ptr, None),
                    "emqx_shard_step_send_fixed")
            else:
                chk(L.emqx_shard_step_send(self.h[s], dtb.ptr, dto.ptr, n, send.ptr, cap, meta.ptr, None),
                    "emqx_shard_step_send")
            sends.append((send, meta, dtb, dto))
        # 2. the meta words back: they give every chunk's place, so they are checked first
        for s in range(G):
            m = sends[s][1].read(np.int64)
            assert_sentinel(m, MW * G, "meta of source %d" % s)
            res.meta.append(m[: MW * G].reshape(G, MW).copy())
            assert np.array_equal(res.meta[s], ref.sends[s].expect_meta(cb)), "meta of source %d" % s
            res.send.append(sends[s][0].read().copy())
        # 3. rank r reads chunk r of every source where it was packed
        base = [ref.sends[s].bases(cb) for s in range(G)]
        recv_f, ans_f, merged_f = ref.fixed_flags(cb, fixed["capq"], fixed["capy"], fixed["chunk_words"],
                                                  fixed.get("bad", ())) if fixed else ([0] * G, [0] * G, 0)
        answers, keep = [], []
        for r in range(G):
            chunks = [sends[s][0].ptr + int(base[s][r]) for s in range(G)]
            mi = np.ascontiguousarray(np.stack([res.meta[s][r] for s in range(G)]))
            exp = [ref.slot_batch(r, e, empty=recv_f[r] != 0) for e in range(E)]
            capq = fixed["capq"][r] if fixed else [len(exp[e][0]) - 1 for e in range(E)]
            capy = fixed["capy"][r] if fixed else [len(exp[e][1]) for e in range(E)]
            qoff = [self.buf(8 * (capq[e] + 1)) for e in range(E)]
            qby = [self.buf(capy[e]) for e in range(E)]
            qb = _ptrs([b.ptr for b in qby])
            # 4. recv
            if fixed:
                chk(L.emqx_shard_step_recv_fixed(self.h[r], _ptrs(chunks), (ctypes.c_uint64 * E)(*capq),
                                                 (ctypes.c_uint64 * E)(*capy), qb, _ptrs([b.ptr for b in qoff]), None),
                    "emqx_shard_step_recv_fixed")
            else:
                chk(L.emqx_shard_step_recv(self.h[r], _ptrs(chunks), mi.ctypes.data, qb, _ptrs([b.ptr for b in qoff]),
                                           None), "emqx_shard_step_recv")
            # 5. the slot batches against the restatement (offsets rebased to 0, bytes)
            csrs = []
            for e in range(E):
                eoff, eby = exp[e]
                ne = len(eoff) - 1
                got = qoff[e].read(np.uint64)
                what = "rank %d slot %d" % (r, e)
                assert_sentinel(got, capq[e] + 1, what + " offsets")
                assert np.array_equal(got[: ne + 1] - got[0], eoff), what + " offsets"
                assert (got[ne + 1: capq[e] + 1] == got[ne]).all(), what + " padding offsets"
                raw = qby[e].read()
                if (qb[e] or 0) != qby[e].ptr:  # matched in place in its one source's chunk
                    assert not fixed and (raw == R.SENTINEL).all(), what + " byte buffer of a slot read in place"
                    src = [s for s in range(G) if ref.sends[s].nq[r, e]]
                    assert len(src) == 1, what
                    at = qb[e] - sends[src[0]][0].ptr + int(got[0])
                    assert 0 <= at and at + len(eby) <= len(res.send[src[0]]), what
                    assert np.array_equal(res.send[src[0]][at: at + len(eby)], eby), what + " bytes"
                else:
                    assert got[0] == 0 and got[ne] == len(eby), what  # (padding topics: empty, at the slot's end)
                    assert_sentinel(raw, len(eby), what + " bytes")
                    assert np.array_equal(raw[: len(eby)], eby), what + " bytes"
                # 6. the synthetic matcher's CSR of the batch as read back, padded to the capacity
                # (fixed["pad_ids"]: the padding topics have ids of their own behind the requests')
                off, ids = R.synth_csr(r, e, eby, eoff)
                off, ids = R.pad_csr(off, ids, capq[e] - ne, bool(fixed and fixed.get("pad_ids")))
                csrs.append((self.buf(data=off), self.buf(data=ids), off, ids))
            n_ids = sum(len(c[3]) for c in csrs)
            n_q = sum(len(c[2]) - 1 for c in csrs)
            # 7. answer
            if fixed:
                cw = fixed["chunk_words"]
                ans = self.buf(4 * G * cw)
                summ = [self.buf(data=np.array([1 if r in fixed.get("bad", ()) else 0] + [0] * 7, np.uint64))
                        for e in range(E)]
                chk(L.emqx_shard_step_answer_fixed(self.h[r], _ptrs([c[0].ptr for c in csrs]),
                                                   _ptrs([c[1].ptr for c in csrs]), _ptrs([b.ptr for b in summ]), r,
                                                   ans.ptr, cw, None), "emqx_shard_step_answer_fixed")
                keep.append((csrs, summ, qoff, qby))
                answers.append((ans, None))
            else:
                ans, am = self.buf(4 * (HW * G + n_q + n_ids)), self.buf(8 * 3 * G)
                chk(L.emqx_shard_step_answer(self.h[r], _ptrs([c[0].ptr for c in csrs]),
                                             _ptrs([c[1].ptr for c in csrs]), None, r, ans.ptr, am.ptr, None),
                    "emqx_shard_step_answer")
                keep.append((csrs, qoff, qby))
                answers.append((ans, am))
        # 8. the answer chunks back in place
        abase = []
        for r in range(G):
            ans, am = answers[r]
            res.answer.append(ans.read(np.uint32).copy())
            if fixed:
                abase.append(np.arange(G) * fixed["chunk_words"])
                continue
            m = am.read(np.int64)
            assert_sentinel(m, 3 * G, "answer meta of rank %d" % r)
            res.ans_meta.append(m[: 3 * G].reshape(G, 3).copy())
            words = ref.answer_words(r)
            assert np.array_equal(res.ans_meta[r][:, 0], words[:, 0]) and not res.ans_meta[r][:, 1].any() \
                and np.array_equal(res.ans_meta[r][:, 2], words[:, 1]), "answer meta of rank %d" % r
            abase.append(np.concatenate([[0], np.cumsum(words[:, 0])]))
            assert_sentinel(res.answer[r], int(abase[r][G]), "answer buffer of rank %d" % r)
        # 9. merge on every source
        want = ref.results()
        for s in range(G):
            n = len(batches[s][1]) - 1
            back = [answers[r][0].ptr + 4 * int(abase[r][s]) for r in range(G)]
            total = 0 if merged_f else len(want[s][1])
            out_off, out_ids = self.buf(8 * (n + 1)), self.buf(4 * total)
            if fixed:
                flag = self.buf(4)
                chk(L.emqx_shard_step_merge_fixed(self.h[s], _ptrs(back), out_off.ptr, out_ids.ptr, flag.ptr, None),
                    "emqx_shard_step_merge_fixed")
                f = flag.read(np.uint32)
                assert_sentinel(f, 1, "flag of rank %d" % s)
                res.flags.append(int(f[0]))
            else:
                ai = np.ascontiguousarray(np.stack([res.ans_meta[r][s] for r in range(G)]))
                chk(L.emqx_shard_step_merge(self.h[s], _ptrs(back), ai.ctypes.data, out_off.ptr, out_ids.ptr, None),
                    "emqx_shard_step_merge")
            off, ids = out_off.read(np.uint64), out_ids.read(np.uint32)
            assert_sentinel(off, n + 1, "out offsets of source %d" % s)
            assert_sentinel(ids, total, "out ids of source %d" % s)
            res.csr.append((off[: n + 1].copy(), ids[:total].copy()))
        return res


def check_result(res, ref, fixed=None):
    """Send buffers and meta by bytes, the final CSRs and (fixed form) the flags, against `ref`."""
    G = ref.world
    cb = fixed["chunk_bytes"] if fixed else 0
    merged = ref.fixed_flags(cb, fixed["capq"], fixed["capy"], fixed["chunk_words"], fixed.get("bad", ()))[2] \
        if fixed else 0
    for s in range(G):
        assert np.array_equal(res.meta[s], ref.sends[s].expect_meta(cb)), "meta of source %d" % s
        want = ref.sends[s].expect_buffer(len(res.send[s]), cb)
        bad = np.nonzero(res.send[s] != want)[0]
        assert not len(bad), "send buffer of source %d: %d bytes differ, the first at %d" % (s, len(bad), bad[0])
        off, ids = ref.results()[s]
        if merged:
            assert not res.csr[s][0].any() and not len(res.csr[s][1]), "a flagged step of source %d" % s
        else:
            assert np.array_equal(res.csr[s][0], off), "CSR offsets of source %d" % s
            assert np.array_equal(res.csr[s][1], ids), "CSR ids of source %d" % s
    if fixed:
        assert res.flags == [merged] * G, (res.flags, merged)


def same_bytes(a, b):
    """Two runs of one case (the device's and host mode's) byte for byte: send buffers, meta,
    answer buffers (and meta), output CSRs, flags."""
    for name in ("send", "meta", "answer", "ans_meta"):
        xa, xb = getattr(a, name), getattr(b, name)
        assert len(xa) == len(xb), name
        for r, (x, y) in enumerate(zip(xa, xb)):
            assert x.tobytes() == y.tobytes(), "%s of rank %d" % (name, r)
    for s, (x, y) in enumerate(zip(a.csr, b.csr)):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes(), "CSR of source %d" % s
    assert a.flags == b.flags


def run_world(world, plan, batches, device, ref=None, fixed=None):
    """One step of `world` ranks on `device` (-1: host mode, 0: the GPU) on fresh handles."""
    w = World(world, plan, device)
    try:
        return w.step(batches, ref if ref is not None else R.Ref(world, plan, batches), fixed)
    finally:
        w.close()


def run_case(c, device, world=None):
    """The case through one step, checked against its restatement; returns what it left."""
    res = world.step(c.batches, c.ref) if world else run_world(c.world, c.plan, c.batches, device, c.ref)
    check_result(res, c.ref)
    return res


# ---- the fixed form's cases ------------------------------------------------------------------------

FIXED_CASES = ("fits", "chunk_small", "slot_small", "answer_small", "summary_bad", "padded", "padded_ids")


def fixed_caps(c, kind):
    """The fixed form's capacities for case c, derived from its classic sizes (the restatement's):
    exactly what the batches need, then one capacity made too small."""
    ref, G = c.ref, c.world
    sizes = np.stack([sd.size for sd in ref.sends])
    fx = {"chunk_bytes": int(sizes.max()),
          "capq": [[int(ref.q0(r, e)[G]) for e in range(E)] for r in range(G)],
          "capy": [[len(ref.slot_batch(r, e)[1]) for e in range(E)] for r in range(G)],
          "chunk_words": int(max(ref.answer_words(r)[:, 0].max() for r in range(G))), "bad": ()}
    if kind == "chunk_small":
        fx["chunk_bytes"] -= 16  # the largest multiple of 16 below the largest chunk
    elif kind == "slot_small":
        e = int(np.argmax(fx["capq"][1]))
        fx["capq"][1][e] -= 1  # rank 1's fullest slot: one request short
    elif kind == "answer_small":
        fx["chunk_words"] -= 1
    elif kind == "summary_bad":
        fx["bad"] = (2,)
    elif kind in ("padded", "padded_ids"):
        extra = pad_extras(c)
        fx["capq"] = [[fx["capq"][r][e] + extra[r][e] for e in range(E)] for r in range(G)]
        fx["capy"] = [[fx["capy"][r][e] + 16 * ((r + 2 * e) % 4) for e in range(E)] for r in range(G)]
        fx["pad_ids"] = kind == "padded_ids"
    else:
        assert kind == "fits"
    return fx


PAD_EXTRA = (0, 1, 17)
PAD_LONG = (1, 0)  # the (rank, slot) padded over one pass of the recv grid


def pad_extras(c):
    """Padding topics per (rank, slot) of the `padded` kinds: 0, 1 or 17 by (rank + slot) % 3, so
    every rank has each and no two neighbours agree; rank 1's slot 0 gets more than one pass of
    shard_recv_fixed_kernel's grid: the smallest 512 * 2^k above the grid's stride, which is
    computed (shard_ref.recv_stride) from the rank's capacities with that padding in them, so the
    padding block's threads write at k and k + stride (pad_slot's second trip)."""
    ref, G = c.ref, c.world
    extra = [[PAD_EXTRA[(r + e) % 3] for e in range(E)] for r in range(G)]
    r, e = PAD_LONG
    need_q = [int(ref.q0(r, k)[G]) for k in range(E)]
    capy = [len(ref.slot_batch(r, k)[1]) + 16 * ((r + 2 * k) % 4) for k in range(E)]
    long = 512
    while True:
        extra[r][e] = long
        if long > R.recv_stride(G, [need_q[k] + extra[r][k] for k in range(E)], capy):
            return extra
        long *= 2


def expected_fixed_flag(kind):
    return {"fits": 0, "chunk_small": 1, "slot_small": 2, "answer_small": 8, "summary_bad": 4, "padded": 0,
            "padded_ids": 0}[kind]


def run_fixed(c, kind, device):
    """Case c in the fixed form with the capacities of `kind`; checked against the restatement and
    the case's description (tests/test_shard_step_cpu.py)."""
    fx = fixed_caps(c, kind)
    ref, G = c.ref, c.world
    res = run_world(G, c.plan, c.batches, device, ref, fx)
    check_result(res, ref, fx)
    recv_f, ans_f, merged = ref.fixed_flags(fx["chunk_bytes"], fx["capq"], fx["capy"], fx["chunk_words"], fx["bad"])
    assert merged == expected_fixed_flag(kind), (kind, merged)
    cw = fx["chunk_words"]
    for r in range(G):  # a flagged rank's answer chunks: a header only, the flag in word 7
        a = res.answer[r]
        for s in range(G):
            if ans_f[r]:
                assert a[s * cw: s * cw + HW].tolist() == [0] * 7 + [ans_f[r]], (kind, r, s)
                assert (a[s * cw + HW: (s + 1) * cw].view(np.uint8) == R.SENTINEL).all(), (kind, r, s)
            else:
                assert a[s * cw + 7] == 0 and a[s * cw] + a[s * cw + 1] + a[s * cw + 2] == \
                    sum(int(ref.sends[s].nq[r, e]) for e in range(E)), (kind, r, s)
    if kind == "chunk_small":
        over = [s for s in range(G) if ref.sends[s].over(fx["chunk_bytes"])]
        assert over and all(f & 1 for f in ans_f)
        for s in over:  # that source's chunks are all header-only with word 3 = 1
            w = res.send[s][: G * fx["chunk_bytes"]].view(np.uint32).reshape(G, -1)
            assert (w[:, : HW + E] == [0, 0, 0, 1] + [0] * 7).all() and (res.meta[s][:, 0] == -1).all()
            assert (w[:, HW + E:].view(np.uint8) == R.SENTINEL).all()
    if kind == "slot_small":
        assert recv_f[1] == 2 and ans_f[1] == 2 and sum(1 for f in recv_f if f) == 1
    if kind == "fits":
        assert all(f == 0 for f in res.flags)
    if kind in ("padded", "padded_ids"):
        # padding costs no answer word and leaves no trace: every send buffer, answer chunk and
        # CSR is the `fits` run's byte for byte (recv's padding offsets and the sentinel behind
        # them are checked in World.step), and no padding id is in any of them
        assert all(f == 0 for f in res.flags)
        extra = pad_extras(c)
        npad = sum(map(sum, extra))
        assert extra[PAD_LONG[0]][PAD_LONG[1]] > R.recv_stride(G, fx["capq"][PAD_LONG[0]], fx["capy"][PAD_LONG[0]]) \
            and {0, 1, 17} <= {x for row in extra for x in row}
        same_bytes(res, fits_run(c, device))
        for r in range(G):
            assert not (res.answer[r] >> 24 == R.PAD_MARK).any(), "a padding id in an answer chunk of rank %d" % r
            assert not (res.csr[r][1] >> 24 == R.PAD_MARK).any(), "a padding id in the CSR of source %d" % r
    return res


@functools.lru_cache(maxsize=None)
def fits_run(c, device):
    """Case c's `fits` run on `device`, once for every padded kind compared with it."""
    return run_fixed(c, "fits", device)


def padded_ids_total(c):
    """The padding ids the synthetic matcher of `padded_ids` writes over all of case c's slots."""
    return sum(int((np.arange(x) % 6).sum()) for row in pad_extras(c) for x in row)
