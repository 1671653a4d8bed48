"""Byte-level edge sweep of the match kernels' tokenizer paths (GPU): phase A of fast_tile, the
deep path's tokenizer, the small-batch kernel's copy, order_kernels.hip and the retained index's
filter tokenizer, on the batches of tests/byte_edge_cases.py (checked against the oracle alone by
tests/test_byte_edges_cpu.py).

Every comparison is bit-exact as sorted filter-id lists per topic, for every topic of every batch,
against oracle/emqx_ref.py: brute_force_routes (mode 0), brute_force_trie (mode 1) and the
wildcard-only trie (mode 2).  Which limit each test pins down:

  vec_ok == false, the bytes around a batch   test_unaligned_pointers_poisoned_surroundings
  use_map == false                            big-tile batches, every variant (test_batched_every_variant)
  level of 4094 / 4095 bytes                  level-length batches + last_deferred, every variant
  tile bytes past 1 MiB                       test_mib_tile_and_deep_limits
  WID_CAP / 8 levels, WID_CAP words           level-count and tile-sum batches + where last_deferred steps
  words of 15 / 16 / 17 bytes, shared heads,  the families batch, every variant and the small-batch kernel
  24-byte words of one hash and one head
  non-ASCII bytes beside separators           the window sweep and the families batch
  65535-byte topics, 65536 levels, EINVAL     test_mib_tile_and_deep_limits
  all-empty batches                           every variant, the small-batch kernel, the walk order

Wall time of the module on one MI355X, the Python reference included: 11 s for its 33 tests (3 s
of it the first test, which computes the reference the others share).
"""

import numpy as np
import pytest

from oracle import retain_ref as RR
from tests import byte_edge_cases as B

pytestmark = pytest.mark.gpu

N_VARIANTS = 18
LIMIT_VARIANTS = [None, 5, 9]      # the default, the smallest and the largest word-id capacity
LEVEL_CAPS = (56, 64, 80, 96, 128)     # WID_CAP / 8 over the variants
WORD_CAPS = (448, 512, 640, 768, 1024)  # WID_CAP over the variants
SUM_F_ERROR = 4                    # include/emqx_match.h
SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
POISON = np.frombuffer(b"/+/#/", dtype=np.uint8)


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (shares the HIP runtime with the engine)
    from emqx_amd.engine import Engine as E
    from emqx_amd import _lib
    _lib.lib()
    return E


_PACKED, _CSR = {}, {}


def packed(case):
    if case.name not in _PACKED:
        _PACKED[case.name] = B.pack(case.topics())
    return _PACKED[case.name]


def exp_csr(case, mode):
    """The reference CSR of a batch: computed once, shared by every test, never changed."""
    key = (case.name, mode)
    if key not in _CSR:
        off, ids = B.expected_csr(case.table, case.topics(), mode)
        off.setflags(write=False)
        ids.setflags(write=False)
        _CSR[key] = (off, ids)
    return _CSR[key]


def engine_for(Engine, tname, variant=None, small=0):
    e = Engine()
    ids = e.insert(B.table(tname))
    assert list(ids) == list(range(len(B.table(tname))))
    e.commit()
    if variant is not None:
        e.set_tuning("fast_variant", variant)
    e.set_tuning("small_batch", small)
    return e


def assert_exact(case, mode, off, ids, what):
    eo, ei = exp_csr(case, mode)
    bad = B.csr_bad_topics(off, ids, eo, ei)
    if bad:
        i = bad[0]
        t = case.topics()[i]
        got = sorted(np.asarray(ids)[int(off[i]):int(off[i + 1])].tolist())
        raise AssertionError("%s, %s (%s), mode %d: %d topics differ, first %d (%d bytes, %r...): got %s, expected %s"
                             % (what, case.name, case.note(), mode, len(bad), i, len(t), t[:48], got[:12],
                                ei[eo[i]:eo[i + 1]].tolist()[:12]))


def run_case(e, case, mode, what):
    off, ids = e.match_packed(*packed(case), mode=mode)
    assert int(off[-1]) == ids.size
    assert_exact(case, mode, off, ids, what)
    return off, ids


# ---- the batched path, every variant ---------------------------------------------------------
@pytest.mark.parametrize("variant", range(N_VARIANTS))
def test_batched_every_variant(Engine, variant):
    engines = {t: engine_for(Engine, t, variant) for t in ("base", "deep")}
    assert engines["base"].stats()["n_words"] * 3 <= 1024   # the 1024-slot vocab table of the CPU test's probe chains
    deferred = {}
    for case in B.EVERY_VARIANT:
        e = engines[case.table]
        for mode in (0, 1, 2):
            run_case(e, case, mode, "variant %d" % variant)
            if mode == 0:
                deferred[case.name] = e.stats()["last_deferred"]
    # a level of 4094 bytes stays on the fast path, one of 4095 bytes defers its topic
    for case in B.LEVEL_LEN:
        assert deferred[case.name] == B.long_level_topics(case.topics()), (variant, case.name, deferred[case.name])
    # both sides of the level-count and the word-count limit ran, and the step from "none deferred"
    # to "some deferred" lies between a capacity of some variant and the next count
    for fam, caps, name in ((B.NLEV, LEVEL_CAPS, "nlev%d"), (B.TILE_SUM, WORD_CAPS, "sum%d")):
        d = [deferred[c.name] for c in fam]
        assert min(d) == 0 and max(d) > 0, (variant, d)
        assert any(deferred[name % c] == 0 and deferred[name % (c + 1)] > 0 for c in caps), (variant, d)
    for e in engines.values():
        e.close()


# ---- device entry points with guarded buffers ----------------------------------------------------
def device_match(e, buf, shift, offs, n, total, mode):
    """emqx_match_batch_device on `buf[shift:]` with sentinel words around the CSR buffers."""
    import torch
    dev = torch.device("cuda", 0)
    t_bytes = torch.from_numpy(buf).to(dev)
    t_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(dev)
    cap = total + 64
    d_off = torch.full((8 + n + 1 + 8,), SENT64, dtype=torch.int64, device=dev)
    d_ids = torch.full((16 + cap + 16,), SENT32, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    got = e.match_device(t_bytes.data_ptr() + shift, t_offs.data_ptr(), n, d_off.data_ptr() + 64,
                         d_ids.data_ptr() + 64, cap, mode=mode)
    off, ids = d_off.cpu().numpy(), d_ids.cpu().numpy()
    assert got == total, (got, total)
    assert (off[:8] == SENT64).all() and (off[8 + n + 1:] == SENT64).all(), "words around the n + 1 offsets written"
    assert (ids[:16] == SENT32).all() and (ids[16 + total:] == SENT32).all(), "ids past the total written"
    return off[8:8 + n + 1], ids[16:16 + total].view(np.uint32)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("variant", LIMIT_VARIANTS)
def test_unaligned_pointers_poisoned_surroundings(Engine, variant, order):
    """The byte pointer at every alignment within 16 bytes, offsets from 0 and from 5, the bytes
    around the batch filled with separators and wildcards: none of them may reach a result."""
    e = engine_for(Engine, "base", variant)
    e.set_tuning("order", order)
    for case in (B.WINDOW, B.BIG_TILE[3]):
        tb, to = packed(case)
        n, nbytes = len(to) - 1, int(to[-1])
        for k in range(16):
            for start in (0, 5):
                buf = np.resize(POISON, 64 + k + start + nbytes + 64).copy()
                buf[64 + k + start:64 + k + start + nbytes] = tb[:nbytes]
                for mode in ((0, 1, 2) if (k, start) == (3, 5) else (0,)):
                    total = int(exp_csr(case, mode)[0][-1])
                    off, ids = device_match(e, buf, 64 + k, to.astype(np.int64) + start, n, total, mode)
                    assert_exact(case, mode, off, ids, "variant %s order %d shift %d start %d" % (variant, order, k, start))
    e.set_tuning("order", -1)
    e.close()


@pytest.mark.parametrize("variant", LIMIT_VARIANTS)
def test_mib_tile_and_deep_limits(Engine, variant):
    import torch
    from emqx_amd import _lib
    from emqx_amd.engine import EngineError
    # a tile of more than 1 MiB: the topics at and behind the mark defer, nothing else does
    e = engine_for(Engine, "base", variant)
    for mode in (0, 1, 2):
        run_case(e, B.MIB, mode, "variant %s" % variant)
        assert e.stats()["last_deferred"] == B.MIB_BEHIND
    e.close()
    # 65535 bytes are matched: 65536 empty levels, 32768 one-byte levels, 20 levels of up to 4094 bytes
    e = engine_for(Engine, "limit", variant)
    for case in (B.SLASHES, B.ORD65535):
        for mode in (0, 1, 2):
            run_case(e, case, mode, "variant %s" % variant)
    assert e.stats()["last_deferred"] >= 1
    # 65536 bytes on the deep path are refused by every entry point ...
    tb, to = packed(B.TOO_LONG)
    n = len(to) - 1
    with pytest.raises(EngineError) as x:
        e.match_packed(tb, to, mode=0)
    assert x.value.code == _lib.EMQX_EINVAL
    dev = torch.device("cuda", 0)
    d_tb, d_to = torch.from_numpy(tb).to(dev), torch.from_numpy(to.astype(np.int64)).to(dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(4096, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(EngineError) as x:
        e.match_device(d_tb.data_ptr(), d_to.data_ptr(), n, d_off.data_ptr(), d_ids.data_ptr(), d_ids.numel(), mode=0)
    assert x.value.code == _lib.EMQX_EINVAL
    summ = torch.zeros(Engine.SUMMARY_WORDS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    e.match_device_async(d_tb.data_ptr(), d_to.data_ptr(), n, d_off.data_ptr(), d_ids.data_ptr(), d_ids.numel(),
                         summ.data_ptr(), mode=0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(summ[0]) & SUM_F_ERROR
    # ... and the same engine answers the next batches exactly, on both entry points
    for mode in (0, 1, 2):
        run_case(e, B.ORD65535, mode, "after EINVAL, variant %s" % variant)
    tb, to = packed(B.SLASHES)
    total = int(exp_csr(B.SLASHES, 0)[0][-1])
    off, ids = device_match(e, tb, 0, to.astype(np.int64), len(to) - 1, total, 0)
    assert_exact(B.SLASHES, 0, off, ids, "device call after EINVAL, variant %s" % variant)
    e.close()


# ---- the one-launch small-batch kernel -----------------------------------------------------------
def host_batch(e, case, mode):
    from emqx_amd.engine import HostBatch
    hb = HostBatch(e, cap_topics=2048, cap_bytes=1 << 20, cap_ids=1 << 16)
    hb.pack(*packed(case))
    hb.submit(mode)
    off, ids = hb.wait()
    hb.close()
    return off, ids


def test_small_batch_kernel(Engine):
    cases = [B.WINDOW, B.FAMILIES, B.LEVEL_LEN[1], B.LEVEL_LEN[2]] + B.EMPTY
    e = engine_for(Engine, "base", small=1)
    assert e.stats()["max_depth"] <= 12     # the table the small-batch path takes
    for case in cases:
        assert len(case.topics()) <= 1024
        for mode in (0, 1, 2):
            res = []
            for small in (1, 0):
                e.set_tuning("small_batch", small)
                off, ids = host_batch(e, case, mode)
                assert_exact(case, mode, off, ids, "small_batch %d" % small)
                res.append((off, ids))
            assert np.array_equal(res[0][0], res[1][0])
            assert not B.csr_bad_topics(res[0][0], res[0][1], res[1][0].astype(np.int64),
                                        _sorted_ids(*res[1])), (case.name, mode)
    e.close()


def _sorted_ids(off, ids):
    out = np.asarray(ids).astype(np.int64).copy()
    for i in range(len(off) - 1):
        out[int(off[i]):int(off[i + 1])].sort()
    return out


# ---- the walk order ------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["base", "deep", "limit"])
def test_walk_order(Engine, tname):
    """Every batch walked in prefix-key order returns the unordered walk's CSR offsets and the
    reference's sets."""
    from tests.test_gpu_order import SETTINGS, ordered_csr, same_csr
    e = engine_for(Engine, tname)
    for case in B.ALL_MATCHED:
        if case.table != tname:
            continue
        tb, to = packed(case)
        for mode in (0, 1, 2):
            e.set_tuning("order", 0)
            base = run_case(e, case, mode, "unordered")
            for lb, sb, deal in (SETTINGS if mode == 0 else SETTINGS[:1]):
                got = ordered_csr(e, tb, to, mode, lb, sb, deal)
                same_csr(base, got)
                assert_exact(case, mode, got[0], got[1], "order %s" % ((lb, sb, deal),))
    e.set_tuning("order", -1)
    e.close()


# ---- the retained index's filter tokenizer -------------------------------------------------------
@pytest.mark.parametrize("balance", [1, 0])
def test_retained_index_words(balance):
    """retain_kernels.hip tokenizes filters with the same inline-16-byte compare: the vocabulary
    stored as topic levels, matched by '+', a final '#', the 15/16/17-byte families, unknown and
    non-ASCII words, against the retainer's oracle."""
    import torch  # noqa: F401
    from emqx_amd import _lib, retainer
    _lib.lib()
    names, filters = B.retain_names(), B.retain_filters()
    idx = retainer.RetainIndex()
    assert list(idx.store(names)) == list(range(len(names)))
    idx.commit()
    if not balance:
        idx.set_tuning("balance", 0)
    tt = RR.TokenTrie(names, [0] * len(names))
    got = idx.match(filters, 100)
    exp = [tt.dispatch(f, 100) for f in filters]
    assert any(exp) and not all(exp)
    for f, g, x in zip(filters, got, exp):
        assert g == x, (balance, f[:60], g[:8], x[:8])
    idx.close()
