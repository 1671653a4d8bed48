"""The sharded step's host mode (emqx_amd/csrc/shard_step.hip, device < 0) through its C API in
one process (tests/shard_cases.py: one handle per rank, chunks exchanged in place, a synthetic
matcher), against the sequential restatement (tests/shard_ref.py): meta words and send buffers by
bytes, the slot batches, the final CSRs and the fixed form's flags, at every shape the GPU test
(tests/test_gpu_shard_world.py) runs except `large`.  This pins host mode itself and validates the
restatement and the driver before the same cases run on the device."""

import os
import subprocess

import numpy as np
import pytest

from tests import shard_cases as SC
from tests import shard_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not os.path.exists(os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True, capture_output=True)


def test_synth_csr_counts_and_ids():
    """The synthetic matcher is a pure function of (rank, slot, bytes): every count range occurs
    (0, 1-6, and 17-40 for about one request in 16), ids carry rank, slot and a running index."""
    tb, to = SC.random_topics(4000, 99)
    off, ids = R.synth_csr(5, 1, tb, to)
    cnt = np.diff(off.astype(np.int64))
    assert set(np.unique(cnt)) >= {0, 1, 2, 3, 4, 5, 6, 17, 40} and cnt.max() == 40
    assert not ((cnt > 6) & (cnt < 17)).any()
    assert 4000 / 32 < (cnt >= 17).sum() < 4000 / 10
    assert (ids >> 24 == 5 * 3 + 1).all()
    assert np.array_equal(ids & 63, np.arange(len(ids)) - np.repeat(off[:-1].astype(np.int64), cnt))
    # the same request anywhere in a batch gets the same ids; another rank or slot does not
    sub_off, sub_ids = R.synth_csr(5, 1, tb[int(to[100]):], to[100:] - to[100])
    assert np.array_equal(sub_ids, ids[int(off[100]):])
    assert not np.array_equal(R.synth_csr(5, 2, tb, to)[1], ids)


def test_case_shapes():
    """The arithmetic of the cases: the tables they build sit where the module's docstring says."""
    assert SC.scan_shape(SC.case("one_block_full")) == (42, 8106, 0)
    assert SC.scan_shape(SC.case("seg_first")) == (43, 8299, 5) and 8299 - 4 * 2048 == 107
    assert SC.scan_shape(SC.case("seg_exact")) == (640, 10240, 5)
    assert SC.scan_shape(SC.case("skew")) == (43, 8299, 5)
    assert SC.scan_shape(SC.case("tile_edges")[-1])[:2] == (6, 60)
    # world 64: nearly every bucket is hit, so a wave's ballot loop sees tens of distinct keys
    for name in ("one_block_full", "seg_first"):
        sd = SC.case(name).ref.sends[0]
        assert (np.diff(sd.start) > 0).sum() >= 190, name
    # skew: one A and one B bucket hold every request of two sources, > 4,096 (the recv and answer
    # grids' 16 blocks of 256 threads) from each
    ref = SC.case("skew").ref
    for s in (0, 1):
        nq = ref.sends[s].nq
        assert sorted(nq[nq > 0].tolist()) == [10_753, 10_753] and (nq[:, 2] == 0).all()
    assert [c.ref.sends[0].one for c in SC.case("split_plan")] == [True, False]
    assert all(c.ref.sends[0].one for c in SC.case("one_key"))


@pytest.mark.parametrize("name", SC.SMALL_CASES)
def test_host_mode(name):
    for c in SC.cases_of(name):
        SC.run_case(c, -1)


def test_host_mode_handles_reused():
    """Two steps back to back on the same handles (seg_first twice over other topics), then a
    smaller table on them."""
    c = SC.case("seg_first")
    w = SC.World(c.world, c.plan, -1)
    try:
        for name in ("seg_first", "seg_first_again", "one_block_full"):
            SC.run_case(SC.case(name), -1, world=w)
    finally:
        w.close()


@pytest.mark.parametrize("kind", SC.FIXED_CASES)
def test_host_mode_fixed_world3(kind):
    SC.run_fixed(SC.case("fixed3"), kind, -1)


def test_host_mode_fixed_fits_world64():
    SC.run_fixed(SC.case("fixed64"), "fits", -1)


def test_host_mode_fixed_padded_ids_world64():
    SC.run_fixed(SC.case("fixed64"), "padded_ids", -1)


def sparse_slots(c):
    """The (rank, slot) pairs of case c that no source asks and that the padded kinds give topics."""
    extra = SC.pad_extras(c)
    return [(r, e) for r in range(c.world) for e in range(SC.E) if not c.ref.q0(r, e)[c.world] and extra[r][e]]


@pytest.mark.parametrize("kind", ("padded", "padded_ids"))
def test_host_mode_fixed_padded_sparse(kind):
    """A small batch in large capacities (fixed3 and fixed64 leave no slot without requests): slots
    that hold padding topics only."""
    c = SC.case("fixed3_sparse")
    assert len(sparse_slots(c)) >= 2
    SC.run_fixed(c, kind, -1)


def test_padded_shapes():
    """The padded kinds' arithmetic: 0, 1 and 17 padding topics on every rank, and on rank 1's
    slot 0 more than the recv grid's stride for that rank's capacities (a second trip of the
    padding block); `padded_ids` gives the padding thousands of ids."""
    for name, long in (("fixed3", 1024), ("fixed64", 512), ("fixed3_sparse", 512)):
        c = SC.case(name)
        extra = SC.pad_extras(c)
        fx = SC.fixed_caps(c, "padded_ids")
        r, e = SC.PAD_LONG
        assert extra[r][e] == long > R.recv_stride(c.world, fx["capq"][r], fx["capy"][r]), name
        assert all(sorted(row) == [0, 1, 17] for k, row in enumerate(extra) if k != r), name
        assert all(y % 16 == 0 for y in np.subtract(fx["capy"], SC.fixed_caps(c, "fits")["capy"]).ravel())
        assert SC.padded_ids_total(c) > 2 * long, name
    assert R.recv_stride(3, [400_000, 0, 0], [0, 0, 0]) == 256 * 174  # (44,445 items a part)
    assert R.recv_stride(3, [4_000_000, 0, 0], [0, 0, 0]) == 256 * 341  # the cap, 1024 / 3 blocks
    assert R.recv_stride(64, [0, 0, 0], [16 * 192 * 300, 0, 0]) == 256 * 2  # sized by the bytes


def test_host_mode_fixed_equals_classic():
    """`fits`: the fixed form's CSRs are the classic form's."""
    c = SC.case("fixed3")
    classic = SC.run_case(c, -1)
    fixed = SC.run_fixed(c, "fits", -1)
    for a, b in zip(classic.csr, fixed.csr):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
