"""The sharded step's kernels (emqx_amd/csrc/shard_step.hip) at the shapes the end-to-end tests
(tests/test_gpu_shard_step.py) never reach: worlds up to 64 (193 buckets: the ballot loops of
wave_count and shard_sort_scatter_kernel see tens of distinct keys a wave; recv and answer grids
capped at 16 blocks), the segmented sort scan (shard_seg_sums / seg_scan / seg_final, N > 8,192
table entries) next to the largest one-block table, second trips of unpack_part, answer_source,
shard_gather_kernel, shard_merge_kernel and shard_seg_scan_kernel, the fixed form's flags at
world > 1, and its padding topics (slot capacities above the need: the padding block of
shard_recv_fixed_kernel through a second trip, engine outputs that hold padding ids behind the
requests').  One process, no process group, no engines: tests/shard_cases.py drives the C API with
a synthetic matcher (its docstring lists the cases and the thresholds they sit on).

Every case runs on the device against the sequential restatement (tests/shard_ref.py: meta words
and send buffers by bytes over a sentinel, slot batches, final CSRs, flags) and byte for byte
against the host-mode run of the same case (send buffers, meta, answer chunks, output CSRs).  All
comparisons are exact."""

import functools
import os
import subprocess

import pytest

from tests import shard_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not os.path.exists(os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True, capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def host_run(name, i):  # the host-mode run of a case, once for every test that compares with it
    return SC.run_case(SC.cases_of(name)[i], -1)


def device_equals_host(name, world=None):
    for i, c in enumerate(SC.cases_of(name)):
        SC.same_bytes(SC.run_case(c, 0, world=world), host_run(name, i))


@pytest.mark.parametrize("name", SC.SMALL_CASES)
def test_device(name):
    device_equals_host(name)


def test_device_large():
    """1.1 M topics at world 64: 405 segments (two a thread in shard_seg_scan_kernel), 2.2 M
    requests (the second trip of shard_gather_kernel's 8,192 blocks), n > 524,288 (that of
    shard_merge_kernel's)."""
    c = SC.case("large")
    assert SC.scan_shape(c) == (4297, 829_321, 405) and c.ref.sends[0].m > 2_097_152
    device_equals_host("large")


def test_device_handles_reused():
    """Two steps back to back on the same handles (scratch sized by the first is reused), then the
    largest one-block table on them: one step object takes both scan paths."""
    c = SC.case("seg_first")
    w = SC.World(c.world, c.plan, 0)
    try:
        for name in ("seg_first", "seg_first_again", "one_block_full", "seg_first"):
            device_equals_host(name, world=w)
    finally:
        w.close()


@pytest.mark.parametrize("kind", SC.FIXED_CASES)
def test_device_fixed_world3(kind):
    c = SC.case("fixed3")
    got = SC.run_fixed(c, kind, 0)
    SC.same_bytes(got, SC.run_fixed(c, kind, -1))
    if kind == "fits":  # the same CSRs as the classic form
        classic = SC.run_case(c, 0)
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                   for a, b in zip(classic.csr, got.csr))


def test_device_fixed_fits_world64():
    c = SC.case("fixed64")
    SC.same_bytes(SC.run_fixed(c, "fits", 0), SC.run_fixed(c, "fits", -1))


def test_device_fixed_padded_ids_world64():
    """Padding topics with ids of their own at world 64 (the recv grid capped at 16 blocks: rank
    1's slot 0 is padded over two of its passes): answers and CSRs are the `fits` run's."""
    c = SC.case("fixed64")
    SC.same_bytes(SC.run_fixed(c, "padded_ids", 0), SC.run_fixed(c, "padded_ids", -1))


@pytest.mark.parametrize("kind", ("padded", "padded_ids"))
def test_device_fixed_padded_sparse(kind):
    """A small batch in large capacities: slots that hold padding topics only (what a rank's
    engines walk after a large batch taught the capacities)."""
    c = SC.case("fixed3_sparse")
    SC.same_bytes(SC.run_fixed(c, kind, 0), SC.run_fixed(c, kind, -1))
