"""The named cases of the inbox stage, shared by the CPU and the GPU tests: the smallest shapes at
which the passes can go wrong.  Every case carries opts and subids, so a test may leave either
out; the expected outputs come from tests/inbox_ref.py, computed once a case."""

import functools
from typing import NamedTuple, Optional

import numpy as np

from tests import inbox_ref as R

SUMMARY = ("flags", "deliveries", "inboxes", "longest", "messages", "r5", "r6", "r7")
T = 2048  # checked against emqx_amd.inbox.TILE and emqx_amd/csrc/inbox.h by tests/test_inbox_cpu.py


class Case(NamedTuple):
    name: str
    offsets: np.ndarray
    subs: np.ndarray
    filters: np.ndarray
    sub_limit: int
    opts: np.ndarray
    subids: np.ndarray

    @property
    def n(self):
        return self.offsets.size - 1

    @property
    def total(self):
        return self.subs.size

    def args(self, opts=True, subids=True):
        """Positional and keyword arguments of Inbox.group / group_host."""
        return (self.offsets, self.subs, self.filters, self.sub_limit), {
            "opts": self.opts if opts else None, "subids": self.subids if subids else None}

    def reference(self, opts=True, subids=True, cap_boxes=None, cap_in=None):
        return _reference(self.name, opts, subids, cap_boxes, cap_in)


_CASES = {}


@functools.lru_cache(maxsize=None)
def _reference(name, opts, subids, cap_boxes, cap_in):
    c = _CASES[name]
    return R.group(c.offsets, c.subs, c.filters, c.sub_limit, c.opts if opts else None, c.subids if subids else None,
                   cap_boxes=cap_boxes, cap_in=cap_in)


def _offsets(total, rng, n_hint=None):
    """Messages of mixed sizes with empty ones among them, summing to `total`."""
    sizes = []
    left = total
    while left:
        k = int(min(left, rng.choice([0, 1, 1, 2, 7, 70, 300])))
        sizes.append(k)
        left -= k
    if n_hint:
        sizes += [0] * max(0, n_hint - len(sizes))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _case(name, offsets, subs, sub_limit, filters=None, seed=1):
    rng = np.random.default_rng(seed)
    subs = np.asarray(subs, dtype=np.uint32)
    k = subs.size
    if filters is None:
        filters = rng.integers(0, 1 << 30, size=k, dtype=np.uint32)
        filters |= np.where(rng.random(k) < 0.2, R.SHARED_BIT, 0).astype(np.uint32)
    c = Case(name, np.asarray(offsets, dtype=np.uint64), subs, np.asarray(filters, dtype=np.uint32), int(sub_limit),
             rng.integers(0, 256, size=k, dtype=np.uint8), rng.integers(0, 1 << 28, size=k, dtype=np.uint32))
    assert int(c.offsets[-1]) == k and c.offsets[0] == 0
    _CASES[name] = c
    return c


# ---- 0 and 1 deliveries --------------------------------------------------------------------
def tiny(name):
    if name == "n0":
        return _case("n0", [0], [], 16)
    if name == "n3_total0":
        return _case("n3_total0", [0, 0, 0, 0], [], 16)
    assert name == "one"
    return _case("one", [0, 0, 1], [5], 16)


TINY_CASES = ["n0", "n3_total0", "one"]

# ---- the wave and tile boundaries ----------------------------------------------------------
TOTALS = [63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
MODES = ["one_sub", "distinct_desc", "alternating"]
SHAPE_CASES = [(t, m) for t in TOTALS for m in MODES]


def shape(total, mode):
    name = "shape_%d_%s" % (total, mode)
    rng = np.random.default_rng(total)
    if mode == "one_sub":  # stability across waves, rows and tiles: the output is the input order
        subs, limit = np.full(total, 300), 1000
    elif mode == "distinct_desc":  # every delivery its own inbox, the whole order reversed
        subs, limit = np.arange(total - 1, -1, -1), total
    else:  # two inboxes interleaved, the ids two digits apart
        subs, limit = np.where(np.arange(total) % 2 == 0, 0x10203, 3), 1 << 17
    return _case(name, _offsets(total, rng), subs, limit, seed=total)


# ---- digit edges ---------------------------------------------------------------------------
SUB_LIMITS = [1, 2, 255, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 1 << 32]


def digit_edge(sub_limit):
    """Ids that differ only in the lowest digit, ids that differ only in the highest digit in
    use, and 0, sub_limit - 1 (and 0xFFFFFFFE below 2^32), shuffled with repeats."""
    top = sub_limit - 1
    shift = 8 * ((max(top.bit_length(), 1) - 1) // 8)  # of the highest digit in use
    ids = {0, top}
    ids |= {(top & ~0xFF) | x for x in (0, 1, 0x7F, 0x80, 0xFE, 0xFF) if ((top & ~0xFF) | x) <= top}
    low = 0x5A5A5A5A & ((1 << shift) - 1)
    ids |= {(v << shift) | low for v in range(0, (top >> shift) + 1, max(1, (top >> shift) // 5))
            if ((v << shift) | low) <= top}
    if sub_limit == 1 << 32:
        ids.add(0xFFFFFFFE)
    ids = sorted(ids)
    rng = np.random.default_rng(sub_limit % 1000003)
    subs = rng.choice(np.array(ids, dtype=np.uint64), size=200).astype(np.uint32)
    subs[:len(ids)] = np.array(ids[::-1], dtype=np.uint32)  # each at least once, descending
    return _case("digit_%d" % sub_limit, _offsets(200, rng), subs, sub_limit, seed=7)


# ---- order inside an inbox -----------------------------------------------------------------
def two_filters():
    """Message 1 reaches subscriber 9 through two filters (one of them a $share pick on its
    retry): both deliveries stay, in input order, the bits untouched."""
    offsets = [0, 2, 6, 7]
    subs = [9, 4, 9, 7, 9, 4, 9]
    filters = [11, 12, 21 | R.SHARED_BIT | R.RETRY_BIT, 22, 23, 24 | R.SHARED_BIT, 31 | R.RETRY_BIT]
    return _case("two_filters", offsets, subs, 10, filters=filters)


def empty_messages():
    """Empty messages at the start, in the middle (runs of equal offsets) and at the end."""
    offsets = [0, 0, 0, 3, 3, 3, 3, 5, 70, 70, 71, 71, 71]
    rng = np.random.default_rng(11)
    return _case("empty_messages", offsets, rng.integers(0, 6, size=71), 6)


# ---- fuzz ----------------------------------------------------------------------------------
def fuzz():
    """300 messages, about 5 000 deliveries over 1 000 subscribers, Zipf: one inbox of hundreds."""
    rng = np.random.default_rng(2024)
    sizes = rng.poisson(17, size=300)
    sizes[rng.random(300) < 0.1] = 0
    total = int(sizes.sum())
    subs = np.minimum(rng.zipf(1.3, size=total) - 1, 999)
    return _case("fuzz", np.concatenate([[0], np.cumsum(sizes)]), subs, 1000, seed=3)


def fuzz_wide():
    """About 8 T deliveries over 2^20 ids: three passes, several tiles."""
    rng = np.random.default_rng(2025)
    total = 8 * T + 37
    subs = rng.integers(0, 1 << 20, size=total)
    subs[rng.random(total) < 0.05] = (1 << 20) - 1  # one inbox that spans tiles
    return _case("fuzz_wide", _offsets(total, rng), subs, 1 << 20, seed=4)


# ---- comparison ----------------------------------------------------------------------------
def check(ref, got, opts=True, subids=True, src=True):
    """Every output array and the summary exactly."""
    assert [got.summary[k] for k in SUMMARY] == ref["summary"]
    assert got.inbox_subs.tolist() == ref["inbox_subs"]
    assert got.inbox_offsets.tolist() == ref["inbox_offsets"]
    assert got.msgs.tolist() == ref["msgs"]
    assert got.filters.tolist() == ref["filters"]
    if opts:
        assert got.opts.tolist() == ref["opts"]
    else:
        assert got.opts is None
    if subids:
        assert got.subids.tolist() == ref["subids"]
    else:
        assert got.subids is None
    if src:
        assert got.src.tolist() == ref["src"]
    else:
        assert got.src is None


def same(a, b):
    """Two results byte for byte."""
    assert a.summary == b.summary
    for x, y in zip(a[:-1], b[:-1]):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
