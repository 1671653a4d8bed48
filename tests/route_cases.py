"""Named cases of the route stage (include/emqx_route.h), shared by tests/test_route_cpu.py (the
host evaluator) and tests/test_gpu_route.py (the device forms).  A case is a route table given as
``(filter id, node id, group id or None)`` triples in insertion order, this node's id and a match
CSR.  The expected result comes from tests/route_ref.py, once per case.

Sizes are the smallest at which the kernels take another path: a tile holds 2 048 entries, a
wave 64 consecutive ones, a node is a mask bit 0..63.
"""

from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from tests import route_ref as R

TILE = 2048
NO_GROUP = 0xFFFFFFFF


class Case(NamedTuple):
    name: str
    local: int
    dests: Tuple[Tuple[int, int, Optional[int]], ...]
    offsets: np.ndarray  # uint64 [n + 1]
    filters: np.ndarray  # uint32


def node_name(v: int) -> str:
    return "n%02d@emqx" % v


def group_name(g: int) -> bytes:
    return b"g%d" % g


def filter_name(f: int) -> bytes:
    return b"t/%d/+" % f


def ref_table(case: Case) -> Tuple[R.RouteTab, Dict[int, bytes]]:
    tab = R.RouteTab(node_name(case.local))
    names: Dict[int, bytes] = {}
    for f, v, g in case.dests:
        names[f] = filter_name(f)
        tab.do_add_route(names[f], node_name(v) if g is None else (group_name(g), node_name(v)))
    return tab, names


def _csr(counts, filters) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(counts, dtype=np.uint64))
    f = np.asarray(filters, dtype=np.uint32).reshape(-1)
    assert int(off[-1]) == f.size
    return off, f


def _split(rng, total: int, n: int) -> List[int]:
    """n message sizes summing to total, some of them 0."""
    if n == 0:
        return []
    cuts = np.sort(rng.integers(0, total + 1, size=n - 1))
    return np.diff(np.concatenate(([0], cuts, [total]))).astype(int).tolist()


def small_table(rng, n_filters: int, n_nodes: int) -> List[Tuple[int, int, Optional[int]]]:
    """Every kind of filter over n_nodes nodes: one plain node, several, grouped only, mixed, and
    ids without a dest in between."""
    dests: List[Tuple[int, int, Optional[int]]] = []
    for f in range(n_filters):
        kind = f % 7
        if kind == 6:
            continue  # a hole: the id has a slot and no dest
        v = int(rng.integers(0, n_nodes))
        if kind in (0, 1, 2):
            dests.append((f, v, None))
        elif kind == 3:
            for w in sorted({v, int(rng.integers(0, n_nodes)), int(rng.integers(0, n_nodes))}):
                dests.append((f, w, None))
        elif kind == 4:
            dests.append((f, v, f % 3))
            dests.append((f, (v + 1) % n_nodes, f % 3))
        else:
            dests.append((f, v, None))
            dests.append((f, (v + 1) % n_nodes, 5))
            dests.append((f, (v + 1) % n_nodes, None))
    return dests


def _sized(total: int, n: int, seed: int, n_nodes: int = 3, local: int = 1) -> Case:
    rng = np.random.default_rng(seed)
    dests = small_table(rng, 40, n_nodes)
    off, f = _csr(_split(rng, total, n), rng.integers(0, 42, size=total))
    return Case("total_%d_n_%d" % (total, n), local, tuple(dests), off, f)


def fuzz(seed: int, n_msgs: int = 300, total: int = 5000, n_nodes: int = 9, n_filters: int = 700) -> Case:
    rng = np.random.default_rng(1000 + seed)
    local = int(rng.integers(0, n_nodes))
    dests: List[Tuple[int, int, Optional[int]]] = []
    for f in range(n_filters):
        r = rng.random()
        if r < 0.04:
            continue
        nodes = {int(rng.integers(0, n_nodes))}
        if r < 0.30:
            nodes |= {int(x) for x in rng.integers(0, n_nodes, size=int(rng.integers(1, 4)))}
        if r > 0.995:
            nodes = set(range(n_nodes))
        if not 0.80 < r < 0.86:  # those are grouped only
            dests += [(f, v, None) for v in sorted(nodes)]
        if r > 0.80 and r < 0.92:
            for g in {int(x) for x in rng.integers(0, 6, size=int(rng.integers(1, 3)))}:
                dests += [(f, int(v), g) for v in rng.integers(0, n_nodes, size=int(rng.integers(1, 3)))]
    order = rng.permutation(len(dests))  # insertion order is not id order
    dests = [dests[k] for k in order]
    dests = list(dict.fromkeys(dests))
    sizes = _split(rng, total, n_msgs)
    ids = rng.integers(0, n_filters + 8, size=total).astype(np.uint32)
    ids[rng.integers(0, total, size=5)] = 0xFFFFFFFF
    off, f = _csr(sizes, ids)
    # the fuzz must not drift into an easy table
    plain: Dict[int, set] = {}
    for fid, v, g in dests:
        if g is None:
            plain.setdefault(fid, set()).add(v)
    forwarding = sum(1 for x in f.tolist() if plain.get(x, set()) - {local})
    assert forwarding * 3 >= total, (forwarding, total)
    assert sum(1 for s in plain.values() if len(s) >= 2) * 20 >= n_filters, "two or more plain nodes"
    return Case("fuzz_%d" % seed, local, tuple(dests), off, f)


def _all() -> List[Case]:
    cases: List[Case] = []
    for k, total in enumerate((0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)):
        cases.append(_sized(total, 7 if total else 3, seed=k))
    rng = np.random.default_rng(77)
    table = tuple(small_table(rng, 40, 3))
    # one message owns every entry across tiles
    off, f = _csr([3 * TILE + 5], rng.integers(0, 42, size=3 * TILE + 5))
    cases.append(Case("one_message", 0, table, off, f))
    # runs of empty messages at the front, in the middle and at the end
    sizes = [0, 0, 0, 5, 70, 0, 0, 0, 0, TILE, 1, 0, 0]
    off, f = _csr(sizes, rng.integers(0, 42, size=sum(sizes)))
    cases.append(Case("empty_runs", 2, table, off, f))
    cases.append(Case("no_messages", 0, table, np.zeros(1, np.uint64), np.zeros(0, np.uint32)))
    # node counts and placement
    one = tuple((f_, 0, None) for f_ in range(20)) + ((20, 0, 1),)
    off, f = _csr([30, 0, 40], rng.integers(0, 22, size=70))
    cases.append(Case("one_node", 0, one, off, f))
    two = tuple((f_, f_ % 2, None) for f_ in range(20)) + ((3, 0, None), (4, 1, None))
    cases.append(Case("two_nodes_local_0", 0, two, off, f))
    cases.append(Case("two_nodes_local_1", 1, two, off, f))
    for local in (0, 31, 63):
        wide = [(f_, f_ % 64, None) for f_ in range(100)]
        wide += [(100, v, None) for v in range(64)]          # routed to every node ...
        wide += [(101, v, None) for v in range(0, 64, 3)]
        sizes = [64, 1, 130, 0, 64 * 5]
        ids = rng.integers(0, 100, size=sum(sizes))
        ids[[3, 64 + 1 + 17, 64 + 1 + 64 + 2, 300]] = 100    # ... beside single-node filters in one wave
        ids[[10, 301]] = 101
        off64, f64 = _csr(sizes, ids)
        cases.append(Case("64_nodes_local_%d" % local, local, tuple(wide), off64, f64))
    # groups
    groups = (
        (0, 1, 7), (0, 2, 7),                       # one group on two nodes: counts 1
        (1, 0, 3),                                  # only a grouped dest, on this node
        (2, 1, 3), (2, 1, 4), (2, 2, 4),            # two groups
        (3, 0, None), (3, 2, None), (3, 1, 9),      # plain local, plain remote and a group
        (4, 2, 1), (4, 2, None),                    # a group and a plain route on the same remote node
    )
    off, f = _csr([5, 3, 0, 4], [0, 1, 2, 3, 4, 3, 3, 0, 4, 2, 1, 5])
    cases.append(Case("groups", 0, groups, off, f))
    # ids the table does not know: one past the slot count, 2^30, 0xFFFFFFFF
    off, f = _csr([4, 3], [4, 5, 1 << 30, 0xFFFFFFFF, 5, 3, 6])
    cases.append(Case("unknown_ids", 0, groups, off, f))
    # a filter id twice in one message: it forwards twice and counts twice
    off, f = _csr([5, 2], [3, 4, 3, 0, 0, 3, 3])
    cases.append(Case("duplicate_filter", 0, groups, off, f))
    cases += [fuzz(s) for s in (1, 2, 3)]
    return cases


CASES: List[Case] = _all()
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def expected(name: str) -> R.Expected:
    """The reference's answer, computed once and shared (read-only)."""
    c = BY_NAME[name]
    tab, names = ref_table(c)
    return R.route_batch(tab, names, c.offsets.tolist(), c.filters.tolist())


def fill_table(table, case: Case) -> None:
    """The case's dests into an emqx_amd.route.RouteTable, in insertion order, and a commit."""
    if case.dests:
        f, v, g = zip(*case.dests)
        table.add(list(f), list(v), [NO_GROUP if x is None else x for x in g])
    table.commit()


def check(case: Case, got, exp: Optional[R.Expected] = None) -> None:
    """`got` (an emqx_amd.route.Routed) against the reference, exactly."""
    exp = expected(case.name) if exp is None else exp
    n = len(case.offsets) - 1
    assert got.entry_flags.tolist() == exp.entry_flags, case.name
    assert got.msg_routes.tolist() == exp.msg_routes, case.name
    assert int(got.node_offsets[0]) == 0 and got.node_offsets.size == 65
    for v in range(64):
        msgs, fils = got.forwards(v)
        assert list(zip(msgs.tolist(), fils.tolist())) == exp.forwards.get(node_name(v), []), (case.name, v)
    assert int(got.node_offsets[64]) == exp.summary["forwards"] == got.fwd_msgs.size
    lo = got.local_offsets
    assert lo.size == n + 1 and int(lo[0]) == 0
    assert [got.local_filters[int(lo[i]):int(lo[i + 1])].tolist() for i in range(n)] == exp.local, case.name
    assert got.summary == exp.summary, (case.name, got.summary, exp.summary)
