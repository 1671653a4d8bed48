"""The publish fan-out (emqx_amd/csrc/fanout_kernels.hip, fanout.cpp) at chunk and block boundaries,
compared by position with the sequential restatement tests/fanout_ref.py on the synthetic match
CSRs of tests/fanout_cases.py (no engine, no workload generator).

Contract checked: out_off exactly; every match entry's deliveries at the entry's segment of the
output, its plain subscribers first (filter word = the filter id) and then one pick per $share
group (id | FANOUT_SHARED_BIT), so the filter words are compared word by word; inside the plain
part and inside the pick part the subscribers are compared as multisets (their order carries no
meaning; a pick names its group, the table's member sets being disjoint).  Every output buffer
is longer than the call may use and filled with a sentinel that must survive.

hash_clientid and round_robin (counter seeded 0: "rr_seed0") are exact; sticky and random are
checked by their invariants.  Tuning key "max_blocks" gives a block range several chunks and
makes every grid stride.  Untested: the 16 M-delivery side of the saturated count word, and a
chunk total past 32 bits."""

import types

import numpy as np
import pytest

from tests import fanout_cases as FC
from tests import fanout_ref as R

pytestmark = pytest.mark.gpu

T = FC.edge_table()
CASES = FC.cases()
PAD, OFF_PAD = 300, 8
SENT32, SENT64 = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A
F_OVERFLOW, F_MATCH, F_STATE_FULL, F_PICKS = 1, 2, 4, 8
SUM_FLAGS, SUM_TOTAL, SUM_ENTRIES = 0, 1, 2
MANY = 1 << 20  # publishers: about one per topic


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available()
    from emqx_amd import _lib, fanout
    g = types.SimpleNamespace(torch=torch, F=fanout, L=_lib, dev=torch.device("cuda:0"), inputs={}, tables={})
    g.stream = torch.cuda.Stream(device=g.dev)
    yield g
    for st in g.tables.values():
        st.close()


def table(G, max_blocks=None):
    st = G.F.SubTable(0)
    st.set_tuning("rr_seed0", 1)
    if max_blocks is not None:
        st.set_tuning("max_blocks", max_blocks)
    st.add(T.sub_filter, T.sub_id, T.sub_group_id)
    st.commit()
    return st


def shared_table(G, max_blocks=None):
    """For the stateless strategies: one table per grid cap for the module."""
    if max_blocks not in G.tables:
        G.tables[max_blocks] = table(G, max_blocks)
    return G.tables[max_blocks]


def up(G, a):
    a = np.ascontiguousarray(a)
    return G.torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.itemsize]).copy()).to(G.dev)


def dev_case(G, c):
    if c.name not in G.inputs:
        G.inputs[c.name] = (up(G, c.moff), up(G, c.mids))
    return G.inputs[c.name]


def run(G, st, c, keys, strategy, total, mode, cap=None, match_cap=None, filters=True):
    """One call with sentinel-filled outputs PAD (OFF_PAD) words longer than `total` (n + 1)."""
    torch = G.torch
    d_moff, d_mids = dev_case(G, c)
    d_keys = up(G, keys)
    size = total + PAD
    ooff = torch.full((c.n + 1 + OFF_PAD,), SENT64, dtype=torch.int64, device=G.dev)
    osubs = torch.full((size,), int(np.uint32(SENT32).view(np.int32)), dtype=torch.int32, device=G.dev)
    ofil = torch.full((size,), int(np.uint32(SENT32).view(np.int32)), dtype=torch.int32, device=G.dev)
    summ = torch.zeros(4, dtype=torch.int64, device=G.dev)
    cap = size if cap is None else cap
    got = types.SimpleNamespace(overflow=False, summary=None)
    torch.cuda.synchronize()
    if mode == "sync":
        try:
            got.total = st.fanout_device(strategy, d_moff.data_ptr(), d_mids.data_ptr(), c.n, d_keys.data_ptr(),
                                         ooff.data_ptr(), osubs.data_ptr(), ofil.data_ptr() if filters else None, cap)
        except G.L.EngineError as e:
            if e.code != G.L.EMQX_EOVERFLOW:
                raise
            got.overflow, got.total = True, e.needed
    else:
        st.fanout_device_async(strategy, d_moff.data_ptr(), d_mids.data_ptr(), c.n,
                               c.m if match_cap is None else match_cap, d_keys.data_ptr(), ooff.data_ptr(),
                               osubs.data_ptr(), ofil.data_ptr() if filters else None, cap, summ.data_ptr(),
                               stream=G.stream.cuda_stream)
        G.stream.synchronize()
        got.summary = summ.cpu().numpy().view(np.uint64)
        got.total = int(got.summary[SUM_TOTAL])
        got.overflow = bool(int(got.summary[SUM_FLAGS]) & F_OVERFLOW)
    torch.cuda.synchronize()
    got.off = ooff.cpu().numpy().view(np.uint64)
    got.subs = osubs.cpu().numpy().view(np.uint32)
    got.fils = ofil.cpu().numpy().view(np.uint32)
    return got


def first_bad(a, b):
    bad = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return None if not bad.size else (int(bad[0]), int(a[bad[0]]), int(b[bad[0]]), int(bad.size))


def check_offsets(c, r, got):
    assert first_bad(got.off[:c.n + 1], r.out_off) is None, first_bad(got.off[:c.n + 1], r.out_off)
    assert np.all(got.off[c.n + 1:] == SENT64), "out_off written past n + 1"


def check_untouched(got):
    assert np.all(got.subs == SENT32) and np.all(got.fils == SENT32), "ids written by a refused call"


def check_summary(c, r, got, flags=0):
    if got.summary is not None:
        assert int(got.summary[SUM_FLAGS]) == flags, int(got.summary[SUM_FLAGS])
        assert int(got.summary[SUM_TOTAL]) == r.total and int(got.summary[SUM_ENTRIES]) == c.m, got.summary


_LUT = np.full(max(T.sub_group) + 1, -1, np.int64)
_LUT[list(T.sub_group)] = list(T.sub_group.values())


def group_of(subs):
    """The uid of the group each subscriber is a member of (-1: of none)."""
    s = np.asarray(subs, np.int64)
    return np.where(s < len(_LUT), _LUT[np.minimum(s, len(_LUT) - 1)], -1)


def check(c, r, got, filters=True, exact=True):
    """The call's outputs against the restatement r; exact=False (sticky, random): a pick of a
    group of several members is compared by the group it is a member of."""
    assert not got.overflow and got.total == r.total, (got.total, r.total)
    check_offsets(c, r, got)
    check_summary(c, r, got)
    t = r.total
    assert np.all(got.subs[t:] == SENT32) and np.all(got.fils[t:] == SENT32), "ids written past the total"
    if filters:
        assert first_bad(got.fils[:t], r.fils) is None, ("filter word", first_bad(got.fils[:t], r.fils))
    else:
        assert np.all(got.fils == SENT32), "out_filters is null: nothing to write"
    exp, have = r.subs.astype(np.int64), got.subs[:t].astype(np.int64)
    if not exact:
        free = exp == R.NO_PICK
        pos = np.array(r.pick_pos, np.int64)
        uid = np.array([T.group_uid[fg] for fg in r.pick_fg], np.int64)
        exp[pos] = np.where(free[pos], -2 - uid, exp[pos])
        have = np.where(free, -2 - group_of(have), have)
    a, b = R.part_sorted(r.seg, have), R.part_sorted(r.seg, exp)
    assert first_bad(a, b) is None, ("subscriber (sorted inside its part)", first_bad(a, b))


VARIANTS = {"hash": (R.HASH_CLIENTID, 1 << 27), "rr1": (R.ROUND_ROBIN, 1), "rr3": (R.ROUND_ROBIN, 3),
            "rr_many": (R.ROUND_ROBIN, MANY), "sticky": (R.STICKY, 3), "random": (R.RANDOM, 3)}


def drive(G, name, variant, max_blocks=None, filters=True):
    """The case through both entry points.  hash: once each on the shared table.  round_robin: a
    table of its own; synchronous, asynchronous (the state carried over), the publishers forgotten,
    and both again.  sticky: two calls, every (group, publisher)'s pick constant; random: one."""
    c = CASES[name]
    strategy, publishers = VARIANTS[variant]
    keys = c.keys(publishers)
    ref = T.ref()
    if strategy == R.HASH_CLIENTID:
        st = shared_table(G, max_blocks)
        r = R.fanout(ref, c.moff, c.mids, keys, strategy, 1 << 40)
        for mode in ("sync", "async"):
            check(c, r, run(G, st, c, keys, strategy, r.total, mode, filters=filters), filters)
        return
    st = table(G, max_blocks)
    try:
        if strategy == R.ROUND_ROBIN:
            for call, mode in enumerate(("sync", "async", "sync", "async")):
                if call == 2:
                    st.forget_publishers(np.unique(keys))
                    ref.forget(np.unique(keys))
                r = R.fanout(ref, c.moff, c.mids, keys, strategy, 1 << 40)
                check(c, r, run(G, st, c, keys, strategy, r.total, mode, filters=filters), filters)
            return
        r = R.fanout(ref, c.moff, c.mids, keys, strategy, 1 << 40)
        stuck = {}
        for mode in ("sync", "async"):
            got = run(G, st, c, keys, strategy, r.total, mode, filters=filters)
            check(c, r, got, filters, exact=False)
            if strategy == R.STICKY:  # constant per (group, publisher) while alive, over calls too
                pos = np.array(r.pick_pos, np.int64)
                subs = got.subs[pos].tolist()
                for s, g, t in zip(subs, group_of(subs).tolist(), r.pick_topic):
                    assert stuck.setdefault((g, int(keys[t])), s) == s, (g, int(keys[t]))
    finally:
        st.close()


# every case but the pick-list and multi-pick ones (their bounds have tests of their own below)
GENERAL = (FC.COUNT_NAMES + FC.LEAD_TRAIL_NAMES + FC.BOUNDARY_NAMES + FC.TOPIC_NAMES + FC.CHUNK_NAMES +
           [FC.GROUPS_NAME] + FC.BASE_NAMES + FC.GRID_NAMES)
assert len(GENERAL) == len(set(GENERAL)) and set(GENERAL) | set(FC.PICK_NAMES + FC.MULTI_NAMES) == set(CASES)


@pytest.mark.parametrize("variant", ["hash", "rr1", "rr3", "rr_many"])
@pytest.mark.parametrize("name", GENERAL)
def test_positions_exact(G, name, variant):
    drive(G, name, variant)


def test_saturated_group_count_at_a_chunks_last_slot_sticky(G):
    """Filters of 254, 255 and 256 groups (the count word's group field saturates at 255) at slot
    255 of three chunks under the other stateful strategy (hash and round_robin: test_positions_exact)."""
    drive(G, FC.GROUPS_NAME, "sticky")


@pytest.mark.parametrize("strategy", ["sticky", "random"])
@pytest.mark.parametrize("name", FC.COUNT_RAND_NAMES + FC.CHUNK_NAMES + ["empties_at_256", "multi_4096"])
def test_invariant_strategies(G, name, strategy):
    """The pick is a member of its group, at its entry's pick part; a group of one member returns
    it; a sticky pick is constant per (group, publisher) over both calls."""
    drive(G, name, strategy)


@pytest.mark.parametrize("variant", ["hash", "rr_many"])
def test_null_out_filters(G, variant):
    """out_filters null: the same subscribers, nothing else written."""
    drive(G, "m513_rand", variant, filters=False)


def test_max_blocks_range(G):
    st = table(G)
    L = G.L.lib()
    for v in (0, -1, FC.FO_BLOCKS + 1, 1 << 40):
        assert L.emqx_subtab_set_tuning(st.handle, b"max_blocks", v) == G.L.EMQX_EINVAL, v
    for v in (1, FC.FO_BLOCKS):
        assert L.emqx_subtab_set_tuning(st.handle, b"max_blocks", v) == G.L.EMQX_OK, v
    st.close()


@pytest.mark.parametrize("variant", ["hash", "rr1", "rr_many", "sticky"])
@pytest.mark.parametrize("max_blocks", [1, 2, 3])
@pytest.mark.parametrize("name", FC.GRID_NAMES + [FC.GROUPS_NAME, "empty_lead_trail_300"])
def test_block_ranges_of_several_chunks(G, name, max_blocks, variant):
    """"max_blocks": 8 chunks as 4 + 4, as 3 + 3 + 2 and as one range; 66 chunks as one range (the
    earlier-chunks sum takes a second step per lane, the count kernel's waves five trips and more,
    the write kernel strides), $share groups in every chunk so that the pick list's base is summed
    from the chunks' pick counts; every capped grid strides (one publisher: long runs, the large
    resolve path after the first call's rerun; many: the small one)."""
    drive(G, name, variant, max_blocks)


@pytest.mark.parametrize("variant", ["hash", "rr_many"])
@pytest.mark.parametrize("mode", ["sync", "async"])
def test_capacity(G, variant, mode):
    """cap == total succeeds; cap == total - 1 is refused: the needed capacity, every offset, not
    one id, and no round_robin state consumed (the next call starts at member 0)."""
    c = CASES["m513_rand"]
    strategy, publishers = VARIANTS[variant]
    keys = c.keys(publishers)
    ref = T.ref()
    st = table(G)
    full = R.fanout(T.ref(), c.moff, c.mids, keys, strategy, 1 << 40)
    r = R.fanout(ref, c.moff, c.mids, keys, strategy, full.total - 1)
    assert r.overflow
    got = run(G, st, c, keys, strategy, r.total, mode, cap=r.total - 1)
    assert got.overflow and got.total == r.total
    check_offsets(c, r, got)
    check_untouched(got)
    check_summary(c, r, got, flags=F_OVERFLOW)
    r = R.fanout(ref, c.moff, c.mids, keys, strategy, full.total)
    assert np.array_equal(r.subs, full.subs)
    check(c, r, run(G, st, c, keys, strategy, r.total, mode, cap=r.total))
    st.close()


@pytest.mark.parametrize("name", ["m513_rand", "base_256"])
@pytest.mark.parametrize("variant", ["hash", "rr3"])
def test_async_match_cap(G, name, variant):
    """match_cap equal to the entries and well above them; one below: the call is refused with
    FO_SUM_F_MATCH, zero offsets, the raw entry count, no ids."""
    c = CASES[name]
    strategy, publishers = VARIANTS[variant]
    keys = c.keys(publishers)
    ref = T.ref()
    st = table(G)
    for match_cap in (c.m, 4 * c.m + 999):
        r = R.fanout(ref, c.moff, c.mids, keys, strategy, 1 << 40)
        check(c, r, run(G, st, c, keys, strategy, r.total, "async", match_cap=match_cap))
    got = run(G, st, c, keys, strategy, r.total, "async", match_cap=c.m - 1)
    assert int(got.summary[SUM_FLAGS]) == F_MATCH and int(got.summary[SUM_TOTAL]) == 0
    assert int(got.summary[SUM_ENTRIES]) == c.m
    assert not got.off[:c.n + 1].any() and np.all(got.off[c.n + 1:] == SENT64)
    check_untouched(got)
    r = R.fanout(ref, c.moff, c.mids, keys, strategy, 1 << 40)   # (and it consumed no state)
    check(c, r, run(G, st, c, keys, strategy, r.total, "async"))
    st.close()


def flagged_then_exact(G, name, untouched, follow="m513_rand"):
    """A call the pick list or the small resolve path cannot take: the asynchronous call raises
    FO_SUM_F_PICKS (untouched: and writes no id, the list being too short; the small path finds
    out after the write); the synchronous one reruns it and is exact, twice (no state was consumed
    by the refused attempts); a following call, whose path is chosen from the last call's counts,
    is exact again."""
    c = CASES[name]
    keys = c.keys(MANY)
    ref = T.ref()
    st = table(G)
    r = R.fanout(T.ref(), c.moff, c.mids, keys, R.ROUND_ROBIN, 1 << 40)
    got = run(G, st, c, keys, R.ROUND_ROBIN, r.total, "async")
    assert int(got.summary[SUM_FLAGS]) & F_PICKS and not int(got.summary[SUM_FLAGS]) & (F_OVERFLOW | F_MATCH)
    if untouched:
        check_untouched(got)
    for _ in range(2):
        r = R.fanout(ref, c.moff, c.mids, keys, R.ROUND_ROBIN, 1 << 40)
        check(c, r, run(G, st, c, keys, R.ROUND_ROBIN, r.total, "sync"))
    c = CASES[follow]
    keys = c.keys(3)
    for mode in ("sync", "async"):
        r = R.fanout(ref, c.moff, c.mids, keys, R.ROUND_ROBIN, 1 << 40)
        check(c, r, run(G, st, c, keys, R.ROUND_ROBIN, r.total, mode))
    st.close()


def accepted_at_bound(G, name):
    """A call exactly at a bound, asynchronous and first on a fresh table (nothing has grown the
    pick list, the small resolve path is chosen, and no synchronous rerun can hide a flag): the
    summary's flags are 0 and the call is exact; then the usual round_robin sequence goes on."""
    c = CASES[name]
    keys = c.keys(MANY)
    ref = T.ref()
    st = table(G)
    for call, mode in enumerate(("async", "sync", "async", "sync")):
        if call == 2:
            st.forget_publishers(np.unique(keys))
            ref.forget(np.unique(keys))
        r = R.fanout(ref, c.moff, c.mids, keys, R.ROUND_ROBIN, 1 << 40)
        check(c, r, run(G, st, c, keys, R.ROUND_ROBIN, r.total, mode))   # (async: flags == 0)
    st.close()


def test_pick_list_holds_65535_picks(G):
    """picks + 1 == the list's least capacity: the first, asynchronous call of a fresh table is
    not flagged (65 536 picks are: the next test)."""
    accepted_at_bound(G, "picks_65535")


def test_pick_list_65536_picks_flagged_and_rerun(G):
    flagged_then_exact(G, "picks_65536", True)


@pytest.mark.parametrize("M", [2, 3, 4096])
def test_small_path_multi_pick_runs(G, M):
    """M picks in runs of more than one, first and asynchronous on a fresh table (the small resolve
    path, not flagged: 4097 are, the next test): block 0's bitonic sort at sizes 2, 4 and 4096."""
    accepted_at_bound(G, "multi_%d" % M)


def test_small_path_4097_multi_pick_picks_rerun_on_the_large_path(G):
    flagged_then_exact(G, "multi_4097", False)
