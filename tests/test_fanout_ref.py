"""The fan-out restatement (tests/fanout_ref.py) against the oracle, and what the cases of
tests/fanout_cases.py assume: a case must keep exercising what it is named for."""

import numpy as np
import pytest

from oracle import cpp as C
from tests import fanout_cases as FC
from tests import fanout_ref as R

T = FC.edge_table()
CASES = FC.cases()
SMALL = [k for k, c in CASES.items() if c.base == 0 and c.m <= 2000]


def test_edge_table_is_what_the_cases_assume():
    ref = T.ref()
    fid = T.fid
    assert 24 <= T.n_recs <= 48                       # "a few dozen"
    assert ref.deliveries(fid["none"]) == 0
    for k in (1, 2, 3, 4, 7, 8, 9, 300, 1000):
        f = fid["p%d" % k]
        assert ref.n_plain(f) == k and ref.n_groups(f) == 0 and len(set(ref.plain[f])) == k
    # both sides of the inline record's head / ext split and of the inline / arena one
    assert FC.FO_INLINE_HEAD in (2, 3) and 4 > FC.FO_INLINE_HEAD and FC.FO_INLINE == 7
    assert [len(m) for m in ref.groups[fid["g1"]].values()] == [1]
    assert [len(m) for m in ref.groups[fid["g5"]].values()] == [5]
    assert sorted(len(m) for m in ref.groups[fid["g3x"]].values()) == [2, 3, 4]
    assert (ref.n_plain(fid["p1g1"]), ref.n_groups(fid["p1g1"])) == (1, 1)
    assert (ref.n_plain(fid["p7g1"]), ref.n_groups(fid["p7g1"])) == (7, 1)
    for k in (254, 255, 256):                         # the count word's group field saturates at 255
        g = ref.groups[fid["G%d" % k]]
        assert len(g) == k and ref.n_plain(fid["G%d" % k]) == 0
        assert {len(m) for m in g.values()} == {1, 2, 3}
    assert FC.FO_CNT_GROUPS_MAX == 255
    assert ref.n_plain(fid["p1000"]) > FC.FO_ROUND    # more outputs than one write round
    # a member names its group: disjoint member sets over the whole table, none a plain id
    members = [s for mem in T.group_members for s in mem]
    assert len(members) == len(set(members)) == len(T.sub_group)
    assert not set(members) & {s for p in ref.plain.values() for s in p}
    # subscription order is not id order (a sorted list would pick the same members otherwise)
    assert any(m != sorted(m) for m in T.group_members if len(m) > 1)
    assert T.beyond == [T.n_recs, T.n_recs + 1000, FC.FANOUT_ID_LIMIT - 1]
    assert all(ref.deliveries(f) == 0 for f in T.zero)
    # the rows are interleaved over the filters
    assert np.count_nonzero(np.diff(T.sub_filter.astype(np.int64))) > len(T.sub_filter) // 2


@pytest.mark.parametrize("name", list(CASES))
def test_case_assumptions(name):
    c = CASES[name]
    keys = c.keys(3)
    s = FC.stats(T.ref(), c, keys)
    assert c.n == len(c.moff) - 1 and int(c.moff[0]) == c.base and int(c.moff[-1]) == len(c.mids)
    assert s["m"] == c.m == int(c.moff[-1]) - c.base and s["chunks"] == -(-c.m // FC.FO_WCHUNK)
    for k in ("m", "chunks", "picks", "M"):
        if k in c.expect:
            assert s[k] == c.expect[k], (k, s[k])
    assert s["zero_chunks"] == c.expect.get("zero_chunks", ()), s["zero_chunks"]
    if c.expect.get("groups_in_every_chunk"):
        assert s["chunk_picks"].min() > 0
    if c.base:
        assert np.all(c.mids[:c.base] == T.fid["p1000"])
    assert c.mids.max() < FC.FANOUT_ID_LIMIT


def test_every_case_belongs_to_one_family():
    listed = [k for fam in FC.FAMILIES for k in fam]
    assert len(listed) == len(set(listed)) and set(listed) == set(CASES)
    assert set(FC.COUNT_RAND_NAMES) <= set(FC.COUNT_NAMES)


def test_named_positions():
    c, fid = CASES, T.fid
    for k in FC.COUNTS:
        assert c["m%d_one" % k].n == 1 and c["m%d_each" % k].n == k
        assert c["m%d_rand" % k].n == max(1, k // 3)
    assert any((np.diff(c["m%d_rand" % k].moff.astype(np.int64)) == 0).any() for k in FC.COUNTS)
    for k in FC.EMPTY_RUNS:
        cnt = np.diff(c["empty_lead_trail_%d" % k].moff.astype(np.int64))
        assert not cnt[:k].any() and not cnt[len(cnt) - k:].any() and cnt[k] and cnt[len(cnt) - k - 1]
    assert FC.EMPTY_RUNS == (0, 1, 70, 300)           # none, one, > a wave of topics, > a block
    mo = c["empties_at_256"].moff.tolist()
    assert mo[2] == 256 and mo[2:8] == [256] * 6 and mo[1] < 256 < mo[8]
    mo = c["start_256_after_empties"].moff.tolist()
    assert mo[1:72] == [256] * 71 and mo[72] > 256
    mo = c["end_256"].moff.tolist()
    assert 256 in mo[1:-1] and len(set(mo)) == len(mo)
    mo = c["topic_over_256"].moff.tolist()
    assert mo[1] == 255 and mo[2] == 257
    mo = c["topic_three_chunks"].moff.tolist()
    assert mo[1] // 256 == 0 and mo[2] // 256 == 2 and (mo[1] + 255) // 256 == 1
    for n in FC.TOPIC_COUNTS:
        assert c["topics_%d" % n].n == n
    big = fid["p1000"]
    assert c["big_slot0"].mids[256] == big and c["big_slot255"].mids[511] == big
    z = c["big_between_zero_runs"].mids
    assert z[356] == big and set(z[256:356].tolist()) == {fid["none"]} and set(z[357:512].tolist()) == set(T.beyond)
    g = c["many_groups_last_slot"].mids
    assert (g[255], g[511], g[767]) == (fid["G255"], fid["G256"], fid["G254"])
    assert [CASES["base_%d" % b].base for b in FC.BASES] == [5, 256, 1_000_003]
    used = set(np.concatenate([x.mids[x.base:] for x in CASES.values()]).tolist())
    assert used >= set(T.beyond) | set(range(T.n_recs))  # every filter and every id beyond is used


def test_block_ranges_under_max_blocks():
    """The split the "max_blocks" cases are built for (fo_per_block restated)."""
    m8, m66 = CASES["grid_8_chunks"].m, CASES["grid_66_chunks"].m
    assert m8 == 7 * 256 + 5 and m66 == 65 * 256 + 5
    assert FC.block_chunks(m8, 2) == [4, 4] and FC.block_chunks(m8, 3) == [3, 3, 2]
    assert FC.block_chunks(m8, 1) == [8] and FC.block_chunks(m66, 1) == [66]
    # one block: 66 chunks over four waves (a fifth trip and more), the sum over the block's
    # earlier chunks takes a second step per lane past 64 of them
    assert 66 > 4 * 4 and 65 > 64
    assert sum(FC.block_chunks(m66, FC.FO_BLOCKS)) == 66 and max(FC.block_chunks(m66, FC.FO_BLOCKS)) == 1
    # bitonic sizes of the small path's sort
    for M, P in ((2, 2), (3, 4), (4096, 4096)):
        assert CASES["multi_%d" % M].expect["M"] == M and 1 << (M - 1).bit_length() == P
    assert CASES["multi_4097"].expect["M"] == FC.FO_MULTI_CAP + 1


def _oracle():
    return C.FanoutOracle(T.sub_filter, T.sub_id, T.sub_group_id)


@pytest.mark.parametrize("name", SMALL)
def test_hash_equals_oracle(name):
    c = CASES[name]
    keys = c.keys(1 << 27)
    r = R.fanout(T.ref(), c.moff, c.mids, keys, R.HASH_CLIENTID, 1 << 40)
    off, subs, fils = _oracle().publish_list(c.moff, c.mids, keys)
    assert np.array_equal(off, r.out_off) and r.total == len(subs)
    assert R.by_topic(r.out_off, r.subs, r.fils) == R.by_topic(off, subs, fils)
    # the oracle lists a topic in route order, entry by entry: the entries' parts agree too
    assert np.array_equal(fils, r.fils)
    assert np.array_equal(R.part_sorted(r.seg, subs), R.part_sorted(r.seg, r.subs))


@pytest.mark.parametrize("publishers", [1, 3, 1 << 20])
@pytest.mark.parametrize("name", [k for k in SMALL if k not in FC.COUNT_NAMES or k in FC.COUNT_RAND_NAMES])
def test_round_robin_equals_oracle(name, publishers):
    c = CASES[name]
    keys = c.keys(publishers)
    ref, fo = T.ref(), _oracle()
    for call in range(3):
        if call == 2:
            ref.forget(np.unique(keys))
            fo.rr_reset()
        r = R.fanout(ref, c.moff, c.mids, keys, R.ROUND_ROBIN, 1 << 40)
        off, subs, fils = fo.publish_list(c.moff, c.mids, keys, round_robin=True)
        assert np.array_equal(off, r.out_off) and np.array_equal(fils, r.fils)
        assert np.array_equal(R.part_sorted(r.seg, subs), R.part_sorted(r.seg, r.subs)), call


def test_overflow_consumes_nothing_and_invariant_strategies_make_no_pick():
    c = CASES["m257_rand"]
    keys = c.keys(3)
    ref = T.ref()
    full = R.fanout(T.ref(), c.moff, c.mids, keys, R.ROUND_ROBIN, 1 << 40)
    over = R.fanout(ref, c.moff, c.mids, keys, R.ROUND_ROBIN, full.total - 1)
    assert over.overflow and over.subs is None and over.total == full.total and not ref.rr
    assert np.array_equal(over.out_off, full.out_off)
    again = R.fanout(ref, c.moff, c.mids, keys, R.ROUND_ROBIN, full.total)
    assert not again.overflow and np.array_equal(again.subs, full.subs)
    s = R.fanout(ref, c.moff, c.mids, keys, R.STICKY, 1 << 40)
    pos = np.array(s.pick_pos)
    one = np.array([len(T.group_members[T.group_uid[fg]]) == 1 for fg in s.pick_fg])
    assert len(pos) == FC.stats(ref, c)["picks"] and np.all(s.subs[pos[~one]] == R.NO_PICK)
    assert np.all(s.subs[pos[one]] != R.NO_PICK) and np.all(s.fils[pos] & R.SHARED_BIT)
