"""The edge table and the synthetic match CSRs of the fan-out edge tests (test_fanout_ref.py on the
CPU, test_gpu_fanout_edges.py on the device).  No project code: the layout constants are restated
from emqx_amd/csrc/fanout.h, and test_fanout_ref.py asserts what every case assumes of them."""

import functools

import numpy as np

from tests import fanout_ref as R

FANOUT_ID_LIMIT = 0x40000000
FO_BLOCKS, FO_WCHUNK = 1024, 256
FO_INLINE, FO_INLINE_HEAD = 7, 3
FO_CNT_GROUPS_MAX = 255
FO_ROUND = 64 * 4          # outputs of one write round (64 lanes x FO_UNROLL)
FO_MULTI_CAP = 4096
PK_CAP_MIN = 1 << 16       # the pick list's least capacity; a call's picks + 1 must fit


def _cyc(k):               # k groups of 1..3 members
    return tuple(1 + i % 3 for i in range(k))


# name, plain subscribers, members of each $share group
SPECS = [("none", 0, ())]
SPECS += [("p%d" % k, k, ()) for k in (1, 2, 3, 4, 7, 8, 9, 300, 1000)]   # inline: 1..7; arena: 8..
SPECS += [("g1", 0, (1,)), ("g5", 0, (5,)), ("g3x", 0, (2, 3, 4)), ("p1g1", 1, (2,)), ("p7g1", 7, (3,))]
SPECS += [("G254", 0, _cyc(254)), ("G255", 0, _cyc(255)), ("G256", 0, _cyc(256))]
SPECS += [("mix%d" % k, 1 + k % 4, tuple(2 + (k + i) % 3 for i in range(k % 3))) for k in range(10)]


class EdgeTable:
    """Rows in a shuffled subscription order (so that a list's order is not its ids' order).  Every
    $share member id belongs to exactly one group of the whole table: a pick names its group."""

    def __init__(self, seed=20):
        rng = np.random.default_rng(seed)
        self.fid = {name: i for i, (name, _, _) in enumerate(SPECS)}
        self.n_recs = len(SPECS)
        n_members = sum(sum(g) for _, _, g in SPECS)
        member_ids = iter((10_000 + rng.permutation(n_members)).tolist())
        rows, self.group_uid, self.group_members = [], {}, []
        self.sub_group = {}                      # member id -> uid of its group
        for f, (_, n_plain, groups) in enumerate(SPECS):
            rows += [(f, int(s), R.NO_GROUP) for s in rng.choice(4000, size=n_plain, replace=False)]
            for g, k in enumerate(groups):
                uid = self.group_uid[(f, g)] = len(self.group_members)
                mem = [next(member_ids) for _ in range(k)]
                self.group_members.append(mem)
                for s in mem:
                    self.sub_group[s] = uid
                    rows.append((f, s, g))
        rows = [rows[i] for i in rng.permutation(len(rows))]
        self.sub_filter, self.sub_id, self.sub_group_id = (np.array(x, np.uint32) for x in zip(*rows))
        # ids beyond the table: the first, one far past it, the largest a CSR may hold
        self.beyond = [self.n_recs, self.n_recs + 1000, FANOUT_ID_LIMIT - 1]
        light = [n for n, p, g in SPECS if p <= 9 and len(g) <= 3]
        self.light = [self.fid[n] for n in light] + self.beyond
        self.common = self.light + [self.fid["p300"]]
        self.zero = [self.fid["none"]] + self.beyond

    def ref(self):
        """A restatement table of its own (fresh round_robin state)."""
        return R.Table(self.sub_filter, self.sub_id, self.sub_group_id)


@functools.lru_cache(maxsize=None)
def edge_table():
    return EdgeTable()


class Case:
    def __init__(self, name, counts, mids, base=0, keys=None, **expect):
        self.name = name
        counts = np.asarray(counts, np.int64)
        self.n, self.m, self.base = len(counts), int(counts.sum()), base
        assert self.m == len(mids), name
        self.moff = (base + np.concatenate([[0], np.cumsum(counts)])).astype(np.uint64)
        # entries before the CSR's base belong to another call: a heavy filter, never to be read
        self.mids = np.concatenate([np.full(base, edge_table().fid["p1000"]), np.asarray(mids)]).astype(np.uint32)
        self.fixed_keys = None if keys is None else np.asarray(keys, np.uint32)
        self.expect = expect

    def keys(self, publishers):
        """Per-topic pick keys: one of `publishers` values (the phash2 key or the publisher)."""
        if self.fixed_keys is not None:
            return self.fixed_keys
        return np.random.default_rng(self.n * 31 + self.m).integers(0, publishers, size=self.n).astype(np.uint32)

    def __repr__(self):
        return self.name


def stats(table, case, keys=None):
    """What a case exercises, counted from a restatement table: entries, chunks, deliveries and
    picks per chunk, picks, and M = the picks of (filter, group, publisher) runs of more than one."""
    ent = case.mids[case.base:].tolist()
    d = np.array([table.deliveries(f) for f in ent], np.int64)
    g = np.array([table.n_groups(f) for f in ent], np.int64)
    chunks = (case.m + FO_WCHUNK - 1) // FO_WCHUNK
    pad = chunks * FO_WCHUNK - case.m
    cd = np.concatenate([d, np.zeros(pad, np.int64)]).reshape(chunks, FO_WCHUNK).sum(1)
    cg = np.concatenate([g, np.zeros(pad, np.int64)]).reshape(chunks, FO_WCHUNK).sum(1)
    out = {"m": case.m, "chunks": chunks, "chunk_deliveries": cd, "chunk_picks": cg, "picks": int(g.sum()),
           "zero_chunks": tuple(np.nonzero(cd == 0)[0].tolist())}
    if keys is not None:
        runs = {}
        moff = case.moff.astype(np.int64) - case.base
        for t in range(case.n):
            for f in ent[moff[t]:moff[t + 1]]:
                for grp in table.groups.get(f, ()):
                    k = (f, grp, int(keys[t]))
                    runs[k] = runs.get(k, 0) + 1
        out["M"] = sum(v for v in runs.values() if v > 1)
        out["runs"] = len(runs)
    return out


def per_block(m, blocks=FO_BLOCKS):
    """Entries of one block range: m split over `blocks`, rounded up to whole chunks."""
    return ((m + blocks - 1) // blocks + FO_WCHUNK - 1) // FO_WCHUNK * FO_WCHUNK


def block_chunks(m, blocks):
    per, chunks = per_block(m, blocks), (m + FO_WCHUNK - 1) // FO_WCHUNK
    return [min(chunks, (b + 1) * per // FO_WCHUNK) - min(chunks, b * per // FO_WCHUNK) for b in range(blocks)]


def _split(rng, m, how):
    if how == "one":
        return [m]
    if how == "each":
        return [1] * m
    n = max(1, m // 3)
    return np.bincount(rng.integers(0, n, size=m), minlength=n)   # some topics stay empty


def _pick(rng, pool, m):
    return np.asarray(pool, np.int64)[rng.integers(0, len(pool), size=m)]


COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
EMPTY_RUNS = (0, 1, 70, 300)
TOPIC_COUNTS = (1, 64, 65, 256, 257)
BASES = (5, 256, 1_000_003)


@functools.lru_cache(maxsize=None)
def cases():
    T = edge_table()
    fid = T.fid
    out = {}

    def add(c):
        assert c.name not in out
        out[c.name] = c

    # entry counts around the wave (64), the chunk (256) and the block of four chunks (1024)
    for m in COUNTS:
        for how in ("one", "each", "rand"):
            rng = np.random.default_rng(m * 3 + len(how))
            mids = _pick(rng, T.common, m)
            mids[-1] = fid["p7g1"]             # the last entry ends on plain ids and a pick
            add(Case("m%d_%s" % (m, how), _split(rng, m, how), mids, m=m))
    # topics without entries before and after the others: none, one, more than a wave of 64
    # topics, more than a block of 256
    for k in EMPTY_RUNS:
        rng = np.random.default_rng(100 + k)
        body = np.bincount(rng.integers(0, 40, size=300), minlength=40)
        body[0], body[-1] = max(body[0], 1), max(body[-1], 1)
        add(Case("empty_lead_trail_%d" % k, [0] * k + body.tolist() + [0] * k, _pick(rng, T.common, int(body.sum()))))
    rng = np.random.default_rng(7)
    add(Case("empties_at_256", [200, 56, 0, 0, 0, 0, 0, 44, 30], _pick(rng, T.common, 330)))
    add(Case("start_256_after_empties", [256] + [0] * 70 + [100], _pick(rng, T.common, 356)))
    add(Case("end_256", [100, 156, 144], _pick(rng, T.common, 400)))
    add(Case("topic_over_256", [255, 2, 43], _pick(rng, T.common, 300)))
    add(Case("topic_three_chunks", [100, 600, 100], _pick(rng, T.common, 800), chunks=4))
    for n in TOPIC_COUNTS:
        rng = np.random.default_rng(200 + n)
        c = rng.integers(0, 4, size=n)
        c[0] = max(c[0], 1)
        add(Case("topics_%d" % n, c, _pick(rng, T.common, int(c.sum()))))

    # inside the second of three chunks
    def three(name, fill, **expect):
        rng = np.random.default_rng(len(name))
        mids = _pick(rng, T.light, 3 * FO_WCHUNK)
        fill(mids, rng)
        add(Case(name, _split(rng, len(mids), "rand"), mids, chunks=3, **expect))

    def big_at(slot):
        def fill(mids, rng):
            mids[FO_WCHUNK + slot] = fid["p1000"]
        return fill

    def zero_runs(mids, rng):
        mids[256:356] = fid["none"]
        mids[356] = fid["p1000"]
        mids[357:512] = [T.beyond[i % 3] for i in range(155)]

    def zero_chunk(mids, rng):
        mids[256:512] = _pick(rng, T.zero, FO_WCHUNK)

    def groups_last_slot(mids, rng):
        mids[255], mids[511], mids[767] = fid["G255"], fid["G256"], fid["G254"]

    three("big_slot0", big_at(0))
    three("big_slot255", big_at(255))
    three("big_between_zero_runs", zero_runs)
    three("zero_chunk_between", zero_chunk, zero_chunks=(1,))
    three("many_groups_last_slot", groups_last_slot)
    # a CSR that is a slice of a longer one
    for b in BASES:
        rng = np.random.default_rng(300 + b % 1000)
        add(Case("base_%d" % b, _split(rng, 600, "rand"), _pick(rng, T.common, 600), base=b))
    # several chunks per block under "max_blocks": 8 chunks as 4 + 4 and 3 + 3 + 2; 66 chunks in
    # one block (the second step of the earlier-chunks sum, a fifth trip of the count kernel's
    # waves, the write kernel's stride); $share groups in every chunk
    for name, m in (("grid_8_chunks", 7 * FO_WCHUNK + 5), ("grid_66_chunks", 65 * FO_WCHUNK + 5)):
        rng = np.random.default_rng(m)
        add(Case(name, _split(rng, m, "rand"), _pick(rng, T.common, m), m=m, groups_in_every_chunk=True))
    # the pick list's bounds: one run per pick (a publisher per topic)
    add(Case("picks_65535", [1] * 257, [fid["G255"]] * 257, keys=np.arange(257), picks=PK_CAP_MIN - 1, M=0))
    add(Case("picks_65536", [1] * 256, [fid["G256"]] * 256, keys=np.arange(256), picks=PK_CAP_MIN, M=0))

    # M picks in runs of more than one pick: `twos` publishers with two messages, `threes` with
    # three, 30 with one, all to the group of five
    def multi(name, twos, threes):
        rng = np.random.default_rng(twos)
        keys = np.concatenate([np.repeat(np.arange(twos), 2), np.repeat(twos + np.arange(threes), 3),
                               twos + threes + np.arange(30)])
        keys = keys[rng.permutation(len(keys))]
        add(Case(name, [1] * len(keys), [fid["g5"]] * len(keys), keys=keys, M=2 * twos + 3 * threes,
                 picks=len(keys)))

    multi("multi_2", 1, 0)
    multi("multi_3", 0, 1)
    multi("multi_4096", 2048, 0)
    multi("multi_4097", 2047, 1)
    return out


# The cases by explicit name, family by family (test_fanout_ref.py asserts that no case is left out)
COUNT_NAMES = ["m%d_%s" % (m, how) for m in COUNTS for how in ("one", "each", "rand")]
COUNT_RAND_NAMES = ["m%d_rand" % m for m in COUNTS]
LEAD_TRAIL_NAMES = ["empty_lead_trail_%d" % k for k in EMPTY_RUNS]
BOUNDARY_NAMES = ["empties_at_256", "start_256_after_empties", "end_256", "topic_over_256", "topic_three_chunks"]
TOPIC_NAMES = ["topics_%d" % n for n in TOPIC_COUNTS]
CHUNK_NAMES = ["big_slot0", "big_slot255", "big_between_zero_runs", "zero_chunk_between"]
GROUPS_NAME = "many_groups_last_slot"
BASE_NAMES = ["base_%d" % b for b in BASES]
GRID_NAMES = ["grid_8_chunks", "grid_66_chunks"]
PICK_NAMES = ["picks_65535", "picks_65536"]
MULTI_NAMES = ["multi_2", "multi_3", "multi_4096", "multi_4097"]
FAMILIES = (COUNT_NAMES, LEAD_TRAIL_NAMES, BOUNDARY_NAMES, TOPIC_NAMES, CHUNK_NAMES, [GROUPS_NAME], BASE_NAMES,
            GRID_NAMES, PICK_NAMES, MULTI_NAMES)
