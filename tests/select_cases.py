"""Inputs of the select tests (CPU and GPU): owner tables and match CSRs at the id level with
their expected sets computed here from the contract of include/emqx_select.h (plain Python sets,
no library), and worlds of rules, bridges and exhook entries with topics, whose expected answers
come from the restatement (tests/select_ref.py).  Everything is generated from fixed seeds and
every reference is computed once per process."""

import functools

import numpy as np

from tests import select_ref as R

ENABLED, MATCH_ALL = 1, 2
ALL = 0xFFFFFFFF
CLASSES = (0, 1, 5, 31)
# the table of the shapes: plain filter ids, one wide list, two owners with two filters each, ids nobody holds
N_PLAIN = 400
WIDE = 400                      # the filter 65 owners hold
A1, A2, B1, B2 = 430, 431, 432, 433
OWNER_A, OWNER_B = 5000, 5001   # A holds A1 and A2, B holds B1 and B2
UNKNOWN_FROM = 440              # ids from here on are in no list (and 401..429 are below the largest id, but unheld)
MA_OWNERS = ((7000, 0, ENABLED | MATCH_ALL), (7001, 5, ENABLED | MATCH_ALL), (7002, 1, MATCH_ALL),
             (7003, 31, ENABLED | MATCH_ALL))  # the third is disabled


class Case:
    """An owner table (emqx_owntab_set argument tuples) and one batch."""

    def __init__(self, name, owners, offsets, filters, classes):
        self.name = name
        self.owners = owners  # [(owner, class_bit, flags, [filter ids])]
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.filters = np.asarray(filters, dtype=np.uint32)
        self.classes = None if classes is None else np.asarray(classes, dtype=np.uint32)
        self._ref = None

    @property
    def batch(self):
        return self.offsets, self.filters, self.classes

    @property
    def n(self):
        return len(self.offsets) - 1

    def load(self, table, commit=True):
        """Fills an OwnerTable (emqx_amd.select)."""
        for o, c, flags, fids in self.owners:
            table.set_flags(o, c, flags, fids)
        if commit:
            table.commit()
        return table

    def reference(self):
        if self._ref is None:
            self._ref = expected(self.owners, self.offsets, self.filters, self.classes)
        return self._ref


def expected(owners, offsets, filters, classes):
    """The contract, from sets: rows (sorted owner lists) and the eight summary words."""
    word, post, held = {}, {}, set()
    for o, c, flags, fids in owners:  # a later record of the same owner replaces the earlier one
        word[o] = (c, flags, sorted(set(fids)))
    for o, (c, flags, fids) in word.items():
        if not flags & MATCH_ALL:
            for f in fids:
                post.setdefault(f, set()).add(o)
                held.add(f)
    every = sorted(o for o, w in word.items() if w[1] & MATCH_ALL)

    def ok(o, mask):
        c, flags, _ = word[o]
        return bool(flags & ENABLED) and bool((mask >> c) & 1)

    rows, postings, dups, unknown = [], 0, 0, 0
    for i in range(len(offsets) - 1):
        mask = ALL if classes is None else int(classes[i])
        got, passing = set(), 0
        for d in range(int(offsets[i]), int(offsets[i + 1])):
            f = int(filters[d])
            if f not in held:
                unknown += 1
                continue
            postings += len(post[f])
            hits = {o for o in post[f] if ok(o, mask)}
            passing += len(hits)
            got |= hits
        dups += passing - len(got)
        rows.append(sorted(got | {o for o in every if ok(o, mask)}))
    counts = [len(r) for r in rows]
    summary = [0, int(offsets[-1]), postings, sum(counts), sum(1 for c in counts if c), dups, unknown,
               max(counts, default=0)]
    return {"rows": rows, "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64).tolist(),
            "summary": summary}


def check(case, got):
    """A Selected (emqx_amd.select) against the case's reference: the same sets, no owner twice
    (the rows are compared as sorted lists), the same offsets and summary."""
    ref = case.reference()
    assert got.offsets.tolist() == ref["offsets"], case.name
    assert got.rows() == ref["rows"], case.name
    assert [got.summary[k] for k in ("flags", "entries", "postings", "selected", "messages", "duplicates", "unknown",
                                     "max_per_message")] == ref["summary"], case.name


def table(match_all):
    """600 owners on sparse ids with 0..3 of the 400 plain filters each (many filters shared, one
    owner in eleven disabled), 65 owners on WIDE, owners A and B with two filters each, and with
    ``match_all`` the four match-all owners (one of them disabled)."""
    rng = np.random.default_rng(11)
    owners = []
    for k in range(600):
        size = int(rng.integers(0, 4))
        fids = rng.integers(0, N_PLAIN, size=size).tolist()
        if k % 9 == 0 and k < 9 * 65:
            fids.append(WIDE)
        if size == 2 and k % 5 == 0:
            fids.append(fids[0])  # a duplicate within one list
        owners.append((3 * k + 1, CLASSES[k % 4], 0 if k % 11 == 0 else ENABLED, fids))
    owners.append((OWNER_A, 0, ENABLED, [A1, A2]))
    owners.append((OWNER_B, 5, ENABLED, [B1, B2]))
    if match_all:
        owners += [(o, c, f, []) for o, c, f in MA_OWNERS]
    return owners


def _entries(rng, count):
    """Filter ids of one message: mostly plain ones, with repeats, the wide list, unheld and unknown ids."""
    f = rng.integers(0, N_PLAIN, size=count).astype(np.uint32)
    kind = rng.integers(0, 40, size=count)
    f[kind == 0] = WIDE
    f[kind == 1] = 0xFFFFFFFF
    f[kind == 2] = UNKNOWN_FROM + 7
    f[kind == 3] = 415  # below the largest id set, held by nobody
    if count >= 2:
        f[count - 1] = f[0]  # the same id twice in one message
    return f.tolist()


def _masks(n, masked):
    if not masked:
        return None
    cycle = [1 << 0, ALL, 0, 1 << 5, ALL, (1 << 1) | (1 << 31), 1 << 7]
    return [cycle[i % len(cycle)] for i in range(n)]


# name -> entries per message; the totals are 0, 1, 63..65, 255..257 and 10 002, with empty
# messages before, between and after
SHAPES = {
    "n0": [],
    "n1_e0": [0],
    "e0": [0, 0, 0],
    "e1": [0, 1, 0],
    "e63": [0, 20, 0, 0, 43, 0],
    "e64": [64],
    "e65": [0, 64, 1, 0],
    "e255": [0, 100, 0, 155, 0, 0],
    "e256": [1, 255],
    "e257": [0, 200, 0, 57, 0],
    "e10002": [0, 1, 0, 0, 5000] + [0, 0] + [7] * 300 + [0] + [29] * 100 + [1] + [0, 0],
}
SHAPE_CASES = [(name, ma, masked) for name in SHAPES for ma, masked in ((True, True), (False, False))] + \
              [("e257", True, False), ("e257", False, True)]


@functools.lru_cache(maxsize=None)
def shape(name, match_all=True, masked=True):
    counts = SHAPES[name]
    assert name in ("n0", "n1_e0") or sum(counts) == int(name[1:])
    rng = np.random.default_rng(len(counts) * 7919 + sum(counts))
    filters, offsets = [], [0]
    for c in counts:
        filters += _entries(rng, c)
        offsets.append(len(filters))
    return Case("%s/%s/%s" % (name, match_all, masked), table(match_all), offsets, filters, _masks(len(counts), masked))


@functools.lru_cache(maxsize=None)
def straddle(start, match_all=True):
    """One message of 300 entries that begins at entry ``start``, behind an empty message and, for
    start > 0, a short one: owner A is reachable from entries 63 and 64 (the wave boundary),
    owner B from entries 255 and 256 (the tile boundary), one plain filter id sits at entries 10
    and 200, WIDE at entries 100 and 260; two empty messages follow."""
    rng = np.random.default_rng(start + 1)
    filters = rng.integers(0, N_PLAIN, size=start + 300).astype(np.uint32)
    filters[63], filters[64], filters[255], filters[256] = A1, A2, B1, B2
    filters[200] = filters[10]
    filters[100] = filters[260] = WIDE
    offsets = [0, 0] + ([start] if start else []) + [start + 300] * 3
    n = len(offsets) - 1
    case = Case("straddle/%d/%s" % (start, match_all), table(match_all), offsets, filters.tolist(), [ALL] * n)
    row = case.reference()["rows"][n - 3]
    assert row.count(OWNER_A) == 1 and row.count(OWNER_B) == 1
    assert case.reference()["summary"][5] > 65  # the second WIDE entry alone repeats its enabled owners
    return case


# ---- worlds (strings) --------------------------------------------------------------------

WORDS = ["a", "b", "c", "dev", "1", "2", "temp", "x"]


def _pool(rng, k):
    """k distinct filters over a small vocabulary: exact ones, '+' and '#' forms, $SYS and $events names."""
    out = {"#", "+/+", "$SYS/#", "$SYS/+/up", "$events/client_connected", "$events/message_dropped", "$events/+"}
    while len(out) < k:
        depth = int(rng.integers(1, 5))
        ws = [WORDS[int(rng.integers(0, len(WORDS)))] if rng.random() < 0.7 else "+" for _ in range(depth)]
        if rng.random() < 0.25:
            ws[-1] = "#"
        if rng.random() < 0.08:
            ws[0] = "$SYS"
        out.add("/".join(ws))
    return sorted(out)


def _topics(rng, k):
    out = ["$SYS/brokers", "$SYS/a/up", "$events/client_connected", "$events/message_dropped", "$events/other", "a", "zzz/q"]
    while len(out) < k:
        out.append("/".join(WORDS[int(rng.integers(0, len(WORDS)))] for _ in range(int(rng.integers(1, 5)))))
    return out


@functools.lru_cache(maxsize=None)
def world(n_owners, n_filters, seed, ignore_sys_message=True):
    """About 70 % rules, 20 % bridges and 10 % exhook entries over a shared pool of filters; lists
    of 0, 1 and 2 filters, one rule in fifty with 65; bridges ingress, disabled and without an
    ``enable`` key; one exhook entry in four with the empty list."""
    rng = np.random.default_rng(seed)
    pool = _pool(rng, n_filters)
    pick = lambda k: [pool[int(j)] for j in rng.integers(0, len(pool), size=k)]  # noqa: E731
    w = {"ignore_sys_message": ignore_sys_message, "rules": [], "bridges": {"mqtt": {}, "http": {}}, "exhooks": []}
    for k in range(n_owners):
        r = k % 10
        if r < 7:
            w["rules"].append({"id": "r%d" % k, "from": pick(65 if k % 50 == 3 else int(rng.integers(0, 3)))})
        elif r < 9:
            conf = {"direction": "ingress" if k % 6 == 1 else "egress", "local_topic": pick(1)[0]}
            if k % 4:
                conf["enable"] = k % 8 != 3
            w["bridges"]["mqtt" if r == 7 else "http"]["b%d" % k] = conf
        else:
            w["exhooks"].append({"id": "h%d" % k, "topics": [] if k % 40 == 9 else pick(int(rng.integers(1, 3)))})
    return w


@functools.lru_cache(maxsize=None)
def messages(n, distinct, seed):
    """n messages over ``distinct`` topics; $SYS topics carry the sys flag two times in three."""
    rng = np.random.default_rng(seed)
    names = _topics(rng, distinct)
    out = []
    for _ in range(n):
        t = names[int(rng.integers(0, len(names)))]
        out.append({"topic": t, "sys": t.startswith("$SYS") and rng.random() < 0.67})
    return out


def consumers_by_mask(w, topic, mask):
    """The restatement under a class mask (bit 0 rules, bit 1 bridges, bit 2 exhook), without the
    sys rules: what HookIndex.select answers for (topic, mask)."""
    out = []
    if mask & 1:
        out += ["rule:%s" % r["id"] for r in R.get_rules_for_topic(w["rules"], topic)]
    if mask & 2:
        out += ["bridge:%s" % b for b in R.get_matched_bridges(w["bridges"], topic)]
    if mask & 4:
        out += ["exhook:%s" % h["id"] for h in R.exhook_on_message_publish(w["exhooks"], {"topic": topic})]
    return sorted(out)


def world_expected(w, msgs):
    """consumers/2 of the restatement per message, computed once per distinct (topic, sys)."""
    memo = {}
    out = []
    for m in msgs:
        key = (m["topic"], bool(m.get("sys", False)))
        if key not in memo:
            memo[key] = R.consumers(w, m)
        out.append(memo[key])
    return out
