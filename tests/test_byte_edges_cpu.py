"""The byte-edge case generator (tests/byte_edge_cases.py) against the oracle alone: every builder
produces the byte lengths, level counts, tile sums and tile byte spans it is named for, every
batch has topics with and without matches, and emqx_router:match_routes through the oracle's trie
(oracle/emqx_ref.py Router) returns what brute_force_routes returns.

Two documented exceptions: the all-empty batches hold one topic repeated, so they cannot have both
a matching and a non-matching topic (the empty topic matches '+', '#' and the empty filter); and
topics of more than 1000 levels skip the trie walk, whose restatement recurses once per level as
the reference does (the brute force covers them)."""

import sys

import pytest

from oracle import emqx_ref as R
from tests import byte_edge_cases as B

KIB = 1024
MAP_BYTES = [32 * s for s in (256, 384, 512, 768, 1024, 2048)]   # the level map of every STACK_CAP
LEVEL_CAPS = (56, 64, 80, 96, 128)                                    # WID_CAP / 8
WORD_CAPS = (448, 512, 640, 768, 1024)                                 # WID_CAP


def levels(t):
    return t.count(b"/") + 1


def tile0(topics):
    return topics[:B.TILE]


@pytest.fixture(scope="module")
def routers():
    out = {}
    for name in ("base", "deep", "limit"):
        r = R.Router(True)
        for f in B.table(name):
            r.add_route(f)
        out[name] = (r, {f: i for i, f in enumerate(B.table(name))})
    return out


def test_vocabulary_and_tables():
    lens = {len(w) for w in B.SPECIAL}
    assert set(B.WORD_LENS) <= lens
    for fam in (B.FAM_AT16, B.FAM_AT17):
        assert len({w[:16] for w in fam}) == 1 and len(set(fam)) == len(fam)
    assert B.FAM_AT16[0][:16] == B.FAM_AT16[1][:16] and B.FAM_AT16[0][16] != B.FAM_AT16[1][16]
    assert B.FAM_AT17[0][:17] == B.FAM_AT17[1][:17] and B.FAM_AT17[0][17] != B.FAM_AT17[1][17]
    for a, b in zip(B.FAM_LAST[::2], B.FAM_LAST[1::2]):
        assert a[:-1] == b[:-1] and a[-1] != b[-1] and len(a) % 4 != 0
    for a, b in B.PREFIX_PAIRS:
        assert b.startswith(a) and len(a) < len(b)
    assert {15, 16, 17} <= {len(a) for a, _ in B.PREFIX_PAIRS} | {len(b) for _, b in B.PREFIX_PAIRS}
    for byte in B.NEAR_SEP_BYTES:
        assert any(byte in w for w in B.NEAR_SEP)
    base = B.table("base")
    assert 200 <= len(base) <= 700 and len(set(base)) == len(base)
    assert b"+" in base and any(f.endswith(b"/#") for f in base)
    assert max(levels(f) for f in base) <= 12      # the shallow variant and the small-batch path
    assert max(levels(f) for f in B.table("deep")) == 300
    words = set(B.table_words("base"))
    for w in B.SPECIAL + B.FILTER_ONLY + list(B.LONG_KNOWN.values()):
        assert w in words, w
    fam_topics = set()
    for t in B.FAMILIES.topics():
        fam_topics.update(t.split(b"/"))
    for w in B.TOPIC_ONLY:
        assert w not in words and w in fam_topics, w
    only_filters = {b"only-in-filters", b"only-in-filters-17"}
    assert only_filters <= words
    for case in B.ALL_MATCHED:
        if case is not B.FAMILIES:
            for t in case.topics():
                assert not only_filters & set(t.split(b"/"))


@pytest.mark.parametrize("name", ["base", "deep"])
def test_vocab_table_has_probe_chains(name):
    """At least two table words fall on one slot of the vocab table (word_hash & vocab_mask)."""
    words = B.table_words(name)
    assert 3 * (len(words) + 2) <= 1024          # whatever the builder counts as a word: 1024 slots
    mask = B.vocab_mask(len(words))
    assert mask == 1023
    slots = [B.word_hash(w) & mask for w in words]
    assert len(set(slots)) < len(slots)


def test_word_hash_restatement_and_colliding_words():
    # values printed by word_hash_bytes of emqx_amd/csrc/layout.h itself (a host build)
    assert B.word_hash(b"") == 0x177B1B6F and B.word_hash(b"a") == 0xC3238EFB
    assert B.word_hash(b"FAMILY-HEAD-16byA") == 0x69326AC6
    a, b, c = B.COLLIDE
    assert len({a, b, c}) == 3 and {len(a), len(b), len(c)} == {24} and a[:16] == b[:16] == c[:16]
    assert B.word_hash(a) == B.word_hash(b) == B.word_hash(c) == 0x82799F6D
    assert all(b"/" not in w and 0 not in w for w in B.COLLIDE)
    words = set(B.table_words("base"))
    assert a in words and b in words and c not in words
    fam = B.FAMILIES.topics()
    assert b"a/" + a in fam and b"a/" + b in fam and b"a/" + c in fam
    exp = B.expected("base", [b"a/" + a, b"a/" + b, b"a/" + c], 0)
    assert len({tuple(x) for x in exp}) == 3       # three different answers


def test_window_sweep_offsets():
    topics = B.WINDOW.topics()
    assert len(topics) == 40 * 12 and len(B.SWEEP_TAILS) == 12
    off, seen = 0, {b"/": set(), b"+": set(), b"#": set()}
    for t in topics:
        for i, c in enumerate(t):
            ch = bytes([c])
            if ch in seen:
                seen[ch].add((off + i) % 16)
        off += len(t)
    for ch, s in seen.items():
        assert s == set(range(16)), ch
    for k in range(40):
        assert topics[k * 12] == b"h" * k + b"/+"


@pytest.mark.parametrize("case", B.LEVEL_LEN, ids=lambda c: c.name)
def test_level_lengths(case):
    n = case.args[0]
    topics = case.topics()
    longest = [max(len(w) for w in t.split(b"/")) for t in topics]
    assert max(longest) == n
    assert longest[0] < 16 and longest[-1] < 16 and longest.count(n) >= 4
    assert B.long_level_topics(topics) == (longest.count(n) if n >= B.AUX_LEN_MAX else 0)
    words = set(B.table_words("base"))
    assert (B.LW[:n] in words) == (n in (4094, 4096))
    # the largest record of a level that stays on the fast path is below WID_RESOLVED
    assert ((B.AUX_LEN_MAX - 1) << 20 | (B.AUX_OFF_LIM - 1)) < 0xFFFFFFF0


def test_mib_tile_spans():
    topics = B.MIB.topics()
    t0 = tile0(topics)
    assert len(topics) > B.TILE and sum(len(t) for t in t0) > B.AUX_OFF_LIM
    assert all(max(len(w) for w in t.split(b"/")) < B.AUX_LEN_MAX for t in topics)
    ends, e = [], 0
    for t in t0:
        e += len(t)
        ends.append(e)
    behind = [i for i, e in enumerate(ends) if e >= B.AUX_OFF_LIM]
    assert len(behind) == B.MIB_BEHIND and behind[-1] == B.TILE - 1
    first = behind[0]
    assert ends[first - 1] == B.AUX_OFF_LIM - 1            # the last topic that stays
    assert len(t0[first - 1]) < 40 and len(t0[first - 2]) < 40 and all(len(t0[i]) < 40 for i in behind)
    exp = B.expected("base", t0, 0)
    filters = B.table("base")
    for i in behind:                                        # each an exact filter of the table
        assert t0[i] in filters and filters.index(t0[i]) in exp[i]


@pytest.mark.parametrize("case", B.NLEV, ids=lambda c: c.name)
def test_level_counts(case):
    n = case.args[0]
    topics = case.topics()
    lv = [levels(t) for t in topics]
    assert max(lv) == n and lv.count(n) == 5
    assert B.deep_topic(n) in B.table("deep")
    assert any(n == c + d for c in LEVEL_CAPS for d in (-1, 0, 1))


def test_level_counts_cover_every_variant():
    for c in LEVEL_CAPS:
        assert {c - 1, c, c + 1} <= set(B.NLEVS)
    for c in WORD_CAPS:
        assert {c, c + 1} <= set(B.TILE_SUMS)
    for m in MAP_BYTES:
        below = [k for k in B.TILE_KIB if k * KIB <= m]
        above = [k for k in B.TILE_KIB if k * KIB > m]
        assert below and above, m


@pytest.mark.parametrize("case", B.TILE_SUM, ids=lambda c: c.name)
def test_tile_sums(case):
    total = case.args[0]
    topics = case.topics()
    lv = [levels(t) for t in tile0(topics)]
    assert len(topics) > B.TILE and sum(lv) == total
    assert max(lv) <= min(LEVEL_CAPS) and lv == sorted(lv)   # no topic defers for its own depth


@pytest.mark.parametrize("case", B.BIG_TILE, ids=lambda c: c.name)
def test_tile_byte_spans(case):
    kib = case.args[0]
    topics = case.topics()
    assert sum(len(t) for t in tile0(topics)) == kib * KIB and len(topics) > B.TILE
    assert all(max(len(w) for w in t.split(b"/")) < B.AUX_LEN_MAX for t in topics)
    assert max(levels(t) for t in topics) <= 8


def test_deep_limits():
    s = B.SLASHES.topics()
    assert b"/" * 65535 in s and levels(b"/" * 65535) == 65536
    o = B.ORD65535.topics()
    big = [t for t in o if len(t) == B.MAX_TOPIC]
    assert len(big) == 2 and levels(big[0]) == 32768 and levels(big[1]) <= 56
    assert max(len(w) for w in big[1].split(b"/")) == B.AUX_LEN_MAX - 1
    t = [x for x in B.TOO_LONG.topics() if len(x) > B.MAX_TOPIC]
    assert len(t) == 1 and len(t[0]) == 65536 and levels(t[0]) > 128
    assert max(levels(x) for x in B.DEEP300.topics()) == 301 and B.deep_topic(300) in B.DEEP300.topics()


def test_empty_batches():
    assert [len(c.topics()) for c in B.EMPTY] == [1, 64, 65]
    for c in B.EMPTY:
        assert set(c.topics()) == {b""}
        assert B.expected("base", c.topics()[:1], 0)[0]     # '+', '#' and the empty filter


@pytest.mark.parametrize("case", B.ALL_MATCHED + [B.TOO_LONG], ids=lambda c: c.name)
def test_batches_against_the_oracle(case, routers):
    topics = case.topics()
    assert case.note()
    exp = B.expected(case.table, topics, 0)
    if case not in B.EMPTY:
        assert any(exp) and not all(exp)
    router, index = routers[case.table]
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 5000))
    try:
        for t, x in zip(set(topics), B.expected(case.table, list(set(topics)), 0)):
            if levels(t) <= 1000:
                assert R.router_match_ids(router, index, t) == x, t[:60]
    finally:
        sys.setrecursionlimit(old)
    # the three modes are three different questions on these tables
    if case is B.FAMILIES:
        e1, e2 = B.expected(case.table, topics, 1), B.expected(case.table, topics, 2)
        assert exp != e1 and e1 != e2
