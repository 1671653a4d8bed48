"""Case generator of the byte-level edge sweep (tests/test_gpu_byte_edges.py, checked on the CPU
by tests/test_byte_edges_cpu.py): an adversarial vocabulary, three filter tables over it and one
topic-batch builder per limit of the match kernels' tokenizer paths (phase A of fast_tile, the
deep path's tokenizer, the small-batch copy, order_kernels.hip).  Everything is a pure function
of the constants below; no GPU, no engine.

Tables (the filter id is the position in the list):
  "base"   a few hundred filters of at most 6 levels (the engine's shallow default variant and its
           one-launch small-batch path need a table of at most 12 levels)
  "deep"   base + filters of 7 .. 300 levels, for the level-count and tile-sum batches
  "limit"  a few dozen filters, for the topics of 65535 / 65536 bytes: the Python brute force
           splits such a topic once per wildcard filter, so the table is cut, not the check

The reference of every comparison is oracle/emqx_ref.py (`expected`): brute_force_routes,
brute_force_trie, and the wildcard-only trie as tests/test_gpu_parity.py builds it.
"""

from __future__ import annotations

import random
from typing import Callable, Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

from oracle import emqx_ref as R

SEED = 0xB17E


_M32 = 0xFFFFFFFF


def _whash_step(h: int, d: int) -> int:
    h = ((h ^ d) * 0x85EBCA77) & _M32
    return ((h << 13) | (h >> 19)) & _M32


def _whash_state(p: bytes, ndwords: int) -> int:
    """The multiply-rotate chain of word_hash_bytes after the first `ndwords` dwords of p."""
    h = (len(p) * 0x9E3779B1 + 0x7F4A7C15) & _M32
    for i in range(ndwords):
        h = _whash_step(h, int.from_bytes(p[4 * i:4 * i + 4].ljust(4, b"\0"), "little"))
    return h


def word_hash(p: bytes) -> int:
    """word_hash_bytes of emqx_amd/csrc/layout.h, restated."""
    n = len(p)
    h = _whash_state(p, (n + 3) // 4 if n > 16 else 4)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def colliding_words(head16: bytes, count: int) -> List[bytes]:
    """`count` words of 24 bytes with one head of 16 bytes, one length and ONE word_hash: the vocab
    lookup can tell them apart only by the arena compare of bytes 16 .. 23.  (One more dword after
    the head cannot collide: a step of the chain is a bijection of h ^ d.  With two, the second
    dword cancels the difference the first one makes.)"""
    assert len(head16) == 16
    first = head16 + b"tail0000"
    h4 = _whash_state(first, 4)
    s0 = _whash_step(h4, int.from_bytes(first[16:20], "little"))
    d5 = int.from_bytes(first[20:24], "little")
    out, i = [first], 0
    while len(out) < count:
        i += 1
        d4 = b"t%03d" % i
        tail = (d5 ^ s0 ^ _whash_step(h4, int.from_bytes(d4, "little"))).to_bytes(4, "little")
        if 0x2F in tail or 0 in tail:
            continue
        out.append(head16 + d4 + tail)
    return out



# ---- the limits of emqx_amd/csrc/match_kernels.hip the builders aim at -------------------------
AUX_LEN_MAX = 4095            # a level of AUX_LEN_MAX bytes or more defers its topic
AUX_OFF_LIM = 1 << 20         # a topic ending AUX_OFF_LIM bytes or more past the tile's start defers
MAX_TOPIC = 65535             # the deep path's longest topic
TILE = 64                     # topics per tile of the batched kernel
LEVEL_LENS = (4093, 4094, 4095, 4096)
NLEVS = (55, 56, 57, 63, 64, 65, 79, 80, 81, 95, 96, 97, 127, 128, 129)   # WID_CAP / 8 of every variant, +-1
TILE_SUMS = (448, 449, 512, 513, 640, 641, 768, 769, 1024, 1025)  # WID_CAP of every variant, +1
TILE_KIB = (7, 9, 13, 17, 33, 66)                                 # around 32 B * STACK_CAP of every variant

# ---- vocabulary ------------------------------------------------------------------------------
WORD_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65)
_LONG = b"prefix-chain-0123456789-abcdefghijklmnopqrstuvwxyz-ABCDEFGHIJKLMNOPQRSTUVWXYZ"[:65]
assert len(_LONG) == 65
# one prefix chain: every shorter word is a strict prefix of every longer one, and all words of
# 16 bytes or more share VocabSlot::inl
LEN_WORDS = [_LONG[:n] for n in WORD_LENS]

HEAD16 = b"FAMILY-HEAD-16by"
assert len(HEAD16) == 16
# equal in the first 16 bytes; differing at byte 16, at byte 17, and only in the last byte
FAM_AT16 = [HEAD16 + b"A", HEAD16 + b"B"]
FAM_AT17 = [HEAD16 + b"xA", HEAD16 + b"xB"]
FAM_LAST = []        # pairs differing only in the last byte, at lengths that are no multiple of 4
for _n in (5, 7, 15, 17, 18, 33, 65):
    _b = (b"last-byte-family/".replace(b"/", b"_") * 5)[:_n - 1]
    FAM_LAST += [_b + b"0", _b + b"1"]
# one hash, one length, one 16-byte head: two table words and one word of no table
COLLIDE = colliding_words(b"COLLIDE-HEAD-16b", 3)
# in no table: the families' third members and near misses of the prefix chain
FAM_UNKNOWN = [HEAD16 + b"C", HEAD16 + b"xC", HEAD16[:15], HEAD16[:15] + b"z", _LONG[:16] + b"!", _LONG[:14] + b"!!",
               _LONG[:64] + b"!", _LONG[:32] + b"!", COLLIDE[2]] + [w[:-1] + b"2" for w in FAM_LAST[::2]]
PREFIX_PAIRS = [(b"pre", b"prefix"), (HEAD16, HEAD16 + b"A"), (_LONG[:15], _LONG[:16]), (_LONG[:16], _LONG[:17]),
                (_LONG[:63], _LONG[:64]), (_LONG[:64], _LONG[:65])]

# '/', '+', '#' with the top bit set, their neighbours in value, 0x80 and 0xFF
NEAR_SEP_BYTES = (0xAF, 0xAB, 0xA3, 0x2E, 0x30, 0x80, 0xFF)
NEAR_SEP = [bytes([b]) for b in NEAR_SEP_BYTES] + [
    b"\xaf\xab\xa3", b"\x2e\x30", b"\xff\x80\xff", b"\xaf\x2e\xab\x30", b"....", b"0000", b"\xaf" * 16, b"\xab" * 17,
    b"\xa3" * 5, b"*", b",", b'"', b"\xaf\xaf", b"\xab\xa3"]
NEAR_WILD = [b"++", b"+x", b"x+", b"#x", b"x#", b"$", b"$$", b"$SYS"]
ORDINARY = [b"a", b"b", b"c", b"x", b"y", b"dev", b"sensor", b"q"]
FILTER_ONLY = [b"only-in-filters", b"only-in-filters-17", b"of"]
TOPIC_ONLY = [b"only-in-topics", b"only-in-topics-17b", b"ot", b"\xaf\xff", b"\x80\x80", b"+#", b"#+", b"$none"] + FAM_UNKNOWN
# filler: enough table words that the 1024-slot vocab table has probe chains
FILLER = sorted({(b"f%d-" % i + b"fillerfillerfiller")[:4 + i % 17] for i in range(190)})

LW = (b"Lw0123456789" * 400)[:4100]      # long levels are prefixes of one string
LONG_KNOWN = {4094: LW[:4094], 4096: LW[:4096]}
DW = [b"a", b"b", b"dev", b"", b"x", _LONG[:16], _LONG[:17]]   # levels of the deep topics

SPECIAL = (LEN_WORDS + FAM_AT16 + FAM_AT17 + FAM_LAST + COLLIDE[:2] + [HEAD16, b"pre", b"prefix"] + NEAR_SEP + NEAR_WILD +
           ORDINARY)


def _uniq(xs: Sequence[bytes]) -> List[bytes]:
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


TABLE_WORDS = _uniq(SPECIAL + FILTER_ONLY + FILLER + list(LONG_KNOWN.values()))
HEAD_FILL = b"h" * 40          # the window sweep's head
SWEEP_TAILS = [b"/+", b"/#", b"/+/", b"/++", b"/+x", b"/x+", b"#/", b"/\xaf", b"/\xab/", b"/" + _LONG[:16],
               b"/" + _LONG[:17], b"/"]
SWEEP_EXACT_K = (0, 3, 15, 16, 17, 31)   # heads whose wildcard topics are filters of the table too

MATCH_ALL = b"a/b"        # matched in every table
MATCH_NONE = b"$none/zz"  # matched in none ('$' blocks the root wildcards)


# ---- tables ----------------------------------------------------------------------------------
def _base_filters() -> List[bytes]:
    rng = random.Random(SEED)
    f = [b"#", b"+", b"+/#", b"+/+", b"+/+/#", b"a/#", b"a/+", b"a/b", b"/", b"/#", b"/+", b"/+/#", b"+/", b"//", b"",
         b"$SYS/#", b"$SYS/+", b"$/+", b"$", b"$$", b"$$/#", b"++", b"++/#", b"+x/+", b"x+", b"#x", b"#x/+", b"x#/#",
         b"+/++", b"+/+x", b"+/x+", b"+/#x", b"+/x#", b"dev/+/#", b"dev/x", b"+/\xaf", b"+/\xab/", b"+/\xab/#",
         b"\xaf/#", b"+/\xaf/+", b"a/" + _LONG[:17] + b"/b"]
    # the window sweep: filters under the head, and its wildcard topics as exact filters
    for k in SWEEP_EXACT_K:
        h = HEAD_FILL[:k]
        f += [h + b"/+", h + b"/#", h + b"/+/", h + b"/" + _LONG[:16], h + b"/+x"]
    f += [b"+/" + _LONG[:16], b"+/" + _LONG[:17] + b"/#", HEAD_FILL[:20] + b"/#", HEAD_FILL[:33] + b"/+"]
    # the colliding words: each at the first, the middle and the last level
    for w in COLLIDE[:2]:
        f += [w, b"a/" + w, b"+/" + w + b"/#", w + b"/+", b"a/" + w + b"/b"]
    # the long levels
    f += [b"x/" + LONG_KNOWN[4094] + b"/y", b"+/" + LONG_KNOWN[4094] + b"/#", b"x/" + LONG_KNOWN[4096] + b"/+",
          LONG_KNOWN[4096] + b"/y", b"x/" + LONG_KNOWN[4094]]
    # every table word in at least one filter, at the first, a middle or the last level
    for i, w in enumerate(w for w in TABLE_WORDS if len(w) < 100):
        r = i % 4
        f.append([w, b"a/" + w, w + b"/+", b"+/" + w + b"/#"][r])
        if w in SPECIAL and w:
            f.append([b"+/" + w, w + b"/#", b"a/" + w + b"/b", w][r])
    # random filters of 1 .. 6 levels
    words = [w for w in TABLE_WORDS if len(w) < 100]
    for _ in range(110):
        d = rng.randint(1, 6)
        lv = []
        for j in range(d):
            x = rng.random()
            if x < 0.25:
                lv.append(b"+")
            elif x < 0.35 and j == d - 1:
                lv.append(b"#")
            elif x < 0.7:
                lv.append(rng.choice(SPECIAL))
            else:
                lv.append(rng.choice(words))
        f.append(b"/".join(lv))
    return _uniq(f)


def deep_topic(n: int) -> bytes:
    """n levels over DW (known words, among them the empty one and a 16- and a 17-byte word)."""
    return b"/".join(DW[i % len(DW)] for i in range(n))


def _deep_extra() -> List[bytes]:
    f = []
    for n in (7, 8, 9, 10, 11, 12, 13, 16, 17) + NLEVS + (300,):
        f += [deep_topic(n), b"/".join([b"+"] * n)]
    for n in (56, 64, 80, 96, 128):
        f += [deep_topic(n - 1) + b"/#", deep_topic(n) + b"/#", b"/".join([b"+"] * (n - 1)) + b"/#"]
    f += [b"/".join([b""] * 64), b"/".join([b""] * 128) + b"/#"]
    return f


def _limit_filters() -> List[bytes]:
    return _uniq([b"#", b"+/#", b"/#", b"/+/#", b"//+/#", b"a/#", b"a/+/#", b"a/a/#", b"a/b", b"+/a/#", b"+/+", b"a",
                  b"a/+/a/#", b"/", b"$SYS/#", b"+", b"a/a", b"b/#", b"x/" + LONG_KNOWN[4094] + b"/#",
                  b"a/" + LONG_KNOWN[4094] + b"/+/#", deep_topic(300), deep_topic(300) + b"/#",
                  b"/".join([b"+"] * 300), b"dev/x"])


_TABLES: Dict[str, List[bytes]] = {}


def table(name: str) -> List[bytes]:
    if name not in _TABLES:
        if name == "base":
            _TABLES[name] = _base_filters()
        elif name == "deep":
            _TABLES[name] = _uniq(table("base") + _deep_extra())
        elif name == "limit":
            _TABLES[name] = _limit_filters()
        else:
            raise KeyError(name)
    return _TABLES[name]


def table_words(name: str) -> List[bytes]:
    """The distinct literal levels of a table's filters: the words of its vocab table."""
    out = []
    for f in table(name):
        for w in R.words(f):
            if isinstance(w, bytes):
                out.append(w)
            elif w == R.EMPTY:
                out.append(b"")
    return _uniq(out)


def vocab_mask(n_words: int) -> int:
    """VocabState::build_table (tables.cpp): a power of two of at least 3 slots per word, 1024 at least."""
    cap = 1024
    while cap < 3 * n_words:
        cap *= 2
    return cap - 1


# ---- the reference ---------------------------------------------------------------------------
_EXP: Dict[Tuple[str, int, bytes], Tuple[int, ...]] = {}
_WILD: Dict[str, List[bytes]] = {}


def expected(tname: str, topics: Sequence[bytes], mode: int) -> List[List[int]]:
    """Sorted filter ids per topic: mode 0 brute_force_routes, 1 brute_force_trie, 2 the router's
    wildcard-only trie (as `expected` of tests/test_gpu_parity.py).  Computed once per topic."""
    filters = table(tname)
    if mode == 2 and tname not in _WILD:
        _WILD[tname] = [f if R.wildcard(f) else b"\x00never" for f in filters]
    out = []
    for t in topics:
        key = (tname, mode, t)
        v = _EXP.get(key)
        if v is None:
            if mode == 0:
                v = R.brute_force_routes(filters, t)
            elif mode == 1:
                v = R.brute_force_trie(filters, t)
            else:
                v = R.brute_force_trie(_WILD[tname], t)
            v = _EXP[key] = tuple(v)
        out.append(list(v))
    return out


def expected_csr(tname: str, topics: Sequence[bytes], mode: int) -> Tuple[np.ndarray, np.ndarray]:
    exp = expected(tname, topics, mode)
    off = np.zeros(len(topics) + 1, dtype=np.int64)
    if topics:
        off[1:] = np.cumsum([len(x) for x in exp])
    ids = np.array([i for x in exp for i in x], dtype=np.int64)
    return off, ids


def csr_bad_topics(off, ids, exp_off, exp_ids) -> List[int]:
    """Topics whose id set differs from the expected one (every topic is compared)."""
    off = np.asarray(off).astype(np.int64)
    n = len(exp_off) - 1
    assert len(off) == n + 1, (len(off), n + 1)
    cnt, ecnt = np.diff(off), np.diff(exp_off)
    bad = cnt != ecnt
    if not bad.any() and n and int(exp_off[-1]):
        t = np.repeat(np.arange(n, dtype=np.int64), cnt)
        got = np.sort((t << 32) | np.asarray(ids)[off[0]:off[-1]].astype(np.uint32).astype(np.int64))
        want = (t << 32) | exp_ids
        bad[np.unique(got[got != want] >> 32)] = True
        bad[np.unique(want[got != want] >> 32)] = True
    return np.nonzero(bad)[0].tolist()


def pack(topics: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    offs = np.zeros(len(topics) + 1, dtype=np.uint64)
    if topics:
        offs[1:] = np.cumsum([len(t) for t in topics])
    joined = b"".join(topics)
    buf = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(1, dtype=np.uint8)
    return buf, offs


# ---- topic batches -----------------------------------------------------------------------------
ORD_PRE = [MATCH_ALL, MATCH_NONE, b"dev/x"]
ORD_POST = [b"a/only-in-topics", MATCH_NONE, MATCH_ALL, b"sensor/x/y"]


def window_sweep():
    """Every tail behind a head of k = 0 .. 39 filler bytes: each separator and each one-byte
    wildcard lands on every offset relative to a 16-B window edge."""
    topics = [HEAD_FILL[:k] + tail for k in range(40) for tail in SWEEP_TAILS]
    return topics, "window sweep: 40 heads x %d tails" % len(SWEEP_TAILS)


def families():
    """Every vocabulary word as a topic level: the special words first, in the middle and last,
    the filler and topic-only words once."""
    topics = []
    for w in _uniq(SPECIAL + TOPIC_ONLY):
        topics += [w, b"a/" + w, w + b"/b", b"a/" + w + b"/b"]
    topics += [b"a/" + w for w in FILLER + FILTER_ONLY]
    for a, b in PREFIX_PAIRS:
        topics += [a + b"/" + b, b + b"/" + a]
    return topics, "word families: lengths %s, shared 16-byte heads, prefix pairs, near-separators" % (WORD_LENS,)


def level_len(n: int):
    """Levels of n bytes (a prefix of LW: the 4094- and 4096-byte ones are table words) first, in the
    middle and last, between ordinary topics."""
    w = LW[:n]
    special = [b"x/" + w + b"/y", w + b"/y", b"x/" + w, b"x/" + w[:-1] + b"!/y", b"q/" + w + b"/" + w]
    return ORD_PRE + special + ORD_POST, "levels of %d bytes" % n


def long_level_topics(topics: Sequence[bytes]) -> int:
    return sum(1 for t in topics if max(len(w) for w in t.split(b"/")) >= AUX_LEN_MAX)


def _fit(n: int, fill: int) -> bytes:
    """A topic of exactly n bytes under 'a/': levels of at most 4000 bytes of the byte `fill`."""
    assert n >= 3
    out = bytearray(b"a")
    while len(out) < n:
        k = min(4000, n - len(out) - 1)
        out += b"/" + bytes([fill]) * k
    assert len(out) == n
    return bytes(out)


def mib_tile():
    """Tile 0 (the first 64 topics) spans more than 1 MiB: 56 topics of about 18.7 KB, then 8 short
    ones.  The second short topic ends at byte 2^20 - 1 of the tile (the last that stays on the
    fast path); the six behind it end at or past the mark and must defer.  The short topics behind
    the mark are exact filters of the table, so a wrapped 20-bit offset loses their ids."""
    big = [_fit(18723, 0x41 + i % 26) for i in range(55)]
    big.append(_fit(AUX_OFF_LIM - 40 - 55 * 18723, 0x5A))
    before = [b"a/b/c/d/e/f/g", _fit(26, 0x6B)]         # 13 bytes, then 26: ends at 2^20 - 1
    behind = [b"dev/x", b"", b"a/b", b"a/" + _LONG[:17] + b"/b", b"$$", b"//"]
    tile0 = big + before + behind
    assert len(tile0) == TILE
    return tile0 + ORD_POST + [b"dev/x", b"/"], "tile 0 spans %d bytes" % sum(len(t) for t in tile0)


MIB_BEHIND = 6   # topics of mib_tile() at or behind the 1 MiB mark


def nlev(n: int):
    """Topics of exactly n levels: known words (an exact filter for some n), an unknown last word, n
    empty levels, a wildcard topic."""
    t = deep_topic(n)
    special = [t, t[:-1] + b"!" if not t.endswith(b"/") else t + b"!", b"/" * (n - 1),
               b"/".join([b"a"] * (n - 1) + [b"+"]), b"/".join([b"q"] * n)]
    return ORD_PRE + special + ORD_POST, "topics of %d levels" % n


def tile_sum(total: int):
    """64 topics (one tile) whose level counts sum to `total`; the topics with one level more sit
    at the tile's end, so the word past a variant's capacity belongs to the last topic."""
    base, rem = divmod(total, TILE)
    counts = [base] * (TILE - rem) + [base + 1] * rem
    topics = []
    for i, c in enumerate(counts):
        k = i % 4
        topics.append(deep_topic(c) if k == 0 else b"/".join([b"a"] * c) if k == 1 else
                      b"/".join([b"q"] * (c - 1) + [_LONG[:16]]) if k == 2 else b"/" * (c - 1))
    topics[-1] = deep_topic(counts[-1])
    return topics + ORD_POST, "64 topics, %d levels in all" % total


def big_tile(kib: int):
    """64 topics (one tile) of kib KiB in all: 'a/<table word>/<filler level>' each."""
    per = kib * 1024 // TILE
    words = [w for w in _uniq(LEN_WORDS + FAM_AT16 + FAM_AT17 + NEAR_SEP + ORDINARY) if 0 < len(w) < 40]
    topics = []
    for i in range(TILE):
        head = b"a/" + words[(i * 7 + kib) % len(words)] + b"/"
        topics.append(head + bytes([0x61 + i % 26]) * (per - len(head)))
    topics[-1] = b"dev/x/" + b"z" * (per - 6)
    return topics + ORD_POST, "64 topics, %d KiB in all" % kib


def deep300():
    t = deep_topic(300)
    return ORD_PRE + [t, t + b"/x", b"/".join([b"q"] * 300), b"/" * 299] + ORD_POST, "300-level topics"


def slashes_65535():
    """65535 x '/': 65536 empty levels, one wave's deep_wids area (DEEP_MAX_LEVELS) exactly."""
    return [MATCH_ALL, b"/" * MAX_TOPIC, MATCH_NONE], "65535 slashes"


def ordinary_65535():
    """65535-byte topics: 32768 one-byte levels, and 20 levels of up to 4094 bytes."""
    long_levels = [b"a"] + [LONG_KNOWN[4094]] * 15
    rest = MAX_TOPIC - len(b"/".join(long_levels)) - 2
    long_levels += [b"m" * (rest // 2), b"n" * (rest - rest // 2)]
    return [MATCH_NONE, b"a/" * 32767 + b"a", b"/".join(long_levels), MATCH_ALL], "65535-byte topics"


def too_long():
    """A 65536-byte topic of 32769 levels: every variant defers it, and the deep path refuses it."""
    return [MATCH_ALL, b"a/" * 32768, MATCH_NONE], "a 65536-byte topic"


def empty(n: int):
    return [b""] * n, "%d empty topics" % n


_BUILT: Dict[str, Tuple[List[bytes], str]] = {}


class Case(NamedTuple):
    name: str
    table: str
    build: Callable
    args: tuple = ()

    def topics(self) -> List[bytes]:
        if self.name not in _BUILT:
            _BUILT[self.name] = self.build(*self.args)
        return _BUILT[self.name][0]

    def note(self) -> str:
        self.topics()
        return _BUILT[self.name][1]


WINDOW = Case("window", "base", window_sweep)
FAMILIES = Case("families", "base", families)
LEVEL_LEN = [Case("len%d" % n, "base", level_len, (n,)) for n in LEVEL_LENS]
NLEV = [Case("nlev%d" % n, "deep", nlev, (n,)) for n in NLEVS]
TILE_SUM = [Case("sum%d" % s, "deep", tile_sum, (s,)) for s in TILE_SUMS]
BIG_TILE = [Case("tile%dk" % k, "base", big_tile, (k,)) for k in TILE_KIB]
DEEP300 = Case("deep300", "deep", deep300)
EMPTY = [Case("empty%d" % n, "base", empty, (n,)) for n in (1, 64, 65)]
MIB = Case("mib", "base", mib_tile)
SLASHES = Case("slashes65535", "limit", slashes_65535)
ORD65535 = Case("ordinary65535", "limit", ordinary_65535)
TOO_LONG = Case("toolong65536", "limit", too_long)

# run on every variant / the three of the deep limits / everything the engine must answer
EVERY_VARIANT = [WINDOW, FAMILIES] + LEVEL_LEN + NLEV + TILE_SUM + BIG_TILE + [DEEP300] + EMPTY
LIMITS = [MIB, SLASHES, ORD65535]
ALL_MATCHED = EVERY_VARIANT + LIMITS


# ---- the retained index's inverse match --------------------------------------------------------
def retain_names() -> List[bytes]:
    """Stored topics over the vocabulary (no near-wildcard words: published topics carry none)."""
    words = [w for w in _uniq(LEN_WORDS + FAM_AT16 + FAM_AT17 + FAM_LAST + [HEAD16] + NEAR_SEP + ORDINARY)
             if b"+" not in w and b"#" not in w]
    rng = random.Random(SEED + 1)
    names = []
    for w in words:
        names += [w, b"a/" + w, w + b"/b", b"a/" + w + b"/b"]
    for _ in range(150):
        names.append(b"/".join(rng.choice(words) for _ in range(rng.randint(1, 5))))
    return _uniq(names)


def retain_filters() -> List[bytes]:
    words = [w for w in _uniq(LEN_WORDS + FAM_AT16 + FAM_AT17 + FAM_LAST + [HEAD16] + NEAR_SEP + ORDINARY)
             if b"+" not in w and b"#" not in w]
    unknown = [w for w in TOPIC_ONLY if b"+" not in w and b"#" not in w]
    rng = random.Random(SEED + 2)
    f = [b"#", b"+", b"+/#", b"+/+", b"a/#", b"a/+/b", b"", b"/", b"+/+/b", b"a/+/#"]
    for w in words + unknown:
        f += [w, b"a/" + w, w + b"/#", b"+/" + w, b"+/" + w + b"/+", w + b"/+", b"a/" + w + b"/b"]
    for _ in range(200):
        lv = [rng.choice(words + unknown + [b"+"] * 20) for _ in range(rng.randint(1, 5))]
        if rng.random() < 0.3:
            lv[-1] = b"#"
        f.append(b"/".join(lv))
    return _uniq(f)
