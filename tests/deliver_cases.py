"""Inputs of the delivery-options tests (CPU and GPU) and their expected outputs from the
restatement (tests/deliver_ref.py): the truth table, the boundary shapes and the fuzz batch.
Every case is generated from a fixed seed and its reference is computed once per process."""

import functools
import itertools

import numpy as np

from tests import deliver_ref as R

NO_SENDER = R.NO_SENDER


class Case:
    """A table (list of set() argument tuples) and one batch."""

    def __init__(self, name, entries, offsets, subs, filters, qos, flags, frm):
        self.name = name
        self.entries = entries  # [(filter, sub, qos, nl, rap, upgrade_qos, subid or None)]
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.subs = np.asarray(subs, dtype=np.uint32)
        self.filters = np.asarray(filters, dtype=np.uint32)
        self.qos = np.asarray(qos, dtype=np.uint8)
        self.flags = np.asarray(flags, dtype=np.uint8)
        self.frm = None if frm is None else np.asarray(frm, dtype=np.uint32)
        self._ref = None

    @property
    def batch(self):
        return self.offsets, self.subs, self.filters, self.qos, self.flags, self.frm

    def sessions(self):
        s = R.Sessions()
        for f, sub, qos, nl, rap, up, subid in self.entries:
            s.set(f, sub, qos, nl, rap, up, subid)
        return s

    def load(self, table, commit=True):
        """Fills a SubOpts (emqx_amd.deliver) with the entries."""
        if self.entries:
            e = self.entries
            table.set([x[0] for x in e], [x[1] for x in e], qos=[x[2] for x in e], nl=[x[3] for x in e],
                      rap=[x[4] for x in e], upgrade_qos=[x[5] for x in e], subid=[x[6] for x in e])
        if commit:
            table.commit()
        return table

    def reference(self):
        if self._ref is None:
            self._ref = R.run_csr(self.sessions(), *self.batch)
        return self._ref


def check(case, got, compact):
    """An Enriched (emqx_amd.deliver) against the case's reference, exactly."""
    ref = case.reference()
    assert got.opts.tolist() == ref["opts"], case.name
    assert got.subids.tolist() == ref["subids"], case.name
    assert [got.summary[k] for k in ("flags", "deliveries", "kept", "dropped_no_local", "no_subopts", "qos0", "qos1",
                                     "qos2")] == ref["summary"], case.name
    if compact:
        for a, b, what in zip(got.kept, ref["kept"], ("offsets", "subs", "filters", "opts", "subids")):
            assert a.tolist() == b, (case.name, what)
    else:
        assert got.kept is None


# ---- truth table: 48 options words + the absent key, times 36 messages -----------------------

OPTION_CASES = [None] + [dict(qos=q, nl=nl, rap=rap, upgrade_qos=bool(up), subid=sid)
                         for q, nl, rap, up, sid in itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1), (None, 77))]
MESSAGE_CASES = list(itertools.product((0, 1, 2), (0, 1), (0, 2), ("self", "other", "none")))  # qos, retain, hdr, from
assert len(OPTION_CASES) == 49 and len(MESSAGE_CASES) == 36


@functools.lru_cache(maxsize=None)
def truth_table():
    """One message with one delivery per (options, message) pair: subscriber 100 + k holds
    options case k on filter 7; upgrade_qos is the subscriber's session's, as in the reference."""
    entries = [(7, 100 + k, o["qos"], o["nl"], o["rap"], o["upgrade_qos"], o["subid"])
               for k, o in enumerate(OPTION_CASES) if o is not None]
    subs, qos, flags, frm = [], [], [], []
    for k in range(len(OPTION_CASES)):
        for q, retain, hdr, who in MESSAGE_CASES:
            subs.append(100 + k)
            qos.append(q)
            flags.append(retain | hdr)
            frm.append({"self": 100 + k, "other": 5000 + k, "none": NO_SENDER}[who])
    n = len(subs)
    return Case("truth_table", entries, np.arange(n + 1), subs, [7] * n, qos, flags, frm)


# ---- shapes ----------------------------------------------------------------------------------

N_FILTERS, N_SUBS = 64, 512


def _table(rng, n_entries, p_nl):
    """n_entries distinct (filter, sub) pairs over N_FILTERS x N_SUBS with random options;
    upgrade_qos is a property of the subscriber (every third one)."""
    keys = rng.choice(N_FILTERS * N_SUBS, size=n_entries, replace=False)
    out = []
    for key in keys.tolist():
        f, s = key // N_SUBS, key % N_SUBS
        subid = int(rng.integers(1, 268435456)) if rng.random() < 0.5 else None
        out.append((f, s, int(rng.integers(0, 3)), int(rng.random() < p_nl), int(rng.integers(0, 2)), s % 3 == 0, subid))
    return out


def _batch(rng, counts, present, mode, bad_every=0):
    """Deliveries of messages with the given counts.  A message reaches a few subscribers over
    many filters, so that its publisher, when it is one of them, owns a real share of its
    deliveries.  mode: "mixed" (from is a recipient for half of the messages), "all" (every
    delivery goes to the publisher over a No Local subscription), "none" (no sender)."""
    by_sub = {}
    for f, s in present:
        by_sub.setdefault(s, []).append(f)
    subs, filters, qos, flags, frm = [], [], [], [], []
    for i, c in enumerate(counts):
        group = rng.choice(sorted(by_sub), size=int(rng.integers(1, 5)), replace=False)
        sender = NO_SENDER
        if mode == "all":
            group = group[:1]
            sender = int(group[0])
        elif mode == "mixed" and (rng.random() < 0.5 or c == max(counts)):  # the largest message always mixes
            sender = int(group[0])
        elif mode == "mixed" and rng.random() < 0.5:
            sender = int(rng.integers(N_SUBS, 2 * N_SUBS))  # a publisher that subscribes to nothing
        for _ in range(c):
            s = int(group[int(rng.integers(0, len(group)))])
            if mode != "all" and rng.random() < 0.25:
                f = int(rng.integers(N_FILTERS, 2 * N_FILTERS))  # a key that is absent
            else:
                f = by_sub[s][int(rng.integers(0, len(by_sub[s])))]
            bits = (R.SHARED_BIT if rng.random() < 0.2 else 0)
            bits |= R.RETRY_BIT if bits and rng.random() < 0.3 else 0
            subs.append(s)
            filters.append(f | bits)
        bad = bad_every and i % bad_every == bad_every - 1
        qos.append(3 if bad and i % 2 else int(rng.integers(0, 3)))
        flags.append(int(rng.integers(0, 4)) | (0x10 if bad and not i % 2 else 0))
        frm.append(sender)
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(counts) if len(counts) else []
    return off, subs, filters, qos, flags, frm


def _split(total, seed):
    """`total` deliveries over a few messages, with an empty one where there is room."""
    if total <= 1:
        return [total]
    rng = np.random.default_rng(seed)
    cuts = sorted(rng.integers(0, total + 1, size=3).tolist())
    return [cuts[0], 0, cuts[1] - cuts[0], cuts[2] - cuts[1], total - cuts[2]]


SHAPES = {
    "n0": [],
    "empty3": [0, 0, 0],
    "1": [1],
    **{str(t): _split(t, t) for t in (63, 64, 65, 255, 256, 257)},
    "10002": [0, 1, 10000, 0, 1],
}
SHAPE_CASES = [(name, "mixed") for name in SHAPES] + [("257", "all"), ("257", "none"), ("10002", "all"), ("10002", "none")]


@functools.lru_cache(maxsize=None)
def shape(name, mode):
    rng = np.random.default_rng(1000 + sum(map(ord, name + mode)))
    if mode == "all":  # every key present with nl = 1
        entries = [(f, s, qos, 1, rap, up, sid) for f, s, qos, _, rap, up, sid in _table(rng, 4000, 1.0)]
    else:
        entries = _table(rng, 4000, 0.75)
    present = [(e[0], e[1]) for e in entries]
    return Case("shape_%s_%s" % (name, mode), entries, *_batch(rng, SHAPES[name], present, mode))


# ---- fuzz ------------------------------------------------------------------------------------

FUZZ_ENTRIES, FUZZ_MESSAGES = 20_000, 2_000


@functools.lru_cache(maxsize=None)
def fuzz(seed=11):
    rng = np.random.default_rng(seed)
    entries = _table(rng, FUZZ_ENTRIES, 0.75)
    counts = rng.integers(0, 151, size=FUZZ_MESSAGES).tolist()  # about 150 K deliveries
    return Case("fuzz_%d" % seed, entries, *_batch(rng, counts, [(e[0], e[1]) for e in entries], "mixed", bad_every=100))
