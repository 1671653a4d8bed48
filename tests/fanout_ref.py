"""Sequential restatement of the publish fan-out, positions included.

Plain Python and numpy, no project code.  Where the oracle (oracle/broker_ref.py,
oracle/fanout_oracle.cpp) lists a topic's deliveries in route order and the GPU tests compare them
as multisets per topic, this one states where every match entry's deliveries lie in the output:

* topics in order, and inside a topic its match entries in CSR order; entry e's deliveries are the
  segment ``[entry_off[e], entry_off[e + 1])`` of the output, ``out_off[t]`` the start of topic
  t's first entry (of the next topic's for a topic without entries; the total past the last);
* inside a segment the filter's plain subscribers come first (``n_plain[e]`` of them, filter word =
  the filter id), then one pick per live ``$share`` group (filter word = id | SHARED_BIT);
* a filter id without subscriptions, in the table's range or beyond it, has no deliveries.

The order of the plain subscribers inside their part, and of the groups inside theirs, is not part
of the contract: ``seg`` numbers the parts (2 e for entry e's plain part, 2 e + 1 for its picks)
so that a comparison sorts inside each part (``part_sorted``).

Picks: hash_clientid / hash_topic take member ``key % n`` in subscription order; round_robin with
the counter seeded 0 takes member 0 first and then ``(last + 1) % n`` per (filter, group,
publisher) in message order, the state kept in the table across calls (``forget`` drops
publishers); a group of one member is picked without touching the state.  sticky and random have
no restated pick: ``subs`` holds NO_PICK there and ``pick_pos`` / ``pick_fg`` / ``pick_topic``
name each pick's position, (filter, group) and topic for the invariants.  A call that needs more
than ``cap`` deliveries makes no ids and consumes no state."""

import numpy as np

SHARED_BIT = 0x80000000
NO_GROUP = 0xFFFFFFFF
NO_PICK = 0xFFFFFFFF
RANDOM, ROUND_ROBIN, STICKY, HASH_CLIENTID, HASH_TOPIC = 0, 1, 2, 3, 4


class Table:
    """Subscription rows (filter, subscriber, group) in subscription order; group NO_GROUP: plain."""

    def __init__(self, sub_filter, sub_id, sub_group):
        self.plain = {}   # filter -> [subscriber]
        self.groups = {}  # filter -> {group: [member]} (dicts keep first-subscription order)
        for f, s, g in zip(map(int, sub_filter), map(int, sub_id), map(int, sub_group)):
            if g == NO_GROUP:
                self.plain.setdefault(f, []).append(s)
            else:
                self.groups.setdefault(f, {}).setdefault(g, []).append(s)
        self.rr = {}      # (filter, group, publisher) -> last member index

    def n_plain(self, f):
        return len(self.plain.get(f, ()))

    def n_groups(self, f):
        return len(self.groups.get(f, ()))

    def deliveries(self, f):
        return self.n_plain(f) + self.n_groups(f)

    def forget(self, publishers):
        gone = set(map(int, publishers))
        self.rr = {k: v for k, v in self.rr.items() if k[2] not in gone}


class Result:
    """out_off [n + 1], total, entry_off [m + 1], n_plain [m]; overflow: total > cap, and then
    subs / fils / seg are None.  Otherwise subs, fils, seg [total] and the pick lists."""


def fanout(table, moff, mids, keys, strategy, cap):
    moff = [int(x) for x in moff]
    n = len(moff) - 1
    base, m = moff[0], moff[n] - moff[0]
    r = Result()
    entry_off = np.zeros(m + 1, np.uint64)
    n_plain = np.zeros(m, np.uint32)
    out_off = np.zeros(n + 1, np.uint64)
    at = 0
    for t in range(n):
        out_off[t] = at
        for j in range(moff[t], moff[t + 1]):
            f = int(mids[j])
            entry_off[j - base] = at
            n_plain[j - base] = table.n_plain(f)
            at += table.deliveries(f)
    out_off[n] = at
    entry_off[m] = at
    r.out_off, r.total, r.entry_off, r.n_plain = out_off, at, entry_off, n_plain
    r.overflow = at > cap
    r.subs = r.fils = r.seg = None
    r.pick_pos, r.pick_fg, r.pick_topic = [], [], []
    if r.overflow:
        return r
    subs, fils, seg = [], [], []
    rr = table.rr
    for t in range(n):
        key = int(keys[t]) if keys is not None else 0
        for j in range(moff[t], moff[t + 1]):
            f, e = int(mids[j]), j - base
            assert len(subs) == int(entry_off[e])
            p = table.plain.get(f, ())
            subs += p
            fils += [f] * len(p)
            seg += [2 * e] * len(p)
            for g, mem in table.groups.get(f, {}).items():
                k = len(mem)
                if k == 1:
                    pick = mem[0]
                elif strategy in (HASH_CLIENTID, HASH_TOPIC):
                    pick = mem[key % k]
                elif strategy == ROUND_ROBIN:
                    last = rr.get((f, g, key))
                    idx = 0 if last is None else (last + 1) % k
                    rr[(f, g, key)] = idx
                    pick = mem[idx]
                else:
                    pick = NO_PICK
                r.pick_pos.append(len(subs))
                r.pick_fg.append((f, g))
                r.pick_topic.append(t)
                subs.append(pick)
                fils.append(f | SHARED_BIT)
                seg.append(2 * e + 1)
    r.subs = np.array(subs, np.uint32)
    r.fils = np.array(fils, np.uint32)
    r.seg = np.array(seg, np.int64)
    assert len(subs) == at
    return r


def part_sorted(seg, subs):
    """subs sorted inside each part of seg (seg is non-decreasing), the parts left where they are."""
    return np.asarray(subs)[np.lexsort((np.asarray(subs), np.asarray(seg)))]


def by_topic(out_off, subs, fils):
    """The CSR as per-topic sorted (subscriber, filter word) lists (for a comparison with a
    route-order oracle)."""
    return [sorted(zip(subs[int(a):int(b)].tolist(), fils[int(a):int(b)].tolist()))
            for a, b in zip(out_off[:-1], out_off[1:])]
