"""Shared by the authorization tests: the fixture (tests/golden/authz_kats.json) and the two fuzz
generators, each as a list of *tables* — (lists, clients, requests) — that is loaded into the
library and into the restatement (tests/authz_ref.py) alike.  Every rule of a table gets a
distinct tag, so a right verdict from the wrong rule fails the comparison."""

from __future__ import annotations

import functools
import json
import os
import random

from tests import authz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION = {"publish": 1, "subscribe": 2}


def _term(x):
    """{"t": [...]} -> tuple, arrays -> lists."""
    if isinstance(x, dict):
        return tuple(_term(y) for y in x["t"])
    if isinstance(x, list):
        return [_term(y) for y in x]
    return x


def load_kats():
    with open(os.path.join(ROOT, "tests", "golden", "authz_kats.json")) as f:
        doc = json.load(f)
    for c in doc["cases"]:
        for l in c["lists"]:
            l["rules"] = [_term(r) for r in l["rules"]]
    return doc


class Table:
    """lists: [(source, scope, key, rules)], clients: [dict], requests: ([client], [action], [topic])."""

    def __init__(self, name, lists, clients, requests, no_match=None, expect=None):
        self.name, self.lists, self.clients, self.requests = name, lists, clients, requests
        self.no_match, self.expect = no_match, expect
        self._ref = None

    def load(self, t):
        """Fills an emqx_amd.authz.Authz or an authz_ref.RefTable: tags count up across the lists."""
        tag = 0
        for source, scope, key, rules in self.lists:
            t.set_list(source, rules, scope=scope, key=key, tags=list(range(tag, tag + len(rules))))
            tag += len(rules)
        t.set_clients(self.clients)
        return t

    def reference(self):
        """(verdicts, tags) of the restatement, computed once."""
        if self._ref is None:
            self._ref = self.load(R.RefTable()).check(*self.requests, no_match=self.no_match)
        return self._ref


def fixture_tables():
    out = []
    for c in load_kats()["cases"]:
        req = ([x[0] for x in c["checks"]], [ACTION[x[1]] for x in c["checks"]], [x[2].encode() for x in c["checks"]])
        out.append(Table(c["name"], [(l["source"], l["scope"], l["key"], l["rules"]) for l in c["lists"]],
                         c["clients"], req, c.get("no_match"), [x[3] for x in c["checks"]]))
    return out


def _requests(rng, n, n_clients, topic):
    # one request in fifty is bad: an unknown client or an action outside 1..2
    cl = [rng.randrange(n_clients) if rng.random() > 0.01 else n_clients + rng.randrange(3) for _ in range(n)]
    ac = [rng.randint(1, 2) if rng.random() > 0.01 else rng.choice([0, 3, 255]) for _ in range(n)]
    return cl, ac, [topic(rng) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def dense_table(seed, n_rules=8, n_clients=32, n_requests=2000):
    """Dense fuzz: few rules of every shape over a small vocabulary, so that most requests match
    something and every clause of the predicate is taken.  One list in three is keyed."""
    rng = random.Random(seed)
    lists = [(0, "all", None, [R.rand_rule(rng) for _ in range(n_rules)])]
    if seed % 3 == 1:
        lists.append((0, "clientid", rng.choice(R.PRINCIPALS), [R.rand_rule(rng) for _ in range(2)]))
        lists.append((1, "username", rng.choice(R.PRINCIPALS), [R.rand_rule(rng) for _ in range(2)]))
    clients = [R.rand_client(rng, i) for i in range(n_clients)]
    return Table("dense%d" % seed, lists, clients, _requests(rng, n_requests, n_clients, R.rand_topic))


@functools.lru_cache(maxsize=None)
def long_table(seed, n_rules=300, n_clients=64, n_requests=2000):
    """Long-list fuzz: 300 rules that mostly miss (a literal first level out of 40), with allow and
    deny alternating at random, so the deciding entry lies deep in the list and a later hit of
    the opposite permission sits behind it: the first hit must win across chunks of 64 entries,
    across the filters of one rule and across the segments of keyed lists."""
    rng = random.Random(1000 + seed)
    firsts = [b"k%d" % i for i in range(40)]

    def rule():
        topics = [rng.choice(firsts) + b"/" + R.rand_filter_plain(rng) for _ in range(rng.randint(1, 3))]
        who = "all" if rng.random() < 0.7 else R.rand_who(rng)
        return (rng.choice(["allow", "deny"]), who, rng.choice(["publish", "subscribe", "all"]), topics)

    n_keyed = 20
    lists = [(0, "all", None, [rule() for _ in range(n_rules - 2 * n_keyed - 10)]),
             (0, "clientid", b"c1", [rule() for _ in range(n_keyed)]),
             (0, "username", b"u1", [rule() for _ in range(n_keyed)]),
             (2, "all", None, [rule() for _ in range(10)])]
    clients = [R.rand_client(rng, i) for i in range(n_clients)]
    return Table("long%d" % seed, lists, clients,
                 _requests(rng, n_requests, n_clients, lambda r: r.choice(firsts) + b"/" + R.rand_topic(r, 3)))
