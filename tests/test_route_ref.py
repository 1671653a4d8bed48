"""tests/route_ref.py pinned by the known answers the reference has (apps/emqx/test/
emqx_router_SUITE.erl:62-79 idempotent add and delete, :81-95 t_match_routes), and, because the
reference has no test of aggre/1 over several nodes, the literal aggre/1 checked against an
independent set formulation on fuzz tables: unpinned by the reference beyond the router suite."""
import random

from tests import route_ref as R

NODE = "emqx@127.0.0.1"


def test_add_delete_kat():
    """t_add_delete / t_do_add_delete."""
    t = R.RouteTab(NODE)
    t.do_add_route(b"a/b/c")
    t.do_add_route(b"a/b/c", NODE)
    t.do_add_route(b"a/+/b", NODE)
    assert sorted(t.topics()) == [b"a/+/b", b"a/b/c"]
    assert len(t.tab) == 2  # the second add changed nothing
    t.do_delete_route(b"a/b/c", NODE)
    t.do_delete_route(b"a/+/b")
    assert t.topics() == [] and t.tab == []
    t.do_delete_route(b"a/+/b")  # absent: ignored


def test_match_routes_kat():
    """t_match_routes: the trie's answer for a/b/c is given, the bag supplies the records."""
    t = R.RouteTab(NODE)
    for f in (b"a/b/c", b"a/+/c", b"a/b/#", b"#"):
        t.do_add_route(f, NODE)
    matched = [b"a/b/c", b"#", b"a/+/c", b"a/b/#"]  # [Topic | emqx_trie:match(Topic)]
    got = t.match_routes(matched)
    assert sorted(got) == [R.Route(b"#", NODE), R.Route(b"a/+/c", NODE), R.Route(b"a/b/#", NODE), R.Route(b"a/b/c", NODE)]
    for f in (b"a/b/c", b"a/+/c", b"a/b/#", b"#"):
        t.do_delete_route(f, NODE)
    assert t.match_routes(matched) == []
    assert t.has_routes(b"#") is False


def test_aggre_clauses():
    assert R.aggre([]) == []
    assert R.aggre([R.Route(b"t", "n1")]) == [(b"t", "n1")]
    assert R.aggre([R.Route(b"t", (b"g", "n1"))]) == [(b"t", b"g")]
    # the fold conses plain routes and usorts at every grouped one: a group hosted on two nodes is one entry
    got = R.aggre([R.Route(b"t", (b"g", "n1")), R.Route(b"t", "n2"), R.Route(b"t", (b"g", "n2")), R.Route(b"t", "n1")])
    assert sorted(got, key=R.term_key) == [(b"t", "n1"), (b"t", "n2"), (b"t", b"g")]
    assert R.route([], "n1") == "dropped"
    assert R.route(got, "n1").count(("dispatch", b"t")) == 1
    assert ("forward", "n2", b"t") in R.route(got, "n1") and ("share", b"t", b"g") in R.route(got, "n1")


def test_cleanup_routes():
    t = R.RouteTab("n1")
    t.do_add_route(b"a", "n1")
    t.do_add_route(b"a", "n2")
    t.do_add_route(b"b", (b"g", "n2"))
    t.do_add_route(b"b", (b"g", "n1"))
    t.do_add_route(b"c", "n2")
    t.cleanup_routes("n2")
    assert t.tab == [R.Route(b"a", "n1"), R.Route(b"b", (b"g", "n1"))]
    assert not t.has_routes(b"c")


def fuzz_table(rng, n_nodes):
    t = R.RouteTab("n0")
    topics = [b"t/%d" % k for k in range(30)]
    for _ in range(200):
        to = rng.choice(topics)
        node = "n%d" % rng.randrange(n_nodes)
        dest = node if rng.random() < 0.6 else (b"g%d" % rng.randrange(4), node)
        if rng.random() < 0.85:
            t.do_add_route(to, dest)
        else:
            t.do_delete_route(to, dest)
    return t, topics


def test_aggre_against_sets_on_fuzz():
    rng = random.Random(5)
    for n_nodes in (1, 2, 5, 64):
        t, topics = fuzz_table(rng, n_nodes)
        assert len(set(t.tab)) == len(t.tab)  # a bag
        for _ in range(100):
            matched = rng.sample(topics, rng.randrange(0, 6))
            routes = t.match_routes(matched)
            lit, sets = R.aggre(routes), R.aggre_sets(routes)
            assert sorted(lit, key=R.term_key) == sorted(sets, key=R.term_key)
            # distinct filters differ in To: aggregating each filter on its own gives the same multiset
            each = [e for to in matched for e in R.aggre(t.lookup_routes(to))]
            assert sorted(each, key=R.term_key) == sorted(lit, key=R.term_key)


def test_route_batch_counts():
    t = R.RouteTab("n0")
    t.do_add_route(b"x", "n0")
    t.do_add_route(b"x", "n1")
    t.do_add_route(b"y", (b"g", "n1"))
    t.do_add_route(b"y", (b"g", "n2"))
    e = R.route_batch(t, {0: b"x", 1: b"y"}, [0, 2, 2, 4], [0, 1, 9, 0])
    assert e.entry_flags == [R.LOCAL | R.REMOTE, R.SHARE, 0, R.LOCAL | R.REMOTE]
    assert e.msg_routes == [3, 0, 2]
    assert e.forwards == {"n1": [(0, 0), (2, 0)]}
    assert e.local == [[0, 1], [], [0]]
    assert e.summary == dict(flags=0, entries=4, forwards=2, dropped=1, forwarding_messages=2, kept=3, unknown=1,
                             forward_nodes=1)
