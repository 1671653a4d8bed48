"""The batched authorization check on the device (include/emqx_authz.h, authz_kernels.hip)
against the restatement of emqx_authz_rule (tests/authz_ref.py), verdict for verdict and tag
for tag; every rule of a table has its own tag.  Tables stay under 300 rules and 4096 clients,
batches under 20,000 requests."""

import numpy as np
import pytest

from tests import authz_cases as C
from tests import authz_ref as R

pytestmark = pytest.mark.gpu

GROUPS = (1, 4, 16, 64)


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import authz
    return authz


def dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda:0")


def device_batch(requests):
    from emqx_amd.engine import pack
    cl, ac, topics = requests
    buf, offs = pack(list(topics))
    return (dev(np.asarray(cl, np.uint32)), dev(np.asarray(ac, np.uint8)), dev(buf), dev(offs), len(topics))


def run_device(a, batch, asynchronous=False, stream=0):
    """-> (verdicts, tags, summary or None) through the device entry points."""
    import torch
    d_cl, d_ac, d_buf, d_off, n = batch
    d_v = torch.full((max(n, 1),), 77, dtype=torch.uint8, device="cuda:0")
    d_t = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda:0")
    summ = None
    if asynchronous:
        d_s = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
        a.check_device_async(d_cl.data_ptr(), d_ac.data_ptr(), d_buf.data_ptr(), d_off.data_ptr(), n, d_v.data_ptr(),
                             d_t.data_ptr(), d_s.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        summ = d_s.cpu().numpy().tolist()
    else:
        a.check_device(d_cl.data_ptr(), d_ac.data_ptr(), d_buf.data_ptr(), d_off.data_ptr(), n, d_v.data_ptr(),
                       d_t.data_ptr(), stream=stream)
    return d_v.cpu().numpy()[:n].tolist(), d_t.cpu().numpy().view(np.uint32)[:n].tolist(), summ


def apply_default(verdicts, no_match):
    return [R.VERDICT[no_match] if (no_match and v == R.NOMATCH) else v for v in verdicts]


def loaded(A, table):
    a = table.load(A.Authz(0))
    a.commit()
    return a


def test_fixture_through_every_entry_point(A):
    from emqx_amd.engine import pack
    for table in C.fixture_tables():
        a = loaded(A, table)
        ev, et = table.reference()
        v, t = a.check(*table.requests, no_match=table.no_match)
        assert (v.tolist(), t.tolist()) == (ev, et), table.name
        cl, ac, topics = table.requests
        v, t = a.check_packed(cl, ac, *pack(list(topics)), no_match=table.no_match)
        assert (v.tolist(), t.tolist()) == (ev, et), table.name
        batch = device_batch(table.requests)
        v, t, _ = run_device(a, batch)
        assert (apply_default(v, table.no_match), t) == (ev, et), table.name
        v, t, s = run_device(a, batch, asynchronous=True)
        assert (apply_default(v, table.no_match), t) == (ev, et), table.name
        assert s[:5] == [0, v.count(R.ALLOW), v.count(R.DENY), v.count(R.NOMATCH), 0], (table.name, s)
        vh, th = a.check_host(*table.requests, no_match=table.no_match)
        assert (vh.tolist(), th.tolist()) == (ev, et), table.name
        a.close()


@pytest.mark.parametrize("seed", range(20))
def test_dense_fuzz(A, seed):
    table = C.dense_table(seed)
    a = loaded(A, table)
    ev, et = table.reference()
    v, t = a.check(*table.requests)
    assert (v.tolist(), t.tolist()) == (ev, et)
    assert a.stats()["last_group"] in GROUPS and a.stats()["last_evals"] > 0
    for g in GROUPS:  # every launch shape gives the same answers
        a.set_tuning("group", g)
        v, t = a.check(*table.requests)
        assert (v.tolist(), t.tolist()) == (ev, et), g
        assert a.stats()["last_group"] == g


@pytest.mark.parametrize("seed", range(3))
def test_long_list_fuzz(A, seed):
    table = C.long_table(seed)
    a = loaded(A, table)
    ev, et = table.reference()
    assert len(set(et)) > 50  # the deciding rules are spread over the lists
    for g in (0,) + GROUPS:
        a.set_tuning("group", g)
        v, t = a.check(*table.requests)
        assert (v.tolist(), t.tolist()) == (ev, et), g
    a.set_tuning("group", 0)
    a.check(*table.requests)
    assert a.stats()["last_group"] == 64  # a small batch of long requests: a wave each fills the device
    batch = device_batch(table.requests)
    v, t, s = run_device(a, batch, asynchronous=True)
    assert (v, t) == (ev, et)
    assert s[:5] == [1, ev.count(R.ALLOW), ev.count(R.DENY), ev.count(R.NOMATCH), ev.count(R.BAD)]


def staircase_table(n_rules=200):
    """Request K's first matching rule is rule K, and EVERY later rule matches it too, with allow
    and deny alternating: rule i's filter is (n - i) '+' levels and '#', topic K has n - K levels.
    A formulation that lets a later lane, chunk or segment win fails at once."""
    rules = [("allow" if i % 2 == 0 else "deny", "all", "all", [b"+/" * (n_rules - i) + b"#"]) for i in range(n_rules)]
    split = [0, 61, 64, 129, n_rules]  # list boundaries off the chunk boundaries: segments of 61, 3, 65, 71 entries
    lists = [(s, "all", None, rules[split[s]:split[s + 1]]) for s in range(4)]
    topics = [b"/".join([b"x"] * (n_rules - k)) for k in range(n_rules)]
    clients = [{"id": 0, "clientid": "c"}]
    return C.Table("staircase", lists, clients, ([0] * n_rules, [1 + k % 2 for k in range(n_rules)], topics))


def test_first_hit_wins_over_later_rules_of_the_opposite_permission(A):
    table = staircase_table()
    ev, et = table.reference()
    assert et == list(range(200)) and ev == [R.ALLOW if k % 2 == 0 else R.DENY for k in range(200)]
    a = loaded(A, table)
    for g in (0,) + GROUPS:
        a.set_tuning("group", g)
        v, t = a.check(*table.requests)
        assert (v.tolist(), t.tolist()) == (ev, et), g


def test_first_filter_of_a_rule_and_keyed_lists_come_first(A):
    # the same topic is matched by the username list, the clientid list and the all list
    lists = [(0, "all", None, [("deny", "all", "all", ["#"])]),
             (0, "username", "u", [("allow", "all", "all", ["n", "t/#", "t/+"]), ("deny", "all", "all", ["t/x"])]),
             (0, "clientid", "c", [("deny", "all", "publish", ["t/x"])]),
             (1, "clientid", "c", [("allow", "all", "all", ["#"])])]
    clients = [{"id": 0, "clientid": "c", "username": "u"}, {"id": 1, "clientid": "c2", "username": "u"},
               {"id": 2, "clientid": "c"}, {"id": 3}]
    req = ([0, 0, 1, 2, 2, 3], [1, 2, 1, 1, 2, 1], [b"t/x"] * 6)
    table = C.Table("scopes", lists, clients, req)
    ev, et = table.reference()
    assert ev == [R.DENY, R.ALLOW, R.ALLOW, R.DENY, R.DENY, R.DENY] and et == [3, 1, 1, 3, 0, 0]
    a = loaded(A, table)
    for g in (0,) + GROUPS:
        a.set_tuning("group", g)
        v, t = a.check(*req)
        assert (v.tolist(), t.tolist()) == (ev, et), g


def test_bad_requests_do_not_fail_the_batch(A):
    import torch
    a = A.Authz(0)
    a.set_list(0, [("allow", "all", "publish", ["t"]), ("deny", "all")], tags=[10, 11])
    a.set_clients([{"id": 0, "clientid": "c"}, {"id": 2, "clientid": "d"}])
    a.commit()
    cl = [0, 1, 3, 0xFFFFFFFF, 0, 0, 2]
    ac = [1, 1, 1, 1, 0, 3, 2]
    v, t = a.check(cl, ac, [b"t"] * 7)
    assert v.tolist() == [A.ALLOW, 3, 3, 3, 3, 3, A.DENY]
    assert t.tolist() == [10] + [A.TAG_NONE] * 5 + [11]
    # the device entry point: a topic whose offsets decrease is a bad request, its neighbours are answered
    d_cl, d_ac = dev(np.array([0, 0, 0, 2], np.uint32)), dev(np.array([1, 1, 1, 2], np.uint8))
    d_buf, d_off = dev(np.frombuffer(b"ttxx", np.uint8)), dev(np.array([0, 1, 0, 1, 2], np.uint64))
    for asynchronous in (False, True):
        v, t, s = run_device(a, (d_cl, d_ac, d_buf, d_off, 4), asynchronous=asynchronous)
        assert v == [A.ALLOW, 3, A.ALLOW, A.DENY] and t == [10, A.TAG_NONE, 10, 11]
        if asynchronous:
            assert s[:5] == [1, 2, 1, 0, 1]
    # host buffers: the same offsets are an argument error before any launch
    from emqx_amd import _lib
    with pytest.raises(_lib.EngineError) as e:
        a.check_packed([0, 0, 0, 2], [1] * 4, np.frombuffer(b"ttxx", np.uint8), np.array([0, 1, 0, 1, 2], np.uint64))
    assert e.value.code == _lib.EMQX_EINVAL
    # an empty batch and an empty table
    assert a.check([], [], [])[0].size == 0
    b = A.Authz(0)
    b.commit()
    assert b.check([0], [1], [b"t"])[0].tolist() == [3]
    b.set_clients([{"id": 0}])
    b.commit()
    assert b.check([0], [1], [b"t"])[0].tolist() == [A.NOMATCH]
    torch.cuda.synchronize()


def test_maximal_topics_and_principals(A):
    big = b"x" * 65535  # the longest principal and eq filter; `most` + "/#" is the longest plain filter
    most, rest = big[:65533], big[:65532]
    rules = [("allow", ("clientid", big), "publish", [b"p/${clientid}", ("eq", big)]),
             ("deny", ("username", rest), "all", [most + b"/#", b"${username}"]),
             ("allow", "all", "all", [b"+/" + most])]
    clients = [{"id": 0, "clientid": big, "username": big}, {"id": 1, "clientid": rest, "username": rest}]
    topics = [b"p/" + big, big, rest, rest + b"/q", b"z/" + most, b"p/" + most, most, b"q/" + rest]
    req = ([0, 0, 0, 0, 0, 1, 1, 1], [1] * 8, topics)
    table = C.Table("maximal", [(0, "all", None, rules)], clients, req)
    ev, et = table.reference()
    assert ev == [R.ALLOW, R.ALLOW, R.NOMATCH, R.NOMATCH, R.ALLOW, R.ALLOW, R.DENY, R.NOMATCH]
    assert et[:2] == [0, 0] and et[4:7] == [2, 2, 1]
    a = loaded(A, table)
    for g in (0, 1, 64):
        a.set_tuning("group", g)
        v, t = a.check(*req)
        assert (v.tolist(), t.tolist()) == (ev, et), g


def test_default_acl_batch_picks_a_small_group(A):
    table = [t for t in C.fixture_tables() if t.name == "default_acl_conf"][0]
    n = 20000
    clients = [dict(table.clients[i % 3], id=i) for i in range(4096)]
    topics = [b"$SYS/brokers", b"t", b"a/b", b"", b"$SYS/x/y", b"+/#"]
    req = ([(7 * i) % 4096 for i in range(n)], [1 + (i // 3) % 2 for i in range(n)], [topics[i % 6] for i in range(n)])
    big = C.Table("acl20000", table.lists, clients, req)
    ev, et = big.reference()
    a = loaded(A, big)
    v, t = a.check(*req)
    assert (v.tolist(), t.tolist()) == (ev, et)
    s = a.stats()
    assert s["last_group"] == 4 and s["n_clients"] == 4096 and s["n_entries"] == 3
    assert 0 < s["last_evals"] <= 3 * n


def test_async_call_keeps_its_snapshot_across_a_commit(A):
    import torch
    table = C.long_table(0)
    a = loaded(A, table)
    ev, et = table.reference()
    d_cl, d_ac, d_buf, d_off, n = device_batch(table.requests)
    stream = torch.cuda.Stream(device="cuda:0")
    outs = []
    for _ in range(3):
        outs.append((torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0"),
                     torch.zeros(8, dtype=torch.int64, device="cuda:0")))
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        for d_v, d_t, d_s in outs:
            a.check_device_async(d_cl.data_ptr(), d_ac.data_ptr(), d_buf.data_ptr(), d_off.data_ptr(), n, d_v.data_ptr(),
                                 d_t.data_ptr(), d_s.data_ptr(), stream=stream.cuda_stream)
    # replace the table while the calls may still be running: they answer from the old snapshot
    for s in range(4):
        a.clear_source(s)
    a.set_list(0, [("deny", "all")], tags=[999])
    a.commit()
    stream.synchronize()
    for d_v, d_t, d_s in outs:
        assert d_v.cpu().numpy().tolist() == ev
        assert d_t.cpu().numpy().view(np.uint32).tolist() == et
    v, t = a.check(*table.requests)
    known = [x != R.BAD for x in ev]
    assert all((x == R.DENY and y == 999) if k else x == R.BAD for x, y, k in zip(v.tolist(), t.tolist(), known))


def test_chains_in_front_of_the_match_on_one_stream(A):
    """authz -> route match, both asynchronous on the same stream, no host wait between them."""
    import torch
    from emqx_amd.engine import Engine
    table = C.dense_table(3, n_requests=1000)
    a = loaded(A, table)
    e = Engine(0)
    e.insert([b"a/#", b"+/b", b"dev/+"])
    e.commit()
    ev, et = table.reference()
    d_cl, d_ac, d_buf, d_off, n = device_batch(table.requests)
    d_v = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    d_t = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_s = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    cap = 8 * n
    d_oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    d_ids = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
    d_ms = torch.zeros(e.SUMMARY_WORDS, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        a.check_device_async(d_cl.data_ptr(), d_ac.data_ptr(), d_buf.data_ptr(), d_off.data_ptr(), n, d_v.data_ptr(),
                             d_t.data_ptr(), d_s.data_ptr(), stream=stream.cuda_stream)
        e.match_device_async(d_buf.data_ptr(), d_off.data_ptr(), n, d_oo.data_ptr(), d_ids.data_ptr(), cap,
                             d_ms.data_ptr(), mode=0, stream=stream.cuda_stream)
    stream.synchronize()
    assert d_v.cpu().numpy().tolist() == ev and d_t.cpu().numpy().view(np.uint32).tolist() == et
    if int(d_ms[0]) == 0:  # the match call completed in its first scratch: its offsets are final
        want, _ = e.match_packed(d_buf.cpu().numpy(), d_off.cpu().numpy().view(np.uint64), mode=0)
        assert d_oo.cpu().numpy().tolist() == want.astype(np.int64).tolist()


def test_async_calls_do_not_wait_for_each_other(A):
    """A pipeline enqueues call after call: no call may wait on the host for an earlier one to
    drain.  16 calls of a deliberately slow shape (a lane per request over 300 rules) are
    enqueued on one stream; the host must be done enqueueing in less than half the time the
    device needs to run them (a call that waited for its predecessor would take all of it)."""
    import time
    import torch
    table = C.long_table(0)
    a = loaded(A, table)
    a.set_tuning("group", 1)
    cl, ac, topics = table.requests
    d_cl, d_ac, d_buf, d_off, n = device_batch((cl * 10, ac * 10, topics * 10))
    calls = 16
    outs = [(torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0"),
             torch.zeros(8, dtype=torch.int64, device="cuda:0")) for _ in range(calls)]
    stream = torch.cuda.Stream(device="cuda:0")
    stream.wait_stream(torch.cuda.current_stream())
    host_s = device_ms = 0.0
    for timed in (False, True):  # the first round creates the per-call scratch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            t0 = time.perf_counter()
            for d_v, d_t, d_s in outs:
                a.check_device_async(d_cl.data_ptr(), d_ac.data_ptr(), d_buf.data_ptr(), d_off.data_ptr(), n,
                                     d_v.data_ptr(), d_t.data_ptr(), d_s.data_ptr(), stream=stream.cuda_stream)
            host_s = time.perf_counter() - t0
            e1.record()
        stream.synchronize()
        device_ms = e0.elapsed_time(e1)
    print("host enqueue %.3f ms, device %.3f ms for %d calls" % (host_s * 1e3, device_ms, calls))
    ev, et = table.reference()
    for d_v, d_t, _ in outs:
        assert d_v.cpu().numpy().tolist() == ev * 10 and d_t.cpu().numpy().view(np.uint32).tolist() == et * 10
    assert host_s * 1e3 < 0.5 * device_ms, (host_s * 1e3, device_ms)
