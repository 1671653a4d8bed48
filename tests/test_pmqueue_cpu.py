"""CPU-side checks of the priority mqueue stage (include/emqx_pmqueue.h) on a host-only handle: the
literal restatement (tests/pmqueue_ref.py) against the known answers of the reference's own suite
(tests/golden/pmqueue_kats.json), emqx_pmqueue_put_host and emqx_pmqueue_take_host against the
restatement on every case and in a seeded fuzz, the differential against the plain mqueue stage at one
class, the ABI."""

import ctypes
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import pmqueue_cases as C
from tests import pmqueue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, EOVERFLOW, ENOTFOUND = -1, -3, -4, -5
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pmqueue_kats.json")))
PUT_CASES = C.put_cases()
TAKE_CASES = C.take_cases()


@pytest.fixture(scope="module")
def T():
    from emqx_amd import pmqueue
    return pmqueue


def host(T):
    return T.Pmqueue(T.HOST_ONLY)


def put(T, case, update_table=True, h=None, fn="put_host"):
    """One put on copies of the case's tables; a bad subscriber's EINVAL carries the outputs."""
    from emqx_amd import _lib
    sessions, ring, heads = case.sessions.copy(), case.ring.copy(), T.aligned_heads(case.heads)
    want = case.reference()["summary"][0]
    try:
        got = getattr(h or host(T), fn)(case.subs, case.offsets, case.opts, case.verdicts, case.src, case.msg_class, case.tables,
                                      sessions, ring, heads, refs=case.refs, update_table=update_table)
        assert not want & R.F_BAD_SUB
    except _lib.EngineError as e:
        assert e.code == EINVAL and want & R.F_BAD_SUB and e.summary["flags"] == want
        got = e.partial
    return got, sessions, ring, heads


def take(T, case, update_table=True, cap_out="case", h=None, fn="take_host"):
    from emqx_amd import _lib
    sessions, ring, heads = case.sessions.copy(), case.ring.copy(), T.aligned_heads(case.heads)
    cap = case.cap_out if cap_out == "case" else cap_out
    want = case.reference(cap_out)["summary"][0]
    try:
        got = getattr(h or host(T), fn)(case.subs, case.tables, sessions, ring, heads, case.now, deadlines=case.deadlines, cap_out=cap,
                                       update_table=update_table)
        assert not want & (R.F_BAD_SUB | R.F_OUTPUT_FULL)
    except _lib.EngineError as e:
        assert e.code == (EOVERFLOW if want & R.F_OUTPUT_FULL else EINVAL) and e.summary["flags"] == want
        got = e.partial
    return got, sessions, ring, heads


# ---- the known answers -----------------------------------------------------------------------------

def test_kats_cover_the_named_suite_tests():
    assert [k["source"] for k in GOLDEN["kats"]] == ["emqx_mqueue_SUITE:" + t for t in (
        "t_priority_mqueue", "t_priority_order", "t_priority_order2", "t_infinity_priority_mqueue", "t_length_priority_mqueue")]
    assert "by hand" in GOLDEN["comment"]


@pytest.mark.parametrize("kat", GOLDEN["kats"], ids=[k["name"] for k in GOLDEN["kats"]])
def test_restatement_against_the_reference_suite(kat):
    mq = R.MQ(kat["max_len"], kat["mult"], 0)
    for step in kat["steps"]:
        if step[0] == "in":
            R.mq_in((step[2], 1, None), step[1], mq)
        elif step[0] == "len":
            assert mq.len == step[1] and sum(len(dq) for _, dq in mq.q) == step[1]
        elif step[0] == "out":
            assert R.mq_out(mq) is not None
        elif step[0] == "drain":
            got = []
            while mq.len:
                msg, p = R.mq_out(mq)
                got.append([p, msg[0]])
            assert got == step[1] and R.mq_out(mq) is None
        else:
            assert step[0] == "stats" and [mq.len, mq.max_len, mq.dropped] == step[1:]


@pytest.mark.parametrize("kat", [k for k in GOLDEN["kats"] if k["device"]], ids=[k["name"] for k in GOLDEN["kats"] if k["device"]])
def test_host_against_the_reference_suite(T, kat):
    """The same steps through the host calls on one session, a message a put call."""
    prios = kat["priorities"]
    w = C.World([(prios, prios.index(kat["default"]), kat["max_len"], kat["mult"], 0)], 1, len(prios), 8, inflight_max=1)
    h = host(T)
    for step in kat["steps"]:
        if step[0] == "in":
            h.put_host([0], [0, 1], [1], [R.W_QUEUED], [0], [[prios.index(step[1])]], w.tables, w.sessions, w.ring, w.heads, refs=[step[2]])
        elif step[0] == "len":
            assert int(w.sessions["mq_len"][0]) == step[1] == int(w.heads["len"][0].sum())
        elif step[0] == "out":
            t = h.take_host([0], w.tables, w.sessions, w.ring, w.heads, update_table=True)
            assert t.refs.size == 1
            w.sessions["inflight"][0] = 0
        else:
            assert step[0] == "drain"
            w.sessions["inflight_max"][0] = 0
            t = h.take_host([0], w.tables, w.sessions, w.ring, w.heads, update_table=True)
            assert [[prios[c], r] for c, r in zip(t.classes.tolist(), t.refs.tolist())] == step[1]
            assert int(w.sessions["mq_len"][0]) == 0 and T.order_of(w.heads, 0) == []


# ---- the host evaluator against the restatement ------------------------------------------------------

@pytest.mark.parametrize("update_table", [True, False])
@pytest.mark.parametrize("case", PUT_CASES, ids=[c.name for c in PUT_CASES])
def test_put_host_against_the_restatement(T, case, update_table):
    got, sessions, ring, heads = put(T, case, update_table)
    C.check_put(case.reference(), got, case, sessions, ring, heads, update_table)


def test_put_cases_reach_what_they_name():
    by = {c.name: c.reference() for c in PUT_CASES}
    assert by["len_above_max"]["summary"][3:7] == [4, 0, 0, 2] and by["len_above_max"]["summary"][0] == R.F_ROW_FULL
    assert by["row_full"]["summary"][3:7] == [1, 0, 0, 4]
    assert by["c8_q8_full_e6"]["summary"][4] == 8 * 4 and by["c8_q8_full_e6"]["summary"][5] == 8 * 2
    assert by["c2_q64_short_e3"]["summary"][4:6] == [4, 0]
    assert by["default_class"]["classes"] == [2, 2, 2, 1]
    assert by["bad_src"]["summary"][0] == R.F_BAD_SRC and by["bad_src"]["classes"] == [0, 1, 1]
    assert by["two_tables"]["classes"] == [0, 1, 2, 0]
    assert [c[7] for c in by["unfit_tables"]["counts"]] == [R.UNFIT] * 8 + [R.A_OK, R.UNFIT]
    assert [c[7] for c in by["pass_absent_bad_sub"]["counts"]] == [R.A_PASS, R.A_NO_SESSION, R.A_NO_SESSION, R.A_OK]
    assert by["pass_absent_bad_sub"]["summary"][0] == R.F_BAD_SUB
    assert by["malformed_heads"]["summary"][0] == R.F_BAD_HEAD | R.F_ROW_FULL  # (len 200 is read as a full ring)
    assert by["limited_record"]["summary"][0] == R.F_LIMITED | R.F_BAD_VERDICT and by["limited_record"]["summary"][3] == 1
    assert by["inbox_2349"]["summary"][1] == 2353 and by["inbox_2349"]["summary"][5] > 1000
    ev = R.all_events()
    for name in ("activate_onto_rotated", "infinity_rotated_then_keysort", "infinity_last", "infinity_first", "infinity_head_held"):
        case = next(c for c in PUT_CASES if c.name == name)
        R.put_reference(case, ev)
    assert ev["unsorted_activations"] >= 2 and ev["infinity_last"] >= 1
    m = by["activate_onto_rotated"]["models"][0][0]
    assert m.priorities() == [C.T_EIGHT[0][k] for k in (1, 3, 4, 5)]  # the rotation is lost
    m = by["infinity_rotated_then_keysort"]["models"][0][0]
    assert m.priorities() == [2, 0, R.INF]  # a non-head infinity sorts last
    assert by["infinity_head_held"]["models"][0][0].priorities() == [R.INF, 2, 0]
    assert by["infinity_last"]["models"][0][0].priorities() == [R.INF, 2, 0]
    assert by["many_inboxes"]["summary"][7] == 300 and by["many_inboxes"]["summary"][4] > 50
    # the cases at the top of the byte fields, below C classes and at a one-group tile
    case = next(c for c in PUT_CASES if c.name == "q128_full_bytes")
    assert case.ring.shape[1:] == (8, 128) and (case.heads["len"] == 128).all() and sorted(case.heads["head"][0].tolist()) == sorted(C.Q128_HEADS)
    assert [c[:6] for c in by["q128_full_bytes"]["counts"]] == [[8 * e - q, 8 * e - q, q, 0, 1024, 8 * e] for e, q in ((1, 0), (2, 0), (130, 16))]
    ev = R.all_events()
    R.put_reference(case, ev)
    assert ev["evictions"] == 8 * 133 and ev["evictions_across_ring_end"] >= 1024 - sum(128 - h for h in C.Q128_HEADS)
    ev = R.all_events()
    R.put_reference(next(c for c in PUT_CASES if c.name == "q128_above_max"), ev)
    assert by["q128_above_max"]["summary"][0] == R.F_ROW_FULL and by["q128_above_max"]["summary"][3:7] == [6, 0, 0, 4]
    assert ev["len_above_max_puts"] == 3 and ev["row_full_inboxes"] == 1 and ev["evictions"] == 0
    assert by["q128_above_max"]["models"][1][0].plen(5) == 106 and by["q128_above_max"]["models"][1][0].plen(2) == 128
    case = next(c for c in PUT_CASES if c.name == "classes_below_c")
    assert case.ring.shape[1] == 7 and int(case.tables["n_classes"][0]) == 3 and int(case.heads["len"][1][5]) == 3
    assert by["classes_below_c"]["summary"][0] == R.F_BAD_HEAD and by["classes_below_c"]["classes"][:6] == [2, 0, 1, 2, 2, 2]
    assert len(by["classes_below_c"]["models"][1][0].q) == 3 and by["classes_below_c"]["counts"][0] == by["classes_below_c"]["counts"][1]
    ref = by["one_group_last_tile"]
    assert len(ref["counts"]) == 65 and 65 % (256 // 4) == 1 and ref["counts"][64][7] == R.A_OK and ref["counts"][64][:3] == [6, 6, 5]


@pytest.mark.parametrize("update_table", [True, False])
@pytest.mark.parametrize("case", TAKE_CASES, ids=[c.name for c in TAKE_CASES])
def test_take_host_against_the_restatement(T, case, update_table):
    got, sessions, ring, heads = take(T, case, update_table)
    C.check_take(case.reference(), got, case, sessions, ring, heads, update_table)


def test_take_cases_reach_what_they_name():
    by = {c.name: c.reference() for c in TAKE_CASES}
    assert by["full_row_budget_0"]["summary"][3] == 0 and by["full_row_budget_1"]["summary"][3] == 1
    assert by["full_row_budget_4"]["counts"][0][0] == 4 and by["full_row_budget_1000"]["counts"] == [[512, 0, 0, 0]]
    assert by["credit_zero_at_entry"]["classes"][:4] == [1, 0, 0, 0]  # the shift comes first; class 0 has credit 5
    assert by["credit_negative"]["classes"] == [2, 2, 0, 0, 3, 3]
    assert by["head_class_empties_mid_credit"]["classes"] == [0, 0, 1, 1, 1]
    assert by["expired_and_qos0"]["counts"] == [[2, 2, 4, 0]] and by["bad_ref"]["summary"][0] == R.F_BAD_REF
    assert by["ids_wrap"]["pkt_ids"] == [65534, 65535, 1, 2, 3]
    assert by["statuses"]["status"] == [R.A_PASS, R.A_NO_SESSION, R.A_OK, R.UNFIT, R.A_NO_SESSION, R.A_OK]
    assert by["statuses"]["summary"][0] == R.F_BAD_SUB | R.F_UNFIT and by["statuses"]["summary"][7] == 1
    assert by["malformed_heads"]["summary"][0] == R.F_BAD_HEAD and by["limited_record"]["summary"][0] == R.F_LIMITED
    ev = R.all_events()
    for name in ("credit_negative", "negative_priority_reached", "credit_zero_at_entry", "full_row_budget_1000"):
        R.take_reference(next(c for c in TAKE_CASES if c.name == name), events=ev)
    assert ev["negative_credit_steps"] >= 3 and ev["shifts"] >= 2
    # the cases at the top of the byte fields, in the second LDS word, below C classes and at a one-group tile
    case = next(c for c in TAKE_CASES if c.name == "q128_full_bytes")
    assert by["q128_full_bytes"]["counts"] == [[542, 277, 205, 0]] and by["q128_full_bytes"]["summary"][3] == 1024
    two = (case.now > case.deadlines[case.ring["ref"][0]]) | ((case.ring["opts"][0] & 3) == 0)  # [8, 128] by ring position
    assert two.reshape(8, 8, 16).any(axis=2).all(), "every one of the 64 words holds a bit"
    case = next(c for c in TAKE_CASES if c.name == "q32_bits_word1")
    row, live = case.ring[0, 0], [(15 + i) % 32 for i in range(20)]
    marked = [p for p in live if case.now > int(case.deadlines[int(row["ref"][p])]) or int(row["opts"][p]) & 3 == 0]
    assert marked and all(p >= 16 or p <= 2 for p in marked) and {p >> 4 for p in live} == {0, 1} and live[-1] == 2
    ev = R.all_events()
    R.take_reference(case, events=ev)
    ref = by["q32_bits_word1"]
    assert ref["counts"] == [[6, 1, 2, 15]] and ref["refs"] == [0, 1, 2, 3, 4, 5, 40, 6, 7] and 15 + ref["refs"][-1] == 22
    assert ev["expired_at_16_up"] == 2 and ev["qos0_at_16_up"] == 1
    ref = by["classes_below_c"]
    assert ref["summary"][0] == R.F_BAD_HEAD and ref["counts"] == [[7, 0, 0, 0]] * 2 and set(ref["classes"]) == {0, 1, 2}
    ref = by["one_group_last_tile"]
    assert len(ref["status"]) == 65 and ref["status"][64] == R.A_OK and ref["counts"][64] == [5, 1, 0, 0]
    first, again = (next(c for c in TAKE_CASES if c.name == n) for n in ("credit_ends_with_budget", "credit_ends_with_budget_again"))
    ev = R.all_events()
    R.take_reference(first, events=ev)
    assert ev["credit_zero_on_last_send"] == 1 and ev["shifts"] == 0 and by["credit_ends_with_budget"]["counts"] == [[9, 0, 0, 5]]
    mq, t, extra = by["credit_ends_with_budget"]["models"][0]
    assert R.credits(0, mq) == 8 and mq.p_credit == 0 and extra["next_pkt_id"] == int(again.sessions["next_pkt_id"][0])
    assert R.logical(mq, t) == R.logical(R.model_of(again.heads[0], t, again.ring[0], 16)[0], t)  # the second case starts there
    R.take_reference(again, events=ev)
    assert ev["shifts"] == 1 and by["credit_ends_with_budget_again"]["classes"] == [0, 0, 1, 1, 1]


def test_take_output_full_then_repeated(T):
    case = C.overflow_case()
    got, sessions, ring, heads = take(T, case)
    C.check_take(case.reference(), got, case, sessions, ring, heads)
    assert got.summary["flags"] == R.F_OUTPUT_FULL and got.summary["items"] == 5 and got.opts.size == 0
    assert got.offsets.tolist() == [0, 3, 5] and got.counts.tolist() == [[2, 1, 0, 0], [2, 0, 0, 0]]
    again, sessions, ring, heads = take(T, case, cap_out=got.summary["items"])
    C.check_take(case.reference(5), again, case, sessions, ring, heads)
    assert again.summary["flags"] == 0 and sorted(again.refs.tolist()) == [1, 2, 3, 4, 5]


# ---- the seeded fuzz: the restatement reaches what it must, and the host calls follow it ---------------

def fuzz_world(seed=20260101, n=300):
    rnd = random.Random(seed)
    configs = []
    for _ in range(n):
        k = rnd.randrange(2, 5)
        prios = sorted(rnd.sample([R.INF, 5, 2, 0, -1], k), key=lambda p: 10 ** 7 if p == R.INF else p, reverse=True)
        configs.append((prios, rnd.randrange(k), rnd.randrange(2, 4), 1, 0))
    w = C.World(configs, n, 4, 8, table=np.arange(n), inflight_max=np.array([rnd.randrange(1, 5) for _ in range(n)]))
    return rnd, w


def test_fuzz_host_follows_the_restatement(T):
    rnd, w = fuzz_world()
    n = w.sessions.size
    h = host(T)
    events = R.all_events()
    models = {}
    put_in, came_out, lost = {s: [] for s in range(n)}, {s: [] for s in range(n)}, {s: set() for s in range(n)}
    ref_no = 0
    for _round in range(6):
        for _ in range(rnd.randrange(1, 7)):
            subs = rnd.sample(range(n), rnd.randrange(n // 2, n))
            sizes = [rnd.randrange(0, 4) for _ in subs]
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
            total = int(off[-1])
            case = C.PutCase("fuzz", w, subs, off, [rnd.randrange(5) for _ in range(total)], opts=[rnd.randrange(3) for _ in range(total)],
                             refs=np.arange(ref_no, ref_no + total))
            ref_no += total
            before = (w.sessions.copy(), w.ring.copy(), w.heads.copy())
            ref = R.put_reference(case, events, models)
            got = h.put_host(case.subs, case.offsets, case.opts, case.verdicts, case.src, case.msg_class, w.tables, w.sessions, w.ring,
                             w.heads, refs=case.refs)
            assert list(got.summary.values()) == ref["summary"] and got.verdicts.tolist() == ref["verdicts"]
            assert got.classes.tolist() == ref["classes"] and got.counts.tolist() == ref["counts"]
            assert [[int(e["ref"]), int(e["opts"])] for e in got.evicted] == ref["evicted"]
            R.check_tables(ref["models"], w.sessions, w.ring, w.heads, True, before, lambda after: {"dropped": after})
            for sub, (mq, _, _) in ref["models"].items():
                models[sub] = mq
            for k, sub in enumerate(subs):
                for d in range(int(off[k]), int(off[k + 1])):
                    put_in[sub].append((int(case.refs[d]), ref["classes"][d]))
                    if ref["verdicts"][d] & R.W_MASK == R.W_QUEUED_DROPPED:
                        lost[sub].add(int(case.refs[d]))
                    if ref["evicted"][d][0] != R.NO_REF:
                        lost[sub].add(ref["evicted"][d][0])
        for _ in range(rnd.randrange(1, 5)):
            subs = rnd.sample(range(n), rnd.randrange(n // 2, n))
            w.sessions["inflight"][:] = 0  # the acks reopened every window
            case = C.TakeCase("fuzz", w, subs)
            before = (w.sessions.copy(), w.ring.copy(), w.heads.copy())
            ref = R.take_reference(case, None, events, models)
            got = h.take_host(case.subs, w.tables, w.sessions, w.ring, w.heads, update_table=True)
            assert list(got.summary.values()) == ref["summary"] and got.refs.tolist() == ref["refs"]
            assert got.classes.tolist() == ref["classes"] and got.pkt_ids.tolist() == ref["pkt_ids"]
            assert got.verdicts.tolist() == ref["verdicts"] and got.counts.tolist() == ref["counts"]
            R.check_tables(ref["models"], w.sessions, w.ring, w.heads, True, before, lambda extra: extra)
            for sub, (mq, _, _) in ref["models"].items():
                models[sub] = mq
            for k, sub in enumerate(subs):
                came_out[sub] += list(zip(ref["refs"][ref["offsets"][k]:ref["offsets"][k + 1]],
                                          ref["classes"][ref["offsets"][k]:ref["offsets"][k + 1]]))
    # what the workload reached, by the restatement's own count
    assert events["shifts"] >= 100 and events["unsorted_activations"] >= 50 and events["infinity_last"] >= 5, events
    assert events["evictions"] >= 300 and events["negative_credit_steps"] >= 50, events
    # conservation: everything put and not evicted comes out once, FIFO within a class
    w.sessions["inflight_max"][:] = 0
    got = h.take_host(None, w.tables, w.sessions, w.ring, w.heads, update_table=True)
    for sub in range(n):
        came_out[sub] += list(zip(got.refs[int(got.offsets[sub]):int(got.offsets[sub + 1])].tolist(),
                                  got.classes[int(got.offsets[sub]):int(got.offsets[sub + 1])].tolist()))
        assert sorted(r for r, _ in came_out[sub]) == sorted(r for r, _ in put_in[sub] if r not in lost[sub]), sub
        for c in range(4):
            assert [r for r, k in came_out[sub] if k == c] == [r for r, k in put_in[sub] if k == c and r not in lost[sub]], (sub, c)
    assert int(w.sessions["mq_len"].sum()) == 0


# ---- the lattice: C x Qc x group width ---------------------------------------------------------------

LATTICE_REACHED = {}  # (c, qc) -> (the restatement's counters, the flags of put, the flags of take)
# half of what the restatement counts over the eight shapes with the committed seed (the docstring below)
LATTICE_FLOORS = dict(shifts=374, unsorted_activations=95, infinity_last=40, evictions=17860, evictions_across_ring_end=1781,
                      negative_credit_steps=4871, len_above_max_puts=194, row_full_inboxes=109, expired_at_16_up=1492,
                      qos0_at_16_up=971, credit_zero_on_last_send=17)
PUT_FLAGS = R.F_BAD_SUB | R.F_BAD_HEAD | R.F_ROW_FULL | R.F_UNFIT | R.F_BAD_VERDICT | R.F_BAD_SRC | R.F_LIMITED
TAKE_FLAGS = R.F_BAD_SUB | R.F_OUTPUT_FULL | R.F_BAD_REF | R.F_BAD_HEAD | R.F_UNFIT | R.F_LIMITED


def run_lattice(T, c, qc, update_table=True, groups=(4, 16, 64)):
    """The rounds of one shape through the host calls, every one checked against the restatement; the put
    rounds are sized around the group widths in turn.  With ``update_table`` false every call runs twice:
    once leaving heads and records alone, checked, and once more to carry the state on."""
    lat = C.Lattice(c, qc)
    for i, (kind, case) in enumerate(lat.rounds(groups)):
        if kind == "put":
            for update in (update_table, True)[update_table:]:
                got, sessions, ring, heads = put(T, case, update)
                C.check_put(case.reference(), got, case, sessions, ring, heads, update)
            lat.advance(kind, case, sessions, ring, heads)
            continue
        for cap in ("case", case.room)[case.cap_out == case.room:]:  # the short round is repeated with room
            for update in (update_table, True)[update_table:]:
                got, sessions, ring, heads = take(T, case, update, cap)
                C.check_take(case.reference(cap), got, case, sessions, ring, heads, update)
            lat.advance(kind, case, sessions, ring, heads, cap)
    # conservation: everything put and not evicted comes out once, FIFO within a class
    w, h = lat.world, host(T)
    w.sessions["inflight_max"] = 0
    for _ in range(2):  # (a take hands out 1000 sends at the most, 8 rings of 128 hold 1024 entries)
        lat.drained(h.take_host(None, w.tables, w.sessions, w.ring, w.heads, update_table=True))
    lat.check_conservation()
    return lat


@pytest.mark.parametrize("update_table", [True, False])
@pytest.mark.parametrize("c,qc", C.LATTICE_SHAPES, ids=["c%d_q%d" % s for s in C.LATTICE_SHAPES])
def test_lattice_host_follows_the_restatement(T, c, qc, update_table):
    lat = run_lattice(T, c, qc, update_table)
    LATTICE_REACHED[(c, qc)] = (lat.events, lat.flags["put"], lat.flags["take"])


def test_lattice_reaches_what_it_must(T):
    """The restatement's own counters summed over the eight shapes (three put and three take rounds each,
    129 sessions, seed C.LATTICE_SEED), as measured from the restatement on the CPU:

        shifts 749, unsorted_activations 190, infinity_last 80, evictions 35720, evictions_across_ring_end 3562
        (an old entry read behind the ring end after ones in front of it), negative_credit_steps 9743,
        len_above_max_puts 389 (a class of an inbox that meets L > M), row_full_inboxes 219, expired_at_16_up 2984
        and qos0_at_16_up 1943 (an item handed out from a ring position >= 16: an LDS word other than word 0),
        credit_zero_on_last_send 34 (the budget's last send leaves credit 0).

    Every floor is half of its count.  Every flag of either call but INPUT_REFUSED is raised somewhere."""
    total, flags_put, flags_take = R.all_events(), 0, 0
    for c, qc in C.LATTICE_SHAPES:
        if (c, qc) not in LATTICE_REACHED:
            lat = run_lattice(T, c, qc)
            LATTICE_REACHED[(c, qc)] = (lat.events, lat.flags["put"], lat.flags["take"])
        events, fp, ft = LATTICE_REACHED[(c, qc)]
        for k, v in events.items():
            total[k] += v
        flags_put, flags_take = flags_put | fp, flags_take | ft
    print("lattice events:", total)
    assert set(LATTICE_FLOORS) == set(total)
    for k, floor in LATTICE_FLOORS.items():
        assert floor > 0 and total[k] >= floor, (k, total[k], floor)
    assert flags_put == PUT_FLAGS and flags_take == TAKE_FLAGS, (hex(flags_put), hex(flags_take))


# ---- the differential: one class of priority 0 is the plain mqueue -----------------------------------

def test_one_class_is_the_plain_mqueue(T):
    """With C = 1 and one class of priority 0, window (mq_max 0) + this stage leave the same items, queues,
    lengths, packet ids and session records as window (the real mq_max) + the mqueue stage."""
    from emqx_amd import mqueue, window
    rnd = random.Random(5)
    n, q = 40, 8
    maxes = np.array([rnd.randrange(2, 9) for _ in range(n)])
    plain = window.pack_sessions(n, inflight_max=np.array([rnd.randrange(0, 4) for _ in range(n)]), mq_max=maxes)
    prio = plain.copy()
    prio["mq_max"] = 0
    tables = T.pack_tables([([0], 0, int(m), 10, 0) for m in maxes])
    pring, pheads = T.empty_ring(n, 1, q), T.empty_heads(n, np.arange(n))
    mring, mheads = mqueue.empty_ring(n, q), mqueue.empty_heads(n)
    w, hm, hp = window.Window(window.HOST_ONLY), mqueue.Mqueue(mqueue.HOST_ONLY), host(T)
    ref_no = 0
    for _round in range(12):
        subs = rnd.sample(range(n), 25)
        off = np.concatenate([[0], np.cumsum([rnd.randrange(0, 12) for _ in subs])])
        total = int(off[-1])
        opts = [rnd.randrange(3) for _ in range(total)]
        refs = np.arange(ref_no, ref_no + total)
        ref_no += total
        a = w.run_host(subs, off, opts, plain, update_table=True)
        b = w.run_host(subs, off, opts, prio, update_table=True)
        pm = hm.put_host(subs, off, opts, a.verdicts, mring, mheads, refs=refs, sessions=plain)
        pp = hp.put_host(subs, off, opts, b.verdicts, np.arange(total), np.zeros((max(total, 1), n), np.uint8), tables, prio, pring,
                         pheads, refs=refs)
        queued = (b.verdicts & 0x0F) == 3
        assert np.array_equal(np.where(queued, pp.verdicts, a.verdicts), a.verdicts)  # the window's own verdicts, per class
        assert pm.evicted.tobytes() == pp.evicted.tobytes() and pm.summary["stored"] == pp.summary["stored"]
        plain["inflight"] = prio["inflight"] = np.minimum(plain["inflight"], rnd.randrange(0, 3))
        tk = rnd.sample(range(n), 20)
        tm = hm.take_host(tk, plain, mring, mheads, update_table=True)
        tp = hp.take_host(tk, tables, prio, pring, pheads, update_table=True)
        for x, y in zip(tm[:7], (tp.offsets, tp.opts, tp.verdicts, tp.pkt_ids, tp.refs, tp.status, tp.counts)):
            assert x.tobytes() == y.tobytes()
        for name in ("inflight", "mq_len", "next_pkt_id", "dropped", "flags", "inflight_max"):
            assert plain[name].tolist() == prio[name].tolist(), name
        for s in range(n):
            assert mqueue.queue_of(mring, mheads, s).tobytes() == T.queue_of(pring, pheads, s, 0).tobytes(), s
    assert int(plain["dropped"].sum()) > 50 and int(plain["mq_len"].sum()) > 20


# ---- the closed-form order rule against the literal fold ----------------------------------------------

@pytest.mark.parametrize("prios", [[R.INF, 5, 2, 0], [7, 5, 2, -1]], ids=["with_infinity", "numbers_only"])
def test_order_rule_against_the_literal_fold(T, prios):
    """Every list of non-empty classes in every order (sorted, rotated or neither), then one or two
    absent classes activated in one inbox, in both arrival orders: the order word the host call leaves
    against emqx_pqueue:in/3 played on the list."""
    import itertools
    h = host(T)
    n = len(prios)
    checked = 0
    for k in range(n):
        for present in itertools.permutations(range(n), k):
            absent = [c for c in range(n) if c not in present]
            for r in (1, 2):
                for arriving in itertools.permutations(absent, min(r, len(absent))):
                    if not arriving:
                        continue
                    w = C.World([(prios, 0, 3, 1, 0)], 1, n, 8)
                    w.fill(0, {c: [(10 * c, 1)] for c in present}, order=list(present))
                    mq = R.MQ(3, 1, 0)
                    for c in present:
                        mq.q.append([R.negate(prios[c]), __import__("collections").deque([(10 * c, 1, None)])])
                        mq.len += 1
                    for c in arriving:
                        R.mq_in((99, 1, None), prios[c], mq)
                    h.put_host([0], [0, len(arriving)], [1] * len(arriving), [R.W_QUEUED] * len(arriving), list(range(len(arriving))),
                               [[c] for c in arriving], w.tables, w.sessions, w.ring, w.heads)
                    assert [prios[c] for c in T.order_of(w.heads, 0)] == mq.priorities(), (present, arriving)
                    checked += 1
    assert checked == 148  # 16 + 36 + 48 + 48 over lists of 0 to 3 of the 4 classes


# ---- the differential on the cases of the plain mqueue stage ------------------------------------------

def _plain_cases():
    from tests import mqueue_cases as MC
    puts = [c for c in MC.put_cases() if c.q <= 128 and c.sessions is not None and c.sessions.size and
            (c.sessions["mq_max"] >= 2).all() and (c.sessions["mq_max"] <= c.q).all()]
    takes = [c for c in MC.take_cases() + [MC.overflow_case()] if c.q <= 128 and len(c.session_dicts)]
    return puts, takes


PLAIN_PUTS, PLAIN_TAKES = _plain_cases()


def _as_priority_world(T, case, max_len):
    """The tables of a plain mqueue case as one class of priority 0: a table a session with its limit."""
    n, q = case.ring.shape
    tables = T.pack_tables([([0], 0, int(m), 10, 0) for m in max_len])
    ring = np.ascontiguousarray(case.ring.reshape(n, 1, q).copy())
    heads = T.empty_heads(n, np.arange(n))
    heads["head"][:, 0] = case.heads["head"] % q
    heads["len"][:, 0] = np.minimum(case.heads["len"], q)
    heads["order"] = np.where(case.heads["len"] > 0, 0xFFFFFFF0, 0xFFFFFFFF)
    return tables, ring, heads


@pytest.mark.parametrize("case", PLAIN_PUTS, ids=[c.name for c in PLAIN_PUTS])
def test_one_class_put_on_the_plain_cases(T, case):
    """The put cases of tests/mqueue_cases.py whose limits are 2 to Q (Q <= 128, the records given): the
    plain stage takes the window's verdicts at the real limit, this stage the candidates alone (what
    the window says at mq_max 0) and finds the same verdicts, evicted entries, queues and lengths."""
    from emqx_amd import mqueue
    n, q = case.ring.shape
    mring, mheads = case.ring.copy(), case.heads.copy()
    try:
        pm = mqueue.Mqueue(mqueue.HOST_ONLY).put_host(case.subs, case.offsets, case.opts, case.verdicts, mring, mheads, refs=case.refs)
    except Exception as e:  # a subscriber the table lacks: the outputs are complete
        pm = e.partial
    tables, ring, heads = _as_priority_world(T, case, case.sessions["mq_max"])
    sessions = case.sessions.copy()
    sessions["mq_max"] = 0
    sessions["mq_len"] = heads["len"][:, 0]
    sessions["dropped"] = 0
    candidate = np.isin(case.verdicts & 0x0F, (R.W_QUEUED, R.W_QUEUED_DROPPED))
    ver = np.where(candidate, R.W_QUEUED, case.verdicts & 0x0F).astype(np.uint8)
    total = int(case.offsets[-1])
    try:
        pp = host(T).put_host(case.subs, case.offsets, case.opts, ver, np.arange(total), np.zeros((max(total, 1), n), np.uint8), tables,
                              sessions, ring, heads, refs=case.refs)
    except Exception as e:
        pp = e.partial
    served = np.repeat(case.subs < n, np.diff(case.offsets.astype(np.int64)))  # (an inbox of a subscriber the table lacks gets verdict 0)
    assert pp.verdicts[candidate & served].tolist() == case.verdicts[candidate & served].tolist()
    assert not pp.verdicts[~served].any()
    assert pp.evicted.tobytes() == pm.evicted.tobytes()
    assert pp.counts[case.subs < n, 3].tolist() == pm.unstored[case.subs < n].tolist()
    for s in range(n):
        assert mqueue.queue_of(mring, mheads, s).tobytes() == T.queue_of(ring, heads, s, 0).tobytes(), s
        assert int(sessions["mq_len"][s]) == int(mheads["len"][s]) == int(heads["len"][s][0])
    owned = [int(s) for s in case.subs if s < n]
    evictions = sum(int(bool(v & R.W_EVICTS)) for v in case.verdicts)
    assert int(sessions["dropped"][owned].sum()) == evictions if not (pm.summary["flags"] & mqueue.F_ROW_FULL) else True


@pytest.mark.parametrize("case", PLAIN_TAKES, ids=[c.name for c in PLAIN_TAKES])
def test_one_class_take_on_the_plain_cases(T, case):
    """The take cases of tests/mqueue_cases.py with Q <= 128 (a take knows no limit): the same items,
    packet ids, statuses, counts, heads and records from both stages, the full call included."""
    from emqx_amd import _lib, mqueue
    n, q = case.ring.shape
    tables, ring, heads = _as_priority_world(T, case, [q] * n)
    out = []
    for stage in ("plain", "priority"):
        sessions = case.sessions.copy()
        try:
            if stage == "plain":
                mheads = case.heads.copy()
                t = mqueue.Mqueue(mqueue.HOST_ONLY).take_host(case.subs, sessions, case.ring.copy(), mheads, case.now,
                                                               deadlines=case.deadlines, cap_out=case.cap_out, update_table=True)
            else:
                sessions["mq_max"] = 0
                t = host(T).take_host(case.subs, tables, sessions, ring, heads, case.now, deadlines=case.deadlines, cap_out=case.cap_out,
                                      update_table=True)
            code = 0
        except _lib.EngineError as e:
            t, code = e.partial, e.code
        out.append((code, [x.tobytes() for x in (t.offsets, t.opts, t.verdicts, t.pkt_ids, t.refs, t.status, t.counts)],
                    [sessions[f].tolist() for f in ("inflight", "mq_len", "next_pkt_id", "dropped")]))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    keep = [s for s in range(n) if int(case.sessions["mq_len"][s]) == min(int(case.heads["len"][s]), q)]  # (a stale mq_len stays the plain stage's finding)
    for a, b in zip(out[0][2], out[1][2]):
        assert [a[s] for s in keep] == [b[s] for s in keep]
    for s in range(n):
        assert (int(mheads["head"][s]) % q if int(heads["len"][s][0]) else 0, min(int(mheads["len"][s]), q)) == (
            int(heads["head"][s][0]) if int(heads["len"][s][0]) else 0, int(heads["len"][s][0])), s


# ---- the ABI -----------------------------------------------------------------------------------------

def test_exports_every_pmqueue_symbol(T):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_pmqueue.h")
    assert len(declared) == 13
    assert sorted(_lib.PMQUEUE_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def test_package_exports_the_module(T):
    import emqx_amd
    assert emqx_amd.Pmqueue is T.Pmqueue


def test_struct_sizes_and_constants(T):
    from emqx_amd import _lib
    assert T.TABLE.itemsize == 56 and T.HEAD.itemsize == 64 and T.HEAD.fields["order"][1] == 32 and T.TABLE.fields["prio"][1] == 24
    assert ctypes.sizeof(_lib.PmqueuePutArgs) == 25 * 8 and ctypes.sizeof(_lib.PmqueueTakeArgs) == 25 * 8
    assert ctypes.sizeof(_lib.PmqueueStats) == 56
    header = open(os.path.join(ROOT, "include", "emqx_pmqueue.h")).read()
    for name, value in (("EMQX_PMQ_UNFIT", T.UNFIT), ("EMQX_PMQ_NO_CLASS", T.NO_CLASS), ("EMQX_PMQ_MIN_QC", T.MIN_QC),
                        ("EMQX_PMQ_MAX_QC", T.MAX_QC), ("EMQX_PMQ_MAX_CLASSES", T.MAX_CLASSES), ("EMQX_PMQ_MAX_MULT", T.MAX_MULT),
                        ("EMQX_PMQ_H_LAST_DEFINED", T.H_LAST_DEFINED),
                        ("EMQX_PMQ_F_INPUT_REFUSED", T.F_INPUT_REFUSED), ("EMQX_PMQ_F_BAD_SUB", T.F_BAD_SUB),
                        ("EMQX_PMQ_F_OUTPUT_FULL", T.F_OUTPUT_FULL), ("EMQX_PMQ_F_BAD_REF", T.F_BAD_REF),
                        ("EMQX_PMQ_F_BAD_HEAD", T.F_BAD_HEAD), ("EMQX_PMQ_F_ROW_FULL", T.F_ROW_FULL), ("EMQX_PMQ_F_UNFIT", T.F_UNFIT),
                        ("EMQX_PMQ_F_BAD_VERDICT", T.F_BAD_VERDICT), ("EMQX_PMQ_F_BAD_SRC", T.F_BAD_SRC),
                        ("EMQX_PMQ_F_LIMITED", T.F_LIMITED)):
        m = re.search(r"#define %s (\S+?)u\b" % name, header)
        assert m and int(m.group(1), 0) == value, name
    for name, value in (("EMQX_PMQ_PRIO_INFINITY", T.PRIO_INFINITY), ("EMQX_PMQ_MAX_PRIO", T.MAX_PRIO)):
        m = re.search(r"#define %s (\S+)" % name, header)
        assert m and int(m.group(1), 0) == value, name
    assert (R.F_BAD_HEAD, R.F_UNFIT, R.F_LIMITED, R.UNFIT, R.NO_CLASS) == (T.F_BAD_HEAD, T.F_UNFIT, T.F_LIMITED, T.UNFIT, T.NO_CLASS)
    s = host(T).stats()
    assert set(s) == {"cap_in", "cap_boxes", "scratch_bytes", "group", "calls", "last_call_ms"} and s["calls"] == 0 and s["group"] == 4
    short = _lib.PmqueueStats()
    short.size = 16
    h = host(T)
    assert _lib.lib().emqx_pmqueue_stats_get(h._h, ctypes.byref(short)) == 0 and short.size == 16
    short.size = 4
    assert _lib.lib().emqx_pmqueue_stats_get(h._h, ctypes.byref(short)) == EINVAL


def _args(T, **kw):
    """A valid put and a valid take block on one small world, with what keeps their buffers alive."""
    from emqx_amd import _lib
    w = C.World([C.T_TWO], 2, 2, 8)
    keep = dict(w=w, subs=np.zeros(1, np.uint32), off=np.array([0, 1], np.uint64), opts=np.ones(1, np.uint8), ver=np.full(1, 3, np.uint8),
                src=np.zeros(1, np.uint32), mc=np.zeros(1, np.uint8), ov=np.zeros(1, np.uint8), oc=np.zeros(1, np.uint8),
                ev=np.zeros(1, T.ENTRY), cnt=np.zeros(8, np.uint32), toff=np.zeros(2, np.uint64), o=np.zeros(8, np.uint8),
                v=np.zeros(8, np.uint8), p=np.zeros(8, np.uint16), r=np.zeros(8, np.uint32), cl=np.zeros(8, np.uint8),
                st=np.zeros(1, np.uint8), tcnt=np.zeros(4, np.uint32))
    d = {k: (x.ctypes.data if isinstance(x, np.ndarray) else None) for k, x in keep.items()}
    pb = _lib.PmqueuePutArgs(inbox_subs=d["subs"], inbox_offsets=d["off"], box_opts=d["opts"], n_boxes=None, m=1, cap_in=1, cap_boxes=1,
                             verdicts=d["ver"], refs=None, box_src=d["src"], msg_class=d["mc"], n_msgs=1, tables=w.tables.ctypes.data,
                             n_tables=1, sessions=w.sessions.ctypes.data, sub_limit=2, update_table=1, ring=w.ring.ctypes.data,
                             heads=w.heads.ctypes.data, c=2, qc=8, out_verdicts=d["ov"], out_class=d["oc"], out_evicted=d["ev"],
                             out_counts=d["cnt"])
    tb = _lib.PmqueueTakeArgs(subs=d["subs"], n_boxes=None, m=1, cap_boxes=1, sessions=w.sessions.ctypes.data, sub_limit=2, update_table=0,
                              tables=w.tables.ctypes.data, n_tables=1, ring=w.ring.ctypes.data, heads=w.heads.ctypes.data, c=2, qc=8,
                              now_ms=5, deadlines=None, ref_limit=0, cap_out=8, out_offsets=d["toff"], out_opts=d["o"],
                              out_verdicts=d["v"], out_pkt_ids=d["p"], out_refs=d["r"], out_class=d["cl"], out_status=d["st"],
                              out_counts=d["tcnt"])
    for b in (pb, tb):
        for k, v in kw.items():
            if any(k == f for f, _ in b._fields_):
                setattr(b, k, v)
    return pb, tb, keep


def test_argument_errors(T):
    from emqx_amd import _lib
    L, h = _lib.lib(), host(T)
    pb, tb, keep = _args(T)
    assert L.emqx_pmqueue_put_host(h._h, ctypes.byref(pb), None) == 0 and L.emqx_pmqueue_take_host(h._h, ctypes.byref(tb), None) == 0
    for bad in (dict(qc=0), dict(qc=4), dict(qc=12), dict(qc=256), dict(c=0), dict(c=9)):
        pb, tb, keep = _args(T, **bad)
        assert L.emqx_pmqueue_put_host(h._h, ctypes.byref(pb), None) == EINVAL, bad
        assert L.emqx_pmqueue_take_host(h._h, ctypes.byref(tb), None) == EINVAL, bad
    for field in ("inbox_offsets", "inbox_subs", "verdicts", "box_opts", "box_src", "msg_class", "tables", "sessions", "ring", "heads",
                  "out_verdicts", "out_class", "out_evicted"):
        pb, tb, keep = _args(T, **{field: None})
        assert L.emqx_pmqueue_put_host(h._h, ctypes.byref(pb), None) == EINVAL, field
    for field in ("sessions", "tables", "ring", "heads", "out_offsets", "out_opts", "out_verdicts", "out_pkt_ids", "out_refs", "out_class",
                  "out_status"):
        pb, tb, keep = _args(T, **{field: None})
        assert L.emqx_pmqueue_take_host(h._h, ctypes.byref(tb), None) == EINVAL, field
    pb, tb, keep = _args(T, now_ms=1 << 45)
    assert L.emqx_pmqueue_take_host(h._h, ctypes.byref(tb), None) == EINVAL
    pb, tb, keep = _args(T, m=2)
    assert L.emqx_pmqueue_put_host(h._h, ctypes.byref(pb), None) == EINVAL  # m > cap_boxes
    assert L.emqx_pmqueue_put_host(None, ctypes.byref(pb), None) == EINVAL and L.emqx_pmqueue_put_host(h._h, None, None) == EINVAL
    summary = np.zeros(8, np.uint64)
    n = np.array([3], np.uint64)
    pb, tb, keep = _args(T, n_boxes=n.ctypes.data)
    assert L.emqx_pmqueue_put_host(h._h, ctypes.byref(pb), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [T.F_INPUT_REFUSED, 0, 3, 0, 0, 0, 0, 0]
    assert L.emqx_pmqueue_take_host(h._h, ctypes.byref(tb), summary.ctypes.data) == EINVAL
    assert summary.tolist() == [T.F_INPUT_REFUSED, 0, 3, 0, 0, 0, 0, 0]


def test_tuning_keys(T):
    h = host(T)
    from emqx_amd import _lib
    for key, hi in (("max_blocks", 4096), ("scan_chunk", 1024)):
        h.set_tuning(key, 1)
        h.set_tuning(key, hi)
        for bad in (0, hi + 1, -1):
            with pytest.raises(_lib.EngineError) as e:
                h.set_tuning(key, bad)
            assert e.value.code == EINVAL
    for g in T.GROUPS:
        h.set_tuning("group", g)
        assert h.stats()["group"] == g
    for bad in (0, 1, 2, 12, 128, -8):
        with pytest.raises(_lib.EngineError) as e:
            h.set_tuning("group", bad)
        assert e.value.code == EINVAL
    with pytest.raises(_lib.EngineError) as e:
        h.set_tuning("rematch", 1)
    assert e.value.code == ENOTFOUND


def test_host_only_handle_has_no_device_calls(T):
    from emqx_amd import _lib
    L, h = _lib.lib(), host(T)
    pb, tb, keep = _args(T)
    s = np.zeros(8, np.uint64)
    assert L.emqx_pmqueue_reserve(h._h, 10, 10) == EDEVICE
    assert L.emqx_pmqueue_put_batch(h._h, ctypes.byref(pb), None) == EDEVICE
    assert L.emqx_pmqueue_take_batch(h._h, ctypes.byref(tb), None) == EDEVICE
    for fn, b in ((L.emqx_pmqueue_put_batch_device, pb), (L.emqx_pmqueue_put_batch_device_async, pb),
                  (L.emqx_pmqueue_take_batch_device, tb), (L.emqx_pmqueue_take_batch_device_async, tb)):
        assert fn(h._h, ctypes.byref(b), s.ctypes.data, None) == EDEVICE
