"""Rates of the rel stage (emqx_amd/rel.py) for DESIGN.md §3.17.

Populations of 1 K to 10 M connected sessions at W = 128 with a limit of 100 (the defaults) and at
W = 32 with a limit of 32.  Every session awaits ids 1 .. 4 at entry (slots 0 .. 3) and gets 1 to 4
events: a quarter are PUBRELs of ids awaiting at entry, the rest QoS 2 PUBLISHes of fresh ids (four
in five) and QoS 0/1 ones.  Timed, each call between two events on one stream:

  run       emqx_rel_run_batch_device_async with ts[] and src[] given;
  ack_run   emqx_ack_run_batch_device_async on the same population with as many PUBACKs a session
            as the run call has events (rows of min(W, 64) slots, four messages inflight): the
            yardstick, the closest stage in bytes (a row plus a record per session);
  expire    emqx_rel_expire_batch_device_async over the whole table (subs NULL) with nothing due,
            the entries of one session in a hundred due, and everything due;
  lanes     the run call at every legal value of the tuning key "lanes" (at 1 M sessions);
  skew      the run call where session 0 holds 10 % of all events (publish, rel, publish, ...), the
            rest spread as before; the same total (at 1 M sessions);
  host      emqx_rel_run_host on 16 threads, each over its own share of the sessions (at 1 M).

The tables of a population exist in `copies` instances (at least 4) that the calls rotate over, so
no row stays in the Infinity Cache between two calls on it; every timed call starts from the same
rows, restored from a pristine copy outside the events.  A window is ~0.25 s of calls after a
warm-up pass over every instance; the median of three windows is reported.  Up to 100 K sessions the
first call on instance 0 is checked byte for byte against emqx_rel_run_host and
emqx_rel_expire_host.  The byte models are the stage's own (see run_bytes_model and friends); no
target is set in advance and every line goes to the output file as measured.

  python tools/rel_bench.py [--out profiles/rel_sweep.jsonl] [--populations 1000,...]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from emqx_amd import ack as AK  # noqa: E402
from emqx_amd import rel as RL  # noqa: E402
from emqx_amd import window as WN  # noqa: E402

POPULATIONS = (1_000, 10_000, 100_000, 1_000_000, 10_000_000)
SHAPES = ((128, 100), (32, 32))  # (W, limit)
AWAITING = 4
NOW = 1_700_000_000_000
OLD = 1_000_000  # the age of the entries of one session in a hundred


def run_bytes_model(w: int, sessions: int, events: int, routed: int, changed_rows: int, ts: bool, src: bool) -> float:
    """Bytes a run call moves: per named row 8 W read and, where it changed, a 16-byte pair per
    changed entry written (counted as 8 W for a changed row, an upper bound); per session the id,
    two offsets, the 32-byte record, 16 bytes of counts and the arm byte; per event the event read
    by the fold and twice by the route passes, the verdict written and read twice (4 * 3 + 1 * 3),
    8 more where ts[] is given (the fold loads the stamps with the events) and per routed event src
    read and out_route written (4 + 4)."""
    return 8.0 * w * (sessions + changed_rows) + (4 + 16 + 32 + 16 + 1) * sessions + (15.0 + (8 if ts else 0)) * events + (
        (4 if src else 0) + 4.0) * routed


def ack_bytes_model(w: int, sessions: int, acks: int, changed_rows: int) -> float:
    """The same accounting for the ack run call: per row 8 W read by the rows pass and written
    where it changed, first[] and comp[] of 4 W each written by the init pass and read by the rows
    pass; per session the id, two offsets, the record, the counts; per ack the ack read by three
    passes, the slot byte written and read twice, the verdict and the ref written (12 + 3 + 1 + 4),
    and the 16 bytes of row each of the first and verdict passes reads to find and judge its slot
    (a lower bound: a match scans until it hits)."""
    return (8.0 * w + 16.0 * w) * sessions + 8.0 * w * changed_rows + (4 + 16 + 32 + 16) * sessions + (20.0 + 32.0) * acks


def expire_bytes_model(w: int, sessions: int, changed_pairs: int) -> float:
    """Per session the row read, the record's 32-byte sector, status and counts written; per changed
    16-byte pair its store."""
    return (8.0 * w + 32 + 1 + 16) * sessions + 16.0 * changed_pairs


def events_of(P: int, rng, skew: bool):
    """offsets, events, ts, src of the population's batch."""
    counts = rng.integers(1, 5, P).astype(np.int64)
    total = int(counts.sum())
    if skew:
        big = total // 10
        rest = np.diff(np.linspace(0, total - big, P).astype(np.int64))
        counts = np.concatenate([[big], rest])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    j = np.arange(total, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), counts)
    u = rng.random(total)
    kind = np.where(u < 0.25, RL.PUBREL, np.where(u < 0.85, RL.PUBLISH, RL.DIRECT)).astype(np.uint32)
    ids = np.where(kind == RL.PUBREL, j % AWAITING + 1, 100 + j % 60000).astype(np.uint32)
    if skew:  # session 0 hovers: publish of a fresh id, rel of it, publish of the next, ...
        big = int(counts[0])
        kind[:big] = np.where(np.arange(big) % 2 == 0, RL.PUBLISH, RL.PUBREL)
        ids[:big] = 100 + (np.arange(big) // 2) % 60000
    ts = (NOW + rng.integers(0, 1000, total)).astype(np.uint64)
    return off, RL.pack_events(kind, ids), ts, np.arange(total, dtype=np.uint32)[::-1].copy(), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rel_sweep.jsonl"))
    ap.add_argument("--populations", default=",".join(map(str, POPULATIONS)))
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--extras-at", type=int, default=1_000_000, help="the population of the lanes A/B, the skewed run and the host run")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "rel_bench needs a HIP device"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def up(a, view=np.int64):
        return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=view).copy()).to(dev)

    z = lambda size, dt: torch.zeros(max(size, 1), dtype=dt, device=dev)  # noqa: E731
    ts_ = torch.cuda.Stream(device=dev)
    stream = ts_.cuda_stream
    copies = max(args.copies, 4)
    emit({"record": "setup", "shapes": SHAPES, "awaiting_at_entry": AWAITING, "events_per_session": "1..4", "instances": copies,
          "device": torch.cuda.get_device_name(0)})

    def timed(call, restore):
        """ms per call: `call(i)` enqueues one call on instance i between two events, `restore(i)`
        puts its rows back before, outside the events."""
        def one(i):
            with torch.cuda.stream(ts_):
                restore(i)
                m = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                m[0].record(ts_)
                call(i)
                m[1].record(ts_)
            return m
        probe = [one(i) for i in range(copies)]  # the warm-up, and how long a call takes
        torch.cuda.synchronize()
        ms = sum(m[0].elapsed_time(m[1]) for m in probe) / len(probe)
        reps = int(min(200, max(1, args.window_ms / max(ms * copies, 1e-3))))
        per_round = []
        for _ in range(args.rounds):
            marks = [one(i) for _ in range(reps) for i in range(copies)]
            torch.cuda.synchronize()
            per_round.append(float(np.mean([m[0].elapsed_time(m[1]) for m in marks])))
        return round(float(np.median(per_round)), 4), reps

    words = lambda t, names: dict(zip(names, t.cpu().numpy().view(np.uint64).tolist()))  # noqa: E731

    for population in [int(p) for p in args.populations.split(",")]:
        for w, limit in SHAPES:
            P = population
            rng = np.random.default_rng(P + w)
            try:
                # ---- the tables ------------------------------------------------------------------
                table = up(WN.pack_sessions(P, inflight=AWAITING, inflight_max=64))
                ages = torch.full((P,), NOW, dtype=torch.int64, device=dev)
                ages[::100] -= OLD
                rows0 = torch.zeros((P, w), dtype=torch.int64, device=dev)
                for s in range(AWAITING):
                    rows0[:, s] = (ages << 17) | (1 << 16) | (s + 1)
                rows0 = rows0.view(-1)
                wa = min(w, 64)
                slots0 = AK.empty_slots(1, wa)
                for s in range(AWAITING):
                    slots0[0, s] = (s + 1, AK.MSG, 1, s)
                slots0 = up(slots0).repeat(P)
                inst = [dict(rows=rows0.clone(), slots=slots0.clone()) for _ in range(copies)]
                r, a = RL.Rel(0), AK.Ack(0)
                variants = [False] + ([True] if P == args.extras_at else [])
                for skew in variants:
                    off, ev, ts, src, total = events_of(P, rng, skew)
                    d_off, d_ev, d_ts, d_src = up(off), up(ev, np.int32), up(ts), up(src, np.int32)
                    kinds = ev >> 16
                    acks = up(AK.pack_acks(np.full(total, AK.PUBACK), (ev & 0xFFFF) % AWAITING + 1), np.int32)
                    subs = up(np.arange(P, dtype=np.uint32), np.int32)
                    r.reserve(total, P, w)
                    a.reserve(total, P, wa)
                    for g in inst:
                        g.update(ver=z(total, torch.uint8), route=z(total, torch.int32), cnt=z(4 * P, torch.int32), arm=z(P, torch.uint8),
                                 rsum=z(8, torch.int64), aver=z(total, torch.uint8), arefs=z(total, torch.int32), acnt=z(4 * P, torch.int32),
                                 asum=z(8, torch.int64), xst=z(P, torch.uint8), xcnt=z(4 * P, torch.int32), xsum=z(8, torch.int64))
                        g["r"] = RL.Rel.run_args(subs.data_ptr(), d_off.data_ptr(), d_ev.data_ptr(), P, total, P, table.data_ptr(), P,
                                                 g["rows"].data_ptr(), w, g["ver"].data_ptr(), g["route"].data_ptr(), g["cnt"].data_ptr(),
                                                 g["arm"].data_ptr(), max_awaiting=limit, now_ms=NOW, d_ts=d_ts.data_ptr(), d_src=d_src.data_ptr())
                        g["a"] = AK.Ack.run_args(subs.data_ptr(), d_off.data_ptr(), acks.data_ptr(), P, total, P, table.data_ptr(), P,
                                                 g["slots"].data_ptr(), wa, g["aver"].data_ptr(), g["arefs"].data_ptr(), g["acnt"].data_ptr())
                    restore_rows = lambda i: inst[i]["rows"].copy_(rows0)  # noqa: E731
                    restore_slots = lambda i: inst[i]["slots"].copy_(slots0)  # noqa: E731
                    run_call = lambda i: r.run_device_async(inst[i]["r"], inst[i]["rsum"].data_ptr(), stream=stream)  # noqa: E731
                    ack_call = lambda i: a.run_device_async(inst[i]["a"], inst[i]["asum"].data_ptr(), stream=stream)  # noqa: E731
                    # ---- one checked call ------------------------------------------------------
                    with torch.cuda.stream(ts_):
                        restore_rows(0)
                        run_call(0)
                    torch.cuda.synchronize()
                    rs = words(inst[0]["rsum"], RL.RUN_SUMMARY)
                    assert rs["flags"] == 0 and rs["events"] == total and rs["sessions"] == P, rs
                    changed_rows = int((inst[0]["rows"].view(P, w) != rows0.view(P, w)).any(dim=1).sum().item())
                    checked = P <= 100_000
                    if checked:
                        h_rows = rows0.cpu().numpy().view(np.uint64).reshape(P, w).copy()
                        h_tab = np.frombuffer(table.cpu().numpy().tobytes(), dtype=WN.SESSION).copy()
                        ref = RL.Rel(RL.HOST_ONLY).run_host(np.arange(P), off, ev, h_tab, h_rows, max_awaiting=limit, now_ms=NOW, ts=ts, src=src)
                        assert ref.summary == rs, (ref.summary, rs)
                        g = inst[0]
                        for got, exp in ((g["ver"][:total], ref.verdicts), (g["route"][:rs["routed"]], ref.route), (g["cnt"][:4 * P], ref.counts),
                                         (g["arm"][:P], ref.arm), (g["rows"], h_rows)):
                            assert got.cpu().numpy().tobytes() == exp.tobytes(), (P, w, skew)
                    run_ms, reps = timed(run_call, restore_rows)
                    ack_ms, _ = timed(ack_call, restore_slots)
                    acs = words(inst[0]["asum"], AK.RUN_SUMMARY)
                    moved = run_bytes_model(w, P, total, rs["routed"], changed_rows, True, True)
                    amoved = ack_bytes_model(wa, P, total, P)
                    emit({"record": "skew" if skew else "run", "population": P, "w": w, "limit": limit, "events": total,
                          "largest_session": int(np.diff(off.astype(np.int64)).max()), "lanes": RL.default_lanes(w), "instances": copies,
                          "calls_per_window": reps * copies, "checked_against_host": checked,
                          "summary": {k: rs[k] for k in RL.RUN_SUMMARY[3:]}, "kinds": {k: int((kinds == v).sum()) for k, v in
                                                                                       (("publish", 1), ("pubrel", 2), ("direct", 3))},
                          "changed_rows": changed_rows, "run_ms": run_ms, "m_events_per_s": round(total / (run_ms * 1e-3) / 1e6, 1),
                          "m_sessions_per_s": round(P / (run_ms * 1e-3) / 1e6, 1),
                          "model": {"bytes_per_call": int(moved), "gb_per_s": round(moved / (run_ms * 1e-3) / 1e9, 1)},
                          "ack_run": {"w": wa, "ms": ack_ms, "oks": acs["oks"], "bytes_per_call": int(amoved),
                                      "gb_per_s": round(amoved / (ack_ms * 1e-3) / 1e9, 1)},
                          "ratio_to_ack_run": round(run_ms / ack_ms, 3), "ratio_of_byte_models": round(moved / amoved, 3)})
                    # ---- the lanes A/B, the host evaluator ---------------------------------------
                    if P == args.extras_at and not skew:
                        ab = {}
                        for lanes in [v for v in RL.LANES if v <= w // 2]:
                            r.set_tuning("lanes", lanes)
                            ab[str(lanes)], _ = timed(run_call, restore_rows)
                        r.set_tuning("lanes", 0)
                        emit({"record": "lanes", "population": P, "w": w, "events": total, "run_ms_by_lanes": ab, "default": RL.default_lanes(w)})
                        emit(host_rate(P, w, limit, rows0.cpu().numpy().view(np.uint64).reshape(P, w), off, ev, ts, src, total, args.host_threads))
                    del d_off, d_ev, d_ts, d_src, acks
                # ---- the expire sweep --------------------------------------------------------------
                r.reserve(0, P, w)
                for name, timeout in (("nothing_due", 2 * OLD), ("one_percent_due", OLD // 2), ("everything_due", 0)):
                    for g in inst:
                        g["x"] = RL.Rel.expire_args(P, P, table.data_ptr(), P, g["rows"].data_ptr(), w, NOW, g["xst"].data_ptr(),
                                                    g["xcnt"].data_ptr(), timeout_ms=timeout)
                    x_call = lambda i: r.expire_device_async(inst[i]["x"], inst[i]["xsum"].data_ptr(), stream=stream)  # noqa: E731
                    with torch.cuda.stream(ts_):
                        restore_rows(0)
                        x_call(0)
                    torch.cuda.synchronize()
                    xs = words(inst[0]["xsum"], RL.EXPIRE_SUMMARY)
                    assert xs["flags"] == 0 and xs["ok_sessions"] == P and xs["expired"] + xs["remaining"] == AWAITING * P, xs
                    if P <= 100_000:
                        h_rows = rows0.cpu().numpy().view(np.uint64).reshape(P, w).copy()
                        h_tab = np.frombuffer(table.cpu().numpy().tobytes(), dtype=WN.SESSION).copy()
                        ref = RL.Rel(RL.HOST_ONLY).expire_host(h_tab, h_rows, NOW, timeout_ms=timeout)
                        assert ref.summary == xs and inst[0]["rows"].cpu().numpy().tobytes() == h_rows.tobytes()
                        assert inst[0]["xcnt"][:4 * P].cpu().numpy().tobytes() == ref.counts.tobytes()
                    x_ms, reps = timed(x_call, restore_rows)
                    moved = expire_bytes_model(w, P, xs["expired"] // 2)
                    emit({"record": "expire", "case": name, "population": P, "w": w, "timeout_ms": timeout, "instances": copies,
                          "calls_per_window": reps * copies, "checked_against_host": P <= 100_000,
                          "summary": {k: xs[k] for k in RL.EXPIRE_SUMMARY[1:6]}, "expire_ms": x_ms,
                          "m_sessions_per_s": round(P / (x_ms * 1e-3) / 1e6, 1),
                          "model": {"bytes_per_call": int(moved), "gb_per_s": round(moved / (x_ms * 1e-3) / 1e9, 1)}})
            except Exception as e:  # a line that could not be measured says so
                emit({"record": "error", "population": population, "w": w, "error": repr(e)[:300]})
                torch.cuda.synchronize()
            inst = r = a = rows0 = slots0 = table = None
            torch.cuda.empty_cache()
    out.close()


def host_rate(P, w, limit, rows0, off, ev, ts, src, total, threads):
    """The host evaluator over the table sharded by session, a handle a thread."""
    tab = WN.pack_sessions(P)
    cuts = np.linspace(0, P, threads + 1).astype(np.int64)
    times = []
    for _ in range(2):
        rows = rows0.copy()
        jobs = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            h = RL.Rel(RL.HOST_ONLY)
            ids = np.arange(lo, hi, dtype=np.uint32)
            o = (off[lo:hi + 1] - off[lo]).astype(np.uint64)
            a, b = int(off[lo]), int(off[hi])
            jobs.append(lambda h=h, ids=ids, o=o, a=a, b=b: h.run_host(ids, o, ev[a:b], tab, rows, max_awaiting=limit, now_ms=NOW,
                                                                       ts=ts[a:b], src=src[a:b]))
        ths = [threading.Thread(target=j) for j in jobs]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        times.append(time.perf_counter() - t0)
    ms = round(min(times) * 1e3, 2)
    return {"record": "host", "population": P, "w": w, "threads": threads, "run_ms": ms, "m_events_per_s": round(total / ms / 1e3, 1)}


if __name__ == "__main__":
    main()
