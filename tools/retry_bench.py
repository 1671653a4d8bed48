"""Rates of the retry stage (emqx_amd/retry.py) for DESIGN.md §3.15.

The sweep: W = 32, subs NULL (the whole table), populations of 1 K to 10 M connected sessions filled
as tools/ack_bench.py fills them (1 to 8 QoS 1 messages inflight in the lowest slots of each row),
swept at an interval of 30 s with 0 %, 1 % and 100 % of the sessions due (every entry of a due
session is one interval old, the others half of it); a tenth of the due messages are past their
deadline.  A sweep changes what it sweeps, so every timed call starts from the same state: the rows,
stamps and records of an instance are restored from a pristine copy before it, outside the events
(which also leaves the caches cold).  The tables of a population exist in `copies` instances that the
calls rotate over, at least --rotate-bytes (1 GiB) in all where 12 instances reach it.  Each call
lies between two events on one stream; a window is ~0.3 s of calls and the median of three windows is
reported.  Before timing, the first call on instance 0 is checked byte for byte against
emqx_retry_sweep_host.  The host path is emqx_retry_sweep_host on 16 threads, each over its own share
of the sessions with a handle of its own.

The stamp call is measured where it runs, on the ack bench's cycle (window -> record -> stamp -> the
acks -> run -> stamp, every send acked): after record it stamps every send, after run it clears every
stamp.  The run call of that cycle is the yardstick of the sweep, measured in the same process on the
same population; the figure of profiles/ack_sweep.jsonl is quoted next to it.  No target is set in
advance; every line goes to the output file as measured.

  python tools/retry_bench.py [--out profiles/retry_sweep.jsonl] [--populations 1000,...]
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
from emqx_amd import retry as RT  # noqa: E402
from emqx_amd import window as WN  # noqa: E402

POPULATIONS = (1_000, 10_000, 100_000, 1_000_000, 10_000_000)
FRACTIONS = (0.0, 0.01, 1.0)
W = 32
NOW, INTERVAL = 1_700_000_000_000, 30_000
EXPIRED_SHARE = 0.1


def bytes_model(population: int, items: int, expired: int, w: int = W) -> float:
    """Bytes a sweep moves: per session the row, its stamps and the record read by
    the count and by the emit pass (2 * (16 w + 32)) and the offset, status, counts and timer written
    (8 + 1 + 16 + 4); per item the item written, its deadline read and the 16 bytes of stamps it
    shares with its neighbour written (8 + 8 + 16); per expired item 16 bytes of slots written."""
    return (2.0 * (16 * w + 32) + 29) * population + 32.0 * items + 16.0 * expired


def stamp_bytes_model(population: int, changed: int, w: int = W) -> float:
    """Of a stamp call: per row the id, the row and its stamps read (4 + 16 w); per changed stamp
    the 16 bytes it shares with its neighbour written."""
    return (4.0 + 16 * w) * population + 16.0 * changed


def fill(population, fraction, rng):
    """The tables of one population: (table, slots, stamps, deadlines, items due)."""
    lens = rng.integers(1, 9, population)
    total = int(lens.sum())
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    slots = AK.empty_slots(population, W)
    stamps = RT.empty_stamps(population, W)
    due = rng.random(population) < fraction if 0 < fraction < 1 else np.full(population, fraction >= 1)
    ts = np.where(due, NOW - INTERVAL, NOW - INTERVAL // 2).astype(np.uint64)
    base = rng.integers(1, 65536 - 8, population)
    for j in range(8):
        on = lens > j
        ids = (base + j).astype(np.uint64)
        slots["pkt_id"][on, j] = ids[on]
        slots["phase"][on, j] = AK.MSG
        slots["qos"][on, j] = 1
        slots["ref"][on, j] = (first + j)[on]
        stamps[on, j] = ((ts << np.uint64(19)) | np.uint64(AK.MSG << 16) | ids)[on]
    deadlines = np.full(total, RT.NO_EXPIRY, dtype=np.uint64)
    deadlines[rng.random(total) < EXPIRED_SHARE] = NOW - 1
    table = WN.pack_sessions(population, inflight=lens)
    return table, slots, stamps, deadlines, int(lens[due].sum())


def host_rate(table, slots, stamps, deadlines, threads):
    """Sessions/s of emqx_retry_sweep_host over the table sharded by session, a handle a thread."""
    population = table.size
    cuts = np.linspace(0, population, threads + 1).astype(np.int64)
    times = []
    for _ in range(2):
        t, s, st = table.copy(), slots.copy(), stamps.copy()
        shards = [(RT.Retry(RT.HOST_ONLY), np.arange(a, b, dtype=np.uint32)) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        ths = [threading.Thread(target=lambda x=x: x[0].sweep_host(x[1], t, s, st, NOW, INTERVAL, deadlines=deadlines, update_table=True))
               for x in shards]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        times.append(time.perf_counter() - t0)
    return population / min(times)


def ack_yardstick(population):
    """ms per run call at this population from profiles/ack_sweep.jsonl (the even mix)."""
    path = os.path.join(ROOT, "profiles", "ack_sweep.jsonl")
    if not os.path.exists(path):
        return None
    for line in open(path):
        rec = json.loads(line)
        if rec.get("record") == "sweep" and rec["population"] == population and not rec["skewed"]:
            return rec["run"]["ms_per_call"]
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retry_sweep.jsonl"))
    ap.add_argument("--populations", default=",".join(map(str, POPULATIONS)))
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30, help="the instances of a population hold at least this much")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "retry_bench needs a HIP device"
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
    ts = torch.cuda.Stream(device=dev)
    stream = ts.cuda_stream
    emit({"record": "setup", "w": W, "interval_ms": INTERVAL, "inflight_per_session": "1..8", "expired_share_of_due": EXPIRED_SHARE,
          "device": torch.cuda.get_device_name(0)})

    def timed(calls, n_inst, rounds):
        """ms per call: `calls(i, events)` enqueues one call on instance i between two events."""
        probe = []
        for i in range(n_inst):
            calls(i, probe)
        torch.cuda.synchronize()
        one = sum(a.elapsed_time(b) for a, b in probe) / len(probe)
        reps = int(min(100, max(1, 300.0 / max(one * n_inst, 1e-3))))
        per_round = []
        for _ in range(rounds):
            events = []
            for _ in range(reps):
                for i in range(n_inst):
                    calls(i, events)
            torch.cuda.synchronize()
            per_round.append(float(np.mean([a.elapsed_time(b) for a, b in events])))
        return float(np.median(per_round)), per_round, reps

    for population in [int(p) for p in args.populations.split(",")]:
        # ---- the ack cycle: the run call (the yardstick) and the two stamp calls ---------------------
        rng = np.random.default_rng(population)
        lens = rng.integers(1, 9, population)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        total = int(off[-1])
        subs = np.arange(population, dtype=np.uint32)
        table = WN.pack_sessions(population, next_pkt_id=rng.integers(1, 65536, population))
        per = (32 + 16 * W) * population + 16 * total
        copies = int(min(12, max(2, -(-args.rotate_bytes // per))))
        win, ack, rt = WN.Window(0), AK.Ack(0), RT.Retry(0)
        win.reserve(total, population)
        ack.reserve(total, population, W)
        rt.reserve(population, W)
        d_subs, d_off, d_opts = up(subs, np.int32), up(off), torch.ones(total, dtype=torch.uint8, device=dev)
        sums = [z(8, torch.int64) for _ in range(5)]
        inst = []
        for c in range(copies):
            g = {"table": up(table), "rows": z(population * W, torch.int64), "stamps": z(population * W, torch.int64),
                 "ver": z(total, torch.uint8), "ids": z(total, torch.int16), "recs": z(4 * population, torch.int64),
                 "cnt": z(4 * population, torch.int32), "unrec": z(population, torch.int32), "acks": z(total, torch.int32),
                 "aver": z(total, torch.uint8), "arefs": z(total, torch.int32), "acnt": z(4 * population, torch.int32)}
            g["w"] = WN.Window.batch(d_subs.data_ptr(), d_off.data_ptr(), d_opts.data_ptr(), population, total, population,
                                     g["table"].data_ptr(), population, g["ver"].data_ptr(), g["ids"].data_ptr(), g["recs"].data_ptr(),
                                     g["cnt"].data_ptr(), update_table=True)
            g["r"] = AK.Ack.record_args(d_subs.data_ptr(), d_off.data_ptr(), d_opts.data_ptr(), population, total, population,
                                        g["ver"].data_ptr(), g["ids"].data_ptr(), g["rows"].data_ptr(), W, population,
                                        g["unrec"].data_ptr())
            g["a"] = AK.Ack.run_args(d_subs.data_ptr(), d_off.data_ptr(), g["acks"].data_ptr(), population, total, population,
                                     g["table"].data_ptr(), population, g["rows"].data_ptr(), W, g["aver"].data_ptr(),
                                     g["arefs"].data_ptr(), g["acnt"].data_ptr(), update_table=True)
            g["s"] = RT.Retry.stamp_args(d_subs.data_ptr(), population, population, g["rows"].data_ptr(), g["stamps"].data_ptr(), W,
                                         population, NOW)
            inst.append(g)
        marks_of = {"stamp_after_record": (2, 3), "run": (4, 5), "stamp_after_run": (5, 6)}

        def cycle(i, events, which=None):
            g = inst[i]
            with torch.cuda.stream(ts):
                m = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
                m[0].record(ts)
                win.run_device_async(g["w"], sums[0].data_ptr(), stream=stream)
                m[1].record(ts)
                ack.record_device_async(g["r"], sums[1].data_ptr(), stream=stream)
                m[2].record(ts)
                rt.stamp_device_async(g["s"], sums[2].data_ptr(), stream=stream)
                m[3].record(ts)
                g["acks"][:total] = (g["ids"][:total].to(torch.int32) & 0xFFFF) | (AK.PUBACK << 16)
                m[4].record(ts)
                ack.run_device_async(g["a"], sums[3].data_ptr(), stream=stream)
                m[5].record(ts)
                rt.stamp_device_async(g["s"], sums[4].data_ptr(), stream=stream)
                m[6].record(ts)
                if which is not None:
                    a, b = marks_of[which]
                    events.append((m[a], m[b]))

        torch.cuda.synchronize()
        cycle(0, None)
        torch.cuda.synchronize()
        s1, s2 = (dict(zip(RT.STAMP_SUMMARY, sums[k].cpu().numpy().view(np.uint64).tolist())) for k in (2, 4))
        assert s1["stamped"] == total and s1["cleared"] == 0 and s2["cleared"] == total and s2["stamped"] == 0, (s1, s2)
        assert not inst[0]["stamps"].any().item() and not inst[0]["rows"].any().item()
        cyc = {}
        for which in marks_of:
            med, rounds, reps = timed(lambda i, ev, which=which: cycle(i, ev, which), copies, args.rounds)
            cyc[which] = {"ms_per_call": round(med, 4), "rounds_ms": [round(x, 4) for x in rounds], "cycles_per_window": reps}
        run_ms = cyc["run"]["ms_per_call"]
        for which in ("stamp_after_record", "stamp_after_run"):
            moved = stamp_bytes_model(population, total)
            cyc[which]["model"] = {"bytes_per_call": int(moved), "gb_per_s": round(moved / (cyc[which]["ms_per_call"] * 1e-3) / 1e9, 1)}
            cyc[which]["ratio_to_run"] = round(cyc[which]["ms_per_call"] / run_ms, 3)
        emit({"record": "cycle", "population": population, "sends": total, "instances": copies, **cyc,
              "ack_sweep_yardstick_run_ms": ack_yardstick(population)})
        del inst, win, ack
        torch.cuda.empty_cache()

        # ---- the sweep --------------------------------------------------------------------------------
        for fraction in FRACTIONS:
            rng = np.random.default_rng(population + int(fraction * 1000))
            table, slots, stamps, deadlines, items = fill(population, fraction, rng)
            cap_out = max(items, 1)
            per = (32 + 16 * W) * population * 2 + 8 * deadlines.size + 29 * population + 8 * cap_out
            copies = int(min(12, max(2, -(-args.rotate_bytes // per))))
            d_dead = up(deadlines)
            summary = z(8, torch.int64)
            inst = []
            for c in range(copies):
                g = {"table0": up(table), "rows0": up(slots), "stamps0": up(stamps)}
                for k in ("table", "rows", "stamps"):
                    g[k] = g[k + "0"].clone()
                g.update(off=z(population + 1, torch.int64), items=z(cap_out, torch.int64), status=z(population, torch.uint8),
                         cnt=z(4 * population, torch.int32), timers=z(population, torch.int32))
                g["args"] = RT.Retry.sweep_args(0, population, population, g["table"].data_ptr(), population, g["rows"].data_ptr(),
                                                g["stamps"].data_ptr(), W, NOW, INTERVAL, cap_out, g["off"].data_ptr(),
                                                g["items"].data_ptr(), g["status"].data_ptr(), g["cnt"].data_ptr(), g["timers"].data_ptr(),
                                                d_deadlines=d_dead.data_ptr(), ref_limit=deadlines.size, update_table=True)
                inst.append(g)

            def call(i, events):
                g = inst[i]
                with torch.cuda.stream(ts):
                    for k in ("table", "rows", "stamps"):
                        g[k].copy_(g[k + "0"])
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(ts)
                    rt.sweep_device_async(g["args"], summary.data_ptr(), stream=stream)
                    b.record(ts)
                    events.append((a, b))

            # the first call on instance 0 against the host evaluator, byte for byte
            torch.cuda.synchronize()
            call(0, [])
            torch.cuda.synchronize()
            h_table, h_slots, h_stamps = table.copy(), slots.copy(), stamps.copy()
            ref = RT.Retry(RT.HOST_ONLY).sweep_host(None, h_table, h_slots, h_stamps, NOW, INTERVAL, deadlines=deadlines, cap_out=cap_out,
                                                    update_table=True)
            words = dict(zip(RT.SWEEP_SUMMARY, summary.cpu().numpy().view(np.uint64).tolist()))
            assert words == ref.summary and words["items"] == items, (words, ref.summary, items)
            g = inst[0]
            for got, want in ((g["off"], ref.offsets), (g["items"][:items], ref.items), (g["status"], ref.status), (g["cnt"], ref.counts),
                              (g["timers"], ref.timers), (g["rows"], h_slots), (g["stamps"], h_stamps), (g["table"], h_table)):
                assert got.cpu().numpy().tobytes() == want.tobytes(), (population, fraction)
            med, rounds, reps = timed(call, copies, args.rounds)
            moved = bytes_model(population, items, words["expired"])
            emit({"record": "sweep", "population": population, "due_fraction": fraction, "items": items, "instances": copies,
                  "calls_per_window": reps, "summary": {k: words[k] for k in RT.SWEEP_SUMMARY[3:]},
                  "ms_per_call": round(med, 4), "rounds_ms": [round(x, 4) for x in rounds],
                  "m_sessions_per_s": round(population / (med * 1e-3) / 1e6, 2), "m_items_per_s": round(items / (med * 1e-3) / 1e6, 2),
                  "model": {"bytes_per_call": int(moved), "gb_per_s": round(moved / (med * 1e-3) / 1e9, 1)},
                  "ack_run_same_population_ms": run_ms, "ratio_to_ack_run": round(med / run_ms, 3),
                  "scratch_bytes": rt.stats()["scratch_bytes"],
                  "host_%d_threads_m_sessions_per_s" % args.host_threads: round(
                      host_rate(table, slots, stamps, deadlines, args.host_threads) / 1e6, 2)})
            del inst
            torch.cuda.empty_cache()
        del rt
    out.close()


if __name__ == "__main__":
    main()
