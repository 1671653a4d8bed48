"""Rates of the ack stage (emqx_amd/ack.py) for DESIGN.md §3.14, measured in the cycle a broker
runs: the window stage admits a batch (emqx_window_run_batch_device_async, update_table), the
record call stores its sends in the slot table, the clients' acks come back and the run call
releases the slots and reopens the window (update_table), and the next batch finds the window open
again.  Every session is connected with inflight_max 32 and W = 32 slots; a batch gives each
session 1 to 8 QoS 1 deliveries and every one of them is acked with a PUBACK, so the cycle is in a
steady state and every call does the same work each time.

Populations of 1 K to 10 M sessions (the even mix), plus the case in which one session sends 10 %
of all acks, all but its own few bogus (ids it does not hold).  The tables of a population (rows,
records, outputs) exist in `copies` instances that the cycle rotates over, enough that they exceed
the 256 MiB Infinity Cache wherever one instance does not on its own.  Each call lies between two
events on one stream; a window is ~0.3 s of cycles and the median over the windows is reported.
Before timing, the first cycle on instance 0 is checked byte for byte against the host evaluators
of the three stages.  The host path is emqx_ack_run_host on 16 threads, each over its own share
of the sessions with a handle of its own.  The window stage's time per delivery from
profiles/window_sweep.jsonl (connected_32, the same population) is quoted next to the one measured
here.  No target is set in advance; every line goes to the output file as measured.

  python tools/ack_bench.py [--out profiles/ack_sweep.jsonl] [--populations 1000,...]
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
from emqx_amd import window as WN  # noqa: E402

POPULATIONS = (1_000, 10_000, 100_000, 1_000_000, 10_000_000)
SKEW_POPULATION, SKEW_SHARE = 1_000_000, 0.10
W = 32


def bytes_model(total: int, m: int, w: int = W) -> float:
    """Bytes a run call moves: per ack the ack word read by three passes, its
    slot index written once and read twice, the verdict and the ref written, its slot and its two
    minima read, one atomic (12 + 3 + 5 + 16 + 4), and its row read once to find the slot (8 w,
    served by the L2 for the acks of one session that share a tile); per session first[] and comp[]
    initialised and read back (16 w), the row read and its changed slots written (up to 16 w), the
    record, the offsets, the id and the counts (32 + 16 + 4 + 16)."""
    return (40.0 + 8 * w) * total + (32.0 * w + 68) * m


def record_bytes_model(total: int, m: int, w: int = W) -> float:
    """Of a record call: per delivery the verdict read by both tile passes (2); per send the id,
    the opts byte, the ref, its inbox's offsets, prefix and mask and the slot written (2 + 1 + 4 +
    16 + 8 + 8 + 8); per inbox the row read (8 w), the mask, the prefixes and the count (8 + 8 +
    4 + 12)."""
    return 2.0 * total + 47.0 * total + (8.0 * w + 32) * m


def host_rate(subs, off, acks, table, slots, threads):
    """Acks/s of emqx_ack_run_host over one batch sharded by session, a handle a thread; the rows
    and records of distinct sessions are distinct, so the shards share the tables."""
    m = len(subs)
    cuts = np.searchsorted(off, np.linspace(0, int(off[-1]), threads + 1)).clip(0, m)
    cuts[0], cuts[-1] = 0, m
    shards = []
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if b > a:
            lo, hi = int(off[a]), int(off[b])
            shards.append((AK.Ack(AK.HOST_ONLY), subs[a:b].copy(), np.ascontiguousarray(off[a:b + 1] - off[a]), acks[lo:hi].copy()))
    times = []
    for _ in range(3):
        rows = slots.copy()
        ths = [threading.Thread(target=lambda s=s: s[0].run_host(s[1], s[2], s[3], table, rows)) for s in shards]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        times.append(time.perf_counter() - t0)
    return int(off[-1]) / min(times)


def window_yardstick(population):
    """ns per delivery of the window stage at this population from profiles/window_sweep.jsonl."""
    path = os.path.join(ROOT, "profiles", "window_sweep.jsonl")
    if not os.path.exists(path):
        return None
    total = None
    for line in open(path):
        rec = json.loads(line)
        if rec.get("record") == "workload":
            total = rec["kept_deliveries"]
        if rec.get("record") == "sweep" and rec["population"] == population and rec["mix"] == "connected_32" and not rec["skewed"]:
            return {"ms_per_call": rec["window"]["ms_per_call"], "deliveries": total,
                    "ns_per_delivery": round(rec["window"]["ms_per_call"] * 1e6 / total, 4)}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ack_sweep.jsonl"))
    ap.add_argument("--populations", default=",".join(map(str, POPULATIONS)))
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30, help="the instances of a population hold at least this much")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "ack_bench needs a HIP device"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def up(a, view):
        return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(dev)

    z = lambda size, dt: torch.zeros(size, dtype=dt, device=dev)  # noqa: E731
    ts = torch.cuda.Stream(device=dev)
    stream = ts.cuda_stream
    emit({"record": "setup", "w": W, "tile": AK.TILE, "acks_per_session": "1..8", "inflight_max": 32,
          "device": torch.cuda.get_device_name(0)})
    cases = [(int(p), False) for p in args.populations.split(",")] + [(SKEW_POPULATION, True)]
    for population, skew in cases:
        rng = np.random.default_rng(population + skew)
        lens = rng.integers(1, 9, population)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        total = int(off[-1])
        subs = np.arange(population, dtype=np.uint32)
        opts = np.ones(total, dtype=np.uint8)  # QoS 1
        table = WN.pack_sessions(population, next_pkt_id=rng.integers(1, 65536, population))
        # the ack lists: every send acked; skewed: session population // 2 also sends bogus ones
        n_bogus = int(total * SKEW_SHARE / (1 - SKEW_SHARE)) if skew else 0
        hot = population // 2
        cut = int(off[hot + 1])
        a_off = off.copy()
        a_off[hot + 1:] += n_bogus
        a_total = total + n_bogus
        bogus = ((AK.PUBACK << 16) | rng.integers(0, 65536, n_bogus)).astype(np.uint32)
        per = 32 * population + 8 * W * population + 7 * total + 9 * a_total
        copies = int(min(12, max(2, -(-args.rotate_bytes // per))))
        win, ack = WN.Window(0), AK.Ack(0)
        win.reserve(total, population)
        ack.reserve(a_total, population, W)
        d_subs, d_off, d_aoff, d_opts = up(subs, np.int32), up(off, np.int64), up(a_off, np.int64), up(opts, np.uint8)
        w_sum, r_sum, a_sum = z(8, torch.int64), z(8, torch.int64), z(8, torch.int64)
        inst = []
        for c in range(copies):
            g = {"table": torch.from_numpy(np.frombuffer(table.tobytes(), dtype=np.int64).copy()).to(dev),
                 "rows": z(population * W, torch.int64), "ver": z(total, torch.uint8), "ids": z(total, torch.int16),
                 "recs": z(4 * population, torch.int64), "cnt": z(4 * population, torch.int32), "unrec": z(population, torch.int32),
                 "acks": z(a_total, torch.int32), "aver": z(a_total, torch.uint8), "arefs": z(a_total, torch.int32),
                 "acnt": z(4 * population, torch.int32)}
            if n_bogus:
                g["acks"][cut:cut + n_bogus] = up(bogus, np.int32)
            g["w"] = WN.Window.batch(d_subs.data_ptr(), d_off.data_ptr(), d_opts.data_ptr(), population, total, population,
                                     g["table"].data_ptr(), population, g["ver"].data_ptr(), g["ids"].data_ptr(), g["recs"].data_ptr(),
                                     g["cnt"].data_ptr(), update_table=True)
            g["r"] = AK.Ack.record_args(d_subs.data_ptr(), d_off.data_ptr(), d_opts.data_ptr(), population, total, population,
                                        g["ver"].data_ptr(), g["ids"].data_ptr(), g["rows"].data_ptr(), W, population,
                                        g["unrec"].data_ptr())
            g["a"] = AK.Ack.run_args(d_subs.data_ptr(), d_aoff.data_ptr(), g["acks"].data_ptr(), population, a_total, population,
                                     g["table"].data_ptr(), population, g["rows"].data_ptr(), W, g["aver"].data_ptr(),
                                     g["arefs"].data_ptr(), g["acnt"].data_ptr(), update_table=True)
            inst.append(g)

        def pack_acks(g):
            """The acks of this cycle: a PUBACK for every id the window stage just handed out."""
            packed = (g["ids"].to(torch.int32) & 0xFFFF) | (AK.PUBACK << 16)
            g["acks"][:cut] = packed[:cut]
            g["acks"][cut + n_bogus:] = packed[cut:]

        def cycle(g, events=None):
            with torch.cuda.stream(ts):
                marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if events is not None else None
                if marks:
                    marks[0].record(ts)
                win.run_device_async(g["w"], w_sum.data_ptr(), stream=stream)
                if marks:
                    marks[1].record(ts)
                ack.record_device_async(g["r"], r_sum.data_ptr(), stream=stream)
                if marks:
                    marks[2].record(ts)
                pack_acks(g)
                if marks:
                    marks[3].record(ts)
                ack.run_device_async(g["a"], a_sum.data_ptr(), stream=stream)
                if marks:
                    marks[4].record(ts)
                    events.append(marks)

        # ---- the first cycle on instance 0 against the host evaluators ---------------------------
        g = inst[0]
        torch.cuda.synchronize()
        cycle(g)
        torch.cuda.synchronize()
        h_table = table.copy()
        wref = WN.Window(WN.HOST_ONLY).run_host(subs, off, opts, h_table, update_table=True)
        assert g["ver"].cpu().numpy().tobytes() == wref.verdicts.tobytes() and wref.summary["sends"] == total
        h_rows = AK.empty_slots(population, W)
        rref = AK.Ack(AK.HOST_ONLY).record_host(subs, off, opts, wref.verdicts, wref.pkt_ids, h_rows)
        assert dict(zip(AK.RECORD_SUMMARY, r_sum.cpu().numpy().view(np.uint64).tolist())) == rref.summary, rref.summary
        h_acks = np.empty(a_total, dtype=np.uint32)
        packed = AK.pack_acks(AK.PUBACK, wref.pkt_ids)
        h_acks[:cut], h_acks[cut:cut + n_bogus], h_acks[cut + n_bogus:] = packed[:cut], bogus, packed[cut:]
        assert g["acks"].cpu().numpy().view(np.uint32).tobytes() == h_acks.tobytes()
        rows_before = h_rows.copy()
        aref = AK.Ack(AK.HOST_ONLY).run_host(subs, a_off, h_acks, h_table, h_rows, update_table=True)
        words = dict(zip(AK.RUN_SUMMARY, a_sum.cpu().numpy().view(np.uint64).tolist()))
        assert words == aref.summary, (words, aref.summary)
        for got, want in ((g["aver"], aref.verdicts), (g["arefs"], aref.refs), (g["acnt"], aref.counts), (g["rows"], h_rows),
                          (g["table"], h_table)):
            assert got.cpu().numpy().tobytes() == want.tobytes(), (population, skew)
        assert words["oks"] >= total - 64 and words["released"] == words["oks"]
        # ---- timing --------------------------------------------------------------------------------
        for g in inst[1:]:
            cycle(g)  # every instance is one cycle in
        torch.cuda.synchronize()
        probe = []
        for g in inst:
            cycle(g, probe)
        torch.cuda.synchronize()
        one = sum(m[0].elapsed_time(m[4]) for m in probe) / len(probe)
        reps = int(min(100, max(1, 300.0 / max(one * copies, 1e-3))))
        per_round = {"window": [], "record": [], "run": []}
        for _ in range(args.rounds):
            events = []
            for _ in range(reps):
                for g in inst:
                    cycle(g, events)
            torch.cuda.synchronize()
            for key, (i, j) in (("window", (0, 1)), ("record", (1, 2)), ("run", (3, 4))):
                per_round[key].append(float(np.mean([m[i].elapsed_time(m[j]) for m in events])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        moved, rmoved = bytes_model(a_total, population), record_bytes_model(total, population)
        rec = {"record": "sweep", "population": population, "skewed": skew, "acks": a_total, "sends": total, "bogus_acks": n_bogus,
               "instances": copies, "cycles_per_window": reps, "summary": {k: words[k] for k in AK.RUN_SUMMARY[3:]},
               "run": {"ms_per_call": round(med["run"], 4), "rounds_ms": [round(x, 4) for x in per_round["run"]],
                       "g_acks_per_s": round(a_total / (med["run"] * 1e-3) / 1e9, 3),
                       "model": {"bytes_per_call": int(moved), "gb_per_s": round(moved / (med["run"] * 1e-3) / 1e9, 1)}},
               "record_call": {"ms_per_call": round(med["record"], 4), "rounds_ms": [round(x, 4) for x in per_round["record"]],
                               "g_sends_per_s": round(total / (med["record"] * 1e-3) / 1e9, 3),
                               "model": {"bytes_per_call": int(rmoved), "gb_per_s": round(rmoved / (med["record"] * 1e-3) / 1e9, 1)}},
               "window_stage_same_batch": {"ms_per_call": round(med["window"], 4),
                                           "ns_per_delivery": round(med["window"] * 1e6 / total, 4)},
               "window_sweep_yardstick": window_yardstick(population),
               "scratch_bytes": ack.stats()["scratch_bytes"],
               "host_%d_threads_m_acks_per_s" % args.host_threads: round(
                   host_rate(subs, a_off, h_acks, h_table, rows_before, args.host_threads) / 1e6, 2)}
        emit(rec)
        del inst, win, ack
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
