"""Rates of the batched route stage (emqx_amd/route.py) behind config B's match, for DESIGN.md
§3.13: device-resident match CSRs (config B's generator at 1 M filters, EMQX_MODE_ROUTES on the
device) against route tables of clusters of 2, 8, 23 and 64 nodes: every filter on one uniformly
drawn node, 10 % of them on 2 to 4 nodes, 0.1 % on every node, 5 % with a grouped dest.  The timed
calls are the asynchronous form on one stream, rotated over 8 batches of 262 144 messages (a
rotation touches more than the 256 MiB Infinity Cache), between device
events around ~0.3 s of calls (100 sweeps at most), three windows, the median reported with all
three.  Copy 0 is compared with emqx_route_host before timing.  Path 1 (expand, library radix
sort, gather) is timed the same way; the host path is emqx_route_host sharded by message over 16
threads on copy 0.  One more row spreads the table over 10 M filter ids (a 160 MB record array):
there the CSRs keep config B's offsets and draw their ids uniformly from the 10 M, because the
engine holds 1 M filters.  No target is set in advance; every line goes to the output file as
measured.

  python tools/route_bench.py [--out profiles/route_sweep.jsonl] [--filters 1000000] [--topics 2097152]
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

from emqx_amd import route as RT  # noqa: E402
from emqx_amd import workloads as W  # noqa: E402

CLUSTERS = (2, 8, 23, 64)
HBM_PEAK_GBS = 8000.0  # MI355X


def table_dests(ids: np.ndarray, n_nodes: int, seed: int):
    """(filter ids, nodes, groups) of the sweep's table over the given filter ids."""
    r = np.random.default_rng(seed)
    n = ids.size
    f, v, g = [ids], [r.integers(0, n_nodes, n).astype(np.uint32)], [np.full(n, RT.NO_GROUP, np.uint32)]
    more = np.flatnonzero(r.random(n) < 0.10)
    for k in range(3):  # 1 to 3 more draws: 2 to 4 nodes where they differ
        sel = more[r.integers(0, 3, more.size) >= k]
        f.append(ids[sel])
        v.append(r.integers(0, n_nodes, sel.size).astype(np.uint32))
        g.append(np.full(sel.size, RT.NO_GROUP, np.uint32))
    every = np.flatnonzero(r.random(n) < 0.001)
    for node in range(n_nodes):
        f.append(ids[every])
        v.append(np.full(every.size, node, np.uint32))
        g.append(np.full(every.size, RT.NO_GROUP, np.uint32))
    grouped = np.flatnonzero(r.random(n) < 0.05)
    f.append(ids[grouped])
    v.append(r.integers(0, n_nodes, grouped.size).astype(np.uint32))
    g.append(r.integers(0, 16, grouped.size).astype(np.uint32))
    return np.concatenate(f).astype(np.uint32), np.concatenate(v), np.concatenate(g)


def host_rate(t, off, ids, threads):
    """Entries/s of emqx_route_host over one batch, sharded by message."""
    n = len(off) - 1
    cuts = np.searchsorted(off, np.linspace(0, int(off[-1]), threads + 1)).clip(0, n)
    cuts[0], cuts[-1] = 0, n
    shards = []
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if b > a:
            shards.append((np.ascontiguousarray(off[a:b + 1] - off[a]), ids[int(off[a]):int(off[b])].copy()))
    times = []
    for _ in range(3):
        ths = [threading.Thread(target=lambda s=s: t.route_host(*s)) for s in shards]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        times.append(time.perf_counter() - t0)
    return int(off[-1]) / min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_sweep.jsonl"))
    ap.add_argument("--filters", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=1 << 21, help="messages in all (split over --batches)")
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clusters", default=",".join(map(str, CLUSTERS)))
    ap.add_argument("--big", type=int, default=10_000_000, help="filter ids of the spread-out row (0: skip it)")
    args = ap.parse_args()
    import torch
    from emqx_amd.engine import Engine
    assert torch.cuda.is_available(), "route_bench needs a HIP device"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    t0 = time.time()
    wl = W.config_b(n_filters=args.filters, n_topics=args.topics)
    eng = Engine(0)
    fids = eng.insert_packed(*wl.filters)
    eng.commit()
    tb, to = wl.topics
    per = args.topics // args.batches
    csrs = []
    for k in range(args.batches):
        lo, hi = k * per, (k + 1) * per
        o = to[lo:hi + 1].astype(np.uint64)
        d_tb = torch.from_numpy(np.array(tb[int(o[0]):int(o[-1])])).to(dev)
        d_to = torch.from_numpy((o - o[0]).view(np.int64)).to(dev)
        mcap = 64 * per
        moff = torch.empty(per + 1, dtype=torch.int64, device=dev)
        mids = torch.empty(mcap, dtype=torch.int32, device=dev)
        total = eng.match_device(d_tb.data_ptr(), d_to.data_ptr(), per, moff.data_ptr(), mids.data_ptr(), mcap, mode=0)
        csrs.append((moff, mids[:max(total, 1)].clone(), total))
    eng.close()
    per_msg = np.diff(csrs[0][0].cpu().numpy().astype(np.int64))
    emit({"record": "workload", "config": "B", "filters": int(wl.n_filters), "messages_per_batch": per,
          "batches": args.batches, "entries_per_batch": [c[2] for c in csrs],
          "max_entries_per_message": int(per_msg.max()), "messages_without_entries": float(round((per_msg == 0).mean(), 4)),
          "setup_s": round(time.time() - t0, 1)})
    stream = torch.cuda.current_stream().cuda_stream

    def row(label, n_nodes, ids, csrs):
        tb0 = time.time()
        t = RT.RouteTable(0, 0)
        t.add(*table_dests(ids, n_nodes, seed=n_nodes))
        fill_s = time.time() - tb0
        t.commit()
        s = t.stats()
        batches = []
        probe = torch.zeros(per, dtype=torch.int32, device=dev)
        node_probe = torch.zeros(RT.MAX_NODES + 1, dtype=torch.int64, device=dev)
        for moff, mids, total in csrs:
            try:  # a probe without room tells the forwards of this batch: both paths get exactly that much
                cap_fwd = t.route_device(RT.RouteTable.batch(moff.data_ptr(), mids.data_ptr(), per, total, 0, probe.data_ptr(),
                                                             node_probe.data_ptr(), 0, 0, 0))["forwards"]
            except RT.EngineError as e:
                if e.code != -4:
                    raise
                cap_fwd = e.needed
            cap_fwd = max(cap_fwd, 1)
            b = {"n": per, "total": total, "cap_fwd": cap_fwd,
                 "flags": torch.zeros(max(total, 1), dtype=torch.uint8, device=dev),
                 "routes": torch.zeros(per, dtype=torch.int32, device=dev),
                 "node_off": torch.zeros(RT.MAX_NODES + 1, dtype=torch.int64, device=dev),
                 "fm": torch.zeros(cap_fwd, dtype=torch.int32, device=dev),
                 "ff": torch.zeros(cap_fwd, dtype=torch.int32, device=dev),
                 "loff": torch.zeros(per + 1, dtype=torch.int64, device=dev),
                 "lfil": torch.zeros(max(total, 1), dtype=torch.int32, device=dev),
                 "sum": torch.zeros(8, dtype=torch.int64, device=dev)}
            b["args"] = RT.RouteTable.batch(moff.data_ptr(), mids.data_ptr(), per, total, b["flags"].data_ptr(),
                                            b["routes"].data_ptr(), b["node_off"].data_ptr(), b["fm"].data_ptr(),
                                            b["ff"].data_ptr(), cap_fwd, b["loff"].data_ptr(), b["lfil"].data_ptr())
            batches.append(b)
        entries = [b["total"] for b in batches]
        host0 = (csrs[0][0].cpu().numpy().view(np.uint64), csrs[0][1][:csrs[0][2]].cpu().numpy().view(np.uint32))
        ref = t.route_host(*host0)

        def sweep():
            for b in batches:
                t.route_device_async(b["args"], b["sum"].data_ptr(), stream=stream)

        def timed():
            sweep()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sweep()
            e1.record()
            e1.synchronize()
            reps = int(min(100, max(1, 300.0 / max(e0.elapsed_time(e1), 1e-3))))
            for _ in range(reps):  # one untimed window: a call in flight takes a scratch of its own, so the
                sweep()            # handle's pool (path 1: with its sort buffers) grows to the queue's depth here
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    sweep()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / (reps * len(batches)))
            return ms, reps

        res = {}
        for path in (0, 1, 2):  # 2: path 0 with the second pass reading pass 1's per-entry word
            t.set_tuning("path", path % 2)
            t.set_tuning("stored_mask", 1 if path == 2 else 0)
            ms, reps = timed()
            # copy 0 against the host evaluator, byte for byte
            b = batches[0]
            sm = dict(zip(RT.SUMMARY, b["sum"].cpu().numpy().view(np.uint64).tolist()))
            assert sm == ref.summary, (path, sm, ref.summary)
            k = sm["forwards"]
            assert b["fm"][:k].cpu().numpy().view(np.uint32).tobytes() == ref.fwd_msgs.tobytes(), path
            assert b["ff"][:k].cpu().numpy().view(np.uint32).tobytes() == ref.fwd_filters.tobytes(), path
            assert b["node_off"].cpu().numpy().view(np.uint64).tobytes() == ref.node_offsets.tobytes(), path
            assert b["routes"].cpu().numpy().view(np.uint32).tobytes() == ref.msg_routes.tobytes(), path
            assert b["flags"][:b["total"]].cpu().numpy().tobytes() == ref.entry_flags.tobytes(), path
            assert b["lfil"][:sm["kept"]].cpu().numpy().view(np.uint32).tobytes() == ref.local_filters.tobytes(), path
            res[path] = (ms, reps)
        summ = [dict(zip(RT.SUMMARY, b["sum"].cpu().numpy().view(np.uint64).tolist())) for b in batches]
        tot = sum(x["entries"] for x in summ)
        fwd = sum(x["forwards"] for x in summ)
        kept = sum(x["kept"] for x in summ)
        best = 0 if float(np.median(res[0][0])) <= float(np.median(res[2][0])) else 2
        ms0 = float(np.median(res[best][0]))
        mean_entries = tot / len(batches)
        # the bytes model: per entry the filter id (4) and the 16-byte record, gathered by the count pass and
        # again by the scatter pass (or, with the stored mask, the id again and 8 written + 8 read), and the
        # flags byte; per forward 8; per message msg_routes and local_offsets (12)
        gathers = 2 if best == 0 else 1
        model = tot * (4 + 16 * gathers + 1 + (0 if best == 0 else 4 + 16)) + fwd * 8 + per * len(batches) * 12
        gbs = model / len(batches) / (ms0 * 1e-3) / 1e9
        emit({"record": "sweep", "row": label, "nodes": n_nodes, "slots": int(ids.max()) + 1, "filters_with_dests": s["n_filters"],
              "plain": s["n_plain"], "grouped": s["n_grouped"], "fill_s": round(fill_s, 1), "build_ms": round(s["last_build_ms"], 1),
              "ms_per_batch_regather": [round(x, 4) for x in res[0][0]],
              "ms_per_batch_stored_mask": [round(x, 4) for x in res[2][0]],
              "ms_per_batch_path1": [round(x, 4) for x in res[1][0]], "reported": "regather" if best == 0 else "stored_mask",
              "sweeps_per_window": [res[0][1], res[2][1], res[1][1]],
              "m_entries_per_s": round(mean_entries / ms0 / 1e3, 1),
              "m_forwards_per_s": round(fwd / len(batches) / ms0 / 1e3, 1),
              "path1_over_path0": round(float(np.median(res[1][0])) / ms0, 2),
              "forwards_per_entry": round(fwd / max(tot, 1), 3), "kept_per_entry": round(kept / max(tot, 1), 3),
              "unknown_fraction": round(sum(x["unknown"] for x in summ) / max(tot, 1), 4),
              "model_bytes_per_batch": int(model / len(batches)), "model_gb_per_s": round(gbs, 1),
              "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
              "host_%d_threads_m_entries_per_s" % args.host_threads: round(host_rate(t, *host0, args.host_threads) / 1e6, 2)})
        t.close()

    for n_nodes in [int(x) for x in args.clusters.split(",")]:
        row("config B, %d filters" % args.filters, n_nodes, np.asarray(fids, dtype=np.uint32), csrs)
    if args.big:
        r = np.random.default_rng(10)
        spread = []
        for moff, mids, total in csrs:
            ids = torch.from_numpy(r.integers(0, args.big, max(total, 1)).astype(np.int32)).to(dev)
            spread.append((moff, ids, total))
        row("ids uniform over %d slots, config B's offsets" % args.big, 23, np.arange(args.big, dtype=np.uint32), spread)
    out.close()


if __name__ == "__main__":
    main()
