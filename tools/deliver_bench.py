"""Rates of the batched enrich stage (emqx_amd/deliver.py) behind workload E's fan-out, for
DESIGN.md §3.9: device-resident delivery CSRs (config E's tables, match + fan-out on the device),
annotate-only and compacting, over options tables of 1 K to 10 M entries (the first K of a fixed
shuffle of config E's subscriptions; every other delivery's key is absent).  The timed calls are
the asynchronous form on one stream, rotated over >= 4 distinct batches so that no batch is
served from the Infinity Cache, between device events around ~0.3 s of calls, three rounds.  The
host path is emqx_deliver_enrich_host sharded by message over 16 threads on the same inputs.
No target is set in advance; every line goes to the output file as measured.

  python tools/deliver_bench.py [--out profiles/deliver_sweep.jsonl] [--topics 1048576] [--batches 4]
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

from emqx_amd import deliver as D  # noqa: E402
from emqx_amd import workloads as W  # noqa: E402

SIZES = (1_000, 10_000, 100_000, 1_000_000, 10_000_000)


def host_rate(t, batch, threads):
    """Deliveries/s of emqx_deliver_enrich_host over one batch, sharded by message."""
    off, subs, fils, qos, flags, frm = batch
    n = len(off) - 1
    cuts = np.searchsorted(off, np.linspace(0, int(off[-1]), threads + 1)).clip(0, n)
    cuts[0], cuts[-1] = 0, n
    shards = []
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if b > a:
            lo, hi = int(off[a]), int(off[b])
            shards.append((np.ascontiguousarray(off[a:b + 1] - off[a]), subs[lo:hi].copy(), fils[lo:hi].copy(),
                           qos[a:b].copy(), flags[a:b].copy(), frm[a:b].copy()))
    best = None
    for compact in (False, True):
        times = []
        for _ in range(3):
            ths = [threading.Thread(target=lambda s=s: t.enrich_host(*s, compact=compact)) for s in shards]
            t0 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            times.append(time.perf_counter() - t0)
        rate = int(off[-1]) / min(times)
        best = (best or {})
        best["compact" if compact else "annotate"] = round(rate / 1e6, 2)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deliver_sweep.jsonl"))
    ap.add_argument("--topics", type=int, default=1 << 20, help="messages in all (split over --batches)")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    args = ap.parse_args()
    import torch
    from emqx_amd.engine import Engine
    from emqx_amd.fanout import SubTable
    assert torch.cuda.is_available(), "deliver_bench needs a HIP device"
    assert args.batches >= 4
    torch.cuda.set_device(0)
    dev = "cuda:0"
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    t0 = time.time()
    fw = W.config_e(n_topics=args.topics)
    eng = Engine(0)
    eng.insert_packed(*fw.wl.filters)
    eng.commit()
    st = SubTable(0)
    st.add(fw.sub_filter, fw.sub_id, fw.sub_group)
    st.commit()
    tb, to = fw.wl.topics
    per = args.topics // args.batches
    rng = np.random.default_rng(3)
    batches, host0 = [], None
    for k in range(args.batches):
        lo, hi = k * per, (k + 1) * per
        o = to[lo:hi + 1].astype(np.uint64)
        d_tb = torch.from_numpy(np.array(tb[int(o[0]):int(o[-1])])).to(dev)
        d_to = torch.from_numpy((o - o[0]).view(np.int64)).to(dev)
        mcap, cap = 64 * per, 256 * per
        moff = torch.empty(per + 1, dtype=torch.int64, device=dev)
        mids = torch.empty(mcap, dtype=torch.int32, device=dev)
        eng.match_device(d_tb.data_ptr(), d_to.data_ptr(), per, moff.data_ptr(), mids.data_ptr(), mcap)
        keys = torch.from_numpy(np.array(fw.keys[lo:hi]).view(np.int32)).to(dev)
        doff = torch.empty(per + 1, dtype=torch.int64, device=dev)
        subs = torch.empty(cap, dtype=torch.int32, device=dev)
        fils = torch.empty(cap, dtype=torch.int32, device=dev)
        total = st.fanout_device("hash_clientid", moff.data_ptr(), mids.data_ptr(), per, keys.data_ptr(), doff.data_ptr(),
                                 subs.data_ptr(), fils.data_ptr(), cap)
        subs, fils = subs[:total].clone(), fils[:total].clone()
        del mids, moff
        h_off, h_subs = doff.cpu().numpy().view(np.uint64), subs.cpu().numpy().view(np.uint32)
        qos = rng.integers(0, 3, per).astype(np.uint8)
        flags = rng.integers(0, 4, per).astype(np.uint8)
        # the publisher is the message's first recipient for half of the messages that have one
        first = h_subs[np.minimum(h_off[:-1], max(total - 1, 0)).astype(np.int64)] if total else np.zeros(per, np.uint32)
        mine = (rng.random(per) < 0.5) & (h_off[1:] > h_off[:-1])
        frm = np.where(mine, first, np.uint32(D.NO_SENDER)).astype(np.uint32)
        m = max(total, 1)
        b = {"n": per, "total": total, "doff": doff, "subs": subs, "fils": fils,
             "qos": torch.from_numpy(qos).to(dev), "flags": torch.from_numpy(flags).to(dev),
             "frm": torch.from_numpy(frm.view(np.int32)).to(dev),
             "out": torch.zeros(m, dtype=torch.uint8, device=dev), "ids": torch.zeros(m, dtype=torch.int32, device=dev),
             "koff": torch.zeros(per + 1, dtype=torch.int64, device=dev),
             "ksubs": torch.zeros(m, dtype=torch.int32, device=dev), "kfils": torch.zeros(m, dtype=torch.int32, device=dev),
             "kopts": torch.zeros(m, dtype=torch.uint8, device=dev), "kids": torch.zeros(m, dtype=torch.int32, device=dev),
             "sum": torch.zeros(8, dtype=torch.int64, device=dev)}
        for compact in (False, True):
            b[compact] = D.SubOpts.batch(
                doff.data_ptr(), subs.data_ptr(), fils.data_ptr(), per, total, b["qos"].data_ptr(), b["flags"].data_ptr(),
                b["frm"].data_ptr(), b["out"].data_ptr(), b["ids"].data_ptr(),
                *((b["koff"].data_ptr(), b["ksubs"].data_ptr(), b["kfils"].data_ptr(), b["kopts"].data_ptr(),
                   b["kids"].data_ptr(), total) if compact else ()))
        batches.append(b)
        if k == 0:
            host0 = (h_off, h_subs, fils.cpu().numpy().view(np.uint32), qos, flags, frm)
    deliveries = [b["total"] for b in batches]
    emit({"record": "workload", "config": "E", "filters": int(fw.wl.n_filters), "subscriptions": int(fw.n_subscriptions),
          "messages_per_batch": per, "batches": args.batches, "deliveries_per_batch": deliveries,
          "setup_s": round(time.time() - t0, 1)})

    order = np.random.default_rng(4).permutation(len(fw.sub_id))
    stream = torch.cuda.current_stream().cuda_stream
    for size in [int(x) for x in args.sizes.split(",")]:
        idx = order[:size]
        n = len(idx)
        t = D.SubOpts(0)
        r = np.random.default_rng(size)
        t.set(fw.sub_filter[idx], fw.sub_id[idx], qos=r.integers(0, 3, n), nl=r.random(n) < 0.75, rap=r.integers(0, 2, n),
              upgrade_qos=fw.sub_id[idx] % 3 == 0, subid=np.where(r.random(n) < 0.5, r.integers(1, 1 << 28, n), 0))
        t.commit()
        s = t.stats()
        # check: the first 2000 messages of batch 0, device against host, both modes
        k = 2000
        sample = (host0[0][:k + 1], host0[1][:int(host0[0][k])], host0[2][:int(host0[0][k])], host0[3][:k], host0[4][:k],
                  host0[5][:k])
        for compact in (False, True):
            a, h = t.enrich_packed(*sample, compact=compact), t.enrich_host(*sample, compact=compact)
            assert a.opts.tolist() == h.opts.tolist() and a.subids.tolist() == h.subids.tolist() and a.summary == h.summary
            if compact:
                assert all(x.tolist() == y.tolist() for x, y in zip(a.kept, h.kept))
        rec = {"record": "sweep", "entries": s["n_entries"], "slots": s["n_slots"], "table_mb": round(s["table_bytes"] / 2**20, 2),
               "max_probe": s["max_probe"], "build_ms": round(s["last_build_ms"], 1)}
        for compact in (False, True):
            def sweep():
                for b in batches:
                    t.enrich_device_async(b[compact], b["sum"].data_ptr(), stream=stream)
            sweep()
            torch.cuda.synchronize()
            summ = [b["sum"].cpu().numpy().view(np.uint64).tolist() for b in batches]
            assert all(x[0] == 0 and x[1] == b["total"] for x, b in zip(summ, batches))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sweep()
            e1.record()
            e1.synchronize()
            reps = int(min(100, max(1, 300.0 / max(e0.elapsed_time(e1), 1e-3))))
            rates = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    sweep()
                e1.record()
                e1.synchronize()
                rates.append(sum(deliveries) * reps / (e0.elapsed_time(e1) * 1e-3))
            tot, kept, none = (sum(x[i] for x in summ) for i in (1, 2, 4))
            # algorithmic bytes per delivery: sub + filter read (8), one 16-byte probe, opts byte +
            # subid written (5); compacting re-reads the opts byte, sub, filter and subid (13) and
            # writes the kept copies (13 per kept delivery)
            bytes_per = 8 + 16 + 5 + ((13 + 13 * kept / tot) if compact else 0)
            name = "compact" if compact else "annotate"
            rec[name] = {"g_deliveries_per_s": [round(x / 1e9, 2) for x in rates], "sweeps_per_window": reps,
                         "bytes_per_delivery": round(bytes_per, 1),
                         "gb_per_s": round(float(np.median(rates)) * bytes_per / 1e9, 1)}
            rec["kept_fraction"] = round(kept / tot, 4)
            rec["absent_fraction"] = round(none / tot, 4)
        rec["host_%d_threads_m_deliveries_per_s" % args.host_threads] = host_rate(t, host0, args.host_threads)
        emit(rec)
        t.close()
    out.close()


if __name__ == "__main__":
    main()
