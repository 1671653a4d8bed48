"""Rates of the batched select stage (emqx_amd/select.py) behind config B's match, for DESIGN.md
§3.10: device-resident match CSRs (config B's generator, EMQX_MODE_ROUTES on the device) against
owner tables of 1 K to 1 M owners with 1..3 filters each, drawn uniformly from the engine's filter
ids, three classes, every class applying to every message.  The timed calls are the asynchronous
form on one stream, rotated over >= 4 distinct batches, between device events around ~0.3 s of
calls (100 sweeps at most), three rounds.  The host path is emqx_select_host sharded by message
over 16 threads on the same inputs.  No target is set in advance; every line goes to the output file as measured.

  python tools/select_bench.py [--out profiles/select_sweep.jsonl] [--filters 1000000] [--topics 262144]
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

from emqx_amd import select as S  # noqa: E402
from emqx_amd import workloads as W  # noqa: E402

SIZES = (1_000, 10_000, 100_000, 1_000_000)


def host_rate(t, off, ids, threads):
    """Entries/s of emqx_select_host over one batch, sharded by message."""
    n = len(off) - 1
    cuts = np.searchsorted(off, np.linspace(0, int(off[-1]), threads + 1)).clip(0, n)
    cuts[0], cuts[-1] = 0, n
    shards = []
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if b > a:
            shards.append((np.ascontiguousarray(off[a:b + 1] - off[a]), ids[int(off[a]):int(off[b])].copy()))
    times = []
    for _ in range(3):
        ths = [threading.Thread(target=lambda s=s: t.select_host(*s)) for s in shards]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        times.append(time.perf_counter() - t0)
    return int(off[-1]) / min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_sweep.jsonl"))
    ap.add_argument("--filters", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=1 << 18, help="messages in all (split over --batches)")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    args = ap.parse_args()
    import torch
    from emqx_amd.engine import Engine
    assert torch.cuda.is_available(), "select_bench needs a HIP device"
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
    wl = W.config_b(n_filters=args.filters, n_topics=args.topics)
    eng = Engine(0)
    fids = eng.insert_packed(*wl.filters)
    eng.commit()
    tb, to = wl.topics
    per = args.topics // args.batches
    batches, host0 = [], None
    for k in range(args.batches):
        lo, hi = k * per, (k + 1) * per
        o = to[lo:hi + 1].astype(np.uint64)
        d_tb = torch.from_numpy(np.array(tb[int(o[0]):int(o[-1])])).to(dev)
        d_to = torch.from_numpy((o - o[0]).view(np.int64)).to(dev)
        mcap = 64 * per
        moff = torch.empty(per + 1, dtype=torch.int64, device=dev)
        mids = torch.empty(mcap, dtype=torch.int32, device=dev)
        total = eng.match_device(d_tb.data_ptr(), d_to.data_ptr(), per, moff.data_ptr(), mids.data_ptr(), mcap, mode=0)
        mids = mids[:max(total, 1)].clone()
        cap_out = 8 * max(total, 1) + per
        b = {"n": per, "total": total, "moff": moff, "mids": mids,
             "ooff": torch.zeros(per + 1, dtype=torch.int64, device=dev),
             "own": torch.zeros(cap_out, dtype=torch.int32, device=dev),
             "sum": torch.zeros(8, dtype=torch.int64, device=dev)}
        b["args"] = S.OwnerTable.batch(moff.data_ptr(), mids.data_ptr(), per, total, 0, b["ooff"].data_ptr(),
                                       b["own"].data_ptr(), cap_out)
        batches.append(b)
        if k == 0:
            host0 = (moff.cpu().numpy().view(np.uint64), mids[:total].cpu().numpy().view(np.uint32))
    entries = [b["total"] for b in batches]
    h_off = host0[0]
    per_msg = np.diff(h_off.astype(np.int64))
    emit({"record": "workload", "config": "B", "filters": int(wl.n_filters), "messages_per_batch": per,
          "batches": args.batches, "entries_per_batch": entries, "max_entries_per_message": int(per_msg.max()),
          "messages_without_entries": float(round((per_msg == 0).mean(), 4)), "setup_s": round(time.time() - t0, 1)})

    stream = torch.cuda.current_stream().cuda_stream
    for size in [int(x) for x in args.sizes.split(",")]:
        t = S.OwnerTable(0)
        r = np.random.default_rng(size)
        counts = r.integers(1, 4, size)
        picks = fids[r.integers(0, len(fids), int(counts.sum()))]
        at = 0
        for o in range(size):
            c = int(counts[o])
            t.set(o, o % 3, picks[at:at + c])
            at += c
        t.commit()
        s = t.stats()
        # check: the first 2000 messages of batch 0, device against host
        k = min(2000, per)
        sample = (host0[0][:k + 1], host0[1][:int(host0[0][k])])
        a, h = t.select_packed(*sample), t.select_host(*sample)
        assert a.rows() == h.rows() and a.summary == h.summary

        def sweep():
            for b in batches:
                t.select_device_async(b["args"], b["sum"].data_ptr(), stream=stream)
        sweep()
        torch.cuda.synchronize()
        summ = [b["sum"].cpu().numpy().view(np.uint64).tolist() for b in batches]
        assert all(x[0] == 0 and x[1] == b["total"] for x, b in zip(summ, batches)), summ
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
            rates.append(sum(entries) * reps / (e0.elapsed_time(e1) * 1e-3))
        tot, postings, selected, dups, unknown = (sum(x[i] for x in summ) for i in (1, 2, 3, 5, 6))
        # algorithmic bytes per entry, the look-back over the earlier entries of the message (re-reads of
        # lines the same wave has just touched) left out: the count pass and the write pass each read the
        # filter id (4), its two list offsets (8) and per posting the owner and its word (8); the count pass
        # writes and the write pass reads the entry's count (8); 4 per owner written
        bytes_per = 2 * (12 + 8 * postings / tot) + 8 + 4 * selected / tot
        rec = {"record": "sweep", "owners": s["n_owners"], "filters_held": s["n_filters"], "postings": s["n_postings"],
               "max_list": s["max_list"], "build_ms": round(s["last_build_ms"], 1),
               "m_entries_per_s": [round(x / 1e6, 1) for x in rates],
               "m_messages_per_s": [round(x / 1e6 * per * args.batches / sum(entries), 1) for x in rates],
               "sweeps_per_window": reps, "bytes_per_entry": round(bytes_per, 1),
               "gb_per_s": round(float(np.median(rates)) * bytes_per / 1e9, 2),
               "postings_per_entry": round(postings / tot, 4), "selected_per_entry": round(selected / tot, 4),
               "duplicates": dups, "unknown_fraction": round(unknown / tot, 4),
               "host_%d_threads_m_entries_per_s" % args.host_threads: round(host_rate(t, *host0, args.host_threads) / 1e6, 2)}
        emit(rec)
        t.close()
    out.close()


if __name__ == "__main__":
    main()
