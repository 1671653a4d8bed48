"""Rates of the inbox stage (emqx_amd/inbox.py) behind workload E's fan-out, for DESIGN.md §3.11:
the device-resident kept CSR of one batch of config E (match and fan-out on the device, the enrich
stage's compaction by its host evaluator; about 11.4 M deliveries for 262 144 messages) grouped by subscriber over populations
of 1 K to 10 M ids, plus one skewed case in which a single subscriber takes 10 % of all
deliveries.  Config E has 1 M subscribers; a population P maps subscriber s of a delivery through
filter f to (s + 1 M * (f mod ceil(P / 1 M))) mod P: E's own distribution folded onto fewer ids,
or split by filter onto more.  The timed calls are the asynchronous form on one stream, rotated
over >= 4 distinct input batches (the same CSR with the ids rotated by a per-batch constant, in
buffers of their own) so that no input is served from the Infinity Cache, between device events on
that stream around ~0.3 s of calls, three rounds, for path 0 (the stage's own passes) and path 1 (the library
sort and a gather).  The host path is emqx_inbox_group_host on 16 threads, each grouping its own
shard of the messages with a handle of its own (16 concurrent per-call users, not one merged
result).  No target is set in advance; every line goes to the output file as measured.

  python tools/inbox_bench.py [--out profiles/inbox_sweep.jsonl] [--topics 262144] [--batches 4]
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
from emqx_amd import inbox as IB  # noqa: E402
from emqx_amd import workloads as W  # noqa: E402

POPULATIONS = (1_000, 10_000, 100_000, 1_000_000, 10_000_000)
SKEW_POPULATION, SKEW_SHARE = 1_000_000, 0.10
HBM_PEAK = 8.0e12  # bytes/s, the datasheet figure


def bytes_per_delivery(passes: int, boxes_per_delivery: float) -> float:
    """The byte model of path 0.  A pass reads the key for its histogram (4),
    reads key and position for the scatter and writes them (16; the first pass reads no position,
    the last writes none: 8 less in all); the first pass writes the message index (4); the last
    pass reads message index, filter, opts byte and subid of the source (13) and writes the five
    box_* payloads (17); the boundary step reads the sorted keys twice (8) and writes start, id
    and offset of each inbox and reads the start back (20 an inbox)."""
    return 20 * passes - 8 + 4 + 13 + 17 + 8 + 20 * boxes_per_delivery


def remap(subs, fils, population, n_subscribers, salt):
    split = -(-population // n_subscribers)
    f = (fils & np.uint32(0x3FFFFFFF)).astype(np.uint64)
    return ((subs.astype(np.uint64) + np.uint64(n_subscribers) * (f % np.uint64(split)) + np.uint64(salt))
            % np.uint64(population)).astype(np.uint32)


def host_rate(kept, subs, population, threads):
    """Deliveries/s of emqx_inbox_group_host over one batch sharded by message, a handle a thread."""
    off = kept.offsets
    n = len(off) - 1
    cuts = np.searchsorted(off, np.linspace(0, int(off[-1]), threads + 1)).clip(0, n)
    cuts[0], cuts[-1] = 0, n
    shards = []
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if b > a:
            lo, hi = int(off[a]), int(off[b])
            shards.append((IB.Inbox(IB.HOST_ONLY), np.ascontiguousarray(off[a:b + 1] - off[a]), subs[lo:hi].copy(),
                           kept.filters[lo:hi].copy(), kept.opts[lo:hi].copy(), kept.subids[lo:hi].copy()))
    times = []
    for _ in range(3):
        ths = [threading.Thread(target=lambda s=s: s[0].group_host(s[1], s[2], s[3], population, opts=s[4], subids=s[5]))
               for s in shards]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        times.append(time.perf_counter() - t0)
    return int(off[-1]) / min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbox_sweep.jsonl"))
    ap.add_argument("--topics", type=int, default=1 << 18, help="messages of the batch")
    ap.add_argument("--batches", type=int, default=4, help="rotated input copies")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--entries", type=int, default=100_000, help="entries of the delivery-options table in front")
    ap.add_argument("--populations", default=",".join(map(str, POPULATIONS)))
    args = ap.parse_args()
    import torch
    from emqx_amd.engine import Engine
    from emqx_amd.fanout import SubTable
    assert torch.cuda.is_available(), "inbox_bench needs a HIP device"
    assert args.batches >= 4
    torch.cuda.set_device(0)
    dev = "cuda:0"
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    # ---- one batch of config E through match, fan-out and the enrich stage's compaction --
    t0 = time.time()
    n = args.topics
    fw = W.config_e(n_topics=n)
    n_subscribers = int(fw.sub_id.max()) + 1
    eng = Engine(0)
    eng.insert_packed(*fw.wl.filters)
    eng.commit()
    st = SubTable(0)
    st.add(fw.sub_filter, fw.sub_id, fw.sub_group)
    st.commit()
    tb, to = fw.wl.topics
    o = to[:n + 1].astype(np.uint64)
    d_tb = torch.from_numpy(np.array(tb[int(o[0]):int(o[-1])])).to(dev)
    d_to = torch.from_numpy((o - o[0]).view(np.int64)).to(dev)
    mcap, cap = 64 * n, 256 * n
    moff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    mids = torch.empty(mcap, dtype=torch.int32, device=dev)
    eng.match_device(d_tb.data_ptr(), d_to.data_ptr(), n, moff.data_ptr(), mids.data_ptr(), mcap)
    keys = torch.from_numpy(np.array(fw.keys[:n]).view(np.int32)).to(dev)
    doff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    subs = torch.empty(cap, dtype=torch.int32, device=dev)
    fils = torch.empty(cap, dtype=torch.int32, device=dev)
    total = st.fanout_device("hash_clientid", moff.data_ptr(), mids.data_ptr(), n, keys.data_ptr(), doff.data_ptr(),
                             subs.data_ptr(), fils.data_ptr(), cap)
    h_off = doff.cpu().numpy().view(np.uint64)
    h_subs, h_fils = subs[:total].cpu().numpy().view(np.uint32), fils[:total].cpu().numpy().view(np.uint32)
    del mids, moff, subs, fils, d_tb, d_to
    torch.cuda.empty_cache()
    rng = np.random.default_rng(3)
    idx = np.random.default_rng(4).permutation(len(fw.sub_id))[:args.entries]
    k = len(idx)
    opt = D.SubOpts(D.HOST_ONLY)
    opt.set(fw.sub_filter[idx], fw.sub_id[idx], qos=rng.integers(0, 3, k), nl=rng.random(k) < 0.75, rap=rng.integers(0, 2, k),
            subid=np.where(rng.random(k) < 0.5, rng.integers(1, 1 << 28, k), 0))
    opt.commit()
    qos, flags = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 4, n).astype(np.uint8)
    # the publisher is one of the message's recipients for half of the messages that have one
    size = (h_off[1:] - h_off[:-1]).astype(np.int64)
    pick = h_off[:-1].astype(np.int64) + (rng.random(n) * size).astype(np.int64)
    one = h_subs[np.minimum(pick, max(total - 1, 0))]
    frm = np.where((rng.random(n) < 0.5) & (size > 0), one, np.uint32(D.NO_SENDER)).astype(np.uint32)
    kept = opt.enrich_host(h_off, h_subs, h_fils, qos, flags, frm, compact=True).kept
    opt.close()
    kept_total = int(kept.offsets[-1])
    emit({"record": "workload", "config": "E", "filters": int(fw.wl.n_filters), "subscriptions": int(fw.n_subscriptions),
          "subscribers": n_subscribers, "messages": n, "deliveries": total, "kept_deliveries": kept_total,
          "input_copies": args.batches, "tile": IB.TILE, "setup_s": round(time.time() - t0, 1)})

    def up(a, view):
        return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(dev)

    d_off = up(kept.offsets, np.int64)
    copies = [{"fils": up(kept.filters, np.int32), "opts": up(kept.opts, np.uint8), "ids": up(kept.subids, np.int32),
               "subs": torch.empty(kept_total, dtype=torch.int32, device=dev)} for _ in range(args.batches)]
    m = max(kept_total, 1)
    z = lambda size, dt: torch.zeros(size, dtype=dt, device=dev)  # noqa: E731
    x_msgs, x_fils, x_opts, x_ids, x_src = z(m, torch.int32), z(m, torch.int32), z(m, torch.uint8), z(m, torch.int32), z(m, torch.int32)
    d_sum = z(8, torch.int64)
    # a stream of the tool's own, not the null stream: the stage maps a null stream to its handle's
    # stream, and events recorded on the null stream would not follow the calls
    ts = torch.cuda.Stream(device=dev)
    stream = ts.cuda_stream
    box = IB.Inbox(0)
    cases = [(int(p), False) for p in args.populations.split(",")] + [(SKEW_POPULATION, True)]
    for population, skew in cases:
        torch.cuda.synchronize()  # nothing of the case before is in flight when its buffers go
        cap_boxes = min(kept_total, population)
        x_subs, x_off = z(max(cap_boxes, 1), torch.int32), z(cap_boxes + 1, torch.int64)
        host_subs = None
        for c, b in enumerate(copies):
            s = remap(kept.subs, kept.filters, population, n_subscribers, 7919 * c)
            if skew:  # one subscriber takes a tenth of all deliveries, wherever they are
                s[np.random.default_rng(100 + c).random(kept_total) < SKEW_SHARE] = population // 2
            if c == 0:
                host_subs = s
            b["subs"].copy_(up(s, np.int32))
            b["args"] = IB.Inbox.batch(d_off.data_ptr(), b["subs"].data_ptr(), b["fils"].data_ptr(), n, kept_total, population,
                                       x_msgs.data_ptr(), x_fils.data_ptr(), x_subs.data_ptr(), x_off.data_ptr(), cap_boxes,
                                       d_opts=b["opts"].data_ptr(), d_subids=b["ids"].data_ptr(), d_box_opts=x_opts.data_ptr(),
                                       d_box_subids=x_ids.data_ptr(), d_box_src=x_src.data_ptr())
        box.reserve(kept_total, population)
        passes = IB.passes(population)
        rec = {"record": "sweep", "population": population, "skewed": skew, "passes": passes}
        # check: copy 0 on both paths against the host evaluator over the whole batch
        ref = IB.Inbox(IB.HOST_ONLY).group_host(kept.offsets, host_subs, kept.filters, population, opts=kept.opts,
                                                subids=kept.subids)
        for path in (0, 1):
            box.set_tuning("path", path)
            torch.cuda.synchronize()
            box.group_device_async(copies[0]["args"], d_sum.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            words = d_sum.cpu().numpy().view(np.uint64).tolist()
            assert dict(zip(IB.SUMMARY, words)) == ref.summary, (path, words, ref.summary)
            mb = words[2]
            for got, want in ((x_subs[:mb], ref.inbox_subs), (x_off[:mb + 1], ref.inbox_offsets), (x_msgs, ref.msgs),
                              (x_fils, ref.filters), (x_opts, ref.opts), (x_ids, ref.subids), (x_src, ref.src)):
                assert got.cpu().numpy().tobytes() == want.tobytes(), (population, skew, path)

            def sweep():
                for b in copies:
                    box.group_device_async(b["args"], d_sum.data_ptr(), stream=stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            sweep()
            e1.record(ts)
            e1.synchronize()
            reps = int(min(100, max(1, 300.0 / max(e0.elapsed_time(e1), 1e-3))))
            rates = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts)
                for _ in range(reps):
                    sweep()
                e1.record(ts)
                e1.synchronize()
                rates.append(kept_total * len(copies) * reps / (e0.elapsed_time(e1) * 1e-3))
            rec["path%d" % path] = {"g_deliveries_per_s": [round(x / 1e9, 2) for x in rates], "sweeps_per_window": reps,
                                    "ms_per_call": round(kept_total / float(np.median(rates)) * 1e3, 3)}
        rec["inboxes"], rec["longest"] = ref.summary["inboxes"], ref.summary["longest"]
        bpd = bytes_per_delivery(passes, ref.summary["inboxes"] / max(kept_total, 1))
        r0 = float(np.median([x * 1e9 for x in rec["path0"]["g_deliveries_per_s"]]))
        rec["model"] = {"bytes_per_delivery": round(bpd, 1), "path0_gb_per_s": round(r0 * bpd / 1e9, 1),
                        "path0_fraction_of_hbm_peak": round(r0 * bpd / HBM_PEAK, 4), "hbm_peak_tb_per_s": HBM_PEAK / 1e12}
        rec["host_%d_threads_m_deliveries_per_s" % args.host_threads] = round(
            host_rate(kept, host_subs, population, args.host_threads) / 1e6, 2)
        emit(rec)
        torch.cuda.synchronize()
        del x_subs, x_off
    out.close()


if __name__ == "__main__":
    main()
