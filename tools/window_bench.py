"""Rates of the window stage (emqx_amd/window.py) behind the inbox stage on workload E, for
DESIGN.md §3.12: the kept CSR of one batch of config E (as tools/inbox_bench.py builds it: match
and fan-out on the device, the enrich stage's compaction by its host evaluator; about 11.4 M
deliveries for 262 144 messages) grouped by the inbox stage over the same subscriber populations
of 1 K to 10 M ids plus the case in which one subscriber takes 10 % of all deliveries, then
admitted by the window stage under three session mixes: every session connected with
inflight_max 32; 20 % of the sessions disconnected with mq_max 1000; inflight_max 0 (never full).

The timed calls are the asynchronous form on one stream, rotated over `--batches` distinct grouped
inputs in buffers of their own (the same CSR with the ids rotated by a per-batch constant; 12 of
them and their outputs exceed the 256 MiB Infinity Cache from about 100 K inboxes on, below that
they fit it), between device events around ~0.3 s of calls, three rounds.  The inbox stage's own
time is taken the same way on the same input, next to it.
The host path is emqx_window_run_host on 16 threads, each over its own share of the inboxes with
a handle of its own.  Path 1, the one-wave-per-inbox yardstick, is timed beside path 0.  Copy 0 of
every row is checked byte for byte against the host evaluator on both paths.
No target is set in advance; every line goes to the output file as measured.

  python tools/window_bench.py [--out profiles/window_sweep.jsonl] [--topics 262144] [--batches 12]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from emqx_amd import deliver as D  # noqa: E402
from emqx_amd import inbox as IB  # noqa: E402
from emqx_amd import window as WN  # noqa: E402
from emqx_amd import workloads as W  # noqa: E402
from inbox_bench import POPULATIONS, SKEW_POPULATION, SKEW_SHARE, remap  # noqa: E402

MIXES = ("connected_32", "disconnected_20", "inflight_max_0")
INBOX_COPIES = 4


def sessions_of(mix: str, population: int) -> np.ndarray:
    t = WN.pack_sessions(population)  # connected, inflight_max 32, mq_max 1000
    if mix == "disconnected_20":
        t["flags"][np.random.default_rng(9).random(population) < 0.20] = WN.PRESENT
    if mix == "inflight_max_0":
        t["inflight_max"] = 0
    return t


def bytes_model(total: int, m: int) -> float:
    """Bytes a call moves: per delivery the opts byte read by both tile passes
    and 1 + 2 bytes written; per inbox its offset read by both passes and its id once (8 + 8 + 4),
    the head prefix written and read at both ends of the inbox (8 + 16), the record read and
    written (32 + 32) and the counts (16)."""
    return 5.0 * total + 124.0 * m


def host_rate(subs, off, opts, table, threads):
    """Deliveries/s of emqx_window_run_host over one batch sharded by inbox, a handle a thread."""
    m = len(subs)
    cuts = np.searchsorted(off, np.linspace(0, int(off[-1]), threads + 1)).clip(0, m)
    cuts[0], cuts[-1] = 0, m
    shards = []
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if b > a:
            lo, hi = int(off[a]), int(off[b])
            shards.append((WN.Window(WN.HOST_ONLY), subs[a:b].copy(), np.ascontiguousarray(off[a:b + 1] - off[a]),
                           opts[lo:hi].copy()))
    times = []
    for _ in range(3):
        ths = [threading.Thread(target=lambda s=s: s[0].run_host(s[1], s[2], s[3], table)) for s in shards]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        times.append(time.perf_counter() - t0)
    return int(off[-1]) / min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_sweep.jsonl"))
    ap.add_argument("--topics", type=int, default=1 << 18, help="messages of the batch")
    ap.add_argument("--batches", type=int, default=12, help="rotated grouped inputs of the window stage")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--entries", type=int, default=100_000, help="entries of the delivery-options table in front")
    ap.add_argument("--populations", default=",".join(map(str, POPULATIONS)))
    args = ap.parse_args()
    import torch
    from emqx_amd.engine import Engine
    from emqx_amd.fanout import SubTable
    assert torch.cuda.is_available(), "window_bench needs a HIP device"
    assert args.batches >= INBOX_COPIES
    torch.cuda.set_device(0)
    dev = "cuda:0"
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    # ---- one batch of config E through match, fan-out and the enrich stage's compaction (as
    # tools/inbox_bench.py) --------------------------------------------------------------------
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
    size = (h_off[1:] - h_off[:-1]).astype(np.int64)
    pick = h_off[:-1].astype(np.int64) + (rng.random(n) * size).astype(np.int64)
    one = h_subs[np.minimum(pick, max(total - 1, 0))]
    frm = np.where((rng.random(n) < 0.5) & (size > 0), one, np.uint32(D.NO_SENDER)).astype(np.uint32)
    kept = opt.enrich_host(h_off, h_subs, h_fils, qos, flags, frm, compact=True).kept
    opt.close()
    kept_total = int(kept.offsets[-1])
    live = np.bincount(np.where(kept.opts & 0x50, 3, np.minimum(kept.opts & 3, 1)), minlength=4)
    emit({"record": "workload", "config": "E", "filters": int(fw.wl.n_filters), "subscriptions": int(fw.n_subscriptions),
          "subscribers": n_subscribers, "messages": n, "deliveries": total, "kept_deliveries": kept_total,
          "qos0_deliveries": int(live[0]), "qos12_deliveries": int(live[1]), "grouped_inputs": args.batches, "tile": WN.TILE,
          "setup_s": round(time.time() - t0, 1)})

    def up(a, view):
        return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(dev)

    z = lambda size, dt: torch.zeros(size, dtype=dt, device=dev)  # noqa: E731
    mt = max(kept_total, 1)
    d_off = up(kept.offsets, np.int64)
    d_fils, d_opts = up(kept.filters, np.int32), up(kept.opts, np.uint8)
    in_subs = [torch.empty(mt, dtype=torch.int32, device=dev) for _ in range(INBOX_COPIES)]
    x_msgs, x_fils = z(mt, torch.int32), z(mt, torch.int32)
    grouped = [{"opts": z(mt, torch.uint8)} for _ in range(args.batches)]
    w_ver, w_ids = z(mt, torch.uint8), z(mt, torch.int16)
    i_sum, w_sum = z(8, torch.int64), z(8, torch.int64)
    ts = torch.cuda.Stream(device=dev)
    stream = ts.cuda_stream
    box, win = IB.Inbox(0), WN.Window(0)

    def timed(sweep, calls):
        """Median ms per call of `sweep` (which enqueues `calls` calls) over ~0.3 s windows."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts)
        sweep()
        e1.record(ts)
        e1.synchronize()
        reps = int(min(200, max(1, 300.0 / max(e0.elapsed_time(e1), 1e-3))))
        ms = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(reps):
                sweep()
            e1.record(ts)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / (reps * calls))
        return ms, reps

    cases = [(int(p), False) for p in args.populations.split(",")] + [(SKEW_POPULATION, True)]
    for population, skew in cases:
        torch.cuda.synchronize()
        cap_boxes = min(kept_total, population)
        box.reserve(kept_total, population)
        win.reserve(kept_total, cap_boxes)
        host_in = None
        # ---- the inbox stage groups every rotated copy into buffers of its own ------------------
        for c, g in enumerate(grouped):
            s = remap(kept.subs, kept.filters, population, n_subscribers, 7919 * c)
            if skew:  # one subscriber takes a tenth of all deliveries, wherever they are
                s[np.random.default_rng(100 + c).random(kept_total) < SKEW_SHARE] = population // 2
            src = in_subs[c % INBOX_COPIES]
            src.copy_(up(s, np.int32))
            g["subs"], g["off"] = z(max(cap_boxes, 1), torch.int32), z(cap_boxes + 1, torch.int64)
            g["iargs"] = IB.Inbox.batch(d_off.data_ptr(), src.data_ptr(), d_fils.data_ptr(), n, kept_total, population,
                                        x_msgs.data_ptr(), x_fils.data_ptr(), g["subs"].data_ptr(), g["off"].data_ptr(),
                                        cap_boxes, d_opts=d_opts.data_ptr(), d_box_opts=g["opts"].data_ptr())
            box.group_device_async(g["iargs"], i_sum.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            words = i_sum.cpu().numpy().view(np.uint64).tolist()
            assert words[0] == 0 and words[1] == kept_total, words
            g["m"] = int(words[2])
            g["recs"], g["cnt"] = z(4 * max(g["m"], 1), torch.int64), z(4 * max(g["m"], 1), torch.int32)
            if c == 0:
                host_in = (g["subs"][:g["m"]].cpu().numpy().view(np.uint32), g["off"][:g["m"] + 1].cpu().numpy().view(np.uint64),
                           g["opts"][:kept_total].cpu().numpy(), words[3])
        # the inbox stage's time on this input (its own passes, the rotated inputs it was given last)
        inbox_ms, _ = timed(lambda: [box.group_device_async(g["iargs"], i_sum.data_ptr(), stream=stream)
                                     for g in grouped[-INBOX_COPIES:]], INBOX_COPIES)
        for mix in MIXES:
            table = sessions_of(mix, population)
            d_table = torch.from_numpy(np.frombuffer(table.tobytes(), dtype=np.int64).copy()).to(dev)
            for g in grouped:
                g["wargs"] = WN.Window.batch(g["subs"].data_ptr(), g["off"].data_ptr(), g["opts"].data_ptr(), g["m"],
                                             kept_total, cap_boxes, d_table.data_ptr(), population, w_ver.data_ptr(),
                                             w_ids.data_ptr(), g["recs"].data_ptr(), g["cnt"].data_ptr())
            # check: copy 0 against the host evaluator over the whole batch
            g = grouped[0]
            ref = WN.Window(WN.HOST_ONLY).run_host(host_in[0], host_in[1], host_in[2], table)
            timings = {}
            for path in (0, 1):  # the tile scan, then the one-wave-per-inbox yardstick
                win.set_tuning("path", path)
                for t in (w_ver, w_ids, g["recs"], g["cnt"]):
                    t.zero_()
                torch.cuda.synchronize()
                win.run_device_async(g["wargs"], w_sum.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                words = dict(zip(WN.SUMMARY, w_sum.cpu().numpy().view(np.uint64).tolist()))
                assert words == ref.summary, (path, words, ref.summary)
                for got, want in ((w_ver, ref.verdicts), (w_ids, ref.pkt_ids), (g["recs"][:4 * g["m"]], ref.out_sessions),
                                  (g["cnt"][:4 * g["m"]], ref.counts)):
                    assert got.cpu().numpy().tobytes() == want.tobytes(), (population, skew, mix, path)
                timings[path] = timed(lambda: [win.run_device_async(g["wargs"], w_sum.data_ptr(), stream=stream)
                                               for g in grouped], len(grouped))
            win.set_tuning("path", 0)
            ms, reps = timings[0]
            med = float(np.median(ms))
            moved = bytes_model(kept_total, g["m"])
            rec = {"record": "sweep", "population": population, "skewed": skew, "mix": mix, "inboxes": g["m"],
                   "longest": host_in[3], "summary": {k: words[k] for k in WN.SUMMARY[3:]},
                   "window": {"g_deliveries_per_s": [round(kept_total / (x * 1e-3) / 1e9, 2) for x in ms],
                              "sweeps_per_window": reps, "ms_per_call": round(med, 4)},
                   "path1_wave_per_inbox": {"ms_per_call": [round(x, 4) for x in timings[1][0]],
                                            "sweeps_per_window": timings[1][1]},
                   "inbox_stage_ms_per_call": round(float(np.median(inbox_ms)), 3),
                   "window_over_inbox": round(med / float(np.median(inbox_ms)), 4),
                   "model": {"bytes_per_call": int(moved), "gb_per_s": round(moved / (med * 1e-3) / 1e9, 1)},
                   "host_%d_threads_m_deliveries_per_s" % args.host_threads: round(
                       host_rate(host_in[0], host_in[1], host_in[2], table, args.host_threads) / 1e6, 2)}
            emit(rec)
            torch.cuda.synchronize()
            del d_table
        for g in grouped:
            for key in ("subs", "off", "recs", "cnt"):
                g.pop(key, None)
    out.close()


if __name__ == "__main__":
    main()
