"""Rates of the mqueue stage (emqx_amd/mqueue.py) for DESIGN.md §3.16.

Populations of 1 K to 10 M connected sessions with a window of 4 that is full, a queue limit of 8 and
`backlog` QoS 1 messages queued each (0 to 8), rings of Q = 64 entries for every population and of
Q = 1024 up to 1 M sessions (an 8 GiB ring; 10 M sessions of 1024 entries would be 80 GiB and are
not measured).  Two chains are timed call by call, each call between two events on one stream:

  put chain   window (2 deliveries a session, all queued since the window is full) -> PUT.  With the
              backlog at the limit every delivery evicts an old entry.  `skew`: one inbox holds 10 %
              of all deliveries, the rest are spread evenly; the same total.
  take chain  ack run (2 PUBACKs a session, update_table) -> stamp -> TAKE (pops min(2, backlog)) ->
              ack record fed with the take's outputs -> stamp.  `skew`: the same number of queued
              entries held by an eighth of the sessions, eight times as many each.

Every timed chain starts from the same state: the records, headers, slots and stamps of an instance
are restored from pristine copies before it, outside the events.  The tables of a population exist in
`copies` instances that the calls rotate over.  A window is ~0.25 s of calls and the median of three
windows is reported.  The yardsticks are the window call and the ack run call of these very chains,
measured in the same process on the same population.  Up to 100 K sessions the first chain on
instance 0 is checked byte for byte against emqx_mqueue_put_host and emqx_mqueue_take_host.  The
host path is the two host calls on 16 threads, each over its own share of the sessions with a handle
of its own, at 1 M sessions and Q = 64.  No target is set in advance; every line goes to the output
file as measured.

  python tools/mqueue_bench.py [--out profiles/mqueue_sweep.jsonl] [--populations 1000,...]
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
from emqx_amd import mqueue as MQ  # noqa: E402
from emqx_amd import retry as RT  # noqa: E402
from emqx_amd import window as WN  # noqa: E402

POPULATIONS = (1_000, 10_000, 100_000, 1_000_000, 10_000_000)
BACKLOGS = (0, 1, 2, 4, 8)
W, WINDOW, MQ_MAX, PER_BOX, ACKS = 8, 4, 8, 2, 2
NOW = 1_700_000_000_000
REF_LIMIT = 1 << 22


def put_bytes_model(total: int, boxes: int, stored: int, evicting: int) -> float:
    """Bytes a put call moves: per delivery the verdict read by three passes and
    the evicted entry written (3 + 8); per stored delivery its opts byte read and the entry written
    (1 + 8); per evicting delivery the header and the old entry read (8 + 8); per inbox the id, two
    offsets and the head prefix by three passes, the header read and written, the plan written and
    read, the record's mq_len and out_unstored (3 * 28 + 16 + 16 + 4 + 4)."""
    return 11.0 * total + 9.0 * stored + 16.0 * evicting + 124.0 * boxes


def take_bytes_model(sessions: int, scanned: int, items: int, ids_given: bool) -> float:
    """Bytes a take call moves: per session the record and the header read by two passes, the count
    written and read, offset, status and counts written, the record and the header written
    (2 * 40 + 16 + 25 + 40), 4 more where the ids are listed; per entry scanned the entry and its
    deadline by two passes (2 * 16); per item opts, verdict, id and ref written (8)."""
    return (161.0 + (4 if ids_given else 0)) * sessions + 32.0 * scanned + 8.0 * items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mqueue_sweep.jsonl"))
    ap.add_argument("--populations", default=",".join(map(str, POPULATIONS)))
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--rotate-bytes", type=int, default=1 << 30, help="the instances of a population hold at least this much")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "mqueue_bench needs a HIP device"
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
    emit({"record": "setup", "w": W, "window": WINDOW, "mq_max": MQ_MAX, "deliveries_per_inbox": PER_BOX, "acks_per_session": ACKS,
          "device": torch.cuda.get_device_name(0)})

    def timed(chain, n_inst, n_marks):
        """ms per call of every step: `chain(i)` enqueues one chain on instance i and returns its
        events (n_marks + 1 of them)."""
        probe = [chain(i) for i in range(n_inst)]
        torch.cuda.synchronize()
        one = sum(m[0].elapsed_time(m[-1]) for m in probe) / len(probe)
        reps = int(min(100, max(1, args.window_ms / max(one * n_inst, 1e-3))))
        per_round = []
        for _ in range(args.rounds):
            marks = [chain(i) for _ in range(reps) for i in range(n_inst)]
            torch.cuda.synchronize()
            per_round.append([float(np.mean([m[k].elapsed_time(m[k + 1]) for m in marks])) for k in range(n_marks)])
        return [round(float(x), 4) for x in np.median(np.array(per_round), axis=0)], reps

    for population in [int(p) for p in args.populations.split(",")]:
        for q in (64, 1024):
            if q == 1024 and population > 1_000_000:
                continue
            backlogs = BACKLOGS if q == 64 else (0, 8)
            P = population
            rng = np.random.default_rng(P + q)
            ring_bytes = 8 * P * q
            per = ring_bytes + (32 + 8 + 16 * W) * P
            copies = int(min(12, max(2, -(-args.rotate_bytes // per)))) if ring_bytes < (4 << 30) else 2
            win, ack, rt, mq = WN.Window(0), AK.Ack(0), RT.Retry(0), MQ.Mqueue(0)
            total = PER_BOX * P
            win.reserve(total, P)
            ack.reserve(max(total, ACKS * P), P, W)
            rt.reserve(P, W)
            mq.reserve(total, P)
            subs = up(np.arange(P, dtype=np.uint32), np.int32)
            # slots: four messages inflight a session, ids 1..4; the acks: PUBACK of ids 1 and 2
            slots0 = AK.empty_slots(P, W)
            for j in range(WINDOW):
                slots0["pkt_id"][:, j], slots0["phase"][:, j], slots0["qos"][:, j], slots0["ref"][:, j] = j + 1, AK.MSG, 1, j
            d_slots0 = up(slots0)
            d_stamps0 = z(P * W, torch.int64)
            acks = up(np.tile(AK.pack_acks([AK.PUBACK] * ACKS, list(range(1, ACKS + 1))), P), np.int32)
            a_off = up(np.arange(P + 1, dtype=np.uint64) * ACKS)
            ref_limit = max(REF_LIMIT, total)  # (a put without refs[] names a delivery by its position)
            d_dead = torch.full((ref_limit,), -1, dtype=torch.int64, device=dev)  # EMQX_RETRY_NO_EXPIRY
            opts = torch.ones(total, dtype=torch.uint8, device=dev)
            offs = {False: np.arange(P + 1, dtype=np.uint64) * PER_BOX}
            big = total // 10
            rest = np.diff(np.linspace(0, total - big, P).astype(np.int64))  # P - 1 inboxes share the others
            offs[True] = np.concatenate([[0, big], big + np.cumsum(rest)]).astype(np.uint64)
            assert offs[True][-1] == total and offs[True].size == P + 1
            d_offs = {k: up(v) for k, v in offs.items()}
            inst = []
            for c in range(copies):
                g = {"ring": torch.empty(P * q * 2, dtype=torch.int32, device=dev)}
                pair = g["ring"].view(P * q, 2)
                pair[:, 0] = torch.arange(P * q, dtype=torch.int32, device=dev) % REF_LIMIT
                pair[:, 1] = 1  # QoS 1
                g.update(table=z(4 * P, torch.int64), heads=z(P, torch.int64), slots=d_slots0.clone(), stamps=d_stamps0.clone(),
                         ver=z(total, torch.uint8), ids=z(total, torch.int16), recs=z(4 * P, torch.int64), wcnt=z(4 * P, torch.int32),
                         ev=z(total, torch.int64), unst=z(P, torch.int32), aver=z(ACKS * P, torch.uint8), arefs=z(ACKS * P, torch.int32),
                         acnt=z(4 * P, torch.int32), t_off=z(P + 1, torch.int64), t_opts=z(total, torch.uint8), t_ver=z(total, torch.uint8),
                         t_ids=z(total, torch.int16), t_refs=z(total, torch.int32), t_status=z(P, torch.uint8), t_cnt=z(4 * P, torch.int32),
                         unrec=z(P, torch.int32), sums=[z(8, torch.int64) for _ in range(7)])
                inst.append(g)
            head0 = rng.integers(0, q, P).astype(np.uint32)

            for backlog in backlogs:
                for skew in (False, True):
                    if skew and backlog not in (2, 8):
                        continue
                    try:
                        # ---- the state every chain starts from ---------------------------------
                        lens = np.full(P, backlog, dtype=np.uint32)
                        if skew:  # (the take chain's skew: an eighth of the sessions hold all of it)
                            lens = np.where(np.arange(P) % 8 == 0, min(8 * backlog, q), 0).astype(np.uint32)
                        put_lens = np.full(P, backlog, dtype=np.uint32)  # (the put chain's skew is in the inboxes)
                        table_put = WN.pack_sessions(P, inflight=WINDOW, inflight_max=WINDOW, mq_len=put_lens, mq_max=MQ_MAX)
                        table_take = WN.pack_sessions(P, inflight=WINDOW, inflight_max=WINDOW, mq_len=lens, mq_max=q)
                        heads_put = np.zeros(P, dtype=MQ.RING)
                        heads_put["head"], heads_put["len"] = head0, put_lens
                        heads_take = heads_put.copy()
                        heads_take["len"] = lens
                        st = {"tp": up(table_put), "tt": up(table_take), "hp": up(heads_put), "ht": up(heads_take)}
                        for g in inst:
                            P_ = lambda k, g=g: g[k].data_ptr()  # noqa: E731
                            sm = [t.data_ptr() for t in g["sums"]]
                            g["w"] = WN.Window.batch(subs.data_ptr(), d_offs[skew].data_ptr(), opts.data_ptr(), P, total, P, P_("table"), P,
                                                     P_("ver"), P_("ids"), P_("recs"), P_("wcnt"), update_table=True)
                            g["p"] = MQ.Mqueue.put_args(subs.data_ptr(), d_offs[skew].data_ptr(), opts.data_ptr(), P, total, P, P_("ver"),
                                                        P_("ring"), P_("heads"), q, P, P_("ev"), P_("unst"), d_sessions=P_("table"))
                            g["a"] = AK.Ack.run_args(subs.data_ptr(), a_off.data_ptr(), acks.data_ptr(), P, ACKS * P, P, P_("table"), P,
                                                     P_("slots"), W, P_("aver"), P_("arefs"), P_("acnt"), update_table=True)
                            g["s"] = RT.Retry.stamp_args(subs.data_ptr(), P, P, P_("slots"), P_("stamps"), W, P, NOW)
                            g["t"] = MQ.Mqueue.take_args(subs.data_ptr(), P, P, P_("table"), P, P_("ring"), P_("heads"), q, NOW, total,
                                                         P_("t_off"), P_("t_opts"), P_("t_ver"), P_("t_ids"), P_("t_refs"), P_("t_status"),
                                                         P_("t_cnt"), d_deadlines=d_dead.data_ptr(), ref_limit=ref_limit, update_table=True)
                            g["r"] = AK.Ack.record_args(subs.data_ptr(), P_("t_off"), P_("t_opts"), P, total, P, P_("t_ver"), P_("t_ids"),
                                                        P_("slots"), W, P, P_("unrec"), d_refs=P_("t_refs"))
                            g["sm"] = sm

                        def put_chain(i):
                            g = inst[i]
                            with torch.cuda.stream(ts):
                                g["table"].copy_(st["tp"])
                                g["heads"].copy_(st["hp"])
                                m = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                                m[0].record(ts)
                                win.run_device_async(g["w"], g["sm"][0], stream=stream)
                                m[1].record(ts)
                                mq.put_device_async(g["p"], g["sm"][1], stream=stream)
                                m[2].record(ts)
                            return m

                        def take_chain(i):
                            g = inst[i]
                            with torch.cuda.stream(ts):
                                g["table"].copy_(st["tt"])
                                g["heads"].copy_(st["ht"])
                                g["slots"].copy_(d_slots0)
                                g["stamps"].copy_(d_stamps0)
                                m = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                                m[0].record(ts)
                                ack.run_device_async(g["a"], g["sm"][2], stream=stream)
                                m[1].record(ts)
                                rt.stamp_device_async(g["s"], g["sm"][3], stream=stream)
                                m[2].record(ts)
                                mq.take_device_async(g["t"], g["sm"][4], stream=stream)
                                m[3].record(ts)
                                ack.record_device_async(g["r"], g["sm"][5], stream=stream)
                                m[4].record(ts)
                                rt.stamp_device_async(g["s"], g["sm"][6], stream=stream)
                                m[5].record(ts)
                            return m

                        words = lambda t, names: dict(zip(names, t.cpu().numpy().view(np.uint64).tolist()))  # noqa: E731
                        g = inst[0]
                        # ---- the put chain ------------------------------------------------------
                        torch.cuda.synchronize()
                        ring_before = g["ring"].clone() if P <= 100_000 else None
                        put_chain(0)
                        torch.cuda.synchronize()
                        ps = words(g["sums"][1], MQ.PUT_SUMMARY)
                        assert ps["flags"] == 0 and ps["deliveries"] == total, ps
                        evicting = int((g["ver"][:total] >= 0x80).sum().item())
                        if ring_before is not None:
                            h_ring = np.frombuffer(ring_before.cpu().numpy().tobytes(), dtype=MQ.ENTRY).reshape(P, q).copy()
                            h_heads = heads_put.copy()
                            h_table = np.frombuffer(g["table"].cpu().numpy().tobytes(), dtype=WN.SESSION).copy()
                            ref = MQ.Mqueue(MQ.HOST_ONLY).put_host(np.arange(P), offs[skew], np.ones(total, np.uint8), g["ver"].cpu().numpy()[:total],
                                                                  h_ring, h_heads, sessions=h_table)
                            assert ref.summary == ps, (ref.summary, ps)
                            assert g["ring"].cpu().numpy().tobytes() == h_ring.tobytes() and g["heads"].cpu().numpy().tobytes() == h_heads.tobytes()
                            assert g["ev"][:total].cpu().numpy().tobytes() == ref.evicted.tobytes()
                            assert g["unst"][:P].cpu().numpy().tobytes() == ref.unstored.tobytes()
                        (win_ms, put_ms), reps = timed(put_chain, copies, 2)
                        moved = put_bytes_model(total, P, ps["stored"], evicting)
                        emit({"record": "put", "population": P, "q": q, "backlog": backlog, "skew": skew, "deliveries": total,
                              "largest_inbox": int(np.diff(offs[skew]).max()), "instances": copies, "chains_per_window": reps,
                              "checked_against_host": ring_before is not None,
                              "summary": {k: ps[k] for k in MQ.PUT_SUMMARY[3:]}, "evicting_deliveries": evicting,
                              "window_ms": win_ms, "put_ms": put_ms, "ratio_to_window": round(put_ms / win_ms, 3),
                              "m_deliveries_per_s": round(total / (put_ms * 1e-3) / 1e6, 1),
                              "model": {"bytes_per_call": int(moved), "gb_per_s": round(moved / (put_ms * 1e-3) / 1e9, 1)}})
                        # ---- the take chain -----------------------------------------------------
                        torch.cuda.synchronize()
                        ring_before = g["ring"].clone() if P <= 100_000 else None
                        take_chain(0)
                        torch.cuda.synchronize()
                        tk = words(g["sums"][4], MQ.TAKE_SUMMARY)
                        rc = words(g["sums"][5], AK.RECORD_SUMMARY)
                        want = int(np.minimum(lens, ACKS).sum())
                        assert tk["flags"] == 0 and tk["items"] == tk["sends"] == want and rc["recorded"] == want and rc["unrecorded"] == 0, (tk, rc)
                        if ring_before is not None:
                            h_ring = np.frombuffer(ring_before.cpu().numpy().tobytes(), dtype=MQ.ENTRY).reshape(P, q).copy()
                            h_heads, h_table = heads_take.copy(), table_take.copy()
                            h_table["inflight"] -= ACKS  # what the run call left
                            ref = MQ.Mqueue(MQ.HOST_ONLY).take_host(np.arange(P), h_table, h_ring, h_heads, NOW,
                                                                   deadlines=np.full(ref_limit, MQ.NO_EXPIRY, np.uint64), cap_out=total,
                                                                   update_table=True)
                            assert ref.summary == tk, (ref.summary, tk)
                            n = tk["items"]
                            for got, exp in ((g["t_off"][:P + 1], ref.offsets), (g["t_opts"][:n], ref.opts), (g["t_ver"][:n], ref.verdicts),
                                             (g["t_ids"][:n], ref.pkt_ids), (g["t_refs"][:n], ref.refs), (g["t_status"][:P], ref.status),
                                             (g["t_cnt"][:4 * P], ref.counts), (g["heads"][:P], h_heads), (g["table"][:4 * P], h_table)):
                                assert got.cpu().numpy().tobytes() == exp.tobytes(), (P, q, backlog, skew)
                        (run_ms, st1_ms, take_ms, rec_ms, st2_ms), reps = timed(take_chain, copies, 5)
                        moved = take_bytes_model(P, int(np.minimum(lens, 16).sum()), tk["items"], True)  # (a trip reads 16 entries)
                        emit({"record": "take", "population": P, "q": q, "backlog": backlog, "skew": skew, "queued_entries": int(lens.sum()),
                              "instances": copies, "chains_per_window": reps, "checked_against_host": ring_before is not None,
                              "summary": {k: tk[k] for k in MQ.TAKE_SUMMARY[3:]},
                              "ack_run_ms": run_ms, "stamp_ms": st1_ms, "take_ms": take_ms, "record_ms": rec_ms, "stamp2_ms": st2_ms,
                              "ratio_to_ack_run": round(take_ms / run_ms, 3),
                              "cycle_without_take_ms": round(run_ms + st1_ms, 4),
                              "cycle_with_take_ms": round(run_ms + st1_ms + take_ms + rec_ms + st2_ms, 4),
                              "m_sessions_per_s": round(P / (take_ms * 1e-3) / 1e6, 1),
                              "model": {"bytes_per_call": int(moved), "gb_per_s": round(moved / (take_ms * 1e-3) / 1e9, 1)},
                              "scratch_bytes": mq.stats()["scratch_bytes"]})
                        # ---- the host path ------------------------------------------------------
                        if P == 1_000_000 and q == 64 and backlog == 8 and not skew:
                            emit(host_rates(P, q, heads_put, table_put, heads_take, table_take, offs[False], total, args.host_threads))
                    except Exception as e:  # a line that could not be measured says so
                        emit({"record": "error", "population": P, "q": q, "backlog": backlog, "skew": skew, "error": repr(e)[:300]})
                        torch.cuda.synchronize()
            del inst, win, ack, rt, mq
            torch.cuda.empty_cache()
    out.close()


def host_rates(P, q, heads_put, table_put, heads_take, table_take, off, total, threads):
    """The two host calls over the table sharded by session, a handle a thread."""
    ring = np.zeros((P, q), dtype=MQ.ENTRY)
    ring["ref"] = (np.arange(P * q, dtype=np.uint64) % REF_LIMIT).reshape(P, q)
    ring["opts"] = 1
    ver = np.full(total, 0x83, dtype=np.uint8)  # the backlog is at the limit: every delivery evicts
    opts = np.ones(total, dtype=np.uint8)
    dead = np.full(REF_LIMIT, MQ.NO_EXPIRY, np.uint64)
    cuts = np.linspace(0, P, threads + 1).astype(np.int64)
    res = {}
    for name in ("put", "take"):
        times = []
        for _ in range(2):
            hp, ht, tt = heads_put.copy(), heads_take.copy(), table_take.copy()
            tt["inflight"] -= ACKS
            jobs = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                h = MQ.Mqueue(MQ.HOST_ONLY)
                ids = np.arange(a, b, dtype=np.uint32)
                if name == "put":
                    o = (off[a:b + 1] - off[a]).astype(np.uint64)
                    lo, hi = int(off[a]), int(off[b])
                    jobs.append(lambda h=h, ids=ids, o=o, lo=lo, hi=hi: h.put_host(ids, o, opts[lo:hi], ver[lo:hi], ring, hp))
                else:
                    jobs.append(lambda h=h, ids=ids: h.take_host(ids, tt, ring, ht, NOW, deadlines=dead, cap_out=ACKS * ids.size,
                                                                 update_table=True))
            ths = [threading.Thread(target=j) for j in jobs]
            t0 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            times.append(time.perf_counter() - t0)
        res[name + "_ms"] = round(min(times) * 1e3, 2)
    return {"record": "host", "population": P, "q": q, "backlog": 8, "threads": threads, **res,
            "put_m_deliveries_per_s": round(total / res["put_ms"] / 1e3, 1), "take_m_sessions_per_s": round(P / res["take_ms"] / 1e3, 1)}


if __name__ == "__main__":
    main()
