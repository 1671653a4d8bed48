"""Rates of the priority mqueue stage (emqx_amd/pmqueue.py) for DESIGN.md §3.18.

Populations of 1 K to 10 M connected sessions whose window is full, `C` priority classes (1, 4 and 8) of
rings of Qc = 16 entries, max_len 8, every class holding its max_len of QoS 1 messages (at 10 M sessions
C = 4 and 8 run last, on one instance each: their rings take 5 and 10 GiB).  Two calls are timed,
each between two events on one stream, `update_table` 0 so that every repetition does the same work on
the same state (the rings are written all the same; the heads and records are not):

  put   2 deliveries a session, all EMQX_W_QUEUED, classes drawn evenly: every delivery evicts.  `skew`:
        one inbox holds 10 % of all deliveries.
  take  every session has room for 2: two items a session.  `drain`: 100 K sessions of 8 classes of rings
        of Qc = 64, all full (512 entries a session), two items a session, against the same with session 0
        at a window of 0 (budget 1000), which drains its whole row: 512 dependent fold steps in one group.

THE YARDSTICK is the plain mqueue stage (emqx_amd/mqueue.py), re-measured in the same process on the
same population and batch: its put with rings of Q = 16 full at a limit of 8 and both deliveries
evicting, its take with two items a session.  The group width A/B runs at 1 M sessions and C = 4 on
the even mix, and at 4 and 64 lanes on the skewed put.  The
tables of a population exist in `copies` instances the calls rotate over; a window is ~0.2 s of calls and
the median of three windows is reported.  Up to 100 K sessions the first call on instance 0 is checked
byte for byte against emqx_pmqueue_put_host and emqx_pmqueue_take_host.  The host path is the two host
calls on 16 threads, each over its own share of the sessions with a handle of its own, at 1 M sessions
and C = 4.  No target is set in advance; every line goes to the output file as measured.

  python tools/pmqueue_bench.py [--out profiles/pmqueue_sweep.jsonl] [--populations 1000,...]
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

from emqx_amd import mqueue as MQ  # noqa: E402
from emqx_amd import pmqueue as PQ  # noqa: E402
from emqx_amd import window as WN  # noqa: E402

POPULATIONS = (1_000, 10_000, 100_000, 1_000_000, 10_000_000)
QC, MAX_LEN, PER_BOX = 16, 8, 2
PRIOS = [7, 6, 5, 4, 3, 2, 1, 0]


def put_bytes_model(total: int, boxes: int, evicting: int) -> float:
    """Bytes a put call moves: per delivery the verdict, the source index and the class byte read by three
    walks, the three outputs written, the opts byte and the entry stored (3 * 6 + 10 + 9); per evicting
    delivery the old entry read (8); per inbox the id, two offsets, the head and the record read and the
    counts written (4 + 16 + 64 + 32 + 32)."""
    return 37.0 * total + 8.0 * evicting + 148.0 * boxes


def take_bytes_model(sessions: int, live: int, items: int) -> float:
    """Bytes a take call moves: per session the id, the head and the record read by two passes, the offset
    written twice, status and counts (2 * 100 + 16 + 17); per live entry its 8 bytes read by two passes;
    per item the entry read again and 10 bytes written."""
    return 233.0 * sessions + 16.0 * live + 18.0 * items


def world(n: int, c: int, rng, qc=QC, max_len=MAX_LEN):
    tables = PQ.pack_tables([(PRIOS[:c], c - 1, max_len, 10, 0)])
    sessions = WN.pack_sessions(n, inflight=2, inflight_max=4, mq_len=c * max_len, mq_max=0)
    ring = PQ.empty_ring(n, c, qc)
    ring["ref"] = rng.integers(0, 1 << 20, size=ring.shape, dtype=np.uint32)
    ring["opts"] = 1
    heads = PQ.empty_heads(n, 0)
    heads["len"][:, :c] = max_len
    heads["head"][:, :c] = rng.integers(0, qc, size=(n, c))
    order = 0xFFFFFFFF
    for p in range(c):
        order = (order & ~(0xF << (4 * p))) | (p << (4 * p))
    heads["order"] = order
    return tables, sessions, ring, heads


def dev(a):
    import torch
    raw = np.frombuffer(a.tobytes(), dtype=np.uint8)
    return torch.from_numpy(raw.copy()).cuda()


def timed(fn, copies, budget=0.2):
    """Median of three windows of ~budget seconds; fn(i) enqueues one call on instance i % copies."""
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(0)
    torch.cuda.synchronize()
    reps = int(max(3, min(2000, budget / max(time.perf_counter() - t0, 1e-6))))
    out = []
    for _ in range(3):
        start.record()
        for i in range(reps):
            fn(i)
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end) / reps)
    return float(np.median(out)), reps


class Instance:
    """One population's tables and call buffers on the device."""

    def __init__(self, n, c, rng, skew=False, qc=QC, max_len=MAX_LEN, drain=False):
        import torch
        self.n, self.c = n, c
        self.host = world(n, c, rng, qc, max_len)
        tables, sessions, ring, heads = self.host
        if drain:
            sessions["inflight_max"][0] = 0  # batch_n/1 is 1000: the whole row
        sizes = np.full(n, PER_BOX, dtype=np.int64)
        if skew:
            total = int(sizes.sum())
            sizes[0] = total // 10
            sizes[1:] = np.bincount(np.arange(total - sizes[0]) % (n - 1), minlength=n - 1)
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        self.total = int(self.off[-1])
        self.subs = np.arange(n, dtype=np.uint32)
        self.opts = np.ones(self.total, np.uint8)
        self.ver = np.full(self.total, 3, np.uint8)
        self.src = np.arange(self.total, dtype=np.uint32)
        self.cls = rng.integers(0, c, size=(self.total, 1), dtype=np.uint8)
        self.d = {k: dev(v) for k, v in dict(tables=tables, sessions=sessions, ring=ring, heads=heads, off=self.off, subs=self.subs,
                                             opts=self.opts, ver=self.ver, src=self.src, cls=self.cls).items()}
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")  # noqa: E731
        cap = n * PER_BOX + (c * max_len if drain else 0)
        self.o = dict(ver=z(self.total, torch.uint8), cls=z(self.total, torch.uint8), ev=z(self.total, torch.int64), cnt=z(8 * n, torch.int32),
                      off=z(n + 1, torch.int64), t_opts=z(cap, torch.uint8), t_ver=z(cap, torch.uint8), t_cls=z(cap, torch.uint8),
                      t_ids=z(cap, torch.int16), t_refs=z(cap, torch.int32), status=z(n, torch.uint8), t_cnt=z(4 * n, torch.int32),
                      summary=z(8, torch.int64))
        self.cap_out = cap
        p = lambda t: t.data_ptr()  # noqa: E731
        self.put_args = PQ.Pmqueue.put_args(
            inbox_subs=p(self.d["subs"]), inbox_offsets=p(self.d["off"]), box_opts=p(self.d["opts"]), n_boxes=0, m=n, cap_in=self.total,
            cap_boxes=n, verdicts=p(self.d["ver"]), refs=0, box_src=p(self.d["src"]), msg_class=p(self.d["cls"]), n_msgs=self.total,
            tables=p(self.d["tables"]), n_tables=1, sessions=p(self.d["sessions"]), sub_limit=n, update_table=0, ring=p(self.d["ring"]),
            heads=p(self.d["heads"]), c=c, qc=qc, out_verdicts=p(self.o["ver"]), out_class=p(self.o["cls"]), out_evicted=p(self.o["ev"]),
            out_counts=p(self.o["cnt"]))
        self.take_args = PQ.Pmqueue.take_args(
            subs=0, n_boxes=0, m=n, cap_boxes=n, sessions=p(self.d["sessions"]), sub_limit=n, update_table=0, tables=p(self.d["tables"]),
            n_tables=1, ring=p(self.d["ring"]), heads=p(self.d["heads"]), c=c, qc=qc, now_ms=0, deadlines=0, ref_limit=0,
            cap_out=self.cap_out, out_offsets=p(self.o["off"]), out_opts=p(self.o["t_opts"]), out_verdicts=p(self.o["t_ver"]),
            out_pkt_ids=p(self.o["t_ids"]), out_refs=p(self.o["t_refs"]), out_class=p(self.o["t_cls"]), out_status=p(self.o["status"]),
            out_counts=p(self.o["t_cnt"]))


class Plain:
    """The plain mqueue stage on the same population and batch: Q = 16, full at its limit of 8."""

    def __init__(self, inst: Instance, rng):
        import torch
        n = inst.n
        sessions = WN.pack_sessions(n, inflight=2, inflight_max=4, mq_len=MAX_LEN, mq_max=MAX_LEN)
        ring = MQ.empty_ring(n, QC)
        ring["ref"] = rng.integers(0, 1 << 20, size=ring.shape, dtype=np.uint32)
        ring["opts"] = 1
        heads = MQ.empty_heads(n)
        heads["len"] = MAX_LEN
        heads["head"] = rng.integers(0, QC, size=n)
        ver = np.full(inst.total, 3 | 0x80, np.uint8)  # QUEUED | EVICTS: the window's verdicts at a full queue
        self.d = dict(sessions=dev(sessions), ring=dev(ring), heads=dev(heads), ver=dev(ver))
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")  # noqa: E731
        self.o = dict(ev=z(inst.total, torch.int64), un=z(n, torch.int32))
        p = lambda t: t.data_ptr()  # noqa: E731
        self.put_args = MQ.Mqueue.put_args(p(inst.d["subs"]), p(inst.d["off"]), p(inst.d["opts"]), n, inst.total, n, p(self.d["ver"]),
                                           p(self.d["ring"]), p(self.d["heads"]), QC, n, p(self.o["ev"]), p(self.o["un"]))
        self.take_args = MQ.Mqueue.take_args(0, n, n, p(self.d["sessions"]), n, p(self.d["ring"]), p(self.d["heads"]), QC, 0, inst.cap_out,
                                             p(inst.o["off"]), p(inst.o["t_opts"]), p(inst.o["t_ver"]), p(inst.o["t_ids"]),
                                             p(inst.o["t_refs"]), p(inst.o["status"]), p(inst.o["t_cnt"]))


def check_against_host(inst: Instance, h):
    """The first call of each kind on the instance, byte for byte against the host evaluator."""
    tables, sessions, ring, heads = inst.host
    hh = PQ.Pmqueue(PQ.HOST_ONLY)
    h.put_device(inst.put_args)
    r2, h2, s2 = ring.copy(), PQ.aligned_heads(heads), sessions.copy()
    want = hh.put_host(inst.subs, inst.off, inst.opts, inst.ver, inst.src, inst.cls, tables, s2, r2, h2, update_table=False)
    assert inst.o["ver"].cpu().numpy()[:inst.total].tobytes() == want.verdicts.tobytes()
    assert inst.o["ev"].cpu().numpy()[:inst.total].tobytes() == want.evicted.tobytes()
    assert inst.o["cnt"].cpu().numpy().tobytes() == want.counts.tobytes()
    assert inst.d["ring"].cpu().numpy().tobytes() == r2.tobytes()
    s = h.take_device(inst.take_args)
    t = hh.take_host(None, tables, s2, r2, h2, cap_out=inst.cap_out)
    assert s == t.summary and inst.o["t_refs"].cpu().numpy()[:t.refs.size].tobytes() == t.refs.tobytes()
    assert inst.o["t_cls"].cpu().numpy()[:t.refs.size].tobytes() == t.classes.tobytes()


def host_path(n, c, rng, threads=16):
    tables, sessions, ring, heads = world(n, c, rng)
    share = n // threads
    parts = []
    for i in range(threads):
        lo = i * share
        k = share * PER_BOX
        parts.append(dict(h=PQ.Pmqueue(PQ.HOST_ONLY), sessions=sessions[lo:lo + share].copy(), ring=ring[lo:lo + share].copy(),
                          heads=PQ.aligned_heads(heads[lo:lo + share]), subs=np.arange(share, dtype=np.uint32),
                          off=np.arange(share + 1, dtype=np.uint64) * PER_BOX, opts=np.ones(k, np.uint8), ver=np.full(k, 3, np.uint8),
                          src=np.arange(k, dtype=np.uint32), cls=rng.integers(0, c, size=(k, 1), dtype=np.uint8)))

    def run(fn):
        ts = [threading.Thread(target=fn, args=(p,)) for p in parts]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        return (time.perf_counter() - t0) * 1e3

    put = min(run(lambda p: p["h"].put_host(p["subs"], p["off"], p["opts"], p["ver"], p["src"], p["cls"], tables, p["sessions"], p["ring"],
                                            p["heads"], update_table=False)) for _ in range(3))
    take = min(run(lambda p: p["h"].take_host(None, tables, p["sessions"], p["ring"], p["heads"])) for _ in range(3))
    return put, take


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pmqueue_sweep.jsonl"))
    ap.add_argument("--populations", default=",".join(map(str, POPULATIONS)))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)
        with open(a.out, "w") as f:  # every line as soon as it is measured
            for line in lines:
                f.write(json.dumps(line) + "\n")

    def measure_drain(n=100_000, c=8, qc=64):
        row = dict(drain=True, sessions=n, classes=c, qc=qc, entries_a_session=c * qc)
        for name, drain in (("even_take_ms", False), ("drain_take_ms", True)):
            insts = [Instance(n, c, rng, qc=qc, max_len=qc, drain=drain) for _ in range(2)]
            h = PQ.Pmqueue(0)
            h.reserve(insts[0].total, n)
            row["group"] = h.stats()["group"]
            summary = h.take_device(insts[0].take_args)
            row[name.replace("_ms", "_items")] = summary["items"]
            with torch.cuda.stream(stream):
                row[name], _ = timed(lambda i: h.take_device_async(insts[i % 2].take_args, insts[i % 2].o["summary"].data_ptr(), stream.cuda_stream), 2)
            del insts
            torch.cuda.empty_cache()
        emit(**row)

    def measure(n, c, group=None, skew=False):
        copies = 1 if n * c > 10_000_000 else 2 if n >= 1_000_000 else 4
        insts = [Instance(n, c, rng, skew=skew) for _ in range(copies)]
        plains = [Plain(i, rng) for i in insts]
        h, hm = PQ.Pmqueue(0), MQ.Mqueue(0)
        if group:
            h.set_tuning("group", group)
        h.reserve(insts[0].total, n)
        hm.reserve(insts[0].total, n)
        if n <= 100_000 and not group:
            check_against_host(insts[0], h)
        s = stream.cuda_stream
        row = dict(sessions=n, classes=c, qc=QC, group=h.stats()["group"], skew=skew, deliveries=insts[0].total)
        with torch.cuda.stream(stream):
            row["put_ms"], _ = timed(lambda i: h.put_device_async(insts[i % copies].put_args, insts[i % copies].o["summary"].data_ptr(), s), copies)
            row["take_ms"], _ = timed(lambda i: h.take_device_async(insts[i % copies].take_args, insts[i % copies].o["summary"].data_ptr(), s), copies)
            row["plain_put_ms"], _ = timed(lambda i: hm.put_device_async(plains[i % copies].put_args, insts[i % copies].o["summary"].data_ptr(), s), copies)
            row["plain_take_ms"], _ = timed(lambda i: hm.take_device_async(plains[i % copies].take_args, insts[i % copies].o["summary"].data_ptr(), s), copies)
        row["put_model_tbps"] = put_bytes_model(insts[0].total, n, insts[0].total) / row["put_ms"] / 1e9
        row["take_model_tbps"] = take_bytes_model(n, n * c * MAX_LEN, n * 2) / row["take_ms"] / 1e9
        emit(**row)
        del insts, plains
        torch.cuda.empty_cache()

    pops = [int(x) for x in a.populations.split(",")]
    for n in pops:
        for c in (1, 4, 8):
            if n * c <= 10_000_000:
                measure(n, c)
    if 1_000_000 in pops:
        for g in PQ.GROUPS:
            measure(1_000_000, 4, group=g)
        measure(1_000_000, 4, skew=True)
        measure(1_000_000, 4, group=64, skew=True)
        measure_drain()
        put, take = host_path(1_000_000, 4, rng)
        emit(host_threads=16, sessions=1_000_000, classes=4, put_ms=put, take_ms=take)
    for n in pops:  # the largest rings last
        for c in (4, 8):
            if n * c > 10_000_000:
                measure(n, c)


if __name__ == "__main__":
    main()
