"""Rates of the batched authorization check (emqx_amd/authz.py) at both ends of its workload,
for DESIGN.md §3.8: the default acl.conf (3 filter entries) and file sources of 8 to 4096 rules
in batches that fill the device, then three small batches, each with every launch shape (lanes
per request 1, 4, 16, 64) and the one the library picks.  Device-resident batches, device events
around ~0.2 s of repeated calls, shapes alternated within a round (two rounds by default); a sample of every batch is compared with emqx_authz_check_host.

  python tools/authz_bench.py [--rounds 2] [--host]      (--host: set up and check on the CPU only)
"""

from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from emqx_amd import authz as A  # noqa: E402
from emqx_amd.engine import pack  # noqa: E402


WORKLOADS = [("acl3", 1 << 20)] + [("file%d" % k, min(1 << 20, (1 << 28) // k)) for k in
                                  (8, 16, 32, 64, 128, 256, 512, 1024, 4096)] + [
    ("acl3", 2048), ("file64", 2048), ("file4096", 2048)]


def workload(name, n, device):
    rng = random.Random(11)
    a = A.Authz(device)
    if name == "acl3":  # apps/emqx_authz/etc/acl.conf
        a.set_list(0, [("allow", ("username", "^dashboard?"), "subscribe", ["$SYS/#"]),
                       ("allow", ("ipaddr", "127.0.0.1"), "all", ["$SYS/#", "#"])])
        topics = [b"sensor/%d/temp" % rng.randrange(1000) if rng.random() < 0.9 else b"$SYS/brokers/n1/uptime" for _ in range(n)]
    else:  # a file source: one rule per device class, most requests scan all of it
        k = int(name[4:])
        a.set_list(0, [("allow" if i % 3 else "deny", "all", "publish" if i % 2 else "all", ["fleet/%d/+/state" % i])
                       for i in range(k)] + [("deny", "all")])
        topics = [b"fleet/%d/dev%d/%s" % (rng.randrange(2 * k), rng.randrange(100), rng.choice([b"state", b"cmd"]))
                  for _ in range(n)]
    n_clients = 4096
    a.set_clients([{"id": i, "clientid": "c%d" % i, "username": "u%d" % (i % 100),
                    "peerhost": "127.0.0.1" if i % 16 == 0 else "10.0.%d.%d" % (i // 256, i % 256)} for i in range(n_clients)])
    a.commit()
    clients = np.array([rng.randrange(n_clients) for _ in range(n)], np.uint32)
    actions = np.array([1 + (rng.random() < 0.2) for _ in range(n)], np.uint8)
    return a, clients, actions, topics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    if args.host:
        for name, n in WORKLOADS:
            a, cl, ac, topics = workload(name, min(n, 2000), A.HOST_ONLY)
            v, _ = a.check_host(cl, ac, topics)
            print(json.dumps({"workload": name, "host_sample": np.bincount(v, minlength=4).tolist(), **a.stats()}))
        return
    import torch
    assert torch.cuda.is_available(), "authz_bench needs a HIP device"
    torch.cuda.set_device(0)
    for name, n in WORKLOADS:
        a, cl, ac, topics = workload(name, n, 0)
        buf, offs = pack(topics)
        d = [torch.from_numpy(x.copy()).to("cuda:0") for x in (cl.view(np.int32), ac, buf, offs.view(np.int64))]
        d_v = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        d_t = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def call():
            a.check_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, d_v.data_ptr(),
                           d_t.data_ptr(), stream=stream)

        hv, ht = a.check_host(cl[:2000], ac[:2000], topics[:2000])
        shapes, reps = (0, 1, 4, 16, 64), {}
        for g in shapes:  # warm up, check, and size the timed window to ~0.2 s
            a.set_tuning("group", g)
            call()
            assert d_v[:2000].cpu().numpy().tolist() == hv.tolist(), (name, g)
            assert d_t[:2000].cpu().numpy().view(np.uint32).tolist() == ht.tolist(), (name, g)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            reps[g] = int(min(200, max(2, 200.0 / max(e0.elapsed_time(e1), 1e-3))))
        rates = {g: [] for g in shapes}
        for _ in range(args.rounds):
            for g in shapes:
                a.set_tuning("group", g)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps[g]):
                    call()
                e1.record()
                e1.synchronize()
                rates[g].append(n * reps[g] / (e0.elapsed_time(e1) * 1e-3))
        a.set_tuning("group", 0)
        call()
        s = a.stats()
        print(json.dumps({"workload": name, "requests": n, "entries": s["n_entries"], "picked_group": s["last_group"],
                          "evals_per_request": round(s["last_evals"] / n, 2), "reps": reps,
                          "mreq_per_s": {("auto" if g == 0 else str(g)): [round(r / 1e6, 2) for r in rates[g]]
                                         for g in shapes}}), flush=True)


if __name__ == "__main__":
    main()
