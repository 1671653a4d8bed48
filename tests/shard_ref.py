"""A sequential restatement of the filter-sharded step (emqx_amd/csrc/shard_step.hip), in plain
numpy and independent of the step's host mode: from every source's batch it derives what each
call of the step has to produce.

* keys: dist.topic_requests + dist.fold_requests on host tensors (routing has its own tests);
  one key a topic at world 1 or with space P replicated, else two (requests 2t and 2t + 1);
* send: a stable sort of the requests by key, per destination the seven int64 meta words (size,
  n0 n1 n2, bytes0 bytes1 bytes2) and the whole send buffer byte for byte over a sentinel fill:
    [u32 n0 n1 n2 0 bytes0 bytes1 bytes2 0][slot 0: n0 offsets + the closing one][slot 1][slot 2]
    pad 16 [slot 0 bytes][slot 1][slot 2] pad 16
  chunks end to end in destination order (fixed form: chunk r at r * chunk_bytes; a send over
  that capacity leaves header-only chunks with word 3 = 1);
* slot batches: for rank r and slot e every source's slot-e requests in rank order, each
  source's in batch order;
* a synthetic matcher: synth_csr, a pure function of (rank, slot, the request's bytes);
* the result: per source the CSR in batch order (per topic the ids of its first request, then of
  its second);
* the fixed form's flag rules (recv_table, answer_plan, merge_plan): bit 1 send over the chunk
  capacity, 2 slot over capacity, 4 summary bad, 8 answer over capacity.
"""

import numpy as np

E = 3         # engine slots of a rank: A, B, AB
HW = 8        # header words of a request / answer chunk
MW = 1 + 2 * E  # meta words per destination
SENTINEL = 0xA5


def al16(x):
    return (x + 15) & ~15


def ragged_gather(src, first, counts):
    """concat(src[first[i] : first[i] + counts[i]])."""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    if not total:
        return src[:0].copy()
    pre = np.cumsum(counts) - counts
    return src[np.repeat(np.asarray(first, dtype=np.int64) - pre, counts) + np.arange(total, dtype=np.int64)]


def topic_keys(tb, to, world, plan):
    """(keys uint32, one): the batch's bucket keys rank * 3 + slot (3 * world = none)."""
    import torch
    from emqx_amd import dist as D
    one = world == 1 or D.plan_p_replicated(plan)
    n = len(to) - 1
    if n == 0:
        return np.zeros(0, np.uint32), one
    req = D.topic_requests(torch.from_numpy(np.ascontiguousarray(tb)), torch.from_numpy(to.astype(np.int64)), world,
                           plan)
    k = D.fold_requests(req, world).numpy()
    if one:
        assert (k[:, 1] == E * world).all()
        return k[:, 0].astype(np.uint32), one
    return k.reshape(-1).astype(np.uint32), one


def _mix(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7FEB352D)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846CA68B)
    h ^= h >> np.uint32(16)
    return h


def synth_csr(rank, slot, tbytes, offsets):
    """The synthetic matcher's CSR (offsets uint64 (n + 1,), ids uint32) of one slot batch: per
    request a hash of its bytes gives the id count (0 for 3 requests in 16, 1-6 for 12, 17-40 for
    one) and every id is (rank * 3 + slot) << 24 | 18 hash bits << 6 | its index in the request's
    list: a misplaced, swapped or truncated answer shows."""
    off = np.asarray(offsets).astype(np.int64)
    n = len(off) - 1
    lens = off[1:] - off[:-1]
    b = np.asarray(tbytes)[off[0]: off[n]].astype(np.uint32)
    pos = (np.arange(len(b), dtype=np.int64) - np.repeat(off[:-1] - off[0], lens)).astype(np.uint32)
    w = _mix((pos + np.uint32(1)) * np.uint32(0x9E3779B1)) | np.uint32(1)
    cs = np.concatenate([[0], np.cumsum(((b + np.uint32(1)) * w).astype(np.uint64))]).astype(np.uint64)
    rel = off - off[0]
    h = _mix(((cs[rel[1:]] - cs[rel[:-1]]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
             ^ (lens.astype(np.uint32) * np.uint32(0x85EBCA6B)))
    sel, hi = h & np.uint32(15), (h >> np.uint32(4)).astype(np.int64)
    cnt = np.where(sel == 0, 17 + hi % 24, np.where(sel <= 3, 0, 1 + hi % 6)).astype(np.int64)
    ooff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    j = np.arange(int(ooff[n]), dtype=np.int64) - np.repeat(ooff[:-1].astype(np.int64), cnt)
    ids = (np.uint32((rank * E + slot) << 24) | ((np.repeat(h, cnt) & np.uint32(0x3FFFF)) << np.uint32(6))
           | j.astype(np.uint32))
    return ooff, ids.astype(np.uint32)


PAD_MARK = 0xFF  # top byte of a padding topic's ids; a request's is rank * 3 + slot <= 191 (world 64)


def pad_csr(off, ids, npad, with_ids):
    """A slot's CSR over its fixed-size batch, as an engine writes it: the requests' CSR (off,
    ids), then npad padding topics.  Without ids every padding offset is the requests' end; with
    them padding topic j has j % 6 ids PAD_MARK << 24 | j << 3 | k behind the requests' ids (an
    empty topic under root-wildcard filters), which no answer chunk and no output may carry."""
    j = np.arange(npad, dtype=np.int64)
    cnt = j % 6 if with_ids else np.zeros(npad, np.int64)
    end = np.uint64(off[-1]) + np.cumsum(cnt).astype(np.uint64)
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    marks = (np.uint32(PAD_MARK << 24) | (np.repeat(j, cnt).astype(np.uint32) << np.uint32(3)) | k.astype(np.uint32))
    return np.concatenate([off, end]).astype(np.uint64), np.concatenate([ids, marks]).astype(np.uint32)


def recv_stride(G, capq, capy):
    """The grid-stride of shard_recv_fixed_kernel for a rank's slot capacities, restating the
    sizing of emqx_shard_step_recv_fixed: per = max(requests, bytes / 16) / (3 G) + 1 items a
    (source, slot) part, x = per / 256 blocks rounded up, at most max(1, 1024 / G), of 256 threads."""
    per = max(sum(capq), sum(capy) // 16) // (E * G) + 1
    x = max(1, min((per + 255) // 256, max(1, 1024 // G)))
    return 256 * x


class Send:
    """One source's send: its requests sorted by key, the meta words and the send buffer."""

    def __init__(self, tb, to, world, plan):
        G = self.world = world
        nb = E * G + 1
        to = np.asarray(to).astype(np.int64)
        self.n = len(to) - 1
        keys, self.one = topic_keys(tb, to, world, plan)
        self.m = m = len(keys)
        order = np.argsort(keys, kind="stable")
        cnt = np.bincount(keys, minlength=nb).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(cnt)])  # nb + 1
        self.nreq = nreq = int(self.start[nb - 1])
        self.perm = order[:nreq]  # the real requests, sorted
        self.key_s = keys[self.perm].astype(np.int64)
        topic_s = self.perm if self.one else self.perm >> 1
        self.len_s = to[topic_s + 1] - to[topic_s]
        self.x = np.concatenate([[0], np.cumsum(self.len_s)])  # byte prefix of every sorted request
        self.bpre = self.x[self.start[:nb]]
        self.X = ragged_gather(np.asarray(tb), to[topic_s], self.len_s)  # the sorted requests' bytes
        self.nq = cnt[: E * G].reshape(G, E)
        self.by = (self.bpre[1:] - self.bpre[:-1]).reshape(G, E)
        self.size = 4 * HW + al16(4 * (self.nq.sum(1) + E)) + al16(self.by.sum(1))
        self.meta = np.column_stack([self.size, self.nq, self.by]).astype(np.int64)
        assert m == (self.n if self.one else 2 * self.n)

    def bases(self, fixed=0):
        return np.arange(self.world) * fixed if fixed else np.concatenate([[0], np.cumsum(self.size)])[:-1]

    def over(self, fixed):
        return bool(fixed) and bool((self.size > fixed).any())

    def expect_meta(self, fixed=0):
        meta = self.meta.copy()
        if self.over(fixed):
            meta[:, 0] = -1
        return meta

    def expect_buffer(self, nbytes, fixed=0):
        """The send buffer of nbytes over the sentinel."""
        buf = np.full(nbytes, SENTINEL, np.uint8)
        w = buf[: nbytes & ~3].view(np.uint32)
        base = self.bases(fixed)
        for r in range(self.world):
            h = int(base[r]) // 4
            if self.over(fixed):
                w[h: h + HW + E] = 0
                w[h + 3] = 1
                continue
            w[h: h + HW] = list(self.nq[r]) + [0] + list(self.by[r]) + [0]
            o = h + HW
            for e in range(E):
                b = E * r + e
                s0, s1 = int(self.start[b]), int(self.start[b + 1])
                w[o: o + s1 - s0] = self.x[s0:s1] - self.bpre[b]
                w[o + s1 - s0] = self.by[r, e]
                o += s1 - s0 + 1
            d = int(base[r]) + 4 * HW + al16(4 * (int(self.nq[r].sum()) + E))
            buf[d: d + int(self.by[r].sum())] = self.X[int(self.bpre[E * r]): int(self.bpre[E * r + E])]
        return buf

    def bucket(self, b):
        """(lengths, bytes) of bucket b's requests in sorted (= batch) order."""
        s0, s1 = int(self.start[b]), int(self.start[b + 1])
        return self.len_s[s0:s1], self.X[int(self.bpre[b]): int(self.bpre[b + 1])]


class Ref:
    """The whole step of `world` ranks over `batches` ((bytes uint8, offsets) per source)."""

    def __init__(self, world, plan, batches):
        assert len(batches) == world
        self.world, self.plan = world, plan
        self.sends = [Send(tb, to, world, plan) for tb, to in batches]
        self.live = [s for s in range(world) if self.sends[s].nreq]
        self._slots, self._csrs, self._results, self._words = {}, {}, None, {}
        nq = np.stack([s.nq for s in self.sends])  # (source, rank, slot)
        self._q0 = np.concatenate([np.zeros((1,) + nq.shape[1:], np.int64), np.cumsum(nq, axis=0)])
        self.slot_bytes = np.stack([s.by for s in self.sends]).sum(0)  # (rank, slot)

    # q0[r][e]: the first slot-e request of every source in rank r's slot-e batch (world + 1)
    def q0(self, r, e):
        return self._q0[:, r, e]

    def slot_batch(self, r, e, empty=False):
        """(offsets uint64 from 0, bytes) of rank r's slot-e batch (empty: a flagged step's)."""
        if empty:
            return np.zeros(1, np.uint64), np.zeros(0, np.uint8)
        key = (r, e)
        if key not in self._slots:
            parts = [self.sends[s].bucket(E * r + e) for s in self.live]
            lens = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.int64)
            byt = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint8)
            self._slots[key] = (np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), byt)
        return self._slots[key]

    def csr(self, r, e):
        if (r, e) not in self._csrs:
            off, byt = self.slot_batch(r, e)
            self._csrs[(r, e)] = synth_csr(r, e, byt, off)
        return self._csrs[(r, e)]

    def answer_words(self, r):
        """Per source the words of rank r's answer chunk and its ids: (world, 2) int64."""
        if r not in self._words:
            nall = np.zeros(self.world, np.int64)
            iall = np.zeros(self.world, np.int64)
            for e in range(E):
                q = self.q0(r, e)
                at = self.csr(r, e)[0].astype(np.int64)[q]
                nall += q[1:] - q[:-1]
                iall += at[1:] - at[:-1]
            words = HW + nall + iall
            words[r] -= iall[r]  # the rank's own chunk carries no ids
            self._words[r] = np.column_stack([words, iall])
        return self._words[r]

    def results(self):
        """Per source (offsets uint64 (n + 1,), ids uint32): per topic its first request's ids,
        then its second's."""
        if self._results is None:
            G = self.world
            pool, base = [], {}
            at = 0
            for r in range(G):
                for e in range(E):
                    ids = self.csr(r, e)[1]
                    base[(r, e)] = at
                    at += len(ids)
                    pool.append(ids)
            pool = np.concatenate(pool) if pool else np.zeros(0, np.uint32)
            q0 = {(r, e): self.q0(r, e) for r in range(G) for e in range(E)}
            self._results = []
            for s, sd in enumerate(self.sends):
                cnt = np.zeros(sd.m, np.int64)
                addr = np.zeros(sd.m, np.int64)
                for b in np.nonzero(sd.start[1: E * G + 1] - sd.start[: E * G])[0]:
                    r, e = divmod(int(b), E)
                    s0, s1 = int(sd.start[b]), int(sd.start[b + 1])
                    off = self.csr(r, e)[0].astype(np.int64)
                    a = int(q0[(r, e)][s])
                    seg = off[a: a + s1 - s0 + 1]
                    cnt[sd.perm[s0:s1]] = seg[1:] - seg[:-1]
                    addr[sd.perm[s0:s1]] = base[(r, e)] + seg[:-1]
                per_topic = cnt if sd.one else cnt.reshape(-1, 2).sum(1)
                off = np.concatenate([[0], np.cumsum(per_topic)]).astype(np.uint64)
                self._results.append((off, ragged_gather(pool, addr, cnt)))  # (requests in batch order)
        return self._results

    # ---- the fixed form ----------------------------------------------------------------------
    def fixed_flags(self, chunk_bytes, capq, capy, chunk_words, bad=()):
        """(recv flag per rank, answer flag per rank, the merge flag every rank ends with).
        capq[r][e] / capy[r][e]: rank r's slot capacities; bad: the ranks given a bad summary."""
        G = self.world
        over = [sd.over(chunk_bytes) for sd in self.sends]
        recv, ans = [], []
        for r in range(G):
            f = 1 if (over[r] or any(over)) else 0
            if not f:
                for e in range(E):
                    if self.q0(r, e)[G] > capq[r][e] or self.slot_bytes[r, e] > capy[r][e]:
                        f |= 2
            recv.append(f)
            if r in bad:
                f |= 4
            if not f and (self.answer_words(r)[:, 0] > chunk_words).any():
                f |= 8
            ans.append(f)
        merged = 0
        for f in ans:
            merged |= f
        return recv, ans, merged
