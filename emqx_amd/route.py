"""The route step of ``emqx_broker:publish/1`` over the C ABI of include/emqx_route.h:
``route(aggre(emqx_router:match_routes(Topic)), Delivery)`` (apps/emqx/src/emqx_broker.erl:213,
:244-272) for a batch.

:class:`RouteTable` holds the route bag (``#route{topic, dest}``, apps/emqx/src/emqx_router.erl:75-83)
by filter id, commits it as one immutable snapshot in device memory and answers match CSRs
(``offsets[n+1]``, ``filters``) with the flags of every entry, ``|aggre(match_routes(T))|`` per
message, one forward list per node and the CSR of the entries this node dispatches itself.
:class:`ClusterRouter` owns a match engine and a route table and speaks the reference's names.
"""

from __future__ import annotations

import ctypes
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import EngineError, RouteBatch, RouteTabStats, check

__all__ = ["RouteTable", "ClusterRouter", "Routed", "Route", "HOST_ONLY", "MAX_NODES", "NO_GROUP", "LOCAL", "SHARE",
           "REMOTE"]

HOST_ONLY = -2
MAX_NODES = 64
NO_GROUP = 0xFFFFFFFF
LOCAL, SHARE, REMOTE = 0x1, 0x2, 0x4
SUMMARY_WORDS = 8
SUMMARY = ("flags", "entries", "forwards", "dropped", "forwarding_messages", "kept", "unknown", "forward_nodes")
F_FWD_OVERFLOW, F_INPUT_REFUSED = 1, 2


class Route(NamedTuple):
    """#route{topic, dest} (apps/emqx/include/emqx.hrl); dest is Node or (Group, Node)."""
    topic: bytes
    dest: object


class Routed(NamedTuple):
    entry_flags: np.ndarray    # uint8 [entries]
    msg_routes: np.ndarray     # uint32 [n]
    node_offsets: np.ndarray   # uint64 [MAX_NODES + 1]
    fwd_msgs: np.ndarray       # uint32 [forwards]
    fwd_filters: np.ndarray    # uint32 [forwards]
    local_offsets: np.ndarray  # uint64 [n + 1]
    local_filters: np.ndarray  # uint32 [kept]
    summary: dict              # SUMMARY words

    def forwards(self, node: int) -> Tuple[np.ndarray, np.ndarray]:
        """(messages, filters) forwarded to ``node``, in entry order."""
        lo, hi = int(self.node_offsets[node]), int(self.node_offsets[node + 1])
        return self.fwd_msgs[lo:hi], self.fwd_filters[lo:hi]


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


class RouteTable:
    """One route table.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device (changes,
    commit and :meth:`route_host` only; the batch calls raise ``EMQX_EDEVICE``)."""

    def __init__(self, device: int = -1, local_node: int = 0):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_routetab_create(device, local_node, ctypes.byref(h)), "emqx_routetab_create")
        self._h = h
        self.local_node = local_node

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_routetab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- changes -------------------------------------------------------------------------
    @staticmethod
    def _dests(filter_ids, nodes, groups):
        f, v = _u32(filter_ids), _u32(nodes)
        g = None if groups is None else _u32(groups)
        if v.size != f.size or (g is not None and g.size != f.size):
            raise ValueError("one node (and group) per filter id")
        return f, v, g

    def add(self, filter_ids, nodes, groups=None) -> None:
        f, v, g = self._dests(filter_ids, nodes, groups)
        check(_lib.lib().emqx_routetab_add(self._h, _p(f), _p(v), _p(g), f.size), "emqx_routetab_add")

    def remove(self, filter_ids, nodes, groups=None) -> None:
        f, v, g = self._dests(filter_ids, nodes, groups)
        check(_lib.lib().emqx_routetab_remove(self._h, _p(f), _p(v), _p(g), f.size), "emqx_routetab_remove")

    def purge_node(self, node: int, cap: Optional[int] = None) -> np.ndarray:
        """cleanup_routes/1; returns the filter ids left without any dest.  With ``cap`` given and
        too small: ``EngineError`` (EOVERFLOW) carrying ``needed``, nothing removed."""
        room = 64 if cap is None else int(cap)
        while True:
            out = np.zeros(max(room, 1), dtype=np.uint32)
            n = ctypes.c_uint64(0)
            rc = _lib.lib().emqx_routetab_purge_node(self._h, node, _p(out), room, ctypes.byref(n))
            if rc == _lib.EMQX_EOVERFLOW:
                if cap is None:
                    room = int(n.value)
                    continue
                err = EngineError(rc, "emqx_routetab_purge_node")
                err.needed = int(n.value)
                raise err
            check(rc, "emqx_routetab_purge_node")
            return out[:int(n.value)]

    def lookup(self, filter_id: int) -> List[Tuple[int, int]]:
        """lookup_routes/1 as (node, group) in insertion order; group ``NO_GROUP``: a plain route."""
        room = 8
        while True:
            nodes, groups = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32)
            n = ctypes.c_uint64(0)
            rc = _lib.lib().emqx_routetab_lookup(self._h, filter_id, _p(nodes), _p(groups), room, ctypes.byref(n))
            if rc == _lib.EMQX_EOVERFLOW:
                room = int(n.value)
                continue
            check(rc, "emqx_routetab_lookup")
            k = int(n.value)
            return list(zip(nodes[:k].tolist(), groups[:k].tolist()))

    def commit(self) -> None:
        check(_lib.lib().emqx_routetab_commit(self._h), "emqx_routetab_commit")

    # ---- route ---------------------------------------------------------------------------
    def _run(self, fn, name, offsets, filters, cap_fwd, cap_in=None) -> Routed:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        if off.size == 0:
            raise ValueError("offsets needs n + 1 entries")
        n = off.size - 1
        f = _u32(filters)
        cap_in = f.size if cap_in is None else int(cap_in)
        cap = max(f.size, 64) if cap_fwd is None else int(cap_fwd)
        while True:
            flags = np.zeros(max(f.size, 1), dtype=np.uint8)
            routes = np.zeros(max(n, 1), dtype=np.uint32)
            node_off = np.zeros(MAX_NODES + 1, dtype=np.uint64)
            fm, ff = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
            loff, lfil = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(f.size, 1), dtype=np.uint32)
            b = RouteBatch(offsets=_p(off), filters=_p(f), n=n, cap_in=cap_in, entry_flags=_p(flags),
                           msg_routes=_p(routes), node_offsets=_p(node_off), fwd_msgs=_p(fm), fwd_filters=_p(ff),
                           cap_fwd=cap, local_offsets=_p(loff), local_filters=_p(lfil))
            n_fwd = ctypes.c_uint64(0)
            summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
            rc = fn(self._h, ctypes.byref(b), ctypes.byref(n_fwd), _p(summary))
            sm = dict(zip(SUMMARY, map(int, summary)))
            if rc == _lib.EMQX_EOVERFLOW:
                if cap_fwd is None:  # the capacity was this method's guess: take what the call asks for
                    cap = int(n_fwd.value)
                    continue
                err = EngineError(rc, name)
                err.needed = int(n_fwd.value)
                err.result = Routed(flags[:f.size], routes[:n], node_off, fm[:cap], ff[:cap], loff, lfil[:sm["kept"]], sm)
                err.summary = sm
                raise err
            check(rc, name)
            k = int(n_fwd.value)
            return Routed(flags[:f.size], routes[:n], node_off, fm[:k], ff[:k], loff, lfil[:sm["kept"]], sm)

    def route_packed(self, offsets, filters, cap_fwd: Optional[int] = None) -> Routed:
        """One device batch from host buffers (emqx_route_batch)."""
        return self._run(_lib.lib().emqx_route_batch, "emqx_route_batch", offsets, filters, cap_fwd)

    def route_host(self, offsets, filters, cap_fwd: Optional[int] = None, cap_in: Optional[int] = None) -> Routed:
        """The same bytes computed on the CPU over the same snapshot (per-call path, checker)."""
        return self._run(_lib.lib().emqx_route_host, "emqx_route_host", offsets, filters, cap_fwd, cap_in)

    @staticmethod
    def batch(d_offsets: int, d_filters: int, n: int, cap_in: int, d_entry_flags: int, d_msg_routes: int,
              d_node_offsets: int, d_fwd_msgs: int, d_fwd_filters: int, cap_fwd: int, d_local_offsets: int = 0,
              d_local_filters: int = 0) -> RouteBatch:
        """The argument block of the device forms from raw HIP pointers (``tensor.data_ptr()``; 0 = NULL)."""
        return RouteBatch(offsets=d_offsets or None, filters=d_filters or None, n=n, cap_in=cap_in,
                          entry_flags=d_entry_flags or None, msg_routes=d_msg_routes or None,
                          node_offsets=d_node_offsets or None, fwd_msgs=d_fwd_msgs or None,
                          fwd_filters=d_fwd_filters or None, cap_fwd=cap_fwd, local_offsets=d_local_offsets or None,
                          local_filters=d_local_filters or None)

    def route_device(self, batch: RouteBatch, stream: int = 0) -> dict:
        """Device-resident batch (:meth:`batch`); returns the summary when done.  Raises
        ``EngineError``: EOVERFLOW carries ``needed`` and ``summary``, EINVAL with summary flag
        bit 1 when the CSR holds more than ``cap_in`` entries."""
        n_fwd = ctypes.c_uint64(0)
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = _lib.lib().emqx_route_batch_device(self._h, ctypes.byref(batch), ctypes.byref(n_fwd), _p(summary),
                                                stream or None)
        if rc != 0:
            err = EngineError(rc, "emqx_route_batch_device")
            err.needed = int(n_fwd.value)
            err.summary = dict(zip(SUMMARY, map(int, summary)))
            raise err
        return dict(zip(SUMMARY, map(int, summary)))

    def route_device_async(self, batch: RouteBatch, summary: int, stream: int = 0) -> None:
        """Enqueues the batch on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the SUMMARY words when the stream reaches it."""
        check(_lib.lib().emqx_route_batch_device_async(self._h, ctypes.byref(batch), summary, stream or None),
              "emqx_route_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_routetab_set_tuning(self._h, key.encode(), int(value)), "emqx_routetab_set_tuning")

    def stats(self) -> dict:
        s = RouteTabStats()
        check(_lib.lib().emqx_routetab_stats_get(self._h, ctypes.byref(s)), "emqx_routetab_stats_get")
        return s.as_dict()


class ClusterRouter:
    """``emqx_router`` on one node of a cluster: the replicated route table with its dests in
    device memory.  ``node`` is this node's name, ``nodes`` the names known in advance (more are
    taken on first use, up to ``MAX_NODES``); a dest is a node name or ``(group, node)``.

    The engine holds every routed filter, inserted with its first dest and deleted with its last
    (as :class:`emqx_amd.router.Router` does), and is asked in ``MODE_ROUTES``."""

    def __init__(self, node: object = "emqx@127.0.0.1", nodes: Sequence[object] = (), device: int = -1):
        from .engine import Engine
        self.node = node
        self._node_ids: Dict[object, int] = {}
        self._node_names: List[object] = []
        for v in (node, *nodes):
            self._nid(v)
        self.engine = Engine(device)
        self.table = RouteTable(device, self._node_ids[node])
        self._group_ids: Dict[object, int] = {}
        self._group_names: List[object] = []
        self._names: Dict[int, bytes] = {}
        self._count: Dict[int, int] = {}  # dests per filter id
        self._dirty = True

    def close(self):
        self.table.close()
        self.engine.close()

    def _nid(self, node) -> int:
        v = self._node_ids.get(node)
        if v is None:
            if len(self._node_names) >= MAX_NODES:
                raise ValueError("more than %d nodes" % MAX_NODES)
            v = self._node_ids[node] = len(self._node_names)
            self._node_names.append(node)
        return v

    def _gid(self, group) -> int:
        g = self._group_ids.get(group)
        if g is None:
            g = self._group_ids[group] = len(self._group_names)
            self._group_names.append(group)
        return g

    def _dest(self, dest) -> Tuple[int, int]:
        dest = self.node if dest is None else dest
        if isinstance(dest, tuple):
            return self._nid(dest[1]), self._gid(dest[0])
        return self._nid(dest), NO_GROUP

    def _name(self, node: int, group: int):
        return self._node_names[node] if group == NO_GROUP else (self._group_names[group], self._node_names[node])

    def node_id(self, node) -> int:
        return self._node_ids[node]

    def filter_name(self, fid: int) -> bytes:
        return self._names[fid]

    # emqx_router.erl:98-124
    def add_route(self, topic: bytes, dest: object = None) -> None:
        v, g = self._dest(dest)
        fid = self.engine.lookup(topic)
        if fid is not None and (v, g) in self.table.lookup(fid):
            return
        if fid is None or not self._count.get(fid):
            fid = int(self.engine.insert([topic])[0])
            self._names[fid] = topic
            self._count[fid] = 0
        self.table.add([fid], [v], [g])
        self._count[fid] += 1
        self._dirty = True

    do_add_route = add_route

    # emqx_router.erl:150-171
    def delete_route(self, topic: bytes, dest: object = None) -> None:
        v, g = self._dest(dest)
        fid = self.engine.lookup(topic)
        if fid is None or (v, g) not in self.table.lookup(fid):
            return
        self.table.remove([fid], [v], [g])
        self._drop(fid, 1)
        self._dirty = True

    do_delete_route = delete_route

    def _drop(self, fid: int, k: int) -> None:
        self._count[fid] -= k
        if self._count[fid] == 0:
            del self._count[fid]
            del self._names[fid]
            self.engine.delete([fid])

    # emqx_router_helper.erl:171-175
    def cleanup_routes(self, node) -> None:
        v = self._node_ids.get(node)
        if v is None:
            return
        hit = {f: sum(1 for d in self.table.lookup(f) if d[0] == v) for f in list(self._count)}
        emptied = self.table.purge_node(v)
        for f, k in hit.items():
            if k:
                self._drop(f, k)
        assert all(int(f) not in self._count for f in emptied)
        self._dirty = True

    def commit(self) -> None:
        if self._dirty:
            self.engine.commit()
            self.table.commit()
            self._dirty = False

    # emqx_router.erl:142-148
    def lookup_routes(self, topic: bytes) -> List[Route]:
        fid = self.engine.lookup(topic)
        if fid is None or not self._count.get(fid):
            return []
        return [Route(topic, self._name(v, g)) for v, g in self.table.lookup(fid)]

    def has_routes(self, topic: bytes) -> bool:
        return bool(self.lookup_routes(topic))

    def topics(self) -> List[bytes]:
        return list(self._names.values())

    # emqx_router.erl:127-133
    def match_routes(self, topic: bytes) -> List[Route]:
        from .engine import pack
        self.commit()
        off, ids = self.engine.match_packed(*pack([topic]), mode=_lib.MODE_ROUTES)
        out: List[Route] = []
        for f in ids[int(off[0]):int(off[1])].tolist():
            out.extend(Route(self._names[f], self._name(v, g)) for v, g in self.table.lookup(f))
        return out

    def route_batch(self, topics: Sequence[bytes], stream=None):
        """Match and route on one stream, nothing read on the host in between.  Returns
        ``(msg_routes, (local_offsets, local_filters), {node name: (msgs, filters)})``."""
        import torch
        from .engine import pack
        self.commit()
        topics = [bytes(t) for t in topics]
        n = len(topics)
        dev = torch.device("cuda", torch.cuda.current_device())
        st = stream if stream is not None else torch.cuda.current_stream()
        buf, offs = pack(topics)
        cap = max(64, 4 * n)
        with torch.cuda.stream(st):
            d_buf = torch.from_numpy(buf.copy() if buf.size else np.zeros(1, np.uint8)).to(dev)
            d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
            while True:
                cap_fwd = cap * max(1, len(self._node_names) - 1)
                i64, i32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.int32, device=dev)
                m_off, m_ids = torch.zeros(n + 1, **i64), torch.zeros(cap, **i32)
                m_sum, r_sum = torch.zeros(8, **i64), torch.zeros(8, **i64)
                routes, node_off = torch.zeros(max(n, 1), **i32), torch.zeros(MAX_NODES + 1, **i64)
                fm, ff = torch.zeros(max(cap_fwd, 1), **i32), torch.zeros(max(cap_fwd, 1), **i32)
                l_off, l_fil = torch.zeros(n + 1, **i64), torch.zeros(cap, **i32)
                self.engine.match_device_async(d_buf.data_ptr(), d_offs.data_ptr(), n, m_off.data_ptr(), m_ids.data_ptr(),
                                               cap, m_sum.data_ptr(), mode=_lib.MODE_ROUTES, stream=st.cuda_stream)
                self.table.route_device_async(
                    RouteTable.batch(m_off.data_ptr(), m_ids.data_ptr(), n, cap, 0, routes.data_ptr(), node_off.data_ptr(),
                                     fm.data_ptr(), ff.data_ptr(), cap_fwd, l_off.data_ptr(), l_fil.data_ptr()),
                    r_sum.data_ptr(), stream=st.cuda_stream)
                st.synchronize()
                ms, rs = m_sum.cpu().numpy().astype(np.uint64), r_sum.cpu().numpy().astype(np.uint64)
                if int(ms[0]) == 0 and int(rs[0]) == 0:
                    break
                if int(ms[0]) & ~3 or (int(ms[0]) == 0 and int(rs[0])):
                    # a topic the engine refuses; or the route stage overflowed a cap_fwd that holds a forward
                    # to every other node for every entry
                    raise EngineError(_lib.EMQX_EINVAL, "ClusterRouter.route_batch")
                if int(ms[0]) & 1:  # the engine's scratch: the synchronous path sizes it
                    self.engine.match_packed(buf, offs, mode=_lib.MODE_ROUTES)
                cap = max(cap, int(ms[1]) + 1)
        node_off = node_off.cpu().numpy().astype(np.uint64)
        fm, ff = fm.cpu().numpy().astype(np.uint32), ff.cpu().numpy().astype(np.uint32)
        l_off_dev, l_off = l_off, l_off.cpu().numpy().astype(np.uint64)
        fwd = {}
        for v, name in enumerate(self._node_names):
            lo, hi = int(node_off[v]), int(node_off[v + 1])
            if hi > lo:
                fwd[name] = (fm[lo:hi], ff[lo:hi])
        # the device buffers of the call, for a stage chained behind it on the same stream
        self.last = dict(n=n, cap=cap, match_offsets=m_off, match_ids=m_ids, local_offsets=l_off_dev, local_filters=l_fil,
                         summary=dict(zip(SUMMARY, map(int, rs))))
        return (routes.cpu().numpy().astype(np.uint32)[:n], (l_off, l_fil.cpu().numpy().astype(np.uint32)[:int(l_off[n])]),
                fwd)
