"""Batched authorization (ACL) check on the device: ``emqx_authz`` rule lists over the C ABI of
include/emqx_authz.h (reference: apps/emqx_authz/src/emqx_authz_rule.erl, emqx_authz.erl:270-314,
emqx_authz_mnesia.erl:95-111).

:class:`Authz` holds up to 8 sources of ordered rule lists and a table of connected clients,
commits them as one immutable snapshot and answers batches of (client, action, topic) with
``allow`` / ``deny`` / ``nomatch`` and the tag of the rule that decided.  Rules are written as
the Erlang terms of ``acl.conf`` with Python tuples for tuples and ``str`` / ``bytes`` for
strings::

    ("allow", ("ipaddr", "127.0.0.1"), "all", ["$SYS/#", "#"])
    ("allow", ("and", [("client", "c1"), ("user", "u1")]), "publish", ["t/${clientid}", ("eq", "a/#")])
    ("deny", "all")

A regex who term is evaluated by the caller once per client (``re:run/2`` at connect time) and
passed as a bit of the client's flag word: ``("flag", 3)`` in the rule, ``flags=1 << 3`` on the
clients it matches.
"""

from __future__ import annotations

import ctypes
import ipaddress
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import AuthzRule, AuthzStats, AuthzWho, EngineError, check
from .engine import _ptr, pack

HOST_ONLY = -2
NOMATCH, ALLOW, DENY, BAD_REQUEST = 0, 1, 2, 3
PUBLISH, SUBSCRIBE, ALL = 1, 2, 3
TAG_NONE = 0xFFFFFFFF
SCOPES = {"all": 0, "clientid": 1, "username": 2}
_PERMISSION = {"allow": ALLOW, "deny": DENY}
_ACTION = {"publish": PUBLISH, "subscribe": SUBSCRIBE, "all": ALL}
_WHO_ALL, _WHO_ONE, _WHO_AND, _WHO_OR = 0, 1, 2, 3
_LEAF_USERNAME, _LEAF_CLIENTID, _LEAF_CIDR, _LEAF_FLAG = 1, 2, 3, 4


def _bin(x) -> bytes:
    return x if isinstance(x, bytes) else str(x).encode()


def _name(x) -> str:
    return x.decode() if isinstance(x, bytes) else str(x)


class _Builder:
    """Flattens rule terms into the arrays emqx_authz_list_set takes."""

    def __init__(self):
        self.rules: List[Tuple[int, int, int, int, int, int, int]] = []
        self.who: List[Tuple[int, int, int]] = []
        self.strings: List[bytes] = []

    def _string(self, s) -> int:
        self.strings.append(_bin(s))
        return len(self.strings) - 1

    def _leaf(self, term) -> None:
        if not isinstance(term, tuple) or len(term) != 2:
            raise ValueError("who term %r" % (term,))
        kind, arg = _name(term[0]), term[1]
        if kind in ("username", "user", "clientid", "client"):
            if isinstance(arg, tuple):
                raise ValueError("regex who term %r: evaluate it per client and pass (\"flag\", bit)" % (term,))
            self.who.append((_LEAF_USERNAME if kind[0] == "u" else _LEAF_CLIENTID, self._string(arg), 0))
        elif kind == "ipaddr":
            self.who.append((_LEAF_CIDR, self._string(arg), 1))
        elif kind == "ipaddrs":
            first = len(self.strings)
            for c in arg:
                self._string(c)
            self.who.append((_LEAF_CIDR, first, len(arg)))
        elif kind == "flag":
            self.who.append((_LEAF_FLAG, int(arg), 0))
        else:
            raise ValueError("who term %r" % (term,))  # 'and' / 'or' inside 'and' / 'or' included

    def rule(self, term, tag: int) -> None:
        if not isinstance(term, tuple) or len(term) not in (2, 4):
            raise ValueError("rule %r" % (term,))
        if len(term) == 2:  # {Permission, all} -> {Permission, all, all, ["#"]} (emqx_authz_rule.erl:55-56)
            if _name(term[1]) != "all":
                raise ValueError("rule %r" % (term,))
            term = (term[0], "all", "all", ["#"])
        permission, who, action, topics = term
        n0 = len(self.who)
        if isinstance(who, tuple) and _name(who[0]) in ("and", "or"):
            op = _WHO_AND if _name(who[0]) == "and" else _WHO_OR
            for leaf in who[1]:
                self._leaf(leaf)
        elif isinstance(who, tuple):
            op = _WHO_ONE
            self._leaf(who)
        elif _name(who) == "all":
            op = _WHO_ALL
        else:
            raise ValueError("who term %r" % (who,))
        first = len(self.strings)
        for t in topics:
            if isinstance(t, tuple):  # {eq, Topic}: the same compiled form as <<"eq ", Topic>> (:82-85)
                if len(t) != 2 or _name(t[0]) != "eq":
                    raise ValueError("topic %r" % (t,))
                self._string(b"eq " + _bin(t[1]))
            else:
                self._string(t)
        # unknown names pass through as 0: the library rejects them with its message
        self.rules.append((_PERMISSION.get(_name(permission), 0), _ACTION.get(_name(action), 0), op, 0,
                           len(self.who) - n0, first, len(topics), tag))


def _actions(actions) -> np.ndarray:
    if isinstance(actions, np.ndarray):
        return np.ascontiguousarray(actions.astype(np.uint8, copy=False))
    return np.array([a if isinstance(a, (int, np.integer)) else _ACTION.get(_name(a), 0) for a in actions], dtype=np.uint8)


class Authz:
    """One authorization table.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device
    (rules, commit and :meth:`check_host` only; the batch calls raise ``EMQX_EDEVICE``)."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_authz_create(device, ctypes.byref(h)), "emqx_authz_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_authz_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- rules ---------------------------------------------------------------------------
    def set_list(self, source: int, rules: Sequence[tuple], scope: str = "all", key=None,
                 tags: Optional[Sequence[int]] = None) -> None:
        """Replaces the rule list (source, scope, key); ``rules=[]`` removes it.  ``tags[i]`` (default
        ``i``) comes back from the checks rule ``i`` decides."""
        b = _Builder()
        for i, r in enumerate(rules):
            b.rule(r, int(tags[i]) if tags is not None else i)
        ra = (AuthzRule * max(len(b.rules), 1))(*[AuthzRule(*r) for r in b.rules])
        wa = (AuthzWho * max(len(b.who), 1))(*[AuthzWho(*w) for w in b.who])
        buf, offs = pack(b.strings)
        k = _bin(key) if key is not None else b""
        err = ctypes.create_string_buffer(256)
        rc = _lib.lib().emqx_authz_list_set(self._h, source, SCOPES[scope], k, len(k), ra, len(b.rules), wa,
                                            len(b.who), _ptr(buf), _ptr(offs), len(b.strings), err, 256)
        if rc != 0:
            raise EngineError(rc, "emqx_authz_list_set: " + err.value.decode(errors="replace"))

    def clear_source(self, source: int) -> None:
        check(_lib.lib().emqx_authz_source_clear(self._h, source), "emqx_authz_source_clear")

    # ---- clients -------------------------------------------------------------------------
    def set_clients(self, clients: Iterable[dict]) -> None:
        """``clients``: dicts with ``id`` and optionally ``clientid``, ``username`` (``None`` =
        undefined), ``peerhost`` (dotted IPv4 string; anything else counts as no IPv4 peer) and
        ``flags``."""
        cl = list(clients)
        n = len(cl)
        ids = np.array([c["id"] for c in cl], dtype=np.uint32)
        present = np.zeros(max(n, 1), dtype=np.uint8)
        ipv4 = np.zeros(max(n, 1), dtype=np.uint32)
        flags = np.array([int(c.get("flags", 0)) for c in cl] or [0], dtype=np.uint64)
        cids, users = [], []
        for i, c in enumerate(cl):
            cid, user, host = c.get("clientid"), c.get("username"), c.get("peerhost")
            cids.append(_bin(cid) if cid is not None else b"")
            users.append(_bin(user) if user is not None else b"")
            present[i] = (1 if cid is not None else 0) | (2 if user is not None else 0)
            if host is not None:
                try:
                    ipv4[i] = int(ipaddress.IPv4Address(_name(host)))
                    present[i] |= 4
                except ValueError:
                    pass
        cb, co = pack(cids)
        ub, uo = pack(users)
        check(_lib.lib().emqx_authz_clients_set(self._h, _ptr(ids), n, _ptr(cb), _ptr(co), _ptr(ub), _ptr(uo),
                                                _ptr(ipv4), _ptr(present), _ptr(flags)), "emqx_authz_clients_set")

    def drop_clients(self, ids) -> None:
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
        check(_lib.lib().emqx_authz_clients_drop(self._h, _ptr(a), a.size), "emqx_authz_clients_drop")

    def commit(self) -> None:
        check(_lib.lib().emqx_authz_commit(self._h), "emqx_authz_commit")

    # ---- checks --------------------------------------------------------------------------
    def _run(self, fn, name, clients, actions, buf, offs, no_match):
        cl = np.ascontiguousarray(np.asarray(clients, dtype=np.uint32).reshape(-1))
        ac = _actions(actions)
        n = len(offs) - 1
        if cl.size != n or ac.size != n:
            raise ValueError("clients, actions and topics differ in length")
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        tag = np.zeros(max(n, 1), dtype=np.uint32)
        offs = np.ascontiguousarray(np.asarray(offs, dtype=np.uint64))
        check(fn(self._h, _ptr(cl), _ptr(ac), _ptr(buf), _ptr(offs), n, _ptr(verdict), _ptr(tag)), name)
        verdict, tag = verdict[:n], tag[:n]
        if no_match is not None:  # the configured default (emqx_authz.erl:294-301), the caller's to apply
            verdict[verdict == NOMATCH] = _PERMISSION[_name(no_match)]
        return verdict, tag

    def check_packed(self, clients, actions, buf: np.ndarray, offs: np.ndarray, no_match=None):
        """One device batch from host buffers -> (verdicts uint8[n], tags uint32[n])."""
        return self._run(_lib.lib().emqx_authz_check_batch, "emqx_authz_check_batch", clients, actions, buf, offs,
                         no_match)

    def check(self, clients, actions, topics: Sequence[bytes], no_match=None):
        return self.check_packed(clients, actions, *pack([_bin(t) for t in topics]), no_match=no_match)

    def check_host(self, clients, actions, topics: Sequence[bytes], no_match=None):
        """The same answers computed on the CPU over the same snapshot (per-call path, checker)."""
        return self._run(_lib.lib().emqx_authz_check_host, "emqx_authz_check_host", clients, actions,
                         *pack([_bin(t) for t in topics]), no_match)

    def check_device(self, d_clients: int, d_actions: int, d_bytes: int, d_offsets: int, n: int, d_verdict: int,
                     d_tag: int = 0, stream: int = 0) -> None:
        """Device-resident batch (raw HIP pointers, e.g. ``tensor.data_ptr()``); returns when done."""
        check(_lib.lib().emqx_authz_check_batch_device(self._h, d_clients, d_actions, d_bytes, d_offsets, n,
                                                       d_verdict, d_tag or None, stream or None),
              "emqx_authz_check_batch_device")

    def check_device_async(self, d_clients: int, d_actions: int, d_bytes: int, d_offsets: int, n: int,
                           d_verdict: int, d_tag: int, summary: int, stream: int = 0) -> None:
        """Enqueues the batch on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets [flags, allow, deny, nomatch, bad, evals] when the stream reaches it."""
        check(_lib.lib().emqx_authz_check_batch_device_async(self._h, d_clients, d_actions, d_bytes, d_offsets, n,
                                                             d_verdict, d_tag or None, summary, stream or None),
              "emqx_authz_check_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_authz_set_tuning(self._h, key.encode(), int(value)), "emqx_authz_set_tuning")

    def stats(self) -> dict:
        s = AuthzStats()
        check(_lib.lib().emqx_authz_stats_get(self._h, ctypes.byref(s)), "emqx_authz_stats_get")
        return s.as_dict()
