"""Hook consumers selected per published message: the 'message.publish' fold of the rule engine,
the egress bridges and the exhook servers, over the C ABI of include/emqx_select.h (reference:
apps/emqx_rule_engine/src/emqx_rule_engine.erl:157-160 ``get_rules_for_topic/1``,
apps/emqx_bridge/src/emqx_bridge.erl:309-328 ``get_matched_bridges/1``,
apps/emqx_exhook/src/emqx_exhook_server.erl:282-285 ``match_topic_filter/2``).

:class:`OwnerTable` maps filter ids to owners (consumers), commits them as one immutable snapshot
and answers match CSRs (``offsets[n+1]``, ``filters``) plus a per-message class mask with the CSR
of owners, each owner at most once per message.  :class:`HookIndex` owns a match engine and an
owner table and speaks the reference's names.
"""

from __future__ import annotations

import ctypes
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import EngineError, OwnTabStats, SelectBatch, check

__all__ = ["OwnerTable", "HookIndex", "Selected", "HOST_ONLY", "ALL_CLASSES", "CLASS_RULE", "CLASS_BRIDGE",
           "CLASS_EXHOOK"]

HOST_ONLY = -2
ALL_CLASSES = 0xFFFFFFFF
OWNER_ENABLED, OWNER_MATCH_ALL = 0x1, 0x2
# summary words
SUMMARY_WORDS = 8
SUMMARY = ("flags", "entries", "postings", "selected", "messages", "duplicates", "unknown", "max_per_message")
F_OUT_OVERFLOW, F_INPUT_REFUSED = 1, 2
# the class bits HookIndex assigns
CLASS_RULE, CLASS_BRIDGE, CLASS_EXHOOK = 0, 1, 2


class Selected(NamedTuple):
    offsets: np.ndarray  # uint64 [n + 1]
    owners: np.ndarray   # uint32, in no particular order within a message
    summary: dict        # SUMMARY words

    def rows(self) -> List[List[int]]:
        """Per message, the owners in ascending order."""
        o = self.offsets
        return [sorted(self.owners[int(o[i]):int(o[i + 1])].tolist()) for i in range(len(o) - 1)]


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


class OwnerTable:
    """One owner table.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device (changes,
    commit and :meth:`select_host` only; the batch calls raise ``EMQX_EDEVICE``)."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_owntab_create(device, ctypes.byref(h)), "emqx_owntab_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_owntab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- changes -------------------------------------------------------------------------
    def set_flags(self, owner: int, class_bit: int, flags: int, filter_ids=()) -> None:
        """emqx_owntab_set with a ready flags word."""
        f = _u32(list(filter_ids))
        check(_lib.lib().emqx_owntab_set(self._h, owner, class_bit, flags, _p(f), f.size), "emqx_owntab_set")

    def set(self, owner: int, class_bit: int, filter_ids=(), enabled: bool = True, match_all: bool = False) -> None:
        """Replaces the owner's record.  No filter ids and no ``match_all``: never selected."""
        self.set_flags(owner, class_bit, (OWNER_ENABLED if enabled else 0) | (OWNER_MATCH_ALL if match_all else 0),
                       filter_ids)

    def enable(self, owners, on: bool = True) -> None:
        o = _u32(owners)
        check(_lib.lib().emqx_owntab_enable(self._h, _p(o), o.size, int(bool(on))), "emqx_owntab_enable")

    def remove(self, owners) -> None:
        o = _u32(owners)
        check(_lib.lib().emqx_owntab_remove(self._h, _p(o), o.size), "emqx_owntab_remove")

    def commit(self) -> None:
        check(_lib.lib().emqx_owntab_commit(self._h), "emqx_owntab_commit")

    # ---- select --------------------------------------------------------------------------
    def _run(self, fn, name, offsets, filters, classes, cap_out) -> Selected:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        if off.size == 0:
            raise ValueError("offsets needs n + 1 entries")
        n = off.size - 1
        f = _u32(filters)
        c = None if classes is None else _u32(classes)
        if c is not None and c.size != n:
            raise ValueError("one class mask per message")
        cap = max(f.size, 64) if cap_out is None else int(cap_out)
        while True:
            out_off = np.zeros(n + 1, dtype=np.uint64)
            owners = np.zeros(max(cap, 1), dtype=np.uint32)
            b = SelectBatch(offsets=_p(off), filters=_p(f), n=n, cap_in=f.size, msg_classes=_p(c),
                            out_offsets=_p(out_off), out_owners=_p(owners), cap_out=cap)
            n_out = ctypes.c_uint64(0)
            summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
            rc = fn(self._h, ctypes.byref(b), ctypes.byref(n_out), _p(summary))
            if rc == _lib.EMQX_EOVERFLOW:
                if cap_out is None:  # the capacity was this method's guess: take what the call asks for
                    cap = int(n_out.value)
                    continue
                err = EngineError(rc, name)
                err.needed = int(n_out.value)
                err.out_offsets = out_off
                err.out_owners = owners[:cap]
                err.summary = dict(zip(SUMMARY, map(int, summary)))
                raise err
            check(rc, name)
            return Selected(out_off, owners[:int(n_out.value)], dict(zip(SUMMARY, map(int, summary))))

    def select_packed(self, offsets, filters, classes=None, cap_out: Optional[int] = None) -> Selected:
        """One device batch from host buffers (emqx_select_batch)."""
        return self._run(_lib.lib().emqx_select_batch, "emqx_select_batch", offsets, filters, classes, cap_out)

    def select_host(self, offsets, filters, classes=None, cap_out: Optional[int] = None) -> Selected:
        """The same sets computed on the CPU over the same snapshot (per-call path, checker)."""
        return self._run(_lib.lib().emqx_select_host, "emqx_select_host", offsets, filters, classes, cap_out)

    @staticmethod
    def batch(d_offsets: int, d_filters: int, n: int, cap_in: int, d_classes: int, d_out_offsets: int,
              d_out_owners: int, cap_out: int) -> SelectBatch:
        """The argument block of the device forms from raw HIP pointers (``tensor.data_ptr()``; 0 = NULL)."""
        return SelectBatch(offsets=d_offsets or None, filters=d_filters or None, n=n, cap_in=cap_in,
                           msg_classes=d_classes or None, out_offsets=d_out_offsets or None,
                           out_owners=d_out_owners or None, cap_out=cap_out)

    def select_device(self, batch: SelectBatch, stream: int = 0) -> dict:
        """Device-resident batch (:meth:`batch`); returns the summary when done.  Raises
        ``EngineError``: EOVERFLOW carries ``needed`` and ``summary``, EINVAL with summary flag
        bit 1 when the CSR holds more than ``cap_in`` entries."""
        n_out = ctypes.c_uint64(0)
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = _lib.lib().emqx_select_batch_device(self._h, ctypes.byref(batch), ctypes.byref(n_out), _p(summary),
                                                 stream or None)
        if rc != 0:
            err = EngineError(rc, "emqx_select_batch_device")
            err.needed = int(n_out.value)
            err.summary = dict(zip(SUMMARY, map(int, summary)))
            raise err
        return dict(zip(SUMMARY, map(int, summary)))

    def select_device_async(self, batch: SelectBatch, summary: int, stream: int = 0) -> None:
        """Enqueues the batch on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the SUMMARY words when the stream reaches it."""
        check(_lib.lib().emqx_select_batch_device_async(self._h, ctypes.byref(batch), summary, stream or None),
              "emqx_select_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_owntab_set_tuning(self._h, key.encode(), int(value)), "emqx_owntab_set_tuning")

    def stats(self) -> dict:
        s = OwnTabStats()
        check(_lib.lib().emqx_owntab_stats_get(self._h, ctypes.byref(s)), "emqx_owntab_stats_get")
        return s.as_dict()


class HookIndex:
    """The consumers of the 'message.publish' fold: rules, egress bridges and exhook entries, each
    an owner of an :class:`OwnerTable`, their filters in a match engine.

    The engine is asked in ``MODE_ROUTES``: for a topic name (no wildcard level) that is
    ``{F : emqx_topic:match(T, F)}``, the exact filters included (a rule ``from "simple/1"``
    matches the topic ``simple/1``; ``MODE_TRIE`` leaves exact filters out).  A filter shared by
    several owners is inserted once and leaves the engine with its last owner.

    ``device=HOST_ONLY``: no engine; topics are matched against every filter on the CPU
    (``emqx_topic_match``) and the owners selected by ``emqx_select_host``."""

    MATCH_MODE = _lib.MODE_ROUTES

    def __init__(self, device: int = -1):
        self.table = OwnerTable(device)
        self.engine = None
        if device != HOST_ONLY:
            from .engine import Engine
            self.engine = Engine(device)
        self._filters: Dict[bytes, List[int]] = {}   # filter -> [id, owners holding it]
        self._ids: Dict[bytes, int] = {}             # host-only: ids ever given (a filter keeps its id)
        self._owners: Dict[Tuple[str, object], int] = {}
        self._keys: Dict[int, Tuple[str, object]] = {}
        self._held: Dict[int, List[bytes]] = {}      # owner -> the filters it holds
        self._free: List[int] = []
        self._dirty = True

    def close(self):
        self.table.close()
        if self.engine is not None:
            self.engine.close()

    # ---- filters and owners --------------------------------------------------------------
    def _hold(self, filt: bytes) -> int:
        e = self._filters.get(filt)
        if e is None:
            if self.engine is not None:
                fid = int(self.engine.insert([filt])[0])
            else:
                fid = self._ids.setdefault(filt, len(self._ids))
            e = self._filters[filt] = [fid, 0]
        e[1] += 1
        return e[0]

    def _drop(self, filt: bytes) -> None:
        e = self._filters[filt]
        e[1] -= 1
        if e[1] == 0:
            del self._filters[filt]
            if self.engine is not None:
                self.engine.delete([e[0]])

    def _owner(self, key) -> int:
        o = self._owners.get(key)
        if o is None:
            o = self._free.pop() if self._free else len(self._keys)
            self._owners[key] = o
            self._keys[o] = key
        return o

    def _set(self, key, class_bit: int, filters: Sequence[bytes], enabled: bool = True, match_all: bool = False) -> None:
        o = self._owner(key)
        new = list(dict.fromkeys(bytes(f) for f in filters))
        ids = [self._hold(f) for f in new]  # before the old ones go: a filter kept by this owner stays in the engine
        for f in self._held.get(o, ()):
            self._drop(f)
        self._held[o] = new
        self.table.set(o, class_bit, ids, enabled=enabled, match_all=match_all)
        self._dirty = True

    def _delete(self, key) -> None:
        o = self._owners.pop(key, None)
        if o is None:
            return
        for f in self._held.pop(o, ()):
            self._drop(f)
        del self._keys[o]
        self._free.append(o)
        self.table.remove([o])
        self._dirty = True

    def owner_key(self, owner: int):
        """(kind, id) of an owner id as the select stage reports it."""
        return self._keys[owner]

    # ---- the reference's names -----------------------------------------------------------
    def insert_rule(self, rule_id, from_filters: Sequence[bytes]) -> None:
        """emqx_rule_engine:insert_rule/1: ``from`` is the rule's list of topic filters."""
        self._set(("rule", rule_id), CLASS_RULE, from_filters)

    def delete_rule(self, rule_id) -> None:
        self._delete(("rule", rule_id))

    def set_bridge(self, bridge_id, local_topic: bytes, direction: str = "egress", enable: bool = True) -> None:
        """One bridge of emqx:get_config([bridges]): ``direction = ingress`` never matches
        (emqx_bridge.erl:314-315), ``enable = false`` never matches (:322-323)."""
        if direction not in ("egress", "ingress"):
            raise ValueError("direction is egress or ingress")
        self._set(("bridge", bridge_id), CLASS_BRIDGE, [local_topic] if direction == "egress" else [], enabled=enable)

    def delete_bridge(self, bridge_id) -> None:
        self._delete(("bridge", bridge_id))

    def set_exhook(self, hook_id, topics: Sequence[bytes], class_bit: int = CLASS_EXHOOK) -> None:
        """One message hook of an exhook server; an empty ``topics`` matches every topic
        (emqx_exhook_server.erl:282-283).  ``class_bit``: one bit per hook point."""
        self._set(("exhook", hook_id), class_bit, topics, match_all=len(topics) == 0)

    def delete_exhook(self, hook_id) -> None:
        self._delete(("exhook", hook_id))

    def commit(self) -> None:
        if self._dirty:
            if self.engine is not None:
                self.engine.commit()
            self.table.commit()
            self._dirty = False

    # ---- lookups -------------------------------------------------------------------------
    def _match_host(self, topics: Sequence[bytes]):
        L = _lib.lib()
        off, ids = [0], []
        for t in topics:
            ids += [e[0] for f, e in self._filters.items() if L.emqx_topic_match(t, len(t), f, len(f)) == 1]
            off.append(len(ids))
        return np.asarray(off, dtype=np.uint64), np.asarray(ids, dtype=np.uint32)

    def select(self, topics: Sequence[bytes], classes=None) -> List[List[Tuple[str, object]]]:
        """Per topic the (kind, id) of every consumer selected under ``classes`` (one mask per
        topic, or None for every class), sorted by owner id."""
        self.commit()
        topics = [bytes(t) for t in topics]
        if self.engine is not None:
            from .engine import pack
            off, ids = self.engine.match_packed(*pack(topics), mode=self.MATCH_MODE)
            sel = self.table.select_packed(off, ids, classes)
        else:
            off, ids = self._match_host(topics)
            sel = self.table.select_host(off, ids, classes)
        return [[self._keys[o] for o in row] for row in sel.rows()]

    def get_rules_for_topics(self, topics: Sequence[bytes]) -> List[list]:
        return [[k[1] for k in row] for row in self.select(topics, [1 << CLASS_RULE] * len(topics))]

    def get_rules_for_topic(self, topic: bytes) -> list:
        """emqx_rule_engine:get_rules_for_topic/1, as rule ids."""
        return self.get_rules_for_topics([topic])[0]

    def get_matched_bridges(self, topic: bytes) -> list:
        """emqx_bridge:get_matched_bridges/1, as bridge ids."""
        return [k[1] for k in self.select([topic], [1 << CLASS_BRIDGE])[0]]

    @staticmethod
    def message_classes(sys: bool, ignore_sys_message: bool = True, classes: int = ALL_CLASSES) -> int:
        """The class mask of one published message: a sys message skips the bridges
        (emqx_bridge.erl:85) and, under ``ignore_sys_message``, the rules (emqx_rule_events.erl:608-611)."""
        if sys:
            classes &= ~(1 << CLASS_BRIDGE)
            if ignore_sys_message:
                classes &= ~(1 << CLASS_RULE)
        return classes & ALL_CLASSES

    def on_message_publish(self, messages: Sequence[Tuple[bytes, bool]], ignore_sys_message: bool = True):
        """The fold for a batch of ``(topic, sys flag)``: per message the consumers it reaches."""
        return self.select([m[0] for m in messages], [self.message_classes(m[1], ignore_sys_message) for m in messages])

    def select_device_async(self, d_topic_bytes: int, d_topic_offsets: int, n: int, d_match_offsets: int,
                            d_match_ids: int, cap_match: int, d_match_summary: int, d_classes: int,
                            d_out_offsets: int, d_out_owners: int, cap_out: int, d_summary: int, stream: int = 0) -> None:
        """match -> select on one stream, nothing read on the host in between: the match CSR
        (``d_match_offsets[n+1]``, ``d_match_ids[cap_match]``) stays in device memory and the
        owners arrive in ``d_out_offsets[n+1]`` / ``d_out_owners[cap_out]``; both summaries
        (8 uint64 each) are written when the stream reaches them.  Word 0 of the match summary
        is 1 when the engine's scratch was too small for the batch: run it once through the
        synchronous path (:meth:`select`), which sizes the scratch, as include/emqx_match.h says."""
        if self.engine is None:
            raise EngineError(_lib.EMQX_EDEVICE, "HookIndex.select_device_async")
        self.commit()
        self.engine.match_device_async(d_topic_bytes, d_topic_offsets, n, d_match_offsets, d_match_ids, cap_match,
                                       d_match_summary, mode=self.MATCH_MODE, stream=stream)
        self.table.select_device_async(
            OwnerTable.batch(d_match_offsets, d_match_ids, n, cap_match, d_classes, d_out_offsets, d_out_owners, cap_out),
            d_summary, stream=stream)
