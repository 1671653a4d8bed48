"""The queued messages of every session and ``dequeue/1``, over the C ABI of include/emqx_mqueue.h
(reference: apps/emqx/src/emqx_mqueue.erl:159-202 ``in/2`` and ``out/1`` without a priority table;
apps/emqx/src/emqx_session.erl:453-477 ``dequeue/1``, ``dequeue/3``, :493-536 ``deliver/3``,
``deliver_msg/2``, ``enqueue/2``, :783-787 ``batch_n/1``; apps/emqx/src/emqx_message.erl:239-243
``is_expired/1``).

:class:`Mqueue` keeps nothing itself: next to the session table the caller owns a ring of ``Q``
entries per session (:func:`empty_ring`) and one header per ring (:func:`empty_heads`).
:meth:`Mqueue.put` runs behind every window call and stores what that call queued, reporting the old
entries it evicted; :meth:`Mqueue.take` runs behind every ack run call (or over the whole table on
resume) and pops what the reopened window has room for, in the layout of the window stage's outputs,
so ``Ack.record`` and ``Retry.stamp`` take it unchanged.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import EngineError, MqueuePutArgs, MqueueStats, MqueueTakeArgs, check
from .window import SESSION

__all__ = ["Mqueue", "Put", "Taken", "HOST_ONLY", "ENTRY", "RING", "empty_ring", "empty_heads", "queue_of"]

HOST_ONLY = -2
SUMMARY_WORDS = 8
PUT_SUMMARY = ("flags", "deliveries", "inboxes", "stored", "evicted", "unstored", "full_rows", "len_mismatch")
TAKE_SUMMARY = ("flags", "ok_sessions", "sessions", "items", "sends", "sends_qos0", "expired", "len_mismatch")
F_INPUT_REFUSED, F_BAD_SUB, F_OUTPUT_FULL, F_BAD_REF, F_BAD_RING, F_ROW_FULL, F_LEN_MISMATCH = 2, 4, 8, 0x10, 0x20, 0x40, 0x80
MIN_Q, MAX_Q = 8, 1024
NO_REF = 0xFFFFFFFF
EXPIRED = 10  # the verdict of an expired item (next to window.W_SEND_QOS0 = 1 and W_SEND = 2)
NO_EXPIRY = 0xFFFFFFFFFFFFFFFF
MAX_NOW = 1 << 45
TILE = 1024  # deliveries a tile of the put passes
COUNTS = ("sends", "sends_qos0", "expired", "mq_len_after")

# struct emqx_mqueue_entry and struct emqx_mqueue_ring
ENTRY = np.dtype([("ref", "<u4"), ("opts", "u1"), ("rsv", "u1", (3,))])
RING = np.dtype([("head", "<u4"), ("len", "<u4")])
assert ENTRY.itemsize == 8 and RING.itemsize == 8


def empty_ring(sub_limit: int, q: int) -> np.ndarray:
    """A ring table of ``sub_limit`` rows of ``q`` zero entries."""
    return np.zeros((int(sub_limit), int(q)), dtype=ENTRY)


def empty_heads(sub_limit: int) -> np.ndarray:
    """One ``{head 0, len 0}`` header a session."""
    return np.zeros(int(sub_limit), dtype=RING)


def queue_of(ring: np.ndarray, heads: np.ndarray, sub: int) -> np.ndarray:
    """The queue of session ``sub``, oldest first, as ENTRY records."""
    q = ring.shape[1]
    h, n = int(heads["head"][sub]) % q, min(int(heads["len"][sub]), q)
    return ring[sub][(h + np.arange(n)) % q]


class Put(NamedTuple):
    evicted: np.ndarray   # ENTRY per delivery position: the old entry it evicted, else {NO_REF, 0}
    unstored: np.ndarray  # uint32 [m]: survivors of the inbox the row had no room for
    summary: dict         # PUT_SUMMARY words


class Taken(NamedTuple):
    offsets: np.ndarray   # uint64 [m + 1]: session k's items are [offsets[k]:offsets[k + 1]]
    opts: np.ndarray      # uint8 per item: the delivery's box_opts byte
    verdicts: np.ndarray  # uint8 per item: window.W_SEND_QOS0 / W_SEND / EXPIRED
    pkt_ids: np.ndarray   # uint16 per item (0 unless W_SEND)
    refs: np.ndarray      # uint32 per item
    status: np.ndarray    # uint8 [m]: ack.A_OK / A_NO_SESSION / A_PASS
    counts: np.ndarray    # uint32 [m, 4]: COUNTS
    summary: dict         # TAKE_SUMMARY words


def _p(a):
    return None if a is None else a.ctypes.data


def _tables(ring, heads):
    if not isinstance(ring, np.ndarray) or ring.dtype != ENTRY or ring.ndim != 2 or not ring.flags.c_contiguous:
        raise ValueError("ring is a contiguous [sub_limit, Q] array of ENTRY (empty_ring)")
    if not isinstance(heads, np.ndarray) or heads.dtype != RING or heads.shape != ring.shape[:1] or not heads.flags.c_contiguous:
        raise ValueError("heads is a contiguous array of one RING a row of ring (empty_heads)")
    return ring.shape


def _sessions(sessions, sub_limit, required):
    if sessions is None and not required:
        return
    if not isinstance(sessions, np.ndarray) or sessions.dtype != SESSION or not sessions.flags.c_contiguous:
        raise ValueError("sessions is a contiguous array of window.SESSION records (pack_sessions)")
    if sessions.size != sub_limit:
        raise ValueError("sessions and ring differ in their number of subscribers")


def _raise(rc, name, words, got):
    err = EngineError(rc, name)
    err.summary = words
    err.partial = got  # BAD_SUB and OUTPUT_FULL: what the contract calls complete is
    raise err


class Mqueue:
    """One mqueue stage.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device (the
    ``_host`` calls only; the batch calls raise ``EMQX_EDEVICE``).  The calls of one handle share
    its scratch and run one after the other; concurrent callers take one handle each."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_mqueue_create(device, ctypes.byref(h)), "emqx_mqueue_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_mqueue_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, cap_in: int, cap_boxes: int) -> None:
        """Sizes the device scratch; the asynchronous forms need it done beforehand."""
        check(_lib.lib().emqx_mqueue_reserve(self._h, int(cap_in), int(cap_boxes)), "emqx_mqueue_reserve")

    # ---- host buffers --------------------------------------------------------------------
    def _put(self, fn, name, inbox_subs, inbox_offsets, box_opts, verdicts, ring, heads, refs, sessions) -> Put:
        sub_limit, q = _tables(ring, heads)
        _sessions(sessions, sub_limit, required=False)
        subs = np.ascontiguousarray(np.asarray(inbox_subs, dtype=np.uint32).reshape(-1))
        off = np.ascontiguousarray(np.asarray(inbox_offsets, dtype=np.uint64).reshape(-1))
        if off.size != subs.size + 1:
            raise ValueError("inbox_offsets has one entry more than inbox_subs")
        m = subs.size
        opts = np.ascontiguousarray(np.asarray(box_opts, dtype=np.uint8).reshape(-1))
        ver = np.ascontiguousarray(np.asarray(verdicts, dtype=np.uint8).reshape(-1))
        rf = None if refs is None else np.ascontiguousarray(np.asarray(refs, dtype=np.uint32).reshape(-1))
        cap = opts.size
        if ver.size != cap or (rf is not None and rf.size != cap):
            raise ValueError("box_opts, verdicts and refs differ in length")
        evicted = np.zeros(max(cap, 1), dtype=ENTRY)
        unstored = np.zeros(max(m, 1), dtype=np.uint32)
        b = MqueuePutArgs(inbox_subs=_p(subs), inbox_offsets=_p(off), box_opts=_p(opts), n_boxes=None, m=m, cap_in=cap,
                          cap_boxes=m, verdicts=_p(ver), refs=_p(rf), sessions=_p(sessions), ring=_p(ring), heads=_p(heads),
                          q=q, sub_limit=sub_limit, out_evicted=_p(evicted), out_unstored=_p(unstored))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(PUT_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        got = Put(evicted[:0 if refused else min(words["deliveries"], cap)], unstored[:0 if refused else m], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def put(self, inbox_subs, inbox_offsets, box_opts, verdicts, ring: np.ndarray, heads: np.ndarray, refs=None,
            sessions=None) -> Put:
        """Behind every ``Window.run``: what that call queued goes into ``ring`` and ``heads`` (in
        place), evaluated on the device from host buffers (emqx_mqueue_put_batch).  ``refs``: the
        caller's name of each delivery's message; None: its position.  ``sessions``: the table the
        window call updated, for the check of ``mq_len`` alone."""
        return self._put(_lib.lib().emqx_mqueue_put_batch, "emqx_mqueue_put_batch", inbox_subs, inbox_offsets, box_opts,
                         verdicts, ring, heads, refs, sessions)

    def put_host(self, inbox_subs, inbox_offsets, box_opts, verdicts, ring: np.ndarray, heads: np.ndarray, refs=None,
                 sessions=None) -> Put:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._put(_lib.lib().emqx_mqueue_put_host, "emqx_mqueue_put_host", inbox_subs, inbox_offsets, box_opts,
                         verdicts, ring, heads, refs, sessions)

    def _take(self, fn, name, subs, sessions, ring, heads, now_ms, deadlines, cap_out, update_table) -> Taken:
        sub_limit, q = _tables(ring, heads)
        _sessions(sessions, sub_limit, required=True)
        s = None if subs is None else np.ascontiguousarray(np.asarray(subs, dtype=np.uint32).reshape(-1))
        m = sub_limit if s is None else s.size
        dl = None if deadlines is None else np.ascontiguousarray(np.asarray(deadlines, dtype=np.uint64).reshape(-1))
        cap = m * q if cap_out is None else int(cap_out)
        off = np.zeros(m + 1, dtype=np.uint64)
        opts, ver = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(cap, 1), dtype=np.uint8)
        ids, refs = np.zeros(max(cap, 1), dtype=np.uint16), np.zeros(max(cap, 1), dtype=np.uint32)
        status = np.zeros(max(m, 1), dtype=np.uint8)
        cnt = np.zeros((max(m, 1), 4), dtype=np.uint32)
        b = MqueueTakeArgs(subs=_p(s), n_boxes=None, m=m, cap_boxes=m, sessions=_p(sessions), sub_limit=sub_limit,
                           update_table=1 if update_table else 0, ring=_p(ring), heads=_p(heads), q=q, now_ms=int(now_ms),
                           deadlines=_p(dl), ref_limit=0 if dl is None else dl.size, cap_out=cap, out_offsets=_p(off),
                           out_opts=_p(opts), out_verdicts=_p(ver), out_pkt_ids=_p(ids), out_refs=_p(refs),
                           out_status=_p(status), out_counts=_p(cnt))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(TAKE_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        full = words["flags"] & F_OUTPUT_FULL
        k = 0 if refused else m
        n = 0 if (refused or full) else min(words["items"], cap)
        got = Taken(off[:0 if refused else k + 1], opts[:n], ver[:n], ids[:n], refs[:n], status[:k], cnt[:k], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def take(self, subs, sessions: np.ndarray, ring: np.ndarray, heads: np.ndarray, now_ms: int = 0, deadlines=None,
             cap_out=None, update_table: bool = False) -> Taken:
        """``dequeue/1`` of the sessions ``subs`` names (None: the whole table) at ``now_ms``,
        evaluated on the device from host buffers (emqx_mqueue_take_batch).  With ``update_table``
        ``heads`` and ``sessions`` are rewritten in place.  ``cap_out`` None: room for every entry.
        A call that is full raises ``EngineError`` (EOVERFLOW) with ``partial`` and
        ``summary["items"]`` the capacity it needs; nothing was changed."""
        return self._take(_lib.lib().emqx_mqueue_take_batch, "emqx_mqueue_take_batch", subs, sessions, ring, heads, now_ms,
                          deadlines, cap_out, update_table)

    def take_host(self, subs, sessions: np.ndarray, ring: np.ndarray, heads: np.ndarray, now_ms: int = 0, deadlines=None,
                  cap_out=None, update_table: bool = False) -> Taken:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._take(_lib.lib().emqx_mqueue_take_host, "emqx_mqueue_take_host", subs, sessions, ring, heads, now_ms,
                          deadlines, cap_out, update_table)

    # ---- device buffers ------------------------------------------------------------------
    @staticmethod
    def put_args(d_inbox_subs: int, d_inbox_offsets: int, d_box_opts: int, m: int, cap_in: int, cap_boxes: int,
                 d_verdicts: int, d_ring: int, d_heads: int, q: int, sub_limit: int, d_out_evicted: int, d_out_unstored: int,
                 d_refs: int = 0, d_sessions: int = 0, d_n_boxes: int = 0) -> MqueuePutArgs:
        """The argument block of the device forms of put from raw HIP pointers
        (``tensor.data_ptr()``; 0 = NULL): the window call's inputs and verdicts, the ring tables."""
        return MqueuePutArgs(inbox_subs=d_inbox_subs or None, inbox_offsets=d_inbox_offsets or None, box_opts=d_box_opts or None,
                             n_boxes=d_n_boxes or None, m=m, cap_in=cap_in, cap_boxes=cap_boxes, verdicts=d_verdicts or None,
                             refs=d_refs or None, sessions=d_sessions or None, ring=d_ring or None, heads=d_heads or None, q=q,
                             sub_limit=sub_limit, out_evicted=d_out_evicted or None, out_unstored=d_out_unstored or None)

    @staticmethod
    def take_args(d_subs: int, m: int, cap_boxes: int, d_sessions: int, sub_limit: int, d_ring: int, d_heads: int, q: int,
                  now_ms: int, cap_out: int, d_out_offsets: int, d_out_opts: int, d_out_verdicts: int, d_out_pkt_ids: int,
                  d_out_refs: int, d_out_status: int, d_out_counts: int, d_deadlines: int = 0, ref_limit: int = 0,
                  update_table: bool = False, d_n_boxes: int = 0) -> MqueueTakeArgs:
        """The argument block of the device forms of take.  Behind ``Ack.run``: its ``ack_subs`` and
        count."""
        return MqueueTakeArgs(subs=d_subs or None, n_boxes=d_n_boxes or None, m=m, cap_boxes=cap_boxes,
                              sessions=d_sessions or None, sub_limit=sub_limit, update_table=1 if update_table else 0,
                              ring=d_ring or None, heads=d_heads or None, q=q, now_ms=now_ms, deadlines=d_deadlines or None,
                              ref_limit=ref_limit, cap_out=cap_out, out_offsets=d_out_offsets or None,
                              out_opts=d_out_opts or None, out_verdicts=d_out_verdicts or None,
                              out_pkt_ids=d_out_pkt_ids or None, out_refs=d_out_refs or None, out_status=d_out_status or None,
                              out_counts=d_out_counts or None)

    def _device(self, fn, name, names, args, stream):
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(args), _p(summary), stream or None)
        words = dict(zip(names, map(int, summary)))
        if rc != 0:
            err = EngineError(rc, name)
            err.summary = words
            raise err
        return words

    def put_device(self, args: MqueuePutArgs, stream: int = 0) -> dict:
        """Device-resident put call; returns the summary when done.  Raises ``EngineError``
        (EINVAL) with ``summary`` for a refused input or a subscriber id not below ``sub_limit``."""
        return self._device(_lib.lib().emqx_mqueue_put_batch_device, "emqx_mqueue_put_batch_device", PUT_SUMMARY, args, stream)

    def take_device(self, args: MqueueTakeArgs, stream: int = 0) -> dict:
        """Device-resident take; EOVERFLOW with ``summary["items"]`` the needed ``cap_out``."""
        return self._device(_lib.lib().emqx_mqueue_take_batch_device, "emqx_mqueue_take_batch_device", TAKE_SUMMARY, args, stream)

    def put_device_async(self, args: MqueuePutArgs, summary: int, stream: int = 0) -> None:
        """Enqueues the call on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the summary words when the stream reaches it.  EOVERFLOW, nothing enqueued: the
        scratch :meth:`reserve` sized is too small."""
        check(_lib.lib().emqx_mqueue_put_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_mqueue_put_batch_device_async")

    def take_device_async(self, args: MqueueTakeArgs, summary: int, stream: int = 0) -> None:
        check(_lib.lib().emqx_mqueue_take_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_mqueue_take_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_mqueue_set_tuning(self._h, key.encode(), int(value)), "emqx_mqueue_set_tuning")

    def stats(self) -> dict:
        s = MqueueStats()
        check(_lib.lib().emqx_mqueue_stats_get(self._h, ctypes.byref(s)), "emqx_mqueue_stats_get")
        return s.as_dict()
