"""The queued messages of the sessions whose zone sets ``mqueue_priorities``, over the C ABI of
include/emqx_pmqueue.h (reference: apps/emqx/src/emqx_mqueue.erl:159-254 ``in/2`` and ``out/1`` with a
``p_table`` and ``shift_opts``; apps/emqx/src/emqx_pqueue.erl:98-211; apps/emqx/src/emqx_session.erl:453-477
``dequeue/1``).

:class:`Pmqueue` keeps nothing itself: next to the session table the caller owns the zone
configurations (:func:`pack_tables`), ``C`` rings of ``Qc`` entries per session (:func:`empty_ring`) and
one 64-byte head per session (:func:`empty_heads`).  :meth:`Pmqueue.put_host` / ``put_device`` run behind
every window call (whose records carry ``mq_max = 0`` for these sessions), :meth:`Pmqueue.take_host` /
``take_device`` behind every ack run call (:meth:`Pmqueue.put` and :meth:`Pmqueue.take` take host buffers to the device); the take's outputs have the layout of ``Mqueue.take``'s, plus
the class of every item, so ``Ack.record`` and ``Retry.stamp`` take them unchanged.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import EngineError, PmqueuePutArgs, PmqueueStats, PmqueueTakeArgs, check
from .mqueue import ENTRY, NO_REF
from .window import SESSION

__all__ = ["Pmqueue", "Put", "Taken", "HOST_ONLY", "TABLE", "HEAD", "pack_tables", "empty_ring", "empty_heads", "queue_of",
           "order_of"]

HOST_ONLY = -2
SUMMARY_WORDS = 8
PUT_SUMMARY = ("flags", "deliveries", "inboxes", "stored", "evicted", "dropped_in_batch", "unstored", "ok_inboxes")
TAKE_SUMMARY = ("flags", "ok_sessions", "sessions", "items", "sends", "sends_qos0", "expired", "unfit")
(F_INPUT_REFUSED, F_BAD_SUB, F_OUTPUT_FULL, F_BAD_REF, F_BAD_HEAD, F_ROW_FULL, F_UNFIT, F_BAD_VERDICT, F_BAD_SRC,
 F_LIMITED) = 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400
MAX_CLASSES, MIN_QC, MAX_QC = 8, 8, 128
PRIO_INFINITY = 0x7FFFFFFF
MAX_PRIO, MAX_MULT = 1000000, 1024
NO_CLASS = 0xFF
UNFIT = 7  # the status of a session whose table the stage does not serve (next to ack.A_OK / A_NO_SESSION / A_PASS)
H_LAST_DEFINED = 1
NO_ORDER = 0xFFFFFFFF
GROUPS = (4, 8, 16, 32, 64)
PUT_COUNTS = ("stored", "evicted", "dropped_in_batch", "unstored", "mq_len_after", "dropped_lo", "dropped_hi", "status")
TAKE_COUNTS = ("sends", "sends_qos0", "expired", "mq_len_after")

# struct emqx_pmqueue_table and struct emqx_pmqueue_head
TABLE = np.dtype([("n_classes", "<u4"), ("default_class", "<u4"), ("max_len", "<u4"), ("mult", "<u4"), ("base", "<u4"),
                  ("rsv", "<u4"), ("prio", "<i4", (8,))])
HEAD = np.dtype([("head", "<u2", (8,)), ("len", "<u2", (8,)), ("order", "<u4"), ("credit", "<i4"), ("flags", "<u4"),
                 ("table", "<u4"), ("rsv", "<u4", (4,))])
assert TABLE.itemsize == 56 and HEAD.itemsize == 64


def pack_tables(configs) -> np.ndarray:
    """One TABLE per ``(prios, default_class, max_len, mult, base)``; ``prios`` in descending
    order, ``"infinity"`` (or PRIO_INFINITY) only first."""
    out = np.zeros(len(configs), dtype=TABLE)
    for t, (prios, default_class, max_len, mult, base) in zip(out, configs):
        t["n_classes"], t["default_class"], t["max_len"], t["mult"], t["base"] = len(prios), default_class, max_len, mult, base
        for c, p in enumerate(list(prios)[:8]):
            t["prio"][c] = PRIO_INFINITY if p == "infinity" else p
    return out


def empty_ring(sub_limit: int, c: int, qc: int) -> np.ndarray:
    """``sub_limit`` sessions of ``c`` class rings of ``qc`` zero entries."""
    return np.zeros((int(sub_limit), int(c), int(qc)), dtype=ENTRY)


def empty_heads(sub_limit: int, table=0) -> np.ndarray:
    """One empty head a session (64-byte aligned); ``table``: the table of every session, or one each."""
    raw = np.zeros(int(sub_limit) * 64 + 64, dtype=np.uint8)
    at = (-raw.ctypes.data) % 64
    heads = raw[at:at + int(sub_limit) * 64].view(HEAD)
    heads["order"] = NO_ORDER
    heads["table"] = table
    return heads


def aligned_heads(heads: np.ndarray) -> np.ndarray:
    """A 64-byte aligned copy."""
    out = empty_heads(heads.size)
    out[:] = heads
    return out


def order_of(heads: np.ndarray, sub: int) -> list:
    """The order list of session ``sub`` as class indices."""
    word, out = int(heads["order"][sub]), []
    for p in range(8):
        nib = (word >> (4 * p)) & 0xF
        if nib == 0xF:
            break
        out.append(nib)
    return out


def queue_of(ring: np.ndarray, heads: np.ndarray, sub: int, c: int) -> np.ndarray:
    """Class ``c`` of session ``sub``, oldest first, as ENTRY records."""
    qc = ring.shape[2]
    h, n = int(heads["head"][sub][c]) % qc, min(int(heads["len"][sub][c]), qc)
    return ring[sub, c][(h + np.arange(n)) % qc]


class Put(NamedTuple):
    verdicts: np.ndarray  # uint8 per delivery: window.W_QUEUED / W_QUEUED_DROPPED (| W_EVICTS), 0 for a non-candidate
    classes: np.ndarray   # uint8 per delivery: its class, NO_CLASS for a non-candidate
    evicted: np.ndarray   # ENTRY per delivery: the old entry it evicted, else {NO_REF, 0}
    counts: np.ndarray    # uint32 [m, 8]: PUT_COUNTS
    summary: dict         # PUT_SUMMARY words


class Taken(NamedTuple):
    offsets: np.ndarray   # uint64 [m + 1]
    opts: np.ndarray      # uint8 per item
    verdicts: np.ndarray  # uint8 per item: window.W_SEND_QOS0 / W_SEND / mqueue.EXPIRED
    pkt_ids: np.ndarray   # uint16 per item (0 unless W_SEND)
    refs: np.ndarray      # uint32 per item
    classes: np.ndarray   # uint8 per item: the class it came from
    status: np.ndarray    # uint8 [m]: ack.A_OK / A_NO_SESSION / A_PASS / UNFIT
    counts: np.ndarray    # uint32 [m, 4]: TAKE_COUNTS
    summary: dict         # TAKE_SUMMARY words


def _p(a):
    return None if a is None else a.ctypes.data


def _state(tables, sessions, ring, heads):
    if not isinstance(tables, np.ndarray) or tables.dtype != TABLE or tables.ndim != 1 or not tables.flags.c_contiguous:
        raise ValueError("tables is a contiguous array of TABLE (pack_tables)")
    if not isinstance(ring, np.ndarray) or ring.dtype != ENTRY or ring.ndim != 3 or not ring.flags.c_contiguous:
        raise ValueError("ring is a contiguous [sub_limit, C, Qc] array of mqueue.ENTRY (empty_ring)")
    if not isinstance(heads, np.ndarray) or heads.dtype != HEAD or heads.shape != ring.shape[:1] or not heads.flags.c_contiguous:
        raise ValueError("heads is a contiguous array of one HEAD a session (empty_heads)")
    if not isinstance(sessions, np.ndarray) or sessions.dtype != SESSION or not sessions.flags.c_contiguous or \
            sessions.size != ring.shape[0]:
        raise ValueError("sessions is a contiguous array of one window.SESSION a session (pack_sessions)")
    return ring.shape


def _raise(rc, name, words, got):
    err = EngineError(rc, name)
    err.summary = words
    err.partial = got  # BAD_SUB and OUTPUT_FULL: what the contract calls complete is
    raise err


class Pmqueue:
    """One priority mqueue stage.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device
    (the ``_host`` calls only; the device calls raise ``EMQX_EDEVICE``)."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_pmqueue_create(device, ctypes.byref(h)), "emqx_pmqueue_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_pmqueue_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, cap_in: int, cap_boxes: int) -> None:
        """Sizes the device scratch; the asynchronous forms need it done beforehand."""
        check(_lib.lib().emqx_pmqueue_reserve(self._h, int(cap_in), int(cap_boxes)), "emqx_pmqueue_reserve")

    # ---- host buffers --------------------------------------------------------------------
    def put_host(self, inbox_subs, inbox_offsets, box_opts, verdicts, box_src, msg_class, tables: np.ndarray,
                 sessions: np.ndarray, ring: np.ndarray, heads: np.ndarray, refs=None, update_table: bool = True) -> Put:
        """``in/2`` for a batch on the CPU (emqx_pmqueue_put_host): what the window call queued goes into
        ``ring``; with ``update_table`` ``heads`` and ``sessions`` (mq_len, dropped) are rewritten in place.
        ``msg_class``: uint8 [n_msgs, n_tables]."""
        return self._put(_lib.lib().emqx_pmqueue_put_host, "emqx_pmqueue_put_host", inbox_subs, inbox_offsets, box_opts, verdicts,
                         box_src, msg_class, tables, sessions, ring, heads, refs, update_table)

    def put(self, inbox_subs, inbox_offsets, box_opts, verdicts, box_src, msg_class, tables: np.ndarray,
            sessions: np.ndarray, ring: np.ndarray, heads: np.ndarray, refs=None, update_table: bool = True) -> Put:
        """The same from host buffers, evaluated on the device (emqx_pmqueue_put_batch)."""
        return self._put(_lib.lib().emqx_pmqueue_put_batch, "emqx_pmqueue_put_batch", inbox_subs, inbox_offsets, box_opts, verdicts,
                         box_src, msg_class, tables, sessions, ring, heads, refs, update_table)

    def _put(self, fn, name, inbox_subs, inbox_offsets, box_opts, verdicts, box_src, msg_class, tables, sessions, ring, heads, refs,
             update_table) -> Put:
        sub_limit, c, qc = _state(tables, sessions, ring, heads)
        subs = np.ascontiguousarray(np.asarray(inbox_subs, dtype=np.uint32).reshape(-1))
        off = np.ascontiguousarray(np.asarray(inbox_offsets, dtype=np.uint64).reshape(-1))
        if off.size != subs.size + 1:
            raise ValueError("inbox_offsets has one entry more than inbox_subs")
        m = subs.size
        opts = np.ascontiguousarray(np.asarray(box_opts, dtype=np.uint8).reshape(-1))
        ver = np.ascontiguousarray(np.asarray(verdicts, dtype=np.uint8).reshape(-1))
        src = np.ascontiguousarray(np.asarray(box_src, dtype=np.uint32).reshape(-1))
        rf = None if refs is None else np.ascontiguousarray(np.asarray(refs, dtype=np.uint32).reshape(-1))
        mc = np.ascontiguousarray(np.asarray(msg_class, dtype=np.uint8).reshape(-1, max(tables.size, 1)))
        cap = opts.size
        if ver.size != cap or src.size != cap or (rf is not None and rf.size != cap):
            raise ValueError("box_opts, verdicts, box_src and refs differ in length")
        out_ver, out_cls = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(cap, 1), dtype=np.uint8)
        evicted = np.zeros(max(cap, 1), dtype=ENTRY)
        counts = np.zeros((max(m, 1), 8), dtype=np.uint32)
        b = PmqueuePutArgs(inbox_subs=_p(subs), inbox_offsets=_p(off), box_opts=_p(opts), n_boxes=None, m=m, cap_in=cap,
                           cap_boxes=m, verdicts=_p(ver), refs=_p(rf), box_src=_p(src), msg_class=_p(mc), n_msgs=mc.shape[0],
                           tables=_p(tables), n_tables=tables.size, sessions=_p(sessions), sub_limit=sub_limit,
                           update_table=1 if update_table else 0, ring=_p(ring), heads=_p(heads), c=c, qc=qc,
                           out_verdicts=_p(out_ver), out_class=_p(out_cls), out_evicted=_p(evicted), out_counts=_p(counts))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(PUT_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        n = 0 if refused else min(words["deliveries"], cap)
        got = Put(out_ver[:n], out_cls[:n], evicted[:n], counts[:0 if refused else m], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def take_host(self, subs, tables: np.ndarray, sessions: np.ndarray, ring: np.ndarray, heads: np.ndarray, now_ms: int = 0,
                  deadlines=None, cap_out=None, update_table: bool = False) -> Taken:
        """``dequeue/1`` of the sessions ``subs`` names (None: the whole table) at ``now_ms`` on the CPU
        (emqx_pmqueue_take_host).  A call that is full raises ``EngineError`` (EOVERFLOW) with ``partial``
        and ``summary["items"]`` the capacity it needs; nothing was changed."""
        return self._take(_lib.lib().emqx_pmqueue_take_host, "emqx_pmqueue_take_host", subs, tables, sessions, ring, heads, now_ms,
                          deadlines, cap_out, update_table)

    def take(self, subs, tables: np.ndarray, sessions: np.ndarray, ring: np.ndarray, heads: np.ndarray, now_ms: int = 0,
             deadlines=None, cap_out=None, update_table: bool = False) -> Taken:
        """The same from host buffers, evaluated on the device (emqx_pmqueue_take_batch)."""
        return self._take(_lib.lib().emqx_pmqueue_take_batch, "emqx_pmqueue_take_batch", subs, tables, sessions, ring, heads, now_ms,
                          deadlines, cap_out, update_table)

    def _take(self, fn, name, subs, tables, sessions, ring, heads, now_ms, deadlines, cap_out, update_table) -> Taken:
        sub_limit, c, qc = _state(tables, sessions, ring, heads)
        s = None if subs is None else np.ascontiguousarray(np.asarray(subs, dtype=np.uint32).reshape(-1))
        m = sub_limit if s is None else s.size
        dl = None if deadlines is None else np.ascontiguousarray(np.asarray(deadlines, dtype=np.uint64).reshape(-1))
        cap = m * c * qc if cap_out is None else int(cap_out)
        off = np.zeros(m + 1, dtype=np.uint64)
        opts, ver, cls = (np.zeros(max(cap, 1), dtype=np.uint8) for _ in range(3))
        ids, refs = np.zeros(max(cap, 1), dtype=np.uint16), np.zeros(max(cap, 1), dtype=np.uint32)
        status = np.zeros(max(m, 1), dtype=np.uint8)
        cnt = np.zeros((max(m, 1), 4), dtype=np.uint32)
        b = PmqueueTakeArgs(subs=_p(s), n_boxes=None, m=m, cap_boxes=m, sessions=_p(sessions), sub_limit=sub_limit,
                            update_table=1 if update_table else 0, tables=_p(tables), n_tables=tables.size, ring=_p(ring),
                            heads=_p(heads), c=c, qc=qc, now_ms=int(now_ms), deadlines=_p(dl),
                            ref_limit=0 if dl is None else dl.size, cap_out=cap, out_offsets=_p(off), out_opts=_p(opts),
                            out_verdicts=_p(ver), out_pkt_ids=_p(ids), out_refs=_p(refs), out_class=_p(cls),
                            out_status=_p(status), out_counts=_p(cnt))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(TAKE_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        full = words["flags"] & F_OUTPUT_FULL
        k = 0 if refused else m
        n = 0 if (refused or full) else min(words["items"], cap)
        got = Taken(off[:0 if refused else k + 1], opts[:n], ver[:n], ids[:n], refs[:n], cls[:n], status[:k], cnt[:k], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    # ---- device buffers ------------------------------------------------------------------
    @staticmethod
    def put_args(**kw) -> PmqueuePutArgs:
        """The argument block of the device forms of put from raw HIP pointers (``tensor.data_ptr()``;
        0 = NULL) and counts, by the field names of ``struct emqx_pmqueue_put_args``."""
        return PmqueuePutArgs(**{k: (v or None) if k in _PUT_PTRS else v for k, v in kw.items()})

    @staticmethod
    def take_args(**kw) -> PmqueueTakeArgs:
        """The argument block of the device forms of take, by the field names of
        ``struct emqx_pmqueue_take_args``."""
        return PmqueueTakeArgs(**{k: (v or None) if k in _TAKE_PTRS else v for k, v in kw.items()})

    def _device(self, fn, name, names, args, stream):
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(args), _p(summary), stream or None)
        words = dict(zip(names, map(int, summary)))
        if rc != 0:
            err = EngineError(rc, name)
            err.summary = words
            raise err
        return words

    def put_device(self, args: PmqueuePutArgs, stream: int = 0) -> dict:
        """Device-resident put call; returns the summary when done.  Raises ``EngineError`` (EINVAL) with
        ``summary`` for a refused input or a subscriber id not below ``sub_limit``."""
        return self._device(_lib.lib().emqx_pmqueue_put_batch_device, "emqx_pmqueue_put_batch_device", PUT_SUMMARY, args, stream)

    def take_device(self, args: PmqueueTakeArgs, stream: int = 0) -> dict:
        """Device-resident take; EOVERFLOW with ``summary["items"]`` the needed ``cap_out``."""
        return self._device(_lib.lib().emqx_pmqueue_take_batch_device, "emqx_pmqueue_take_batch_device", TAKE_SUMMARY, args, stream)

    def put_device_async(self, args: PmqueuePutArgs, summary: int, stream: int = 0) -> None:
        """Enqueues the call on ``stream`` and returns; ``summary`` (8 uint64, device or pinned) gets the
        summary words when the stream reaches it.  EOVERFLOW, nothing enqueued: the scratch
        :meth:`reserve` sized is too small."""
        check(_lib.lib().emqx_pmqueue_put_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_pmqueue_put_batch_device_async")

    def take_device_async(self, args: PmqueueTakeArgs, summary: int, stream: int = 0) -> None:
        check(_lib.lib().emqx_pmqueue_take_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_pmqueue_take_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_pmqueue_set_tuning(self._h, key.encode(), int(value)), "emqx_pmqueue_set_tuning")

    def stats(self) -> dict:
        s = PmqueueStats()
        check(_lib.lib().emqx_pmqueue_stats_get(self._h, ctypes.byref(s)), "emqx_pmqueue_stats_get")
        return s.as_dict()


def _ptr_fields(struct):
    return {k for k, t in struct._fields_ if t is ctypes.c_void_p}


_PUT_PTRS, _TAKE_PTRS = _ptr_fields(PmqueuePutArgs), _ptr_fields(PmqueueTakeArgs)

