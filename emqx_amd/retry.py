"""Inflight ages, redelivery lists and retry timers per session, over the C ABI of
include/emqx_retry.h (reference: apps/emqx/src/emqx_session.erl:612-651 ``retry/1`` and
``retry_delivery``, :692-703 ``replay/1``, :780-792 ``sort_fun/0``, ``with_ts/1``, ``age/2``;
apps/emqx/src/emqx_message.erl:239-243 ``is_expired/1``).

:class:`Retry` keeps nothing itself: next to the ack stage's slot table the caller owns a table of
stamps (:func:`empty_stamps`), one ``uint64`` a slot.  :meth:`Retry.stamp` runs behind every record
and run call of the ack stage and notes when each entry went in; :meth:`Retry.sweep` answers
``retry/1`` (or, with ``mode=MODE_REPLAY``, ``replay/1``) for a list of sessions or the whole table:
the items to send again in the reference's order, the expired messages, four counts and the next
timer per session.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import EngineError, RetryStampArgs, RetryStats, RetrySweepArgs, check
from .ack import SLOT
from .window import SESSION

__all__ = ["Retry", "Stamped", "Swept", "HOST_ONLY", "ITEM", "empty_stamps", "pack_stamp", "stamp_fields", "deadline"]

HOST_ONLY = -2
SUMMARY_WORDS = 8
STAMP_SUMMARY = ("flags", "rows", "named", "stamped", "cleared", "reserved5", "reserved6", "reserved7")
SWEEP_SUMMARY = ("flags", "ok_sessions", "sessions", "items", "publishes", "pubrels", "expired", "unstamped")
F_INPUT_REFUSED, F_BAD_SUB, F_OUTPUT_FULL, F_BAD_REF, F_UNSTAMPED = 2, 4, 8, 0x10, 0x20
MODE_RETRY, MODE_REPLAY = 0, 1
PUBLISH_DUP, PUBREL, EXPIRED = 1, 2, 3
NO_TIMER = 0xFFFFFFFF
NO_EXPIRY = 0xFFFFFFFFFFFFFFFF
MAX_INTERVAL = 1 << 31
MAX_NOW = 1 << 45
STAMP_TS_SHIFT, STAMP_DUP, STAMP_PHASE_SHIFT = 19, 1 << 18, 16
COUNTS = ("publishes", "pubrels", "expired", "inflight_after")

# struct emqx_retry_item
ITEM = np.dtype([("pkt_id", "<u2"), ("kind", "u1"), ("qos", "u1"), ("ref", "<u4")])
assert ITEM.itemsize == 8


def empty_stamps(sub_limit: int, w: int) -> np.ndarray:
    """A stamp table of ``sub_limit`` rows of ``w`` zero stamps."""
    return np.zeros((int(sub_limit), int(w)), dtype=np.uint64)


def pack_stamp(ts_ms: int, dup: int, phase: int, pkt_id: int) -> int:
    """``ts_ms << 19 | dup << 18 | phase << 16 | pkt_id``."""
    return (int(ts_ms) << STAMP_TS_SHIFT) | (STAMP_DUP if dup else 0) | ((int(phase) & 3) << STAMP_PHASE_SHIFT) | (int(pkt_id) & 0xFFFF)


def stamp_fields(stamp: int):
    """``(ts_ms, dup, phase, pkt_id)`` of a stamp."""
    s = int(stamp)
    return s >> STAMP_TS_SHIFT, (s >> 18) & 1, (s >> STAMP_PHASE_SHIFT) & 3, s & 0xFFFF


def deadline(created_ms: int, interval_s) -> int:
    """The entry of ``deadlines[]`` of a message created at ``created_ms`` with a Message-Expiry-
    Interval of ``interval_s`` seconds (None: it never expires): ``is_expired/1`` is
    ``now > deadline``."""
    return NO_EXPIRY if interval_s is None else int(created_ms) + int(interval_s) * 1000


class Stamped(NamedTuple):
    summary: dict  # STAMP_SUMMARY words


class Swept(NamedTuple):
    offsets: np.ndarray  # uint64 [m + 1]: session k's items are items[offsets[k]:offsets[k + 1]]
    items: np.ndarray    # ITEM per item (empty when the call was full)
    status: np.ndarray   # uint8 [m]: ack.A_OK / A_NO_SESSION / A_PASS
    counts: np.ndarray   # uint32 [m, 4]: COUNTS
    timers: np.ndarray   # uint32 [m]: ms until the next retry, NO_TIMER
    summary: dict        # SWEEP_SUMMARY words


def _p(a):
    return None if a is None else a.ctypes.data


def _tables(slots, stamps, need_stamps=True):
    if not isinstance(slots, np.ndarray) or slots.dtype != SLOT or slots.ndim != 2 or not slots.flags.c_contiguous:
        raise ValueError("slots is a contiguous [sub_limit, W] array of ack.SLOT (ack.empty_slots)")
    if stamps is None and not need_stamps:
        return slots.shape
    if (not isinstance(stamps, np.ndarray) or stamps.dtype != np.uint64 or stamps.shape != slots.shape
            or not stamps.flags.c_contiguous):
        raise ValueError("stamps is a contiguous uint64 array of the shape of slots (empty_stamps)")
    return slots.shape


def _raise(rc, name, words, got):
    err = EngineError(rc, name)
    err.summary = words
    err.partial = got  # BAD_SUB and OUTPUT_FULL: what the contract calls complete is
    raise err


class Retry:
    """One retry stage.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device (the
    ``_host`` calls only; the batch calls raise ``EMQX_EDEVICE``).  The calls of one handle share
    its scratch and run one after the other; concurrent callers take one handle each."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_retry_create(device, ctypes.byref(h)), "emqx_retry_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_retry_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, cap_boxes: int, w: int) -> None:
        """Sizes the device scratch; the asynchronous forms need it done beforehand."""
        check(_lib.lib().emqx_retry_reserve(self._h, int(cap_boxes), int(w)), "emqx_retry_reserve")

    # ---- host buffers --------------------------------------------------------------------
    def _stamp(self, fn, name, subs, slots, stamps, now_ms) -> Stamped:
        sub_limit, w = _tables(slots, stamps)
        s = None if subs is None else np.ascontiguousarray(np.asarray(subs, dtype=np.uint32).reshape(-1))
        m = sub_limit if s is None else s.size
        b = RetryStampArgs(subs=_p(s), n_boxes=None, m=m, cap_boxes=m, slots=_p(slots), stamps=_p(stamps), w=w,
                           sub_limit=sub_limit, now_ms=int(now_ms))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(STAMP_SUMMARY, map(int, summary)))
        got = Stamped(words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def stamp(self, subs, slots: np.ndarray, stamps: np.ndarray, now_ms: int) -> Stamped:
        """Behind every ``Ack.record`` and ``Ack.run``: the stamps of the rows ``subs`` names (None:
        every row) brought in line with ``slots`` at ``now_ms`` (in place), evaluated on the device
        from host buffers (emqx_retry_stamp_batch)."""
        return self._stamp(_lib.lib().emqx_retry_stamp_batch, "emqx_retry_stamp_batch", subs, slots, stamps, now_ms)

    def stamp_host(self, subs, slots: np.ndarray, stamps: np.ndarray, now_ms: int) -> Stamped:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._stamp(_lib.lib().emqx_retry_stamp_host, "emqx_retry_stamp_host", subs, slots, stamps, now_ms)

    def _sweep(self, fn, name, subs, sessions, slots, stamps, now_ms, interval_ms, intervals, deadlines, mode, cap_out,
               update_table) -> Swept:
        sub_limit, w = _tables(slots, stamps, need_stamps=mode != MODE_REPLAY)
        if not isinstance(sessions, np.ndarray) or sessions.dtype != SESSION or not sessions.flags.c_contiguous:
            raise ValueError("sessions is a contiguous array of window.SESSION records (pack_sessions)")
        if sessions.size != sub_limit:
            raise ValueError("sessions and slots differ in their number of subscribers")
        s = None if subs is None else np.ascontiguousarray(np.asarray(subs, dtype=np.uint32).reshape(-1))
        m = sub_limit if s is None else s.size
        iv = None if intervals is None else np.ascontiguousarray(np.asarray(intervals, dtype=np.uint32).reshape(-1))
        if iv is not None and iv.size != sub_limit:
            raise ValueError("intervals has one entry a session")
        dl = None if deadlines is None else np.ascontiguousarray(np.asarray(deadlines, dtype=np.uint64).reshape(-1))
        cap = m * w if cap_out is None else int(cap_out)
        off = np.zeros(m + 1, dtype=np.uint64)
        items = np.zeros(max(cap, 1), dtype=ITEM)
        status, timers = np.zeros(max(m, 1), dtype=np.uint8), np.zeros(max(m, 1), dtype=np.uint32)
        cnt = np.zeros((max(m, 1), 4), dtype=np.uint32)
        b = RetrySweepArgs(subs=_p(s), n_boxes=None, m=m, cap_boxes=m, sessions=_p(sessions), sub_limit=sub_limit,
                           update_table=1 if update_table else 0, slots=_p(slots), stamps=_p(stamps), w=w, now_ms=int(now_ms),
                           interval_ms=int(interval_ms), intervals=_p(iv), deadlines=_p(dl), ref_limit=0 if dl is None else dl.size,
                           mode=mode, cap_out=cap, out_offsets=_p(off), out_items=_p(items), out_status=_p(status),
                           out_counts=_p(cnt), out_timers=_p(timers))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(SWEEP_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        full = words["flags"] & F_OUTPUT_FULL
        k = 0 if refused else m
        got = Swept(off[:k + 1 if not refused else 0], items[:0 if (refused or full) else min(words["items"], cap)], status[:k],
                    cnt[:k], timers[:k], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def sweep(self, subs, sessions: np.ndarray, slots: np.ndarray, stamps, now_ms: int, interval_ms: int = 0, intervals=None,
              deadlines=None, mode: int = MODE_RETRY, cap_out=None, update_table: bool = False) -> Swept:
        """``retry/1`` (``mode=MODE_REPLAY``: ``replay/1``) of the sessions ``subs`` names (None: the
        whole table) at ``now_ms``, evaluated on the device from host buffers
        (emqx_retry_sweep_batch).  ``slots`` and ``stamps`` are rewritten in place; with
        ``update_table`` so is ``sessions[...]["inflight"]``.  ``cap_out`` None: room for every
        slot.  A call that is full raises ``EngineError`` (EOVERFLOW) with ``partial`` and
        ``summary["items"]`` the capacity it needs; nothing was changed."""
        return self._sweep(_lib.lib().emqx_retry_sweep_batch, "emqx_retry_sweep_batch", subs, sessions, slots, stamps, now_ms,
                           interval_ms, intervals, deadlines, mode, cap_out, update_table)

    def sweep_host(self, subs, sessions: np.ndarray, slots: np.ndarray, stamps, now_ms: int, interval_ms: int = 0, intervals=None,
                   deadlines=None, mode: int = MODE_RETRY, cap_out=None, update_table: bool = False) -> Swept:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._sweep(_lib.lib().emqx_retry_sweep_host, "emqx_retry_sweep_host", subs, sessions, slots, stamps, now_ms,
                           interval_ms, intervals, deadlines, mode, cap_out, update_table)

    # ---- device buffers ------------------------------------------------------------------
    @staticmethod
    def stamp_args(d_subs: int, m: int, cap_boxes: int, d_slots: int, d_stamps: int, w: int, sub_limit: int, now_ms: int,
                   d_n_boxes: int = 0) -> RetryStampArgs:
        """The argument block of the device forms of stamp from raw HIP pointers
        (``tensor.data_ptr()``; 0 = NULL): the record or run call's subscriber list and count."""
        return RetryStampArgs(subs=d_subs or None, n_boxes=d_n_boxes or None, m=m, cap_boxes=cap_boxes, slots=d_slots or None,
                              stamps=d_stamps or None, w=w, sub_limit=sub_limit, now_ms=now_ms)

    @staticmethod
    def sweep_args(d_subs: int, m: int, cap_boxes: int, d_sessions: int, sub_limit: int, d_slots: int, d_stamps: int, w: int,
                   now_ms: int, interval_ms: int, cap_out: int, d_out_offsets: int, d_out_items: int, d_out_status: int,
                   d_out_counts: int, d_out_timers: int, d_intervals: int = 0, d_deadlines: int = 0, ref_limit: int = 0,
                   mode: int = MODE_RETRY, update_table: bool = False, d_n_boxes: int = 0) -> RetrySweepArgs:
        """The argument block of the device forms of sweep."""
        return RetrySweepArgs(subs=d_subs or None, n_boxes=d_n_boxes or None, m=m, cap_boxes=cap_boxes,
                              sessions=d_sessions or None, sub_limit=sub_limit, update_table=1 if update_table else 0,
                              slots=d_slots or None, stamps=d_stamps or None, w=w, now_ms=now_ms, interval_ms=interval_ms,
                              intervals=d_intervals or None, deadlines=d_deadlines or None, ref_limit=ref_limit, mode=mode,
                              cap_out=cap_out, out_offsets=d_out_offsets or None, out_items=d_out_items or None,
                              out_status=d_out_status or None, out_counts=d_out_counts or None, out_timers=d_out_timers or None)

    def _device(self, fn, name, names, args, stream):
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(args), _p(summary), stream or None)
        words = dict(zip(names, map(int, summary)))
        if rc != 0:
            err = EngineError(rc, name)
            err.summary = words
            raise err
        return words

    def stamp_device(self, args: RetryStampArgs, stream: int = 0) -> dict:
        """Device-resident stamp call; returns the summary when done.  Raises ``EngineError``
        (EINVAL) with ``summary`` for a refused input or a subscriber id not below ``sub_limit``."""
        return self._device(_lib.lib().emqx_retry_stamp_batch_device, "emqx_retry_stamp_batch_device", STAMP_SUMMARY, args, stream)

    def sweep_device(self, args: RetrySweepArgs, stream: int = 0) -> dict:
        """Device-resident sweep; EOVERFLOW with ``summary["items"]`` the needed ``cap_out``."""
        return self._device(_lib.lib().emqx_retry_sweep_batch_device, "emqx_retry_sweep_batch_device", SWEEP_SUMMARY, args, stream)

    def stamp_device_async(self, args: RetryStampArgs, summary: int, stream: int = 0) -> None:
        """Enqueues the call on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the summary words when the stream reaches it.  EOVERFLOW, nothing enqueued: the
        scratch :meth:`reserve` sized is too small."""
        check(_lib.lib().emqx_retry_stamp_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_retry_stamp_batch_device_async")

    def sweep_device_async(self, args: RetrySweepArgs, summary: int, stream: int = 0) -> None:
        check(_lib.lib().emqx_retry_sweep_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_retry_sweep_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_retry_set_tuning(self._h, key.encode(), int(value)), "emqx_retry_set_tuning")

    def stats(self) -> dict:
        s = RetryStats()
        check(_lib.lib().emqx_retry_stats_get(self._h, ctypes.byref(s)), "emqx_retry_stats_get")
        return s.as_dict()
