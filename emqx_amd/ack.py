"""Inflight slots and a batch of PUBACK / PUBREC / PUBCOMP per session, over the C ABI of
include/emqx_ack.h (reference: apps/emqx/src/emqx_session.erl:379-389 ``puback/2``, :404-414
``pubrec/2``, :437-447 ``pubcomp/2``, :453-477 ``dequeue/1``, :783-787 ``batch_n/1``, over
``emqx_inflight`` ``lookup/2``, ``update/3`` and ``delete/2``).

:class:`Ack` keeps nothing itself: the caller owns a table of :data:`SLOT` rows, ``W`` slots a
session, next to the window stage's session table.  :meth:`Ack.record` puts the sends of a window
call into the rows; :meth:`Ack.run` evaluates a batch of acks grouped by session against them and
returns a verdict byte and the message ref per ack, four counts per session (released, to_pubrel,
errors, room) and, with ``update_table``, the reopened window in the session table.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import AckRecordArgs, AckRunArgs, AckStats, EngineError, check
from .window import SESSION

__all__ = ["Ack", "Recorded", "Acked", "HOST_ONLY", "TILE", "SLOT", "pack_acks", "empty_slots"]

HOST_ONLY = -2
# emqx_amd/csrc/ack.h: AK_TILE = AK_BLOCK * AK_ROWS, acks or deliveries per tile
BLOCK, ROWS = 256, 4
TILE = BLOCK * ROWS
SUMMARY_WORDS = 8
RECORD_SUMMARY = ("flags", "deliveries", "inboxes", "sends", "recorded", "unrecorded", "full_rows", "reserved")
RUN_SUMMARY = ("flags", "acks", "sessions", "oks", "released", "in_use", "not_found", "rest")
F_INPUT_REFUSED, F_BAD_SUB, F_ROW_FULL = 2, 4, 8
# phase of a slot, kind of an ack, the verdict byte
EMPTY, MSG, PUBREL_AWAIT = 0, 1, 2
PUBACK, PUBREC, PUBCOMP = 1, 2, 3
A_OK, A_IN_USE, A_NOT_FOUND, A_NO_SESSION, A_PASS, A_BAD_KIND = 1, 2, 3, 4, 5, 6
NO_REF = 0xFFFFFFFF
DEFAULT_BATCH_N = 1000
MAX_ACKS = 1 << 31
WIDTHS = (8, 16, 32, 64)
COUNTS = ("released", "to_pubrel", "errors", "room")

# struct emqx_ack_slot
SLOT = np.dtype([("pkt_id", "<u2"), ("phase", "u1"), ("qos", "u1"), ("ref", "<u4")])
assert SLOT.itemsize == 8


def empty_slots(sub_limit: int, w: int) -> np.ndarray:
    """A slot table of ``sub_limit`` rows of ``w`` EMPTY slots."""
    return np.zeros((int(sub_limit), int(w)), dtype=SLOT)


def pack_acks(kinds, pkt_ids) -> np.ndarray:
    """``kind << 16 | pkt_id`` per ack."""
    return (np.asarray(kinds, dtype=np.uint32) << 16) | (np.asarray(pkt_ids, dtype=np.uint32) & 0xFFFF)


class Recorded(NamedTuple):
    unrecorded: np.ndarray  # uint32 [m]: the sends of each inbox its row had no empty slot for
    summary: dict           # RECORD_SUMMARY words


class Acked(NamedTuple):
    verdicts: np.ndarray  # uint8 per ack: A_*
    refs: np.ndarray      # uint32 per ack: the slot's ref of an A_OK, else NO_REF
    counts: np.ndarray    # uint32 [m, 4]: COUNTS
    summary: dict         # RUN_SUMMARY words


def _p(a):
    return None if a is None else a.ctypes.data


def _table(slots):
    if not isinstance(slots, np.ndarray) or slots.dtype != SLOT or slots.ndim != 2 or not slots.flags.c_contiguous:
        raise ValueError("slots is a contiguous [sub_limit, W] array of ack.SLOT (empty_slots)")
    return slots.shape


def _lists(subs, offsets):
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
    if off.size == 0:
        raise ValueError("offsets needs m + 1 entries")
    s = np.ascontiguousarray(np.asarray(subs, dtype=np.uint32).reshape(-1))
    if s.size != off.size - 1:
        raise ValueError("subs and offsets differ in length")
    return s, off


def _raise(rc, name, words, got):
    err = EngineError(rc, name)
    err.summary = words
    err.partial = got  # BAD_SUB: the outputs are complete
    raise err


class Ack:
    """One ack stage.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device (the
    ``_host`` calls only; the batch calls raise ``EMQX_EDEVICE``).  The calls of one handle share
    its scratch and run one after the other; concurrent callers take one handle each."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_ack_create(device, ctypes.byref(h)), "emqx_ack_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_ack_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, cap_in: int, cap_boxes: int, w: int) -> None:
        """Sizes the device scratch; the asynchronous forms need it done beforehand."""
        check(_lib.lib().emqx_ack_reserve(self._h, int(cap_in), int(cap_boxes), int(w)), "emqx_ack_reserve")

    # ---- host buffers --------------------------------------------------------------------
    def _record(self, fn, name, inbox_subs, inbox_offsets, box_opts, verdicts, pkt_ids, slots, refs) -> Recorded:
        subs, off = _lists(inbox_subs, inbox_offsets)
        m = subs.size
        sub_limit, w = _table(slots)
        opts = np.ascontiguousarray(np.asarray(box_opts, dtype=np.uint8).reshape(-1))
        ver = np.ascontiguousarray(np.asarray(verdicts, dtype=np.uint8).reshape(-1))
        ids = np.ascontiguousarray(np.asarray(pkt_ids, dtype=np.uint16).reshape(-1))
        rf = None if refs is None else np.ascontiguousarray(np.asarray(refs, dtype=np.uint32).reshape(-1))
        cap = opts.size
        if ver.size != cap or ids.size != cap or (rf is not None and rf.size != cap):
            raise ValueError("box_opts, verdicts, pkt_ids and refs differ in length")
        unrec = np.zeros(max(m, 1), dtype=np.uint32)
        b = AckRecordArgs(inbox_subs=_p(subs), inbox_offsets=_p(off), box_opts=_p(opts), n_boxes=None, m=m, cap_in=cap,
                          cap_boxes=m, verdicts=_p(ver), pkt_ids=_p(ids), refs=_p(rf), slots=_p(slots), w=w,
                          sub_limit=sub_limit, out_unrecorded=_p(unrec))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(RECORD_SUMMARY, map(int, summary)))
        got = Recorded(unrec[:0 if words["flags"] & F_INPUT_REFUSED else m], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def record(self, inbox_subs, inbox_offsets, box_opts, verdicts, pkt_ids, slots: np.ndarray, refs=None) -> Recorded:
        """The sends of a window call into ``slots`` (in place), evaluated on the device from host
        buffers (emqx_ack_record_batch).  ``refs``: the caller's name of each delivery's message;
        None: its position."""
        return self._record(_lib.lib().emqx_ack_record_batch, "emqx_ack_record_batch", inbox_subs, inbox_offsets, box_opts,
                            verdicts, pkt_ids, slots, refs)

    def record_host(self, inbox_subs, inbox_offsets, box_opts, verdicts, pkt_ids, slots: np.ndarray, refs=None) -> Recorded:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._record(_lib.lib().emqx_ack_record_host, "emqx_ack_record_host", inbox_subs, inbox_offsets, box_opts,
                            verdicts, pkt_ids, slots, refs)

    def _run(self, fn, name, ack_subs, ack_offsets, acks, sessions, slots, update_table) -> Acked:
        subs, off = _lists(ack_subs, ack_offsets)
        m = subs.size
        sub_limit, w = _table(slots)
        if not isinstance(sessions, np.ndarray) or sessions.dtype != SESSION or not sessions.flags.c_contiguous:
            raise ValueError("sessions is a contiguous array of window.SESSION records (pack_sessions)")
        if sessions.size != sub_limit:
            raise ValueError("sessions and slots differ in their number of subscribers")
        a = np.ascontiguousarray(np.asarray(acks, dtype=np.uint32).reshape(-1))
        cap = a.size
        ver, refs = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(cap, 1), dtype=np.uint32)
        cnt = np.zeros((max(m, 1), 4), dtype=np.uint32)
        b = AckRunArgs(ack_subs=_p(subs), ack_offsets=_p(off), acks=_p(a), n_boxes=None, m=m, cap_in=cap, cap_boxes=m,
                       sessions=_p(sessions), sub_limit=sub_limit, update_table=1 if update_table else 0, slots=_p(slots),
                       w=w, verdicts=_p(ver), out_refs=_p(refs), out_counts=_p(cnt))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(RUN_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        total = 0 if refused else min(words["acks"], cap)
        got = Acked(ver[:total], refs[:total], cnt[:0 if refused else m], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def run(self, ack_subs, ack_offsets, acks, sessions: np.ndarray, slots: np.ndarray, update_table: bool = False) -> Acked:
        """One batch of acks (:func:`pack_acks`) grouped by session, evaluated on the device from
        host buffers (emqx_ack_run_batch).  ``slots`` is rewritten in place; with ``update_table``
        so is ``sessions[...]["inflight"]``."""
        return self._run(_lib.lib().emqx_ack_run_batch, "emqx_ack_run_batch", ack_subs, ack_offsets, acks, sessions, slots,
                         update_table)

    def run_host(self, ack_subs, ack_offsets, acks, sessions: np.ndarray, slots: np.ndarray,
                 update_table: bool = False) -> Acked:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._run(_lib.lib().emqx_ack_run_host, "emqx_ack_run_host", ack_subs, ack_offsets, acks, sessions, slots,
                         update_table)

    # ---- device buffers ------------------------------------------------------------------
    @staticmethod
    def record_args(d_inbox_subs: int, d_inbox_offsets: int, d_box_opts: int, m: int, cap_in: int, cap_boxes: int,
                    d_verdicts: int, d_pkt_ids: int, d_slots: int, w: int, sub_limit: int, d_out_unrecorded: int,
                    d_refs: int = 0, d_n_boxes: int = 0) -> AckRecordArgs:
        """The argument block of the device forms of record from raw HIP pointers
        (``tensor.data_ptr()``; 0 = NULL): the window call's inputs and outputs, the slot table."""
        return AckRecordArgs(inbox_subs=d_inbox_subs or None, inbox_offsets=d_inbox_offsets or None,
                             box_opts=d_box_opts or None, n_boxes=d_n_boxes or None, m=m, cap_in=cap_in, cap_boxes=cap_boxes,
                             verdicts=d_verdicts or None, pkt_ids=d_pkt_ids or None, refs=d_refs or None,
                             slots=d_slots or None, w=w, sub_limit=sub_limit, out_unrecorded=d_out_unrecorded or None)

    @staticmethod
    def run_args(d_ack_subs: int, d_ack_offsets: int, d_acks: int, m: int, cap_in: int, cap_boxes: int, d_sessions: int,
                 sub_limit: int, d_slots: int, w: int, d_verdicts: int, d_out_refs: int, d_out_counts: int,
                 update_table: bool = False, d_n_boxes: int = 0) -> AckRunArgs:
        """The argument block of the device forms of run.  Behind the inbox stage grouping raw acks:
        its ``inbox_subs``, ``inbox_offsets``, ``box_filters`` and, as ``d_n_boxes``, its summary
        word 2 (``summary.data_ptr() + 16``)."""
        return AckRunArgs(ack_subs=d_ack_subs or None, ack_offsets=d_ack_offsets or None, acks=d_acks or None,
                          n_boxes=d_n_boxes or None, m=m, cap_in=cap_in, cap_boxes=cap_boxes, sessions=d_sessions or None,
                          sub_limit=sub_limit, update_table=1 if update_table else 0, slots=d_slots or None, w=w,
                          verdicts=d_verdicts or None, out_refs=d_out_refs or None, out_counts=d_out_counts or None)

    def _device(self, fn, name, names, args, stream):
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(args), _p(summary), stream or None)
        words = dict(zip(names, map(int, summary)))
        if rc != 0:
            err = EngineError(rc, name)
            err.summary = words
            raise err
        return words

    def record_device(self, args: AckRecordArgs, stream: int = 0) -> dict:
        """Device-resident record call; returns the summary when done.  Raises ``EngineError``
        (EINVAL) with ``summary`` for a refused input or a subscriber id not below ``sub_limit``."""
        return self._device(_lib.lib().emqx_ack_record_batch_device, "emqx_ack_record_batch_device", RECORD_SUMMARY, args, stream)

    def run_device(self, args: AckRunArgs, stream: int = 0) -> dict:
        return self._device(_lib.lib().emqx_ack_run_batch_device, "emqx_ack_run_batch_device", RUN_SUMMARY, args, stream)

    def record_device_async(self, args: AckRecordArgs, summary: int, stream: int = 0) -> None:
        """Enqueues the call on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the summary words when the stream reaches it.  EOVERFLOW, nothing enqueued: the
        scratch :meth:`reserve` sized is too small."""
        check(_lib.lib().emqx_ack_record_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_ack_record_batch_device_async")

    def run_device_async(self, args: AckRunArgs, summary: int, stream: int = 0) -> None:
        check(_lib.lib().emqx_ack_run_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_ack_run_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_ack_set_tuning(self._h, key.encode(), int(value)), "emqx_ack_set_tuning")

    def stats(self) -> dict:
        s = AckStats()
        check(_lib.lib().emqx_ack_stats_get(self._h, ctypes.byref(s)), "emqx_ack_stats_get")
        return s.as_dict()
