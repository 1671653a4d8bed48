"""Inflight and mqueue admission per inbox, over the C ABI of include/emqx_window.h (reference:
apps/emqx/src/emqx_session.erl:483-536 ``deliver/2``, ``deliver_msg/2`` and ``enqueue/2``;
apps/emqx/src/emqx_inflight.erl:84-87 ``is_full/1``; apps/emqx/src/emqx_mqueue.erl:159-179
``in/2``; apps/emqx/src/emqx_channel.erl:791-814, which picks between them).

:class:`Window` takes the inbox stage's output (``inbox_subs[m]``, ``inbox_offsets[m+1]``,
``box_opts``) and a table of 32-byte session records indexed by subscriber id (:data:`SESSION`,
:func:`pack_sessions`) and decides every delivery of every inbox: send without a packet id, send
with the next packet id, queue, or drop.  Per delivery it returns a verdict byte and a packet id,
per inbox the record after the batch and four counts.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import EngineError, WindowBatch, WindowStats, check

__all__ = ["Window", "Admitted", "HOST_ONLY", "TILE", "SUMMARY", "SESSION", "pack_sessions"]

HOST_ONLY = -2
# emqx_amd/csrc/window.h: WN_TILE = WN_BLOCK * WN_ROWS, deliveries per tile
BLOCK, ROWS = 256, 8
TILE = BLOCK * ROWS
SUMMARY_WORDS = 8
SUMMARY = ("flags", "deliveries", "inboxes", "sends", "sends_qos0", "queued", "drops", "id_wrapped")
F_INPUT_REFUSED, F_BAD_SUB = 2, 4
# the verdict byte
W_SEND_QOS0, W_SEND, W_QUEUED, W_QUEUED_DROPPED, W_DROP_QOS0 = 1, 2, 3, 4, 5
W_SKIP_NO_LOCAL, W_BAD_MESSAGE, W_NO_SESSION, W_PASS = 6, 7, 8, 9
W_VERDICT_MASK, W_EVICTS = 0x0F, 0x80
# flags of a session record
PRESENT, CONNECTED, STORE_QOS0, PASS = 1, 2, 4, 8
COUNTS = ("sends", "sends_qos0", "queued", "evicted_old")

# struct emqx_window_session
SESSION = np.dtype([("inflight", "<u4"), ("inflight_max", "<u4"), ("mq_len", "<u4"), ("mq_max", "<u4"),
                    ("next_pkt_id", "<u4"), ("flags", "<u4"), ("dropped", "<u8")])
assert SESSION.itemsize == 32


def pack_sessions(n: int, inflight=0, inflight_max=32, mq_len=0, mq_max=1000, next_pkt_id=1,
                  flags=PRESENT | CONNECTED, dropped=0) -> np.ndarray:
    """A table of ``n`` session records from columns (scalars or arrays of length ``n``); the
    defaults are EMQX's: a connected session, ``max_inflight`` 32, ``max_mqueue_len`` 1000."""
    t = np.zeros(int(n), dtype=SESSION)
    for name, col in (("inflight", inflight), ("inflight_max", inflight_max), ("mq_len", mq_len), ("mq_max", mq_max),
                      ("next_pkt_id", next_pkt_id), ("flags", flags), ("dropped", dropped)):
        t[name] = col
    return t


class Admitted(NamedTuple):
    verdicts: np.ndarray      # uint8 per delivery: W_*, W_EVICTS or-ed in
    pkt_ids: np.ndarray       # uint16 per delivery: the packet id of a W_SEND, else 0
    out_sessions: np.ndarray  # SESSION [m]: the records after the batch
    counts: np.ndarray        # uint32 [m, 4]: COUNTS
    summary: dict             # SUMMARY words


def _p(a):
    return None if a is None else a.ctypes.data


def _summary(words) -> dict:
    return dict(zip(SUMMARY, map(int, words)))


class Window:
    """One window stage.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device
    (:meth:`run_host` only; the batch calls raise ``EMQX_EDEVICE``).  The calls of one handle share
    its scratch and run one after the other; concurrent callers take one handle each."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_window_create(device, ctypes.byref(h)), "emqx_window_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_window_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, cap_in: int, cap_boxes: int) -> None:
        """Sizes the device scratch; the asynchronous form needs it done beforehand."""
        check(_lib.lib().emqx_window_reserve(self._h, int(cap_in), int(cap_boxes)), "emqx_window_reserve")

    # ---- host buffers --------------------------------------------------------------------
    def _run(self, fn, name, inbox_subs, inbox_offsets, box_opts, sessions, update_table) -> Admitted:
        off = np.ascontiguousarray(np.asarray(inbox_offsets, dtype=np.uint64).reshape(-1))
        if off.size == 0:
            raise ValueError("inbox_offsets needs m + 1 entries")
        m = off.size - 1
        subs = np.ascontiguousarray(np.asarray(inbox_subs, dtype=np.uint32).reshape(-1))
        if subs.size != m:
            raise ValueError("inbox_subs and inbox_offsets differ in length")
        opts = np.ascontiguousarray(np.asarray(box_opts, dtype=np.uint8).reshape(-1))
        if not isinstance(sessions, np.ndarray) or sessions.dtype != SESSION or not sessions.flags.c_contiguous:
            raise ValueError("sessions is a contiguous array of window.SESSION records (pack_sessions)")
        cap = opts.size
        ver, ids = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(cap, 1), dtype=np.uint16)
        recs, cnt = np.zeros(max(m, 1), dtype=SESSION), np.zeros((max(m, 1), 4), dtype=np.uint32)
        b = WindowBatch(inbox_subs=_p(subs), inbox_offsets=_p(off), box_opts=_p(opts), n_boxes=None, m=m, cap_in=cap,
                        cap_boxes=m, sessions=_p(sessions), sub_limit=sessions.size, update_table=1 if update_table else 0,
                        verdicts=_p(ver), pkt_ids=_p(ids), out_sessions=_p(recs), out_counts=_p(cnt))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = _summary(summary)
        total = 0 if words["flags"] & F_INPUT_REFUSED else min(words["deliveries"], cap)
        got = Admitted(ver[:total], ids[:total], recs[:m], cnt[:m], words)
        if rc != 0:
            err = EngineError(rc, name)
            err.summary = words
            err.partial = got  # BAD_SUB: the outputs are complete, the inbox of a bad id is W_NO_SESSION
            raise err
        return got

    def run(self, inbox_subs, inbox_offsets, box_opts, sessions: np.ndarray, update_table: bool = False) -> Admitted:
        """One device batch from host buffers (emqx_window_run_batch).  ``sessions``: the table,
        indexed by subscriber id; with ``update_table`` the records after the batch replace the
        entries of the inboxes' sessions in it."""
        return self._run(_lib.lib().emqx_window_run_batch, "emqx_window_run_batch", inbox_subs, inbox_offsets, box_opts,
                         sessions, update_table)

    def run_host(self, inbox_subs, inbox_offsets, box_opts, sessions: np.ndarray, update_table: bool = False) -> Admitted:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._run(_lib.lib().emqx_window_run_host, "emqx_window_run_host", inbox_subs, inbox_offsets, box_opts,
                         sessions, update_table)

    # ---- device buffers ------------------------------------------------------------------
    @staticmethod
    def batch(d_inbox_subs: int, d_inbox_offsets: int, d_box_opts: int, m: int, cap_in: int, cap_boxes: int,
              d_sessions: int, sub_limit: int, d_verdicts: int, d_pkt_ids: int, d_out_sessions: int, d_out_counts: int,
              update_table: bool = False, d_n_boxes: int = 0) -> WindowBatch:
        """The argument block of the device forms from raw HIP pointers (``tensor.data_ptr()``;
        0 = NULL).  ``d_n_boxes``: where the device reads the inbox count (the inbox stage's summary
        word 2: ``summary.data_ptr() + 16``); ``m`` is ignored then."""
        return WindowBatch(inbox_subs=d_inbox_subs or None, inbox_offsets=d_inbox_offsets or None,
                           box_opts=d_box_opts or None, n_boxes=d_n_boxes or None, m=m, cap_in=cap_in, cap_boxes=cap_boxes,
                           sessions=d_sessions or None, sub_limit=sub_limit, update_table=1 if update_table else 0,
                           verdicts=d_verdicts or None, pkt_ids=d_pkt_ids or None, out_sessions=d_out_sessions or None,
                           out_counts=d_out_counts or None)

    def run_device(self, batch: WindowBatch, stream: int = 0) -> dict:
        """Device-resident batch (:meth:`batch`); returns the summary when done.  Raises
        ``EngineError`` (EINVAL) with ``summary`` for a refused input or an inbox whose subscriber
        id is not below ``sub_limit``."""
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = _lib.lib().emqx_window_run_batch_device(self._h, ctypes.byref(batch), _p(summary), stream or None)
        if rc != 0:
            err = EngineError(rc, "emqx_window_run_batch_device")
            err.summary = _summary(summary)
            raise err
        return _summary(summary)

    def run_device_async(self, batch: WindowBatch, summary: int, stream: int = 0) -> None:
        """Enqueues the batch on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the SUMMARY words when the stream reaches it.  EOVERFLOW, nothing enqueued: the
        scratch :meth:`reserve` sized is too small."""
        check(_lib.lib().emqx_window_run_batch_device_async(self._h, ctypes.byref(batch), summary, stream or None),
              "emqx_window_run_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_window_set_tuning(self._h, key.encode(), int(value)), "emqx_window_set_tuning")

    def stats(self) -> dict:
        s = WindowStats()
        check(_lib.lib().emqx_window_stats_get(self._h, ctypes.byref(s)), "emqx_window_stats_get")
        return s.as_dict()
