"""A batch's deliveries grouped by subscriber, over the C ABI of include/emqx_inbox.h (reference:
apps/emqx/src/emqx_broker.erl:500-524 ``do_dispatch``, one ``{deliver, Topic, Msg}`` per delivery;
apps/emqx/src/emqx_connection.erl:505-509 and apps/emqx/src/emqx_misc.erl:158-172, the connection
draining them back into one list; apps/emqx/src/emqx_channel.erl:776-807 ``handle_deliver/2``,
which takes that list).

:class:`Inbox` transposes the message-major delivery CSR of the fan-out or of the enrich stage's
compacted form (``offsets[n+1]``, ``subs``, ``filters``, optionally ``opts`` and ``subids``) into a
subscriber-major one: ``inbox_subs[m]`` ascending, ``inbox_offsets[m+1]``, and per delivery, in the
stable order by subscriber, the message index, the filter word, the options byte, the subscription
identifier and the input position.  Inside an inbox the deliveries are in batch order.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from ._lib import EngineError, InboxBatch, InboxStats, check

__all__ = ["Inbox", "Grouped", "HOST_ONLY", "TILE", "SUMMARY", "passes"]

HOST_ONLY = -2
MAX_SUB_LIMIT = 1 << 32
# emqx_amd/csrc/inbox.h: IB_TILE = IB_BLOCK * IB_ROWS, deliveries per tile of every pass
BLOCK, ROWS = 256, 8
TILE = BLOCK * ROWS
# summary words
SUMMARY_WORDS = 8
SUMMARY = ("flags", "deliveries", "inboxes", "longest", "messages", "r5", "r6", "r7")
F_BOX_OVERFLOW, F_INPUT_REFUSED, F_BAD_SUB = 1, 2, 4


def passes(sub_limit: int) -> int:
    """Sort passes of a call (ib_passes): 8-bit digits of the key bits below ``sub_limit``, at least one."""
    bits = max(int(sub_limit) - 1, 0).bit_length()
    return max(1, -(-bits // 8))


class Grouped(NamedTuple):
    inbox_subs: np.ndarray     # uint32 [m], ascending
    inbox_offsets: np.ndarray  # uint64 [m + 1]
    msgs: np.ndarray           # uint32 per delivery: the message index
    filters: np.ndarray        # uint32 per delivery, SHARED / RETRY bits untouched
    opts: Optional[np.ndarray]
    subids: Optional[np.ndarray]
    src: Optional[np.ndarray]  # uint32 per delivery: its position in the input CSR
    summary: dict              # SUMMARY words


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def _summary(words) -> dict:
    return dict(zip(SUMMARY, map(int, words)))


class Inbox:
    """One inbox stage.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device
    (:meth:`group_host` only; the batch calls raise ``EMQX_EDEVICE``).  The calls of one handle
    share its scratch and run one after the other; concurrent callers take one handle each."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_inbox_create(device, ctypes.byref(h)), "emqx_inbox_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_inbox_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, cap_in: int, sub_limit: int) -> None:
        """Sizes the device scratch; the asynchronous form needs it done beforehand."""
        check(_lib.lib().emqx_inbox_reserve(self._h, int(cap_in), int(sub_limit)), "emqx_inbox_reserve")

    # ---- host buffers --------------------------------------------------------------------
    def _run(self, fn, name, offsets, subs, filters, sub_limit, opts, subids, want_src, cap_boxes, cap_in) -> Grouped:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        if off.size == 0:
            raise ValueError("offsets needs n + 1 entries")
        n = off.size - 1
        s, f = _u32(subs), _u32(filters)
        if s.size != f.size:
            raise ValueError("subs and filters differ in length")
        o = None if opts is None else np.ascontiguousarray(np.asarray(opts, dtype=np.uint8).reshape(-1))
        i = None if subids is None else _u32(subids)
        if (o is not None and o.size != s.size) or (i is not None and i.size != s.size):
            raise ValueError("opts / subids and subs differ in length")
        cap = s.size if cap_in is None else int(cap_in)
        boxes = min(cap, int(sub_limit)) if cap_boxes is None else int(cap_boxes)
        k = max(cap, 1)
        msgs, fils = np.zeros(k, dtype=np.uint32), np.zeros(k, dtype=np.uint32)
        bo = None if o is None else np.zeros(k, dtype=np.uint8)
        bi = None if i is None else np.zeros(k, dtype=np.uint32)
        src = np.zeros(k, dtype=np.uint32) if want_src else None
        isubs, ioff = np.zeros(max(boxes, 1), dtype=np.uint32), np.zeros(boxes + 1, dtype=np.uint64)
        b = InboxBatch(offsets=_p(off), subs=_p(s), filters=_p(f), opts=_p(o), subids=_p(i), n=n, cap_in=cap,
                       sub_limit=int(sub_limit), box_msgs=_p(msgs), box_filters=_p(fils), box_opts=_p(bo),
                       box_subids=_p(bi), box_src=_p(src), inbox_subs=_p(isubs), inbox_offsets=_p(ioff), cap_boxes=boxes)
        n_boxes = ctypes.c_uint64(0)
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), ctypes.byref(n_boxes), _p(summary))
        words = _summary(summary)
        total = min(words["deliveries"], cap)
        m = min(int(n_boxes.value), boxes)
        cut = lambda a: None if a is None else a[:total]  # noqa: E731
        got = Grouped(isubs[:m], ioff[:m + 1], msgs[:total], fils[:total], cut(bo), cut(bi), cut(src), words)
        if rc != 0:
            err = EngineError(rc, name)
            err.needed = int(n_boxes.value)
            err.summary = words
            err.partial = got  # EOVERFLOW: the box arrays are complete, the first cap_boxes inboxes
            raise err
        return got

    def group(self, offsets, subs, filters, sub_limit: int, opts=None, subids=None, src: bool = True,
              cap_boxes: Optional[int] = None, cap_in: Optional[int] = None) -> Grouped:
        """One device batch from host buffers (emqx_inbox_group_batch)."""
        return self._run(_lib.lib().emqx_inbox_group_batch, "emqx_inbox_group_batch", offsets, subs, filters, sub_limit,
                         opts, subids, src, cap_boxes, cap_in)

    def group_host(self, offsets, subs, filters, sub_limit: int, opts=None, subids=None, src: bool = True,
                   cap_boxes: Optional[int] = None, cap_in: Optional[int] = None) -> Grouped:
        """The same outputs computed on the CPU (per-call path, checker)."""
        return self._run(_lib.lib().emqx_inbox_group_host, "emqx_inbox_group_host", offsets, subs, filters, sub_limit,
                         opts, subids, src, cap_boxes, cap_in)

    # ---- device buffers ------------------------------------------------------------------
    @staticmethod
    def batch(d_offsets: int, d_subs: int, d_filters: int, n: int, cap_in: int, sub_limit: int, d_box_msgs: int,
              d_box_filters: int, d_inbox_subs: int, d_inbox_offsets: int, cap_boxes: int, d_opts: int = 0,
              d_subids: int = 0, d_box_opts: int = 0, d_box_subids: int = 0, d_box_src: int = 0) -> InboxBatch:
        """The argument block of the device forms from raw HIP pointers (``tensor.data_ptr()``; 0 = NULL)."""
        return InboxBatch(offsets=d_offsets or None, subs=d_subs or None, filters=d_filters or None, opts=d_opts or None,
                          subids=d_subids or None, n=n, cap_in=cap_in, sub_limit=sub_limit, box_msgs=d_box_msgs or None,
                          box_filters=d_box_filters or None, box_opts=d_box_opts or None, box_subids=d_box_subids or None,
                          box_src=d_box_src or None, inbox_subs=d_inbox_subs or None,
                          inbox_offsets=d_inbox_offsets or None, cap_boxes=cap_boxes)

    def group_device(self, batch: InboxBatch, stream: int = 0) -> dict:
        """Device-resident batch (:meth:`batch`); returns the summary when done.  Raises
        ``EngineError`` with ``needed`` and ``summary``: EOVERFLOW for more inboxes than
        ``cap_boxes``, EINVAL for a refused input or a subscriber at or above ``sub_limit``."""
        n_boxes = ctypes.c_uint64(0)
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = _lib.lib().emqx_inbox_group_batch_device(self._h, ctypes.byref(batch), ctypes.byref(n_boxes), _p(summary),
                                                      stream or None)
        if rc != 0:
            err = EngineError(rc, "emqx_inbox_group_batch_device")
            err.needed = int(n_boxes.value)
            err.summary = _summary(summary)
            raise err
        return _summary(summary)

    def group_device_async(self, batch: InboxBatch, summary: int, stream: int = 0) -> None:
        """Enqueues the batch on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the SUMMARY words when the stream reaches it.  EOVERFLOW, nothing enqueued: the
        scratch :meth:`reserve` sized is too small."""
        check(_lib.lib().emqx_inbox_group_batch_device_async(self._h, ctypes.byref(batch), summary, stream or None),
              "emqx_inbox_group_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_inbox_set_tuning(self._h, key.encode(), int(value)), "emqx_inbox_set_tuning")

    def stats(self) -> dict:
        s = InboxStats()
        check(_lib.lib().emqx_inbox_stats_get(self._h, ctypes.byref(s)), "emqx_inbox_stats_get")
        return s.as_dict()
