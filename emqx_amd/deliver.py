"""Delivery options behind the publish fan-out: No Local, the granted QoS, Retain As Published
and the Subscription Identifier per delivery, over the C ABI of include/emqx_deliver.h
(reference: apps/emqx/src/emqx_session.erl:280-291 ``ignore_local/3``, :554-598 ``enrich_fun/1``,
``get_subopts/2``, ``enrich_subopts/3``).

:class:`SubOpts` holds the subscription options keyed by the ordered pair (filter id, subscriber
id), commits them as one immutable hash table and answers delivery CSRs as the fan-out writes
them (``offsets[n+1]``, ``subs``, ``filters`` with the SHARED / RETRY bits) plus per-message
``qos``, ``flags`` (bit 0 retain, bit 1 ``headers.retained``) and ``from`` with one options byte
and one subscription identifier per delivery, optionally with the CSR compacted of the No Local
drops.  The predicate is reported per delivery (``ignore_local`` of a one-element list); the
compacted form drops every hit, as MQTT 5 section 3.8.3.1 requires.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import DeliverBatch, EngineError, SubOptsStats, check

__all__ = ["SubOpts", "Enriched", "Kept", "HOST_ONLY", "NO_SENDER", "subopts_word", "decode"]

HOST_ONLY = -2
NO_SENDER = 0xFFFFFFFF
MAX_SUBID = 268435455
# stored options word
OPT_NL, OPT_RAP, OPT_UPGRADE_QOS, OPT_HAS_SUBID = 0x04, 0x08, 0x10, 0x20
# msg_flags
MSG_RETAIN, MSG_RETAINED = 0x01, 0x02
# output byte
OUT_RETAIN, OUT_NL, OUT_DROP_NO_LOCAL, OUT_NO_SUBOPTS, OUT_BAD_MESSAGE = 0x04, 0x08, 0x10, 0x20, 0x40
# summary words
SUMMARY_WORDS = 8
SUMMARY = ("flags", "deliveries", "kept", "dropped_no_local", "no_subopts", "qos0", "qos1", "qos2")
F_KEPT_OVERFLOW, F_INPUT_REFUSED = 1, 2


def subopts_word(qos: int = 0, nl: int = 0, rap: int = 0, upgrade_qos: bool = False, subid: Optional[int] = None) -> int:
    """The stored options word of emqx_types:subopts() (+ the zone's upgrade_qos)."""
    return ((int(qos) & 3) | (OPT_NL if nl else 0) | (OPT_RAP if rap else 0) | (OPT_UPGRADE_QOS if upgrade_qos else 0) |
            (OPT_HAS_SUBID if subid is not None else 0))


def decode(opt: int, subid: int = 0):
    """An output byte as (qos, retain, nl, subid or None); bad messages and drops are the caller's to test."""
    return (opt & 3, bool(opt & OUT_RETAIN), bool(opt & OUT_NL), subid or None)


class Kept(NamedTuple):
    offsets: np.ndarray
    subs: np.ndarray
    filters: np.ndarray
    opts: np.ndarray
    subids: np.ndarray


class Enriched(NamedTuple):
    opts: np.ndarray      # uint8 per delivery
    subids: np.ndarray    # uint32 per delivery, 0: none
    summary: dict         # SUMMARY words
    kept: Optional[Kept]  # the CSR without the No Local drops (compact=True)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))


def _u8(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint8).reshape(-1))


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def _per_key(x, n: int, dtype) -> np.ndarray:
    a = np.asarray(x, dtype=dtype)
    return np.ascontiguousarray(np.broadcast_to(a, (n,)) if a.ndim == 0 else a.reshape(-1))


class SubOpts:
    """One delivery-options table.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no
    device (changes, commit and :meth:`enrich_host` only; the batch calls raise ``EMQX_EDEVICE``)."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_subopts_create(device, ctypes.byref(h)), "emqx_subopts_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_subopts_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- changes -------------------------------------------------------------------------
    def set_words(self, filters, subs, words, subids=None) -> None:
        """emqx_subopts_set with ready options words (``subopts_word``)."""
        f, s, w = _u32(filters), _u32(subs), _u8(words)
        if not (f.size == s.size == w.size):
            raise ValueError("filters, subs and words differ in length")
        i = None if subids is None else _u32(subids)
        check(_lib.lib().emqx_subopts_set(self._h, _p(f), _p(s), _p(w), _p(i), f.size), "emqx_subopts_set")

    def set(self, filters, subs, qos=0, nl=0, rap=0, upgrade_qos=False, subid=None) -> None:
        """Upsert (maps:put in emqx_session:subscribe/4).  Every option is a scalar or one value
        per pair; ``subid``: None, a scalar, or per pair with 0 / None for "none"."""
        f = _u32(filters)
        n = f.size
        w = (_per_key(qos, n, np.uint8) & 3) | np.where(_per_key(nl, n, np.uint8) != 0, OPT_NL, 0).astype(np.uint8)
        w |= np.where(_per_key(rap, n, np.uint8) != 0, OPT_RAP, 0).astype(np.uint8)
        w |= np.where(_per_key(upgrade_qos, n, np.uint8) != 0, OPT_UPGRADE_QOS, 0).astype(np.uint8)
        # qos 3 must reach the library to be rejected there, not be masked away here
        w = np.where(_per_key(qos, n, np.int64) > 2, np.uint8(3), w).astype(np.uint8)
        ids = None
        if subid is not None:
            if isinstance(subid, (int, np.integer)):
                ids = np.full(n, int(subid), dtype=np.uint32)
                w |= np.uint8(OPT_HAS_SUBID)
            else:
                ids = subid.astype(np.uint32) if isinstance(subid, np.ndarray) else \
                    np.array([0 if x is None else int(x) for x in subid], dtype=np.uint32)
                w |= np.where(ids != 0, OPT_HAS_SUBID, 0).astype(np.uint8)
        self.set_words(f, subs, w, ids)

    def remove(self, filters, subs) -> None:
        f, s = _u32(filters), _u32(subs)
        if f.size != s.size:
            raise ValueError("filters and subs differ in length")
        check(_lib.lib().emqx_subopts_remove(self._h, _p(f), _p(s), f.size), "emqx_subopts_remove")

    def drop_subscribers(self, subs) -> None:
        s = _u32(subs)
        check(_lib.lib().emqx_subopts_drop_subscribers(self._h, _p(s), s.size), "emqx_subopts_drop_subscribers")

    def commit(self) -> None:
        check(_lib.lib().emqx_subopts_commit(self._h), "emqx_subopts_commit")

    # ---- enrich --------------------------------------------------------------------------
    def _run(self, fn, name, offsets, subs, filters, qos, flags, frm, compact, cap_kept) -> Enriched:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        if off.size == 0:
            raise ValueError("offsets needs n + 1 entries")
        n = off.size - 1
        s, f, q, fl = _u32(subs), _u32(filters), _u8(qos), _u8(flags)
        if s.size != f.size or q.size != n or fl.size != n:
            raise ValueError("the CSR and the message attributes differ in length")
        fr = None if frm is None else _u32(frm)
        total = s.size
        opts = np.zeros(max(total, 1), dtype=np.uint8)
        subids = np.zeros(max(total, 1), dtype=np.uint32)
        b = DeliverBatch(offsets=_p(off), subs=_p(s), filters=_p(f), n=n, cap_in=total, msg_qos=_p(q), msg_flags=_p(fl),
                         msg_from=_p(fr), out_opts=_p(opts), out_subids=_p(subids))
        keep = None
        if compact:
            cap = total if cap_kept is None else int(cap_kept)
            keep = (np.zeros(n + 1, dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint32),
                    np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint8),
                    np.zeros(max(cap, 1), dtype=np.uint32))
            b.kept_offsets, b.kept_subs, b.kept_filters, b.kept_opts, b.kept_subids = (_p(x) for x in keep)
            b.cap_kept = cap
        n_kept = ctypes.c_uint64(0)
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), ctypes.byref(n_kept), _p(summary))
        if rc == _lib.EMQX_EOVERFLOW:
            err = EngineError(rc, name)
            err.needed = int(n_kept.value)
            err.kept_offsets = keep[0]
            err.summary = dict(zip(SUMMARY, map(int, summary)))
            raise err
        check(rc, name)
        k = int(n_kept.value)
        return Enriched(opts[:total], subids[:total], dict(zip(SUMMARY, map(int, summary))),
                        None if keep is None else Kept(keep[0], keep[1][:k], keep[2][:k], keep[3][:k], keep[4][:k]))

    def enrich_packed(self, offsets, subs, filters, qos, flags, frm=None, compact: bool = False,
                      cap_kept: Optional[int] = None) -> Enriched:
        """One device batch from host buffers (emqx_deliver_enrich_batch)."""
        return self._run(_lib.lib().emqx_deliver_enrich_batch, "emqx_deliver_enrich_batch", offsets, subs, filters, qos,
                         flags, frm, compact, cap_kept)

    def enrich_host(self, offsets, subs, filters, qos, flags, frm=None, compact: bool = False,
                    cap_kept: Optional[int] = None) -> Enriched:
        """The same outputs computed on the CPU over the same snapshot (per-call path, checker)."""
        return self._run(_lib.lib().emqx_deliver_enrich_host, "emqx_deliver_enrich_host", offsets, subs, filters, qos,
                         flags, frm, compact, cap_kept)

    def enrich(self, rows: Sequence[Sequence[tuple]], messages: Sequence[tuple], compact: bool = False) -> Enriched:
        """``rows[i]``: the deliveries ``(subscriber id, filter word)`` of message i;
        ``messages[i]``: ``(qos, flags, from)`` with ``from`` None for no sender."""
        off = np.zeros(len(rows) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in rows]) if rows else []
        flat = [d for r in rows for d in r]
        return self.enrich_packed(off, [d[0] for d in flat], [d[1] for d in flat], [m[0] for m in messages],
                                  [m[1] for m in messages],
                                  [NO_SENDER if m[2] is None else m[2] for m in messages], compact=compact)

    @staticmethod
    def batch(d_offsets: int, d_subs: int, d_filters: int, n: int, cap_in: int, d_qos: int, d_flags: int,
              d_from: int, d_out_opts: int, d_out_subids: int = 0, d_kept_offsets: int = 0, d_kept_subs: int = 0,
              d_kept_filters: int = 0, d_kept_opts: int = 0, d_kept_subids: int = 0, cap_kept: int = 0) -> DeliverBatch:
        """The argument block of the device forms from raw HIP pointers (``tensor.data_ptr()``; 0 = NULL)."""
        return DeliverBatch(offsets=d_offsets or None, subs=d_subs or None, filters=d_filters or None, n=n, cap_in=cap_in,
                            msg_qos=d_qos or None, msg_flags=d_flags or None, msg_from=d_from or None,
                            out_opts=d_out_opts or None, out_subids=d_out_subids or None,
                            kept_offsets=d_kept_offsets or None, kept_subs=d_kept_subs or None,
                            kept_filters=d_kept_filters or None, kept_opts=d_kept_opts or None,
                            kept_subids=d_kept_subids or None, cap_kept=cap_kept)

    def enrich_device(self, batch: DeliverBatch, stream: int = 0) -> dict:
        """Device-resident batch (:meth:`batch`); returns the summary when done.  Raises
        ``EngineError``: EOVERFLOW carries ``needed`` and ``summary``, EINVAL with summary flag
        bit 1 when the CSR holds more than ``cap_in`` deliveries."""
        n_kept = ctypes.c_uint64(0)
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = _lib.lib().emqx_deliver_enrich_batch_device(self._h, ctypes.byref(batch), ctypes.byref(n_kept), _p(summary),
                                                         stream or None)
        if rc != 0:
            err = EngineError(rc, "emqx_deliver_enrich_batch_device")
            err.needed = int(n_kept.value)
            err.summary = dict(zip(SUMMARY, map(int, summary)))
            raise err
        return dict(zip(SUMMARY, map(int, summary)))

    def enrich_device_async(self, batch: DeliverBatch, summary: int, stream: int = 0) -> None:
        """Enqueues the batch on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the SUMMARY words when the stream reaches it."""
        check(_lib.lib().emqx_deliver_enrich_batch_device_async(self._h, ctypes.byref(batch), summary, stream or None),
              "emqx_deliver_enrich_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_subopts_set_tuning(self._h, key.encode(), int(value)), "emqx_subopts_set_tuning")

    def stats(self) -> dict:
        s = SubOptsStats()
        check(_lib.lib().emqx_subopts_stats_get(self._h, ctypes.byref(s)), "emqx_subopts_stats_get")
        return s.as_dict()
