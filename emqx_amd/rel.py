"""awaiting_rel, the inbound QoS 2 path and its expiry per session, over the C ABI of
include/emqx_rel.h (reference: apps/emqx/src/emqx_session.erl:342-369 ``publish/3`` and
``is_awaiting_full/1``, :420-428 ``pubrel/2``, :657-674 ``expire(awaiting_rel, _)``).

:class:`Rel` keeps nothing itself: the caller owns a table of uint64 rows, ``W`` entries a session
(:func:`empty_rows`, :func:`pack_entry`), next to the window stage's session table.
:meth:`Rel.run` evaluates a batch of inbound events grouped by session against it and returns a
verdict byte per event, the route list (the events the match call takes), four counts per session
(routed, released, errors, cnt_after) and whether the session arms its await timer;
:meth:`Rel.expire` drops the entries older than the timeout.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import EngineError, RelExpireArgs, RelRunArgs, RelStats, check
from .window import SESSION

__all__ = ["Rel", "Ran", "Expired", "HOST_ONLY", "TILE", "pack_events", "pack_entry", "entry_id", "entry_ts", "empty_rows",
           "default_lanes"]

HOST_ONLY = -2
# emqx_amd/csrc/rel.h: RL_TILE = RL_BLOCK * RL_ROWS, events per tile of the route passes
BLOCK, ROWS = 256, 4
TILE = BLOCK * ROWS
SUMMARY_WORDS = 8
RUN_SUMMARY = ("flags", "events", "sessions", "routed", "released", "in_use", "not_found", "exceeded")
EXPIRE_SUMMARY = ("flags", "ok_sessions", "sessions", "expired", "remaining", "armed", "reserved6", "reserved7")
F_INPUT_REFUSED, F_BAD_SUB, F_ROW_SMALL, F_BAD_TS = 2, 4, 8, 0x10
# kind of an event, the verdict byte
PUBLISH, PUBREL, DIRECT = 1, 2, 3
OK, IN_USE, NOT_FOUND, EXCEEDED, NO_SESSION, PASS, ROW_SMALL, BAD_KIND, IDLE = 1, 2, 3, 4, 5, 6, 7, 8, 9
DEFAULT_MAX_AWAITING = 100
DEFAULT_TIMEOUT = 300000
NO_TIMEOUT = 0xFFFFFFFF
TS_LIMIT = 1 << 45
MAX_EVENTS = 1 << 31
MAX_W = 128
WIDTHS = (8, 16, 32, 64, 128)
LANES = (4, 8, 16, 32, 64)
RUN_COUNTS = ("routed", "released", "errors", "cnt_after")
EXPIRE_COUNTS = ("expired", "remaining", "timer_armed", "reserved")


def default_lanes(w: int) -> int:
    """The lanes that own one session in the run fold unless the tuning key "lanes" says otherwise."""
    return max(int(w) // 16, 4)


def empty_rows(sub_limit: int, w: int) -> np.ndarray:
    """An awaiting table of ``sub_limit`` rows of ``w`` empty entries."""
    return np.zeros((int(sub_limit), int(w)), dtype=np.uint64)


def pack_events(kinds, pkt_ids) -> np.ndarray:
    """``kind << 16 | pkt_id`` per event."""
    return (np.asarray(kinds, dtype=np.uint32) << 16) | (np.asarray(pkt_ids, dtype=np.uint32) & 0xFFFF)


def pack_entry(ts_ms, pkt_id):
    """``ts_ms << 17 | 1 << 16 | pkt_id``: an entry of the awaiting table."""
    return (np.asarray(ts_ms, dtype=np.uint64) << np.uint64(17)) | np.uint64(1 << 16) | (np.asarray(pkt_id, dtype=np.uint64) & np.uint64(0xFFFF))


def entry_id(e):
    return np.asarray(e, dtype=np.uint64) & np.uint64(0xFFFF)


def entry_ts(e):
    return np.asarray(e, dtype=np.uint64) >> np.uint64(17)


class Ran(NamedTuple):
    verdicts: np.ndarray  # uint8 per event
    route: np.ndarray     # uint32: src[d] (or d) of every routed event, in grouped position order
    counts: np.ndarray    # uint32 [m, 4]: RUN_COUNTS
    arm: np.ndarray       # uint8 [m]: 1 iff the session had an OK QoS 2 PUBLISH
    summary: dict         # RUN_SUMMARY words


class Expired(NamedTuple):
    status: np.ndarray  # uint8 [m]: OK, NO_SESSION, PASS or IDLE
    counts: np.ndarray  # uint32 [m, 4]: EXPIRE_COUNTS
    summary: dict       # EXPIRE_SUMMARY words


def _p(a):
    return None if a is None else a.ctypes.data


def _table(rel):
    if not isinstance(rel, np.ndarray) or rel.dtype != np.uint64 or rel.ndim != 2 or not rel.flags.c_contiguous:
        raise ValueError("rel is a contiguous [sub_limit, W] array of uint64 (empty_rows)")
    return rel.shape


def _sessions(sessions, sub_limit):
    if not isinstance(sessions, np.ndarray) or sessions.dtype != SESSION or not sessions.flags.c_contiguous:
        raise ValueError("sessions is a contiguous array of window.SESSION records (pack_sessions)")
    if sessions.size != sub_limit:
        raise ValueError("sessions and rel differ in their number of subscribers")


def _per_sub(a, sub_limit, what):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
    if a.size != sub_limit:
        raise ValueError("%s needs one entry per subscriber" % what)
    return a


def _raise(rc, name, words, got):
    err = EngineError(rc, name)
    err.summary = words
    err.partial = got  # BAD_SUB: the outputs are complete
    raise err


class Rel:
    """One rel stage.  ``device=-1``: the current HIP device; ``HOST_ONLY``: no device (the
    ``_host`` calls only; the batch calls raise ``EMQX_EDEVICE``).  The calls of one handle share
    its scratch and run one after the other; concurrent callers take one handle each."""

    def __init__(self, device: int = -1):
        h = ctypes.c_void_p()
        check(_lib.lib().emqx_rel_create(device, ctypes.byref(h)), "emqx_rel_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().emqx_rel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, cap_in: int, cap_boxes: int, w: int) -> None:
        """Sizes the device scratch; the asynchronous forms need it done beforehand."""
        check(_lib.lib().emqx_rel_reserve(self._h, int(cap_in), int(cap_boxes), int(w)), "emqx_rel_reserve")

    # ---- host buffers --------------------------------------------------------------------
    def _run(self, fn, name, ev_subs, ev_offsets, events, sessions, rel, max_awaiting, maxes, now_ms, ts, src) -> Ran:
        off = np.ascontiguousarray(np.asarray(ev_offsets, dtype=np.uint64).reshape(-1))
        if off.size == 0:
            raise ValueError("ev_offsets needs m + 1 entries")
        subs = np.ascontiguousarray(np.asarray(ev_subs, dtype=np.uint32).reshape(-1))
        if subs.size != off.size - 1:
            raise ValueError("ev_subs and ev_offsets differ in length")
        m = subs.size
        sub_limit, w = _table(rel)
        _sessions(sessions, sub_limit)
        ev = np.ascontiguousarray(np.asarray(events, dtype=np.uint32).reshape(-1))
        cap = ev.size
        t = None if ts is None else np.ascontiguousarray(np.asarray(ts, dtype=np.uint64).reshape(-1))
        sr = None if src is None else np.ascontiguousarray(np.asarray(src, dtype=np.uint32).reshape(-1))
        if (t is not None and t.size != cap) or (sr is not None and sr.size != cap):
            raise ValueError("events, ts and src differ in length")
        mx = _per_sub(maxes, sub_limit, "maxes")
        ver, route = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(cap, 1), dtype=np.uint32)
        cnt, arm = np.zeros((max(m, 1), 4), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint8)
        b = RelRunArgs(ev_subs=_p(subs), ev_offsets=_p(off), events=_p(ev), n_boxes=None, m=m, cap_in=cap, cap_boxes=m,
                       ts=_p(t), src=_p(sr), sessions=_p(sessions), sub_limit=sub_limit, rel=_p(rel), w=w, now_ms=int(now_ms),
                       max_awaiting=int(max_awaiting), reserved=0, maxes=_p(mx), verdicts=_p(ver), out_route=_p(route),
                       out_counts=_p(cnt), out_arm=_p(arm))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(RUN_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        total = 0 if refused else min(words["events"], cap)
        got = Ran(ver[:total], route[:0 if refused else min(words["routed"], cap)], cnt[:0 if refused else m],
                  arm[:0 if refused else m], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def run(self, ev_subs, ev_offsets, events, sessions: np.ndarray, rel: np.ndarray, max_awaiting: int = DEFAULT_MAX_AWAITING,
            maxes=None, now_ms: int = 0, ts=None, src=None) -> Ran:
        """One batch of inbound events (:func:`pack_events`) grouped by session, evaluated on the
        device from host buffers (emqx_rel_run_batch).  ``rel`` is rewritten in place."""
        return self._run(_lib.lib().emqx_rel_run_batch, "emqx_rel_run_batch", ev_subs, ev_offsets, events, sessions, rel,
                         max_awaiting, maxes, now_ms, ts, src)

    def run_host(self, ev_subs, ev_offsets, events, sessions: np.ndarray, rel: np.ndarray,
                 max_awaiting: int = DEFAULT_MAX_AWAITING, maxes=None, now_ms: int = 0, ts=None, src=None) -> Ran:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._run(_lib.lib().emqx_rel_run_host, "emqx_rel_run_host", ev_subs, ev_offsets, events, sessions, rel,
                         max_awaiting, maxes, now_ms, ts, src)

    def _expire(self, fn, name, subs, m, sessions, rel, now_ms, timeout_ms, timeouts, channel_rule) -> Expired:
        sub_limit, w = _table(rel)
        _sessions(sessions, sub_limit)
        s = None if subs is None else np.ascontiguousarray(np.asarray(subs, dtype=np.uint32).reshape(-1))
        m = int(m if s is None else s.size)
        if s is not None and s.size == 0:
            s = np.zeros(1, dtype=np.uint32)
        to = _per_sub(timeouts, sub_limit, "timeouts")
        status, cnt = np.zeros(max(m, 1), dtype=np.uint8), np.zeros((max(m, 1), 4), dtype=np.uint32)
        b = RelExpireArgs(subs=_p(s), n_boxes=None, m=m, cap_boxes=m, sessions=_p(sessions), sub_limit=sub_limit, rel=_p(rel), w=w,
                          now_ms=int(now_ms), timeout_ms=int(timeout_ms), reserved=0, timeouts=_p(to),
                          channel_rule=1 if channel_rule else 0, out_status=_p(status), out_counts=_p(cnt))
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(b), _p(summary))
        words = dict(zip(EXPIRE_SUMMARY, map(int, summary)))
        refused = words["flags"] & F_INPUT_REFUSED
        got = Expired(status[:0 if refused else m], cnt[:0 if refused else m], words)
        if rc != 0:
            _raise(rc, name, words, got)
        return got

    def expire(self, sessions: np.ndarray, rel: np.ndarray, now_ms: int, timeout_ms: int = DEFAULT_TIMEOUT, timeouts=None,
               subs=None, m: int | None = None, channel_rule: bool = False) -> Expired:
        """``expire(awaiting_rel, _)`` at ``now_ms`` for the sessions ``subs`` names (None: the
        first ``m`` sessions of the table, all of it by default), on the device from host buffers
        (emqx_rel_expire_batch).  ``rel`` is rewritten in place."""
        return self._expire(_lib.lib().emqx_rel_expire_batch, "emqx_rel_expire_batch", subs, rel.shape[0] if m is None else m,
                            sessions, rel, now_ms, timeout_ms, timeouts, channel_rule)

    def expire_host(self, sessions: np.ndarray, rel: np.ndarray, now_ms: int, timeout_ms: int = DEFAULT_TIMEOUT, timeouts=None,
                    subs=None, m: int | None = None, channel_rule: bool = False) -> Expired:
        """The same bytes computed on the CPU (per-call path, checker)."""
        return self._expire(_lib.lib().emqx_rel_expire_host, "emqx_rel_expire_host", subs, rel.shape[0] if m is None else m,
                            sessions, rel, now_ms, timeout_ms, timeouts, channel_rule)

    # ---- device buffers ------------------------------------------------------------------
    @staticmethod
    def run_args(d_ev_subs: int, d_ev_offsets: int, d_events: int, m: int, cap_in: int, cap_boxes: int, d_sessions: int,
                 sub_limit: int, d_rel: int, w: int, d_verdicts: int, d_out_route: int, d_out_counts: int, d_out_arm: int,
                 max_awaiting: int = DEFAULT_MAX_AWAITING, d_maxes: int = 0, now_ms: int = 0, d_ts: int = 0, d_src: int = 0,
                 d_n_boxes: int = 0) -> RelRunArgs:
        """The argument block of the device forms of run from raw HIP pointers
        (``tensor.data_ptr()``; 0 = NULL).  Behind the inbox stage grouping raw events: its
        ``inbox_subs``, ``inbox_offsets``, ``box_filters``, ``box_src`` (as ``d_src``) and, as
        ``d_n_boxes``, its summary word 2 (``summary.data_ptr() + 16``)."""
        return RelRunArgs(ev_subs=d_ev_subs or None, ev_offsets=d_ev_offsets or None, events=d_events or None,
                          n_boxes=d_n_boxes or None, m=m, cap_in=cap_in, cap_boxes=cap_boxes, ts=d_ts or None, src=d_src or None,
                          sessions=d_sessions or None, sub_limit=sub_limit, rel=d_rel or None, w=w, now_ms=int(now_ms),
                          max_awaiting=int(max_awaiting), reserved=0, maxes=d_maxes or None, verdicts=d_verdicts or None,
                          out_route=d_out_route or None, out_counts=d_out_counts or None, out_arm=d_out_arm or None)

    @staticmethod
    def expire_args(m: int, cap_boxes: int, d_sessions: int, sub_limit: int, d_rel: int, w: int, now_ms: int, d_out_status: int,
                    d_out_counts: int, timeout_ms: int = DEFAULT_TIMEOUT, d_timeouts: int = 0, d_subs: int = 0,
                    channel_rule: bool = False, d_n_boxes: int = 0) -> RelExpireArgs:
        """The argument block of the device forms of expire."""
        return RelExpireArgs(subs=d_subs or None, n_boxes=d_n_boxes or None, m=m, cap_boxes=cap_boxes, sessions=d_sessions or None,
                             sub_limit=sub_limit, rel=d_rel or None, w=w, now_ms=int(now_ms), timeout_ms=int(timeout_ms),
                             reserved=0, timeouts=d_timeouts or None, channel_rule=1 if channel_rule else 0,
                             out_status=d_out_status or None, out_counts=d_out_counts or None)

    def _device(self, fn, name, names, args, stream):
        summary = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
        rc = fn(self._h, ctypes.byref(args), _p(summary), stream or None)
        words = dict(zip(names, map(int, summary)))
        if rc != 0:
            err = EngineError(rc, name)
            err.summary = words
            raise err
        return words

    def run_device(self, args: RelRunArgs, stream: int = 0) -> dict:
        """Device-resident run call; returns the summary when done.  Raises ``EngineError``
        (EINVAL) with ``summary`` for a refused input or a subscriber id not below ``sub_limit``."""
        return self._device(_lib.lib().emqx_rel_run_batch_device, "emqx_rel_run_batch_device", RUN_SUMMARY, args, stream)

    def expire_device(self, args: RelExpireArgs, stream: int = 0) -> dict:
        return self._device(_lib.lib().emqx_rel_expire_batch_device, "emqx_rel_expire_batch_device", EXPIRE_SUMMARY, args, stream)

    def run_device_async(self, args: RelRunArgs, summary: int, stream: int = 0) -> None:
        """Enqueues the call on ``stream`` and returns; ``summary`` (8 uint64, device or pinned)
        gets the summary words when the stream reaches it.  EOVERFLOW, nothing enqueued: the
        scratch :meth:`reserve` sized is too small."""
        check(_lib.lib().emqx_rel_run_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_rel_run_batch_device_async")

    def expire_device_async(self, args: RelExpireArgs, summary: int, stream: int = 0) -> None:
        check(_lib.lib().emqx_rel_expire_batch_device_async(self._h, ctypes.byref(args), summary, stream or None),
              "emqx_rel_expire_batch_device_async")

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().emqx_rel_set_tuning(self._h, key.encode(), int(value)), "emqx_rel_set_tuning")

    def stats(self) -> dict:
        s = RelStats()
        check(_lib.lib().emqx_rel_stats_get(self._h, ctypes.byref(s)), "emqx_rel_stats_get")
        return s.as_dict()
