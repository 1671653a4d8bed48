"""Loader for the engine's C ABI (include/emqx_match.h -> emqx_amd/_build/libemqxmatch.so).

The library is built in-tree (``make -C emqx_amd/csrc`` / ``__graft_entry__.build()``).
There is no fallback: if the library is missing this raises, and every match call runs
on the HIP device or fails with ``EngineError``.
"""

from __future__ import annotations

import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# EMQX_LIB: an alternative build of the same library (experiments: `make retain-prof`)
LIB_PATH = os.environ.get("EMQX_LIB") or os.path.join(HERE, "_build", "libemqxmatch.so")

EMQX_OK = 0
EMQX_EINVAL = -1
EMQX_ENOMEM = -2
EMQX_EDEVICE = -3
EMQX_EOVERFLOW = -4
EMQX_ENOTFOUND = -5
EMQX_ETOODEEP = -6
EMQX_EBUSY = -7

MODE_ROUTES = 0
MODE_TRIE = 1
MODE_TRIE_WILDCARD = 2

# Every symbol include/emqx_match.h declares (checked by tests/test_abi_cpu.py).
EXPORTS = (
    "emqx_engine_create", "emqx_engine_destroy", "emqx_insert_filters", "emqx_insert_filters_ext",
    "emqx_delete_filters",
    "emqx_lookup_filter", "emqx_filter_name", "emqx_commit", "emqx_match_batch",
    "emqx_match_batch_device", "emqx_match_batch_device_async", "emqx_stats_get", "emqx_topic_match", "emqx_topic_wildcard",
    "emqx_set_tuning", "emqx_diag_read", "emqx_diag_timeline", "emqx_build_check", "emqx_batcher_create",
    "emqx_batcher_submit", "emqx_batcher_destroy", "emqx_batcher_stats", "emqx_batcher_stats_ext",
    "emqx_batcher_submit_many", "emqx_batcher_try_submit", "emqx_strerror", "emqx_version",
    "emqx_subtab_create", "emqx_subtab_destroy", "emqx_subtab_add", "emqx_subtab_remove", "emqx_subtab_commit",
    "emqx_subtab_commit_wait", "emqx_subtab_stats", "emqx_subtab_commit_stats", "emqx_subtab_forget_publishers", "emqx_subtab_set_alive",
    "emqx_subtab_set_tuning",
    "emqx_share_repick", "emqx_coalescer_create", "emqx_coalescer_insert_filters", "emqx_coalescer_delete_filters",
    "emqx_coalescer_subscribe", "emqx_coalescer_subscribe_many", "emqx_coalescer_set_alive", "emqx_coalescer_flush", "emqx_coalescer_destroy",
    "emqx_coalescer_stats",
    "emqx_fanout_batch_device", "emqx_fanout_batch_device_async", "emqx_publish_batch",
    "emqx_pub_batch_create", "emqx_pub_batch_destroy", "emqx_pub_batch_reserve", "emqx_pub_batch_submit",
    "emqx_pub_batch_wait", "emqx_pub_batch_query",
    "emqx_pub_batcher_create", "emqx_pub_batcher_submit", "emqx_pub_batcher_try_submit",
    "emqx_pub_batcher_submit_many", "emqx_pub_batcher_destroy", "emqx_pub_batcher_stats_ext",
    "emqx_host_batch_create", "emqx_host_batch_destroy", "emqx_host_batch_reserve", "emqx_host_batch_submit",
    "emqx_host_batch_wait", "emqx_host_batch_query",
    "emqx_commit_stats", "emqx_shard_owner", "emqx_shard_owner_device",
    "emqx_shard_plan", "emqx_shard_place", "emqx_shard_route", "emqx_shard_route_device", "emqx_permute_scratch_bytes", "emqx_batch_permute_device", "emqx_owner_sort_scratch_bytes",
    "emqx_owner_sort_device", "emqx_shard_step_create", "emqx_shard_step_destroy", "emqx_shard_send_cap",
    "emqx_shard_step_send", "emqx_shard_step_recv", "emqx_shard_step_answer", "emqx_shard_step_merge",
    "emqx_shard_step_send_fixed", "emqx_shard_step_recv_fixed", "emqx_shard_step_answer_fixed",
    "emqx_shard_step_merge_fixed",
    "emqx_csr_unpermute_device", "emqx_htrie_create", "emqx_htrie_destroy", "emqx_htrie_insert", "emqx_htrie_delete",
    "emqx_htrie_commit", "emqx_htrie_match", "emqx_htrie_check", "emqx_htrie_walk_sim",
)
# Every symbol include/emqx_retain.h declares (retained-message index).
RETAIN_EXPORTS = (
    "emqx_retain_create", "emqx_retain_destroy", "emqx_retain_store", "emqx_retain_delete",
    "emqx_retain_lookup", "emqx_retain_topic", "emqx_retain_expired", "emqx_retain_commit",
    "emqx_retain_match_batch", "emqx_retain_match_batch_device", "emqx_retain_stats_get",
    "emqx_retain_match_spec_batch", "emqx_retain_set_tuning",
)
# Every symbol include/emqx_authz.h declares (batched authorization check).
AUTHZ_EXPORTS = (
    "emqx_authz_create", "emqx_authz_destroy", "emqx_authz_list_set", "emqx_authz_source_clear",
    "emqx_authz_clients_set", "emqx_authz_clients_drop", "emqx_authz_commit", "emqx_authz_check_batch",
    "emqx_authz_check_batch_device", "emqx_authz_check_batch_device_async", "emqx_authz_check_host",
    "emqx_authz_set_tuning", "emqx_authz_stats_get",
)
# Every symbol include/emqx_deliver.h declares (delivery options behind the fan-out).
DELIVER_EXPORTS = (
    "emqx_subopts_create", "emqx_subopts_destroy", "emqx_subopts_set", "emqx_subopts_remove",
    "emqx_subopts_drop_subscribers", "emqx_subopts_commit", "emqx_deliver_enrich_batch",
    "emqx_deliver_enrich_batch_device", "emqx_deliver_enrich_batch_device_async", "emqx_deliver_enrich_host",
    "emqx_subopts_set_tuning", "emqx_subopts_stats_get",
)
# Every symbol include/emqx_select.h declares (hook consumers selected per publish).
SELECT_EXPORTS = (
    "emqx_owntab_create", "emqx_owntab_destroy", "emqx_owntab_set", "emqx_owntab_enable", "emqx_owntab_remove",
    "emqx_owntab_commit", "emqx_select_batch", "emqx_select_batch_device", "emqx_select_batch_device_async",
    "emqx_select_host", "emqx_owntab_set_tuning", "emqx_owntab_stats_get",
)
# Every symbol include/emqx_inbox.h declares (a batch's deliveries grouped by subscriber).
INBOX_EXPORTS = (
    "emqx_inbox_create", "emqx_inbox_destroy", "emqx_inbox_reserve", "emqx_inbox_group_batch",
    "emqx_inbox_group_batch_device", "emqx_inbox_group_batch_device_async", "emqx_inbox_group_host",
    "emqx_inbox_set_tuning", "emqx_inbox_stats_get",
)
# Every symbol include/emqx_window.h declares (inflight and mqueue admission per inbox).
WINDOW_EXPORTS = (
    "emqx_window_create", "emqx_window_destroy", "emqx_window_reserve", "emqx_window_run_batch",
    "emqx_window_run_batch_device", "emqx_window_run_batch_device_async", "emqx_window_run_host",
    "emqx_window_set_tuning", "emqx_window_stats_get",
)
# Every symbol include/emqx_ack.h declares (inflight slots and PUBACK / PUBREC / PUBCOMP per session).
ACK_EXPORTS = (
    "emqx_ack_create", "emqx_ack_destroy", "emqx_ack_reserve", "emqx_ack_record_batch", "emqx_ack_record_batch_device",
    "emqx_ack_record_batch_device_async", "emqx_ack_record_host", "emqx_ack_run_batch", "emqx_ack_run_batch_device",
    "emqx_ack_run_batch_device_async", "emqx_ack_run_host", "emqx_ack_set_tuning", "emqx_ack_stats_get",
)
# Every symbol include/emqx_retry.h declares (inflight ages, redelivery lists and timers per session).
RETRY_EXPORTS = (
    "emqx_retry_create", "emqx_retry_destroy", "emqx_retry_reserve", "emqx_retry_stamp_batch", "emqx_retry_stamp_batch_device",
    "emqx_retry_stamp_batch_device_async", "emqx_retry_stamp_host", "emqx_retry_sweep_batch", "emqx_retry_sweep_batch_device",
    "emqx_retry_sweep_batch_device_async", "emqx_retry_sweep_host", "emqx_retry_set_tuning", "emqx_retry_stats_get",
)
# Every symbol include/emqx_mqueue.h declares (queued messages and dequeue/1 per session).
MQUEUE_EXPORTS = (
    "emqx_mqueue_create", "emqx_mqueue_destroy", "emqx_mqueue_reserve", "emqx_mqueue_put_batch", "emqx_mqueue_put_batch_device",
    "emqx_mqueue_put_batch_device_async", "emqx_mqueue_put_host", "emqx_mqueue_take_batch", "emqx_mqueue_take_batch_device",
    "emqx_mqueue_take_batch_device_async", "emqx_mqueue_take_host", "emqx_mqueue_set_tuning", "emqx_mqueue_stats_get",
)
# Every symbol include/emqx_pmqueue.h declares (queued messages of sessions with a priority table).
PMQUEUE_EXPORTS = (
    "emqx_pmqueue_create", "emqx_pmqueue_destroy", "emqx_pmqueue_reserve", "emqx_pmqueue_put_batch", "emqx_pmqueue_take_batch",
    "emqx_pmqueue_put_batch_device",
    "emqx_pmqueue_put_batch_device_async", "emqx_pmqueue_put_host", "emqx_pmqueue_take_batch_device",
    "emqx_pmqueue_take_batch_device_async", "emqx_pmqueue_take_host", "emqx_pmqueue_set_tuning", "emqx_pmqueue_stats_get",
)
# Every symbol include/emqx_rel.h declares (awaiting_rel, QoS 2 publish/3, pubrel/2 and expiry per session).
REL_EXPORTS = (
    "emqx_rel_create", "emqx_rel_destroy", "emqx_rel_reserve", "emqx_rel_run_batch", "emqx_rel_run_batch_device",
    "emqx_rel_run_batch_device_async", "emqx_rel_run_host", "emqx_rel_expire_batch", "emqx_rel_expire_batch_device",
    "emqx_rel_expire_batch_device_async", "emqx_rel_expire_host", "emqx_rel_set_tuning", "emqx_rel_stats_get",
)
# Every symbol include/emqx_route.h declares (dests, aggre/1 and forward lists per node).
ROUTE_EXPORTS = (
    "emqx_routetab_create", "emqx_routetab_destroy", "emqx_routetab_add", "emqx_routetab_remove",
    "emqx_routetab_purge_node", "emqx_routetab_lookup", "emqx_routetab_commit", "emqx_route_batch",
    "emqx_route_batch_device", "emqx_route_batch_device_async", "emqx_route_host", "emqx_routetab_set_tuning",
    "emqx_routetab_stats_get",
)

NO_GROUP = 0xFFFFFFFF
SHARD_NONE = 0xFFFFFFFF
FANOUT_SHARED_BIT = 0x80000000
FANOUT_RETRY_BIT = 0x40000000
PICK_NONE, PICK_FRESH, PICK_RETRY = 0, 1, 2
SHARE_RANDOM, SHARE_ROUND_ROBIN, SHARE_STICKY, SHARE_HASH_CLIENTID, SHARE_HASH_TOPIC = 0, 1, 2, 3, 4


class EngineError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = lib().emqx_strerror(code).decode(errors="replace")
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


class EngineOpts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("n_filters", ctypes.c_uint64), ("n_ids", ctypes.c_uint64), ("n_nodes", ctypes.c_uint64),
        ("n_slots", ctypes.c_uint64), ("n_words", ctypes.c_uint64), ("table_bytes", ctypes.c_uint64),
        ("epoch", ctypes.c_uint64), ("last_evals", ctypes.c_uint64), ("last_deferred", ctypes.c_uint64),
        ("last_max_stack", ctypes.c_uint64),
        ("last_build_ms", ctypes.c_double), ("last_match_ms", ctypes.c_double),
        ("last_kernel_ms", ctypes.c_double),
        ("delta_filters", ctypes.c_uint64), ("last_commit_kind", ctypes.c_uint64),
        ("max_depth", ctypes.c_uint64), ("last_ordered", ctypes.c_uint64), ("last_order_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class RetainStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("n_ids", ctypes.c_uint64), ("n_live", ctypes.c_uint64), ("n_nodes", ctypes.c_uint64),
        ("n_words", ctypes.c_uint64), ("table_bytes", ctypes.c_uint64), ("epoch", ctypes.c_uint64),
        ("last_ranges", ctypes.c_uint64), ("last_visits", ctypes.c_uint64), ("last_total", ctypes.c_uint64),
        ("last_build_ms", ctypes.c_double), ("last_match_ms", ctypes.c_double), ("last_walk_ms", ctypes.c_double),
        ("last_spill_rounds", ctypes.c_uint64), ("last_spilled", ctypes.c_uint64),
        ("last_spill_full", ctypes.c_uint64),
        ("last_shares", ctypes.c_uint64),
        ("queue_aborts", ctypes.c_uint64),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class AuthzRule(ctypes.Structure):
    """struct emqx_authz_rule (include/emqx_authz.h)."""
    _fields_ = [("permission", ctypes.c_uint8), ("action", ctypes.c_uint8), ("who_op", ctypes.c_uint8),
                ("eq_topics", ctypes.c_uint8), ("n_who", ctypes.c_uint32), ("first_topic", ctypes.c_uint32),
                ("n_topics", ctypes.c_uint32), ("tag", ctypes.c_uint32)]


class AuthzWho(ctypes.Structure):
    """struct emqx_authz_who (include/emqx_authz.h)."""
    _fields_ = [("kind", ctypes.c_uint32), ("operand", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class AuthzStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("n_sources", ctypes.c_uint64), ("n_lists", ctypes.c_uint64), ("n_rules", ctypes.c_uint64),
        ("n_entries", ctypes.c_uint64), ("n_clients", ctypes.c_uint64), ("table_bytes", ctypes.c_uint64),
        ("epoch", ctypes.c_uint64), ("last_evals", ctypes.c_uint64), ("last_group", ctypes.c_uint64),
        ("last_build_ms", ctypes.c_double), ("last_check_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class DeliverBatch(ctypes.Structure):
    """struct emqx_deliver_batch (include/emqx_deliver.h): the buffers of one enrich call."""
    _fields_ = [
        ("offsets", ctypes.c_void_p), ("subs", ctypes.c_void_p), ("filters", ctypes.c_void_p),
        ("n", ctypes.c_uint64), ("cap_in", ctypes.c_uint64),
        ("msg_qos", ctypes.c_void_p), ("msg_flags", ctypes.c_void_p), ("msg_from", ctypes.c_void_p),
        ("out_opts", ctypes.c_void_p), ("out_subids", ctypes.c_void_p),
        ("kept_offsets", ctypes.c_void_p), ("kept_subs", ctypes.c_void_p), ("kept_filters", ctypes.c_void_p),
        ("kept_opts", ctypes.c_void_p), ("kept_subids", ctypes.c_void_p), ("cap_kept", ctypes.c_uint64),
    ]


class SubOptsStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("n_entries", ctypes.c_uint64), ("n_slots", ctypes.c_uint64), ("table_bytes", ctypes.c_uint64),
        ("epoch", ctypes.c_uint64), ("max_probe", ctypes.c_uint64),
        ("last_build_ms", ctypes.c_double), ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class SelectBatch(ctypes.Structure):
    """struct emqx_select_batch (include/emqx_select.h): the buffers of one select call."""
    _fields_ = [
        ("offsets", ctypes.c_void_p), ("filters", ctypes.c_void_p), ("n", ctypes.c_uint64), ("cap_in", ctypes.c_uint64),
        ("msg_classes", ctypes.c_void_p), ("out_offsets", ctypes.c_void_p), ("out_owners", ctypes.c_void_p),
        ("cap_out", ctypes.c_uint64),
    ]


class OwnTabStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("n_owners", ctypes.c_uint64), ("n_filters", ctypes.c_uint64), ("n_postings", ctypes.c_uint64),
        ("n_match_all", ctypes.c_uint64), ("max_list", ctypes.c_uint64), ("epoch", ctypes.c_uint64),
        ("last_build_ms", ctypes.c_double), ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class InboxBatch(ctypes.Structure):
    """struct emqx_inbox_batch (include/emqx_inbox.h): the buffers of one group call."""
    _fields_ = [
        ("offsets", ctypes.c_void_p), ("subs", ctypes.c_void_p), ("filters", ctypes.c_void_p),
        ("opts", ctypes.c_void_p), ("subids", ctypes.c_void_p),
        ("n", ctypes.c_uint64), ("cap_in", ctypes.c_uint64), ("sub_limit", ctypes.c_uint64),
        ("box_msgs", ctypes.c_void_p), ("box_filters", ctypes.c_void_p), ("box_opts", ctypes.c_void_p),
        ("box_subids", ctypes.c_void_p), ("box_src", ctypes.c_void_p),
        ("inbox_subs", ctypes.c_void_p), ("inbox_offsets", ctypes.c_void_p), ("cap_boxes", ctypes.c_uint64),
    ]


class InboxStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("cap_in", ctypes.c_uint64), ("sub_limit", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64),
        ("path", ctypes.c_uint64), ("calls", ctypes.c_uint64), ("last_passes", ctypes.c_uint64),
        ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class WindowBatch(ctypes.Structure):
    """struct emqx_window_batch (include/emqx_window.h): the buffers of one call."""
    _fields_ = [
        ("inbox_subs", ctypes.c_void_p), ("inbox_offsets", ctypes.c_void_p), ("box_opts", ctypes.c_void_p),
        ("n_boxes", ctypes.c_void_p),
        ("m", ctypes.c_uint64), ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64), ("update_table", ctypes.c_uint64),
        ("verdicts", ctypes.c_void_p), ("pkt_ids", ctypes.c_void_p), ("out_sessions", ctypes.c_void_p),
        ("out_counts", ctypes.c_void_p),
    ]


class WindowStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64),
        ("path", ctypes.c_uint64), ("calls", ctypes.c_uint64), ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class AckRecordArgs(ctypes.Structure):
    """struct emqx_ack_record_args (include/emqx_ack.h): the buffers of one record call."""
    _fields_ = [
        ("inbox_subs", ctypes.c_void_p), ("inbox_offsets", ctypes.c_void_p), ("box_opts", ctypes.c_void_p),
        ("n_boxes", ctypes.c_void_p),
        ("m", ctypes.c_uint64), ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("verdicts", ctypes.c_void_p), ("pkt_ids", ctypes.c_void_p), ("refs", ctypes.c_void_p),
        ("slots", ctypes.c_void_p), ("w", ctypes.c_uint64), ("sub_limit", ctypes.c_uint64),
        ("out_unrecorded", ctypes.c_void_p),
    ]


class AckRunArgs(ctypes.Structure):
    """struct emqx_ack_run_args (include/emqx_ack.h): the buffers of one run call."""
    _fields_ = [
        ("ack_subs", ctypes.c_void_p), ("ack_offsets", ctypes.c_void_p), ("acks", ctypes.c_void_p),
        ("n_boxes", ctypes.c_void_p),
        ("m", ctypes.c_uint64), ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64), ("update_table", ctypes.c_uint64),
        ("slots", ctypes.c_void_p), ("w", ctypes.c_uint64),
        ("verdicts", ctypes.c_void_p), ("out_refs", ctypes.c_void_p), ("out_counts", ctypes.c_void_p),
    ]


class AckStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64), ("w", ctypes.c_uint64),
        ("scratch_bytes", ctypes.c_uint64), ("rematch", ctypes.c_uint64), ("calls", ctypes.c_uint64),
        ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class RetryStampArgs(ctypes.Structure):
    """struct emqx_retry_stamp_args (include/emqx_retry.h): the buffers of one stamp call."""
    _fields_ = [
        ("subs", ctypes.c_void_p), ("n_boxes", ctypes.c_void_p), ("m", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("slots", ctypes.c_void_p), ("stamps", ctypes.c_void_p), ("w", ctypes.c_uint64), ("sub_limit", ctypes.c_uint64),
        ("now_ms", ctypes.c_uint64),
    ]


class RetrySweepArgs(ctypes.Structure):
    """struct emqx_retry_sweep_args (include/emqx_retry.h): the buffers of one sweep call."""
    _fields_ = [
        ("subs", ctypes.c_void_p), ("n_boxes", ctypes.c_void_p), ("m", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64), ("update_table", ctypes.c_uint64),
        ("slots", ctypes.c_void_p), ("stamps", ctypes.c_void_p), ("w", ctypes.c_uint64),
        ("now_ms", ctypes.c_uint64), ("interval_ms", ctypes.c_uint64), ("intervals", ctypes.c_void_p),
        ("deadlines", ctypes.c_void_p), ("ref_limit", ctypes.c_uint64), ("mode", ctypes.c_uint64), ("cap_out", ctypes.c_uint64),
        ("out_offsets", ctypes.c_void_p), ("out_items", ctypes.c_void_p), ("out_status", ctypes.c_void_p),
        ("out_counts", ctypes.c_void_p), ("out_timers", ctypes.c_void_p),
    ]


class RetryStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("cap_boxes", ctypes.c_uint64), ("w", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64), ("calls", ctypes.c_uint64),
        ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class MqueuePutArgs(ctypes.Structure):
    """struct emqx_mqueue_put_args (include/emqx_mqueue.h): the buffers of one put call."""
    _fields_ = [
        ("inbox_subs", ctypes.c_void_p), ("inbox_offsets", ctypes.c_void_p), ("box_opts", ctypes.c_void_p),
        ("n_boxes", ctypes.c_void_p),
        ("m", ctypes.c_uint64), ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("verdicts", ctypes.c_void_p), ("refs", ctypes.c_void_p), ("sessions", ctypes.c_void_p),
        ("ring", ctypes.c_void_p), ("heads", ctypes.c_void_p), ("q", ctypes.c_uint64), ("sub_limit", ctypes.c_uint64),
        ("out_evicted", ctypes.c_void_p), ("out_unstored", ctypes.c_void_p),
    ]


class MqueueTakeArgs(ctypes.Structure):
    """struct emqx_mqueue_take_args (include/emqx_mqueue.h): the buffers of one take call."""
    _fields_ = [
        ("subs", ctypes.c_void_p), ("n_boxes", ctypes.c_void_p), ("m", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64), ("update_table", ctypes.c_uint64),
        ("ring", ctypes.c_void_p), ("heads", ctypes.c_void_p), ("q", ctypes.c_uint64), ("now_ms", ctypes.c_uint64),
        ("deadlines", ctypes.c_void_p), ("ref_limit", ctypes.c_uint64), ("cap_out", ctypes.c_uint64),
        ("out_offsets", ctypes.c_void_p), ("out_opts", ctypes.c_void_p), ("out_verdicts", ctypes.c_void_p),
        ("out_pkt_ids", ctypes.c_void_p), ("out_refs", ctypes.c_void_p), ("out_status", ctypes.c_void_p),
        ("out_counts", ctypes.c_void_p),
    ]


class MqueueStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64), ("calls", ctypes.c_uint64),
        ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class PmqueuePutArgs(ctypes.Structure):
    """struct emqx_pmqueue_put_args (include/emqx_pmqueue.h): the buffers of one put call."""
    _fields_ = [
        ("inbox_subs", ctypes.c_void_p), ("inbox_offsets", ctypes.c_void_p), ("box_opts", ctypes.c_void_p),
        ("n_boxes", ctypes.c_void_p),
        ("m", ctypes.c_uint64), ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("verdicts", ctypes.c_void_p), ("refs", ctypes.c_void_p), ("box_src", ctypes.c_void_p), ("msg_class", ctypes.c_void_p),
        ("n_msgs", ctypes.c_uint64), ("tables", ctypes.c_void_p), ("n_tables", ctypes.c_uint64),
        ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64), ("update_table", ctypes.c_uint64),
        ("ring", ctypes.c_void_p), ("heads", ctypes.c_void_p), ("c", ctypes.c_uint64), ("qc", ctypes.c_uint64),
        ("out_verdicts", ctypes.c_void_p), ("out_class", ctypes.c_void_p), ("out_evicted", ctypes.c_void_p),
        ("out_counts", ctypes.c_void_p),
    ]


class PmqueueTakeArgs(ctypes.Structure):
    """struct emqx_pmqueue_take_args (include/emqx_pmqueue.h): the buffers of one take call."""
    _fields_ = [
        ("subs", ctypes.c_void_p), ("n_boxes", ctypes.c_void_p), ("m", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64), ("update_table", ctypes.c_uint64),
        ("tables", ctypes.c_void_p), ("n_tables", ctypes.c_uint64),
        ("ring", ctypes.c_void_p), ("heads", ctypes.c_void_p), ("c", ctypes.c_uint64), ("qc", ctypes.c_uint64),
        ("now_ms", ctypes.c_uint64), ("deadlines", ctypes.c_void_p), ("ref_limit", ctypes.c_uint64), ("cap_out", ctypes.c_uint64),
        ("out_offsets", ctypes.c_void_p), ("out_opts", ctypes.c_void_p), ("out_verdicts", ctypes.c_void_p),
        ("out_pkt_ids", ctypes.c_void_p), ("out_refs", ctypes.c_void_p), ("out_class", ctypes.c_void_p),
        ("out_status", ctypes.c_void_p), ("out_counts", ctypes.c_void_p),
    ]


class PmqueueStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64), ("group", ctypes.c_uint64),
        ("calls", ctypes.c_uint64), ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class RelRunArgs(ctypes.Structure):
    """struct emqx_rel_run_args (include/emqx_rel.h): the buffers of one run call."""
    _fields_ = [
        ("ev_subs", ctypes.c_void_p), ("ev_offsets", ctypes.c_void_p), ("events", ctypes.c_void_p),
        ("n_boxes", ctypes.c_void_p),
        ("m", ctypes.c_uint64), ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("ts", ctypes.c_void_p), ("src", ctypes.c_void_p), ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64),
        ("rel", ctypes.c_void_p), ("w", ctypes.c_uint64), ("now_ms", ctypes.c_uint64),
        ("max_awaiting", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("maxes", ctypes.c_void_p),
        ("verdicts", ctypes.c_void_p), ("out_route", ctypes.c_void_p), ("out_counts", ctypes.c_void_p),
        ("out_arm", ctypes.c_void_p),
    ]


class RelExpireArgs(ctypes.Structure):
    """struct emqx_rel_expire_args (include/emqx_rel.h): the buffers of one expire call."""
    _fields_ = [
        ("subs", ctypes.c_void_p), ("n_boxes", ctypes.c_void_p), ("m", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64),
        ("sessions", ctypes.c_void_p), ("sub_limit", ctypes.c_uint64), ("rel", ctypes.c_void_p), ("w", ctypes.c_uint64),
        ("now_ms", ctypes.c_uint64), ("timeout_ms", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("timeouts", ctypes.c_void_p), ("channel_rule", ctypes.c_uint64),
        ("out_status", ctypes.c_void_p), ("out_counts", ctypes.c_void_p),
    ]


class RelStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("cap_in", ctypes.c_uint64), ("cap_boxes", ctypes.c_uint64), ("w", ctypes.c_uint64),
        ("scratch_bytes", ctypes.c_uint64), ("lanes", ctypes.c_uint64), ("calls", ctypes.c_uint64),
        ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class RouteBatch(ctypes.Structure):
    """struct emqx_route_batch (include/emqx_route.h): the buffers of one route call."""
    _fields_ = [
        ("offsets", ctypes.c_void_p), ("filters", ctypes.c_void_p), ("n", ctypes.c_uint64), ("cap_in", ctypes.c_uint64),
        ("entry_flags", ctypes.c_void_p), ("msg_routes", ctypes.c_void_p), ("node_offsets", ctypes.c_void_p),
        ("fwd_msgs", ctypes.c_void_p), ("fwd_filters", ctypes.c_void_p), ("cap_fwd", ctypes.c_uint64),
        ("local_offsets", ctypes.c_void_p), ("local_filters", ctypes.c_void_p),
    ]


class RouteTabStats(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint64),
        ("n_filters", ctypes.c_uint64), ("n_plain", ctypes.c_uint64), ("n_grouped", ctypes.c_uint64),
        ("n_nodes", ctypes.c_uint64), ("epoch", ctypes.c_uint64),
        ("last_build_ms", ctypes.c_double), ("last_call_ms", ctypes.c_double),
    ]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.size = ctypes.sizeof(self)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class HostBatchStruct(ctypes.Structure):
    """struct emqx_host_batch (include/emqx_match.h): pinned buffers of one host batch."""
    _fields_ = [
        ("topic_bytes", ctypes.POINTER(ctypes.c_uint8)), ("topic_offsets", ctypes.POINTER(ctypes.c_uint64)),
        ("cap_topics", ctypes.c_uint64), ("cap_bytes", ctypes.c_uint64), ("n", ctypes.c_uint64),
        ("out_offsets", ctypes.POINTER(ctypes.c_uint64)), ("out_ids", ctypes.POINTER(ctypes.c_uint32)),
        ("cap_ids", ctypes.c_uint64), ("n_out", ctypes.c_uint64), ("priv", ctypes.c_void_p),
    ]


class PubBatchStruct(ctypes.Structure):
    """struct emqx_pub_batch (include/emqx_match.h): pinned buffers of one publish batch."""
    _fields_ = [
        ("topic_bytes", ctypes.POINTER(ctypes.c_uint8)), ("topic_offsets", ctypes.POINTER(ctypes.c_uint64)),
        ("keys", ctypes.POINTER(ctypes.c_uint32)),
        ("cap_topics", ctypes.c_uint64), ("cap_bytes", ctypes.c_uint64), ("n", ctypes.c_uint64),
        ("out_offsets", ctypes.POINTER(ctypes.c_uint64)), ("out_subs", ctypes.POINTER(ctypes.c_uint32)),
        ("out_filters", ctypes.POINTER(ctypes.c_uint32)),
        ("cap_out", ctypes.c_uint64), ("n_out", ctypes.c_uint64), ("priv", ctypes.c_void_p),
    ]


BATCH_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64)
DONE_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)
PUB_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32),
                          ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64)

_lib = None


def lib():
    """Loads libemqxmatch.so (once).  If torch is already imported its HIP runtime
    (same soname) is reused, so device pointers from torch tensors are valid here."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not built; run `make -C emqx_amd/csrc` or __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    sig = {
        "emqx_engine_create": (i32, [ctypes.POINTER(EngineOpts), ctypes.POINTER(vp)]),
        "emqx_engine_destroy": (i32, [vp]),
        "emqx_insert_filters": (i32, [vp, vp, vp, u64, vp]),
        "emqx_insert_filters_ext": (i32, [vp, vp, vp, u64, vp, vp]),
        "emqx_delete_filters": (i32, [vp, vp, u64]),
        "emqx_lookup_filter": (i32, [vp, vp, u64, ctypes.POINTER(u32)]),
        "emqx_filter_name": (i32, [vp, u32, vp, u64, ctypes.POINTER(u64)]),
        "emqx_commit": (i32, [vp]),
        "emqx_match_batch": (i32, [vp, u32, vp, vp, u64, vp, vp, u64, ctypes.POINTER(u64)]),
        "emqx_match_batch_device": (i32, [vp, u32, vp, vp, u64, vp, vp, u64, ctypes.POINTER(u64), vp]),
        "emqx_match_batch_device_async": (i32, [vp, u32, vp, vp, u64, vp, vp, u64, vp, vp]),
        "emqx_stats_get": (i32, [vp, ctypes.POINTER(Stats)]),
        "emqx_topic_match": (i32, [vp, u64, vp, u64]),
        "emqx_topic_wildcard": (i32, [vp, u64]),
        "emqx_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_diag_read": (i32, [vp, vp, u32, i32]),
        "emqx_diag_timeline": (i32, [vp, vp, u64, ctypes.POINTER(u64)]),
        "emqx_build_check": (i32, [vp, vp, u64, vp, ctypes.c_char_p, u64]),
        "emqx_batcher_create": (i32, [vp, u32, u32, u32, BATCH_CB, ctypes.POINTER(vp)]),
        "emqx_batcher_submit": (i32, [vp, vp, u64, vp]),
        "emqx_batcher_destroy": (i32, [vp]),
        "emqx_batcher_stats": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "emqx_batcher_stats_ext": (i32, [vp, vp, u32]),
        "emqx_batcher_submit_many": (i32, [vp, vp, vp, u64, vp]),
        "emqx_batcher_try_submit": (i32, [vp, vp, u64, vp]),
        "emqx_subtab_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_subtab_destroy": (i32, [vp]),
        "emqx_subtab_add": (i32, [vp, vp, vp, vp, u64]),
        "emqx_subtab_remove": (i32, [vp, vp, vp, vp, u64]),
        "emqx_subtab_commit": (i32, [vp]),
        "emqx_subtab_commit_wait": (i32, [vp]),
        "emqx_subtab_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_subtab_stats": (i32, [vp, vp]),
        "emqx_subtab_commit_stats": (i32, [vp, vp, u32]),
        "emqx_subtab_forget_publishers": (i32, [vp, vp, u64]),
        "emqx_subtab_set_alive": (i32, [vp, vp, u64, i32]),
        "emqx_share_repick": (i32, [vp, u32, u64, vp, vp, vp, vp, vp, vp, vp]),
        "emqx_coalescer_create": (i32, [vp, vp, u32, DONE_CB, ctypes.POINTER(vp)]),
        "emqx_coalescer_insert_filters": (i32, [vp, vp, vp, u64, vp, vp]),
        "emqx_coalescer_delete_filters": (i32, [vp, vp, u64, vp]),
        "emqx_coalescer_subscribe": (i32, [vp, vp, vp, vp, u64, i32, vp]),
        "emqx_coalescer_subscribe_many": (i32, [vp, vp, vp, vp, vp, u64, vp]),
        "emqx_coalescer_set_alive": (i32, [vp, vp, u64, i32, vp]),
        "emqx_coalescer_flush": (i32, [vp]),
        "emqx_coalescer_destroy": (i32, [vp]),
        "emqx_coalescer_stats": (i32, [vp, vp, u32]),
        "emqx_pub_batch_create": (i32, [vp, vp, u32, u64, u64, u64, ctypes.POINTER(ctypes.POINTER(PubBatchStruct))]),
        "emqx_pub_batch_destroy": (i32, [ctypes.POINTER(PubBatchStruct)]),
        "emqx_pub_batch_reserve": (i32, [ctypes.POINTER(PubBatchStruct), u64, u64, u64]),
        "emqx_pub_batch_submit": (i32, [ctypes.POINTER(PubBatchStruct)]),
        "emqx_pub_batch_wait": (i32, [ctypes.POINTER(PubBatchStruct)]),
        "emqx_pub_batch_query": (i32, [ctypes.POINTER(PubBatchStruct)]),
        "emqx_pub_batcher_create": (i32, [vp, vp, u32, u32, u32, PUB_CB, ctypes.POINTER(vp)]),
        "emqx_pub_batcher_submit": (i32, [vp, vp, u64, u32, vp]),
        "emqx_pub_batcher_try_submit": (i32, [vp, vp, u64, u32, vp]),
        "emqx_pub_batcher_submit_many": (i32, [vp, vp, vp, vp, u64, vp]),
        "emqx_pub_batcher_destroy": (i32, [vp]),
        "emqx_pub_batcher_stats_ext": (i32, [vp, vp, u32]),
        "emqx_fanout_batch_device": (i32, [vp, u32, vp, vp, u64, vp, vp, vp, vp, u64, ctypes.POINTER(u64), vp]),
        "emqx_fanout_batch_device_async": (i32, [vp, u32, vp, vp, u64, u64, vp, vp, vp, vp, u64, vp, vp]),
        "emqx_publish_batch": (i32, [vp, vp, u32, vp, vp, u64, vp, vp, vp, vp, u64, ctypes.POINTER(u64)]),
        "emqx_retain_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_retain_destroy": (i32, [vp]),
        "emqx_retain_store": (i32, [vp, vp, vp, u64, vp, vp]),
        "emqx_retain_delete": (i32, [vp, vp, u64]),
        "emqx_retain_lookup": (i32, [vp, vp, u64, ctypes.POINTER(u32)]),
        "emqx_retain_topic": (i32, [vp, u32, vp, u64, ctypes.POINTER(u64)]),
        "emqx_retain_expired": (i32, [vp, ctypes.c_int64, vp, u64, ctypes.POINTER(u64)]),
        "emqx_retain_commit": (i32, [vp]),
        "emqx_retain_match_batch": (i32, [vp, vp, vp, u64, ctypes.c_int64, vp, vp, u64, ctypes.POINTER(u64)]),
        "emqx_retain_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_retain_match_spec_batch": (i32, [vp, vp, vp, u64, ctypes.c_int64, vp, vp, u64, ctypes.POINTER(u64)]),
        "emqx_retain_match_batch_device": (i32, [vp, vp, vp, u64, ctypes.c_int64, vp, vp, u64,
                                                 ctypes.POINTER(u64), vp]),
        "emqx_retain_stats_get": (i32, [vp, ctypes.POINTER(RetainStats)]),
        "emqx_authz_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_authz_destroy": (i32, [vp]),
        "emqx_authz_list_set": (i32, [vp, u32, u32, vp, u64, vp, u64, vp, u64, vp, vp, u64, vp, u64]),
        "emqx_authz_source_clear": (i32, [vp, u32]),
        "emqx_authz_clients_set": (i32, [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]),
        "emqx_authz_clients_drop": (i32, [vp, vp, u64]),
        "emqx_authz_commit": (i32, [vp]),
        "emqx_authz_check_batch": (i32, [vp, vp, vp, vp, vp, u64, vp, vp]),
        "emqx_authz_check_batch_device": (i32, [vp, vp, vp, vp, vp, u64, vp, vp, vp]),
        "emqx_authz_check_batch_device_async": (i32, [vp, vp, vp, vp, vp, u64, vp, vp, vp, vp]),
        "emqx_authz_check_host": (i32, [vp, vp, vp, vp, vp, u64, vp, vp]),
        "emqx_authz_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_authz_stats_get": (i32, [vp, ctypes.POINTER(AuthzStats)]),
        "emqx_subopts_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_subopts_destroy": (i32, [vp]),
        "emqx_subopts_set": (i32, [vp, vp, vp, vp, vp, u64]),
        "emqx_subopts_remove": (i32, [vp, vp, vp, u64]),
        "emqx_subopts_drop_subscribers": (i32, [vp, vp, u64]),
        "emqx_subopts_commit": (i32, [vp]),
        "emqx_deliver_enrich_batch": (i32, [vp, ctypes.POINTER(DeliverBatch), ctypes.POINTER(u64), vp]),
        "emqx_deliver_enrich_batch_device": (i32, [vp, ctypes.POINTER(DeliverBatch), ctypes.POINTER(u64), vp, vp]),
        "emqx_deliver_enrich_batch_device_async": (i32, [vp, ctypes.POINTER(DeliverBatch), vp, vp]),
        "emqx_deliver_enrich_host": (i32, [vp, ctypes.POINTER(DeliverBatch), ctypes.POINTER(u64), vp]),
        "emqx_subopts_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_subopts_stats_get": (i32, [vp, ctypes.POINTER(SubOptsStats)]),
        "emqx_owntab_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_owntab_destroy": (i32, [vp]),
        "emqx_owntab_set": (i32, [vp, u32, u32, u32, vp, u64]),
        "emqx_owntab_enable": (i32, [vp, vp, u64, ctypes.c_int32]),
        "emqx_owntab_remove": (i32, [vp, vp, u64]),
        "emqx_owntab_commit": (i32, [vp]),
        "emqx_select_batch": (i32, [vp, ctypes.POINTER(SelectBatch), ctypes.POINTER(u64), vp]),
        "emqx_select_batch_device": (i32, [vp, ctypes.POINTER(SelectBatch), ctypes.POINTER(u64), vp, vp]),
        "emqx_select_batch_device_async": (i32, [vp, ctypes.POINTER(SelectBatch), vp, vp]),
        "emqx_select_host": (i32, [vp, ctypes.POINTER(SelectBatch), ctypes.POINTER(u64), vp]),
        "emqx_owntab_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_owntab_stats_get": (i32, [vp, ctypes.POINTER(OwnTabStats)]),
        "emqx_inbox_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_inbox_destroy": (i32, [vp]),
        "emqx_inbox_reserve": (i32, [vp, u64, u64]),
        "emqx_inbox_group_batch": (i32, [vp, ctypes.POINTER(InboxBatch), ctypes.POINTER(u64), vp]),
        "emqx_inbox_group_batch_device": (i32, [vp, ctypes.POINTER(InboxBatch), ctypes.POINTER(u64), vp, vp]),
        "emqx_inbox_group_batch_device_async": (i32, [vp, ctypes.POINTER(InboxBatch), vp, vp]),
        "emqx_inbox_group_host": (i32, [vp, ctypes.POINTER(InboxBatch), ctypes.POINTER(u64), vp]),
        "emqx_inbox_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_inbox_stats_get": (i32, [vp, ctypes.POINTER(InboxStats)]),
        "emqx_window_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_window_destroy": (i32, [vp]),
        "emqx_window_reserve": (i32, [vp, u64, u64]),
        "emqx_window_run_batch": (i32, [vp, ctypes.POINTER(WindowBatch), vp]),
        "emqx_window_run_batch_device": (i32, [vp, ctypes.POINTER(WindowBatch), vp, vp]),
        "emqx_window_run_batch_device_async": (i32, [vp, ctypes.POINTER(WindowBatch), vp, vp]),
        "emqx_window_run_host": (i32, [vp, ctypes.POINTER(WindowBatch), vp]),
        "emqx_window_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_window_stats_get": (i32, [vp, ctypes.POINTER(WindowStats)]),
        "emqx_ack_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_ack_destroy": (i32, [vp]),
        "emqx_ack_reserve": (i32, [vp, u64, u64, u64]),
        "emqx_ack_record_batch": (i32, [vp, ctypes.POINTER(AckRecordArgs), vp]),
        "emqx_ack_record_batch_device": (i32, [vp, ctypes.POINTER(AckRecordArgs), vp, vp]),
        "emqx_ack_record_batch_device_async": (i32, [vp, ctypes.POINTER(AckRecordArgs), vp, vp]),
        "emqx_ack_record_host": (i32, [vp, ctypes.POINTER(AckRecordArgs), vp]),
        "emqx_ack_run_batch": (i32, [vp, ctypes.POINTER(AckRunArgs), vp]),
        "emqx_ack_run_batch_device": (i32, [vp, ctypes.POINTER(AckRunArgs), vp, vp]),
        "emqx_ack_run_batch_device_async": (i32, [vp, ctypes.POINTER(AckRunArgs), vp, vp]),
        "emqx_ack_run_host": (i32, [vp, ctypes.POINTER(AckRunArgs), vp]),
        "emqx_ack_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_ack_stats_get": (i32, [vp, ctypes.POINTER(AckStats)]),
        "emqx_retry_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_retry_destroy": (i32, [vp]),
        "emqx_retry_reserve": (i32, [vp, u64, u64]),
        "emqx_retry_stamp_batch": (i32, [vp, ctypes.POINTER(RetryStampArgs), vp]),
        "emqx_retry_stamp_batch_device": (i32, [vp, ctypes.POINTER(RetryStampArgs), vp, vp]),
        "emqx_retry_stamp_batch_device_async": (i32, [vp, ctypes.POINTER(RetryStampArgs), vp, vp]),
        "emqx_retry_stamp_host": (i32, [vp, ctypes.POINTER(RetryStampArgs), vp]),
        "emqx_retry_sweep_batch": (i32, [vp, ctypes.POINTER(RetrySweepArgs), vp]),
        "emqx_retry_sweep_batch_device": (i32, [vp, ctypes.POINTER(RetrySweepArgs), vp, vp]),
        "emqx_retry_sweep_batch_device_async": (i32, [vp, ctypes.POINTER(RetrySweepArgs), vp, vp]),
        "emqx_retry_sweep_host": (i32, [vp, ctypes.POINTER(RetrySweepArgs), vp]),
        "emqx_retry_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_retry_stats_get": (i32, [vp, ctypes.POINTER(RetryStats)]),
        "emqx_mqueue_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_mqueue_destroy": (i32, [vp]),
        "emqx_mqueue_reserve": (i32, [vp, u64, u64]),
        "emqx_mqueue_put_batch": (i32, [vp, ctypes.POINTER(MqueuePutArgs), vp]),
        "emqx_mqueue_put_batch_device": (i32, [vp, ctypes.POINTER(MqueuePutArgs), vp, vp]),
        "emqx_mqueue_put_batch_device_async": (i32, [vp, ctypes.POINTER(MqueuePutArgs), vp, vp]),
        "emqx_mqueue_put_host": (i32, [vp, ctypes.POINTER(MqueuePutArgs), vp]),
        "emqx_mqueue_take_batch": (i32, [vp, ctypes.POINTER(MqueueTakeArgs), vp]),
        "emqx_mqueue_take_batch_device": (i32, [vp, ctypes.POINTER(MqueueTakeArgs), vp, vp]),
        "emqx_mqueue_take_batch_device_async": (i32, [vp, ctypes.POINTER(MqueueTakeArgs), vp, vp]),
        "emqx_mqueue_take_host": (i32, [vp, ctypes.POINTER(MqueueTakeArgs), vp]),
        "emqx_mqueue_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_mqueue_stats_get": (i32, [vp, ctypes.POINTER(MqueueStats)]),
        "emqx_pmqueue_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_pmqueue_destroy": (i32, [vp]),
        "emqx_pmqueue_reserve": (i32, [vp, u64, u64]),
        "emqx_pmqueue_put_batch": (i32, [vp, ctypes.POINTER(PmqueuePutArgs), vp]),
        "emqx_pmqueue_take_batch": (i32, [vp, ctypes.POINTER(PmqueueTakeArgs), vp]),
        "emqx_pmqueue_put_batch_device": (i32, [vp, ctypes.POINTER(PmqueuePutArgs), vp, vp]),
        "emqx_pmqueue_put_batch_device_async": (i32, [vp, ctypes.POINTER(PmqueuePutArgs), vp, vp]),
        "emqx_pmqueue_put_host": (i32, [vp, ctypes.POINTER(PmqueuePutArgs), vp]),
        "emqx_pmqueue_take_batch_device": (i32, [vp, ctypes.POINTER(PmqueueTakeArgs), vp, vp]),
        "emqx_pmqueue_take_batch_device_async": (i32, [vp, ctypes.POINTER(PmqueueTakeArgs), vp, vp]),
        "emqx_pmqueue_take_host": (i32, [vp, ctypes.POINTER(PmqueueTakeArgs), vp]),
        "emqx_pmqueue_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_pmqueue_stats_get": (i32, [vp, ctypes.POINTER(PmqueueStats)]),
        "emqx_rel_create": (i32, [ctypes.c_int32, ctypes.POINTER(vp)]),
        "emqx_rel_destroy": (i32, [vp]),
        "emqx_rel_reserve": (i32, [vp, u64, u64, u64]),
        "emqx_rel_run_batch": (i32, [vp, ctypes.POINTER(RelRunArgs), vp]),
        "emqx_rel_run_batch_device": (i32, [vp, ctypes.POINTER(RelRunArgs), vp, vp]),
        "emqx_rel_run_batch_device_async": (i32, [vp, ctypes.POINTER(RelRunArgs), vp, vp]),
        "emqx_rel_run_host": (i32, [vp, ctypes.POINTER(RelRunArgs), vp]),
        "emqx_rel_expire_batch": (i32, [vp, ctypes.POINTER(RelExpireArgs), vp]),
        "emqx_rel_expire_batch_device": (i32, [vp, ctypes.POINTER(RelExpireArgs), vp, vp]),
        "emqx_rel_expire_batch_device_async": (i32, [vp, ctypes.POINTER(RelExpireArgs), vp, vp]),
        "emqx_rel_expire_host": (i32, [vp, ctypes.POINTER(RelExpireArgs), vp]),
        "emqx_rel_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_rel_stats_get": (i32, [vp, ctypes.POINTER(RelStats)]),
        "emqx_routetab_create": (i32, [ctypes.c_int32, u32, ctypes.POINTER(vp)]),
        "emqx_routetab_destroy": (i32, [vp]),
        "emqx_routetab_add": (i32, [vp, vp, vp, vp, u64]),
        "emqx_routetab_remove": (i32, [vp, vp, vp, vp, u64]),
        "emqx_routetab_purge_node": (i32, [vp, u32, vp, u64, ctypes.POINTER(u64)]),
        "emqx_routetab_lookup": (i32, [vp, u32, vp, vp, u64, ctypes.POINTER(u64)]),
        "emqx_routetab_commit": (i32, [vp]),
        "emqx_route_batch": (i32, [vp, ctypes.POINTER(RouteBatch), ctypes.POINTER(u64), vp]),
        "emqx_route_batch_device": (i32, [vp, ctypes.POINTER(RouteBatch), ctypes.POINTER(u64), vp, vp]),
        "emqx_route_batch_device_async": (i32, [vp, ctypes.POINTER(RouteBatch), vp, vp]),
        "emqx_route_host": (i32, [vp, ctypes.POINTER(RouteBatch), ctypes.POINTER(u64), vp]),
        "emqx_routetab_set_tuning": (i32, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "emqx_routetab_stats_get": (i32, [vp, vp]),
        "emqx_commit_stats": (i32, [vp, vp, u32]),
        "emqx_shard_owner": (i32, [vp, vp, u64, u32, u32, i32, vp]),
        "emqx_shard_owner_device": (i32, [vp, vp, u64, u32, u32, vp, vp]),
        "emqx_shard_plan": (i32, [vp, vp, u64, u32, u32, u32, vp, u32, ctypes.POINTER(u32)]),
        "emqx_shard_place": (i32, [vp, vp, u64, u32, vp, u32, vp, vp, vp]),
        "emqx_shard_route": (i32, [vp, vp, u64, u32, vp, u32, vp]),
        "emqx_shard_route_device": (i32, [vp, vp, u64, u32, vp, u32, vp, vp]),
        "emqx_permute_scratch_bytes": (u64, [u64]),
        "emqx_owner_sort_scratch_bytes": (u64, [u64, u32]),
        "emqx_owner_sort_device": (i32, [vp, u64, u32, vp, vp, vp]),
        "emqx_shard_step_create": (i32, [i32, u32, vp, u32, ctypes.POINTER(vp)]),
        "emqx_shard_step_destroy": (i32, [vp]),
        "emqx_shard_send_cap": (u64, [u64, u64, u32]),
        "emqx_shard_step_send": (i32, [vp, vp, vp, u64, vp, u64, vp, vp]),
        "emqx_shard_step_recv": (i32, [vp, vp, vp, vp, vp, vp]),
        "emqx_shard_step_answer": (i32, [vp, vp, vp, vp, u32, vp, vp, vp]),
        "emqx_shard_step_merge": (i32, [vp, vp, vp, vp, vp, vp]),
        "emqx_shard_step_send_fixed": (i32, [vp, vp, vp, u64, vp, u64, vp, vp]),
        "emqx_shard_step_recv_fixed": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "emqx_shard_step_answer_fixed": (i32, [vp, vp, vp, vp, u32, vp, u64, vp]),
        "emqx_shard_step_merge_fixed": (i32, [vp, vp, vp, vp, vp, vp]),
        "emqx_batch_permute_device": (i32, [vp, vp, u64, vp, vp, vp, vp, vp]),
        "emqx_csr_unpermute_device": (i32, [vp, vp, u64, vp, vp, vp, vp, vp]),
        "emqx_host_batch_create": (i32, [vp, u64, u64, u64, ctypes.POINTER(ctypes.POINTER(HostBatchStruct))]),
        "emqx_host_batch_destroy": (i32, [ctypes.POINTER(HostBatchStruct)]),
        "emqx_host_batch_reserve": (i32, [ctypes.POINTER(HostBatchStruct), u64, u64, u64]),
        "emqx_host_batch_submit": (i32, [ctypes.POINTER(HostBatchStruct), u32]),
        "emqx_host_batch_wait": (i32, [ctypes.POINTER(HostBatchStruct)]),
        "emqx_host_batch_query": (i32, [ctypes.POINTER(HostBatchStruct)]),
        "emqx_htrie_create": (i32, [u64, i32, ctypes.POINTER(vp)]),
        "emqx_htrie_destroy": (i32, [vp]),
        "emqx_htrie_insert": (i32, [vp, vp, vp, u64, vp]),
        "emqx_htrie_delete": (i32, [vp, vp, u64]),
        "emqx_htrie_commit": (i32, [vp, i32, vp]),
        "emqx_htrie_match": (i32, [vp, u32, vp, vp, u64, vp, vp, u64, ctypes.POINTER(u64)]),
        "emqx_htrie_check": (i32, [vp, ctypes.c_char_p, u64]),
        "emqx_htrie_walk_sim": (i32, [vp, vp, vp, u64, vp, vp, u32]),
        "emqx_strerror": (ctypes.c_char_p, [i32]),
        "emqx_version": (ctypes.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc: int, what: str = "") -> int:
    if rc != EMQX_OK:
        raise EngineError(rc, what)
    return rc


def loaded_path() -> str:
    return LIB_PATH if _lib is not None else ""


if __name__ == "__main__":  # pragma: no cover
    print(lib().emqx_version().decode())
    sys.exit(0)
