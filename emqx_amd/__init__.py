"""emqx_amd — MI355X-native route lookup for EMQX (topic -> matching filters).

Modules mirror the reference's Erlang modules on the hot path:
  :mod:`emqx_amd.topic`   emqx_topic   (CPU topic algebra, match/2)
  :mod:`emqx_amd.trie`    emqx_trie    (insert/delete/match/empty on the device engine)
  :mod:`emqx_amd.router`  emqx_router  (add/delete/match_routes/lookup_routes)
  :mod:`emqx_amd.engine`  the C-ABI engine handle (batched, device-resident matching)
  :mod:`emqx_amd.workloads` synthetic subscription tables / topic streams (BASELINE configs)
  :mod:`emqx_amd.deliver` emqx_session ignore_local/3 + enrich_subopts/3 (No Local, granted QoS, RAP, subid
                          per delivery behind the fan-out)
  :mod:`emqx_amd.select`  emqx_rule_engine get_rules_for_topic/1, emqx_bridge get_matched_bridges/1, emqx_exhook
                          match_topic_filter/2 (the hook consumers a published topic selects, each once)
  :mod:`emqx_amd.inbox`   emqx_connection's drain of {deliver, ...} into emqx_channel:handle_deliver/2's list (a
                          batch's deliveries grouped by subscriber, in batch order)
  :mod:`emqx_amd.window`  emqx_session deliver/2 + enqueue/2, emqx_inflight is_full/1, emqx_mqueue in/2 (inflight and
                          mqueue admission of every inbox: packet ids, what is queued, what is dropped)
  :mod:`emqx_amd.ack`     emqx_session puback/2 + pubrec/2 + pubcomp/2 + batch_n/1 over emqx_inflight (which packet ids
                          are inflight per session; a batch of acks against them: reason codes, refs, the freed window)
  :mod:`emqx_amd.retry`   emqx_session retry/1 + replay/1, emqx_message is_expired/1 (when each inflight entry went in:
                          redelivery lists in timestamp order, expired messages dropped, the next retry timer)
  :mod:`emqx_amd.mqueue`  emqx_mqueue in/2 + out/1, emqx_session dequeue/1 (the queued messages of every session in
                          device memory: what the window queued is stored, what an ack made room for is popped)
  :mod:`emqx_amd.pmqueue` emqx_mqueue in/2 + out/1 with a p_table and shift_opts (the same for the sessions of a zone that
                          sets mqueue_priorities: one ring per priority class, the order list and the credit per session)
  :mod:`emqx_amd.rel`     emqx_session publish/3 + pubrel/2 + expire(awaiting_rel, _) (which QoS 2 packet ids await their
                          PUBREL per session; an inbound batch against them: reason codes and the list to route)
  :mod:`emqx_amd.route`   emqx_broker aggre/1 + route/2 + do_route/2, emqx_router_helper cleanup_routes/1 (the route
                          bag in device memory: routes per message, forward lists per node, the local CSR)
  :mod:`emqx_amd.dist`    multi-GPU: replicated tables + data-parallel topic split,
                          filter-sharded tables with broadcast + gather
"""

__version__ = "0.1.0"

from ._lib import EngineError, MODE_ROUTES, MODE_TRIE, MODE_TRIE_WILDCARD  # noqa: F401
from .deliver import SubOpts  # noqa: F401,E402  (delivery options behind the fan-out)
from .select import HookIndex, OwnerTable  # noqa: F401,E402  (hook consumers selected per publish)
from .inbox import Inbox  # noqa: F401,E402  (a batch's deliveries grouped by subscriber)
from .window import Window  # noqa: F401,E402  (inflight and mqueue admission per inbox)
from .ack import Ack  # noqa: F401,E402  (inflight slots and PUBACK / PUBREC / PUBCOMP per session)
from .retry import Retry  # noqa: F401,E402  (inflight ages, redelivery lists and timers per session)
from .mqueue import Mqueue  # noqa: F401,E402  (queued messages and dequeue/1 per session)
from .pmqueue import Pmqueue  # noqa: F401,E402  (the same with a priority table: per-class rings, order list, credit)
from .rel import Rel  # noqa: F401,E402  (awaiting_rel, QoS 2 publish/3, pubrel/2 and expiry per session)
from .route import ClusterRouter, RouteTable  # noqa: F401,E402  (dests, aggre/1 and forward lists per node)
