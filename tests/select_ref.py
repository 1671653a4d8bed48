"""Restatement, clause for clause, of the reference's 'message.publish' consumers (EMQX
5.0.0-beta.3), from topic strings alone: no filter ids, no library.

  emqx_rule_engine:get_rules_for_topic/1        apps/emqx_rule_engine/src/emqx_rule_engine.erl:157-160
  emqx_plugin_libs_rule:can_topic_match_oneof/2 apps/emqx_plugin_libs/src/emqx_plugin_libs_rule.erl:265-268
  emqx_rule_events:ignore_sys_message/1         apps/emqx_rule_engine/src/emqx_rule_events.erl:608-611
  emqx_rule_events:on_message_publish/2         emqx_rule_events.erl:98-107
  emqx_bridge:on_message_publish/1              apps/emqx_bridge/src/emqx_bridge.erl:84-91
  emqx_bridge:get_matched_bridges/1             emqx_bridge.erl:309-320
  emqx_bridge:get_matched_bridge_id/5           emqx_bridge.erl:322-328
  emqx_exhook_server:match_topic_filter/2       apps/emqx_exhook/src/emqx_exhook_server.erl:282-285

A "world" is plain data, as tests/golden/select_kats.json holds it:
  {"rules": [{"id", "from": [filter]}], "bridges": {type: {name: {"direction", "enable"?, "local_topic"}}},
   "exhooks": [{"id", "topics": [filter]}], "ignore_sys_message": bool}
A message is {"topic", "sys"?}.  Topics and filters are str in the data, bytes in the calls of
oracle/emqx_ref.py's match/2.
"""

from oracle import emqx_ref as E


def _b(x):
    return x if isinstance(x, bytes) else x.encode()


def can_topic_match_oneof(topic, filters):
    """lists:any(fun(Fltr) -> emqx_topic:match(Topic, Fltr) end, Filters)."""
    for fltr in filters:
        if E.match(_b(topic), _b(fltr)):
            return True
    return False  # lists:any(_, []) -> false


def get_rules_for_topic(rules, topic):
    """[Rule || Rule = #{from := From} <- get_rules(), can_topic_match_oneof(Topic, From)]."""
    return [rule for rule in rules if can_topic_match_oneof(topic, rule["from"])]


def ignore_sys_message(message, config):
    """maps:get(sys, Flags, false) andalso emqx:get_config([rule_engine, ignore_sys_message])."""
    return bool(message.get("sys", False)) and bool(config["ignore_sys_message"])


def rule_on_message_publish(rules, message, config):
    """emqx_rule_events:on_message_publish/2: the rules apply_rules/2 is called with."""
    if ignore_sys_message(message, config):  # true -> ok
        return []
    return get_rules_for_topic(rules, message["topic"])


def bridge_id(btype, bname):
    return "%s:%s" % (btype, bname)


def get_matched_bridge_id(conf, topic, btype, bname, acc):
    if conf.get("enable") is False:  # (#{enable := false}, ...) -> Acc
        return acc
    if E.match(_b(topic), _b(conf["local_topic"])):  # true -> [bridge_id(BType, BName) | Acc]
        return [bridge_id(btype, bname)] + acc
    return acc  # false -> Acc


def get_matched_bridges(bridges, topic):
    acc = []
    for btype, confs in bridges.items():  # maps:fold over the types, then over the names
        for bname, conf in confs.items():
            if conf["direction"] == "ingress":  # (_BName, #{direction := ingress}, Acc1) -> Acc1
                continue
            assert conf["direction"] == "egress"
            acc = get_matched_bridge_id(conf, topic, btype, bname, acc)
    return acc


def bridge_on_message_publish(bridges, message):
    """emqx_bridge:on_message_publish/1: the bridges send_message/2 is called for."""
    if message.get("sys", False):  # true -> ok
        return []
    return get_matched_bridges(bridges, message["topic"])


def match_topic_filter(topic, topic_filter):
    if topic_filter == []:  # match_topic_filter(_, []) -> true
        return True
    for f in topic_filter:
        if E.match(_b(topic), _b(f)):
            return True
    return False


def exhook_on_message_publish(exhooks, message):
    """The hooks whose NeedCall is true (emqx_exhook_server.erl:259-264); the sys flag plays no part."""
    return [h for h in exhooks if match_topic_filter(message["topic"], list(h.get("topics", [])))]


def consumers(world, message):
    """Every consumer one published message reaches, as sorted "kind:id" strings."""
    out = ["rule:%s" % r["id"] for r in rule_on_message_publish(world.get("rules", []), message, world)]
    out += ["bridge:%s" % b for b in bridge_on_message_publish(world.get("bridges", {}), message)]
    out += ["exhook:%s" % h["id"] for h in exhook_on_message_publish(world.get("exhooks", []), message)]
    assert len(out) == len(set(out))
    return sorted(out)


def load(world, index):
    """Fills an emqx_amd.select.HookIndex with a world."""
    for r in world.get("rules", []):
        index.insert_rule(r["id"], [_b(f) for f in r["from"]])
    for btype, confs in world.get("bridges", {}).items():
        for bname, conf in confs.items():
            index.set_bridge(bridge_id(btype, bname), _b(conf["local_topic"]), direction=conf["direction"],
                             enable=conf.get("enable") is not False)
    for h in world.get("exhooks", []):
        index.set_exhook(h["id"], [_b(f) for f in h.get("topics", [])])
    return index


def selected(index, world, messages):
    """What the index answers for the messages, in consumers/2's form."""
    rows = index.on_message_publish([(_b(m["topic"]), bool(m.get("sys", False))) for m in messages],
                                    ignore_sys_message=bool(world["ignore_sys_message"]))
    return [sorted("%s:%s" % k for k in row) for row in rows]
