"""Pure-Python restatement of the reference's in-memory authorization check, written from the
Erlang and independent of the library.  Line numbers: apps/emqx_authz/src/emqx_authz_rule.erl
unless another file is named.

Erlang terms in Python: atoms are ``str`` ('' '+' '#' 'all' 'allow' ...), binaries are ``bytes``,
tuples are tuples, ``undefined`` is ``None``.  A regex who term is not restated: it is the term
``("flag", Bit)``, true iff the client's ``flags`` has that bit (the caller ran re:run/2).
"""

from __future__ import annotations

import ipaddress

PH_CLIENTID = b"${clientid}"  # apps/emqx/include/emqx_placeholder.hrl:31
PH_USERNAME = b"${username}"  # :33

NOMATCH, ALLOW, DENY, BAD = 0, 1, 2, 3
TAG_NONE = 0xFFFFFFFF
VERDICT = {"allow": ALLOW, "deny": DENY}


def _bin(x) -> bytes:
    return x if isinstance(x, bytes) else x.encode()


def _atom(x) -> str:
    return x.decode() if isinstance(x, bytes) else x


# ---- emqx_topic (apps/emqx/src/emqx_topic.erl) -----------------------------------------------
def word(b: bytes):
    """word/1, :161-164."""
    if b == b"":
        return ""
    if b == b"+":
        return "+"
    if b == b"#":
        return "#"
    return b


def words(topic: bytes):
    """words/1, :158-159: binary:split(Topic, <<"/">>, [global]) then word/1."""
    return [word(w) for w in topic.split(b"/")]


def topic_match(name, filt) -> bool:
    """match/2 on word lists, emqx_topic.erl:74-87, clause by clause (the binary '$' clauses
    :68-71 never see a list)."""
    if not name and not filt:                      # match([], []) -> true
        return True
    if name and filt and _same(name[0], filt[0]):  # match([H | T1], [H | T2])
        return topic_match(name[1:], filt[1:])
    if name and filt and filt[0] == "+" and isinstance(filt[0], str):  # match([_H | T1], ['+' | T2])
        return topic_match(name[1:], filt[1:])
    if len(filt) == 1 and filt[0] == "#" and isinstance(filt[0], str):  # match(_, ['#'])
        return True
    return False                                   # the three false clauses


def _same(a, b) -> bool:
    """Erlang =:= of two words: an atom never equals a binary."""
    return type(a) is type(b) and a == b


# ---- compile/1, :55-94 ------------------------------------------------------------------------
def parse_cidr(s):
    """esockd_cidr:parse(S, true) for IPv4 (emqx_authz_rule_SUITE.erl:64-72): {Start, End, Len},
    the start masked down to the network."""
    net = ipaddress.IPv4Network(_atom(s), strict=False)
    return (int(net.network_address), int(net.broadcast_address), net.prefixlen)


def compile_who(who):
    """compile_who/1, :62-80."""
    if not isinstance(who, tuple):
        assert _atom(who) == "all"
        return "all"
    k = _atom(who[0])
    if k in ("user", "username"):
        return ("username", ("eq", _bin(who[1])))
    if k in ("client", "clientid"):
        return ("clientid", ("eq", _bin(who[1])))
    if k == "ipaddr":
        return ("ipaddr", parse_cidr(who[1]))
    if k == "ipaddrs":
        return ("ipaddrs", [parse_cidr(c) for c in who[1]])
    if k in ("and", "or"):
        return (k, [compile_who(w) for w in who[1]])
    if k == "flag":
        return ("flag", int(who[1]))
    raise ValueError(who)


def compile_topic(t):
    """compile_topic/1, :82-91."""
    if isinstance(t, tuple):                       # {eq, Topic}
        assert _atom(t[0]) == "eq"
        return ("eq", words(_bin(t[1])))
    t = _bin(t)
    if t.startswith(b"eq "):                       # <<"eq ", Topic/binary>>
        return ("eq", words(t[3:]))
    ws = words(t)
    if PH_USERNAME in ws or PH_CLIENTID in ws:     # pattern/1, :93-94
        return ("pattern", ws)
    return ws


def compile_rule(rule):
    """compile/1, :55-60."""
    if len(rule) == 2:
        assert _atom(rule[1]) == "all"
        return (_atom(rule[0]), "all", "all", [compile_topic(b"#")])
    permission, who, action, topics = rule
    return (_atom(permission), compile_who(who), _atom(action), [compile_topic(t) for t in topics])


# ---- match/4, :117-195 ------------------------------------------------------------------------
def match_action(pubsub, action) -> bool:
    """:127-130."""
    return action == "all" or pubsub == action


def match_who(client, who) -> bool:
    """:132-165."""
    if who == "all":
        return True
    k, v = who
    if k == "username":
        return client["username"] is not None and client["username"] == v[1]
    if k == "clientid":
        return client["clientid"] is not None and client["clientid"] == v[1]
    if k == "ipaddr":
        return client["peerhost"] is not None and cidr_match(client["peerhost"], v)
    if k == "ipaddrs":
        return client["peerhost"] is not None and any(cidr_match(client["peerhost"], c) for c in v)
    if k == "and":                                 # foldl from true, :157-160
        acc = True
        for p in v:
            acc = match_who(client, p) and acc
        return acc
    if k == "or":                                  # foldl from false, :161-164
        acc = False
        for p in v:
            acc = match_who(client, p) or acc
        return acc
    if k == "flag":
        return bool((client.get("flags", 0) >> v) & 1)
    return False


def cidr_match(ip, cidr) -> bool:
    """esockd_cidr:match/2: Start =< Ip =< End; a peer that is not IPv4 never lies in an IPv4 range."""
    if not isinstance(ip, int):
        return False
    return cidr[0] <= ip <= cidr[1]


def feed_var(client, pattern):
    """feed_var/3, :182-195: the value becomes ONE word, as it is."""
    out = []
    for w in pattern:
        if w == PH_CLIENTID and isinstance(w, bytes):
            out.append(w if client["clientid"] is None else client["clientid"])
        elif w == PH_USERNAME and isinstance(w, bytes):
            out.append(w if client["username"] is None else client["username"])
        else:
            out.append(w)
    return out


def match_topic(topic_words, filt) -> bool:
    """:177-180."""
    if isinstance(filt, tuple) and filt[0] == "eq":
        return len(topic_words) == len(filt[1]) and all(_same(a, b) for a, b in zip(topic_words, filt[1]))
    return topic_match(topic_words, filt)


def match_topics(client, topic, filters) -> bool:
    """:167-175."""
    for f in filters:
        if isinstance(f, tuple) and f[0] == "pattern":
            f = feed_var(client, f[1])
        if match_topic(words(topic), f):
            return True
    return False


def match(client, pubsub, topic, rule):
    """:119-125 -> 'allow' | 'deny' | None."""
    permission, who, action, filters = rule
    if match_action(pubsub, action) and match_who(client, who) and match_topics(client, topic, filters):
        return permission
    return None


def matches(client, pubsub, topic, rules):
    """:110-115 over (compiled rule, tag) pairs -> (verdict, tag)."""
    for rule, tag in rules:
        m = match(client, pubsub, topic, rule)
        if m is not None:
            return VERDICT[m], tag
    return NOMATCH, TAG_NONE


# ---- sources and scopes -----------------------------------------------------------------------
class RefTable:
    """Up to 8 sources tried in index order (do_authorize/4, emqx_authz.erl:304-314: the first
    source that matches decides); inside a source the clientid list, the username list, the all
    list, concatenated (emqx_authz_mnesia.erl:95-111)."""

    ACTIONS = {1: "publish", 2: "subscribe", "publish": "publish", "subscribe": "subscribe"}

    def __init__(self):
        self.lists = {}    # (source, scope, key) -> [(compiled rule, tag)]
        self.clients = {}  # id -> clientinfo

    def set_list(self, source, rules, scope="all", key=None, tags=None):
        k = (source, scope, None if scope == "all" else _bin(key))
        if not rules:
            self.lists.pop(k, None)
            return
        self.lists[k] = [(compile_rule(r), tags[i] if tags is not None else i) for i, r in enumerate(rules)]

    def set_clients(self, clients):
        for c in clients:
            host = c.get("peerhost")
            if host is not None:
                try:
                    host = int(ipaddress.IPv4Address(_atom(host)))
                except ValueError:
                    host = "not-ipv4"
            self.clients[c["id"]] = {
                "clientid": None if c.get("clientid") is None else _bin(c["clientid"]),
                "username": None if c.get("username") is None else _bin(c["username"]),
                "peerhost": host, "flags": int(c.get("flags", 0))}

    def drop_clients(self, ids):
        for i in ids:
            self.clients.pop(i, None)

    def check_one(self, client_id, action, topic):
        client = self.clients.get(client_id)
        pubsub = self.ACTIONS.get(action)
        if client is None or pubsub is None:
            return BAD, TAG_NONE
        for source in range(8):
            rules = []
            if client["clientid"] is not None:
                rules += self.lists.get((source, "clientid", client["clientid"]), [])
            if client["username"] is not None:
                rules += self.lists.get((source, "username", client["username"]), [])
            rules += self.lists.get((source, "all", None), [])
            v, tag = matches(client, pubsub, _bin(topic), rules)
            if v != NOMATCH:
                return v, tag
        return NOMATCH, TAG_NONE

    def check(self, clients, actions, topics, no_match=None):
        out = [self.check_one(c, a, t) for c, a, t in zip(clients, actions, topics)]
        if no_match is not None:
            out = [(VERDICT[no_match], t) if v == NOMATCH else (v, t) for v, t in out]
        return [v for v, _ in out], [t for _, t in out]


# ---- fuzz generators shared by the CPU and GPU tests -------------------------------------------
VOCAB = [b"a", b"b", b"c", b"", b"$SYS", b"dev", b"${clientid}", b"${username}", b"+", b"#",
         b"long-word-over-sixteen-bytes"]
PRINCIPALS = [b"a", b"b", b"dev", b"", b"+", b"#", b"a/b", b"long-word-over-sixteen-bytes", b"c1", b"u1"]
CIDRS = ["10.0.0.0/8", "10.1.0.0/16", "192.168.1.7", "0.0.0.0/0", "10.1.2.128/25"]
HOSTS = ["10.1.2.3", "10.1.2.200", "192.168.1.7", "172.16.0.1", None, "::1"]


def rand_topic(rng, max_levels=5):
    return b"/".join(rng.choice(VOCAB) for _ in range(rng.randint(1, max_levels)))


def rand_filter_plain(rng, max_levels=3):
    return b"/".join(rng.choice(VOCAB[:10]) for _ in range(rng.randint(1, max_levels)))


def rand_filter(rng, max_levels=5):
    # levels from the first ten words of VOCAB (all but the long word; '+' and '#' are the ninth
    # and tenth), '#' anywhere: a non-final '#' is a plain word to match/2.  One filter in five
    # is an eq filter, half of those by the "eq " prefix.
    f = b"/".join(rng.choice(VOCAB[:10]) for _ in range(rng.randint(1, max_levels)))
    r = rng.random()
    if r < 0.1:
        return ("eq", f)
    if r < 0.2:
        return b"eq " + f
    return f


def rand_leaf(rng):
    k = rng.randrange(5)
    if k == 0:
        return ("username", rng.choice(PRINCIPALS))
    if k == 1:
        return ("clientid", rng.choice(PRINCIPALS))
    if k == 2:
        return ("ipaddr", rng.choice(CIDRS))
    if k == 3:
        return ("ipaddrs", [rng.choice(CIDRS) for _ in range(rng.randrange(3))])
    return ("flag", rng.randrange(4))


def rand_who(rng):
    k = rng.randrange(6)
    if k < 2:
        return "all"
    if k < 4:
        return rand_leaf(rng)
    return (rng.choice(["and", "or"]), [rand_leaf(rng) for _ in range(rng.randrange(4))])


def rand_rule(rng, max_topics=3):
    if rng.random() < 0.05:
        return (rng.choice(["allow", "deny"]), "all")
    return (rng.choice(["allow", "deny"]), rand_who(rng), rng.choice(["publish", "subscribe", "all"]),
            [rand_filter(rng) for _ in range(rng.randrange(max_topics + 1))])


def rand_client(rng, cid):
    return {"id": cid,
            "clientid": rng.choice(PRINCIPALS + [None]), "username": rng.choice(PRINCIPALS + [None]),
            "peerhost": rng.choice(HOSTS), "flags": rng.randrange(16)}
