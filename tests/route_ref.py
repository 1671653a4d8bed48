"""Sequential restatement of the reference's route step on Erlang-shaped terms: a node is a
``str`` (an atom), a group a ``bytes`` (a binary), the route table an ordered list of
``#route{topic, dest}`` (a bag: no record twice).  Paths are relative to the reference checkout:

  do_add_route/2      apps/emqx/src/emqx_router.erl:111-124
  do_delete_route/2   emqx_router.erl:163-171
  lookup_routes/1     emqx_router.erl:142-144
  match_routes/1      emqx_router.erl:127-133 (the matched filters are given: the engine's job)
  cleanup_routes/1    apps/emqx/src/emqx_router_helper.erl:171-175
  aggre/1             apps/emqx/src/emqx_broker.erl:261-272
  route/2, do_route/2 emqx_broker.erl:244-259

Nothing here shares code with emqx_amd: it is what tests/test_route_cpu.py and
tests/test_gpu_route.py compare the C ABI against.
"""

from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

LOCAL, SHARE, REMOTE = 1, 2, 4
MAX_NODES = 64


class Route(NamedTuple):
    topic: bytes
    dest: object  # Node :: str | {Group :: bytes, Node :: str}


def is_atom(x) -> bool:
    return isinstance(x, str)


def term_key(x):
    """Erlang term order as far as aggre/1's usort needs it: atom < tuple < binary."""
    if isinstance(x, str):
        return (0, x)
    if isinstance(x, tuple):
        return (1, len(x), tuple(term_key(e) for e in x))
    return (2, bytes(x))


def usort(terms: list) -> list:
    out = []
    for t in sorted(terms, key=term_key):
        if not out or out[-1] != t:
            out.append(t)
    return out


class RouteTab:
    """?ROUTE_TAB: ets bag, keyed by topic."""

    def __init__(self, node: str):
        self.node = node
        self.tab: List[Route] = []
        self._index: Optional[Dict[bytes, List[Route]]] = None

    def _by_topic(self) -> Dict[bytes, List[Route]]:
        if self._index is None:
            self._index = {}
            for r in self.tab:
                self._index.setdefault(r.topic, []).append(r)
        return self._index

    def lookup_routes(self, topic: bytes) -> List[Route]:
        return list(self._by_topic().get(topic, ()))

    def has_routes(self, topic: bytes) -> bool:
        return topic in self._by_topic()

    def topics(self) -> List[bytes]:
        return list(self._by_topic())

    def do_add_route(self, topic: bytes, dest=None) -> None:
        route = Route(topic, self.node if dest is None else dest)
        if route in self.lookup_routes(topic):  # lists:member(Route, lookup_routes(Topic))
            return
        self.tab.append(route)
        self._index = None

    def do_delete_route(self, topic: bytes, dest=None) -> None:
        route = Route(topic, self.node if dest is None else dest)
        if route in self.tab:
            self.tab.remove(route)
            self._index = None

    def match_routes(self, matched: Sequence[bytes]) -> List[Route]:
        """lists:append([lookup_routes(To) || To <- Matched]); ``Matched`` is what the trie and
        the exact lookup give for the topic."""
        out: List[Route] = []
        for to in matched:
            out += self.lookup_routes(to)
        return out

    def cleanup_routes(self, node: str) -> None:
        patterns = (lambda d: d == node, lambda d: isinstance(d, tuple) and d[1] == node)
        for pat in patterns:
            for route in [r for r in self.tab if pat(r.dest)]:
                self.tab.remove(route)
        self._index = None


def aggre(routes: List[Route]) -> list:
    if routes == []:
        return []
    if len(routes) == 1 and is_atom(routes[0].dest):
        return [(routes[0].topic, routes[0].dest)]
    if len(routes) == 1:
        group, _node = routes[0].dest
        return [(routes[0].topic, group)]
    acc: list = []
    for r in routes:  # lists:foldl
        if is_atom(r.dest):
            acc = [(r.topic, r.dest)] + acc
        else:
            group, _node = r.dest
            acc = usort([(r.topic, group)] + acc)
    return acc


def aggre_sets(routes: List[Route]) -> list:
    """The independent formulation: the plain routes, one each, and the distinct (To, Group)."""
    plain = [(r.topic, r.dest) for r in routes if is_atom(r.dest)]
    groups = {(r.topic, r.dest[0]) for r in routes if not is_atom(r.dest)}
    return plain + sorted(groups)


def do_route(entry, node: str):
    to, dest = entry
    if is_atom(dest) and dest == node:
        return ("dispatch", to)
    if is_atom(dest):
        return ("forward", dest, to)
    return ("share", to, dest)


def route(entries: list, node: str):
    if entries == []:
        return "dropped"  # 'message.dropped', no_subscribers
    acc = []
    for e in entries:
        acc = [do_route(e, node)] + acc
    return acc


class Expected(NamedTuple):
    entry_flags: List[int]
    msg_routes: List[int]
    forwards: Dict[str, List[Tuple[int, int]]]  # node -> [(message, filter id)] in entry order
    local: List[List[int]]                       # per message the filter ids kept
    summary: Dict[str, int]


def route_batch(tab: RouteTab, names: Dict[int, bytes], offsets: Sequence[int], filters: Sequence[int]) -> Expected:
    """The route step for a batch given as a CSR of filter ids; ``names`` maps an id to its topic
    filter (an id it lacks matches nothing the table knows).  Each entry is aggregated on its
    own: for distinct ids within a message that is aggre/1 of the concatenation, because the
    entries differ in ``To`` (tests/test_route_ref.py checks it)."""
    n = len(offsets) - 1
    flags, counts, local = [], [], []
    fwd: Dict[str, List[Tuple[int, int]]] = {}
    dropped = fwd_msgs = 0
    for i in range(n):
        total, any_fwd, keep = 0, False, []
        for d in range(int(offsets[i]), int(offsets[i + 1])):
            f = int(filters[d])
            to = names.get(f)
            done = route(aggre(tab.lookup_routes(to)) if to is not None else [], tab.node)
            fl = 0
            if done != "dropped":
                total += len(done)
                for r in reversed(done):  # in the order aggre/1 listed them
                    if r[0] == "dispatch":
                        fl |= LOCAL
                    elif r[0] == "share":
                        fl |= SHARE
                    else:
                        fl |= REMOTE
                        fwd.setdefault(r[1], []).append((i, f))
                        any_fwd = True
            flags.append(fl)
            if fl & (LOCAL | SHARE):
                keep.append(f)
        counts.append(total)
        local.append(keep)
        dropped += total == 0
        fwd_msgs += any_fwd
    summary = dict(flags=0, entries=len(flags), forwards=sum(map(len, fwd.values())), dropped=dropped,
                   forwarding_messages=fwd_msgs, kept=sum(map(len, local)), unknown=sum(1 for x in flags if x == 0),
                   forward_nodes=len(fwd))
    return Expected(flags, counts, fwd, local, summary)
