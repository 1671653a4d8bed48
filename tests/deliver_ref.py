"""A line-for-line restatement of the delivery path of a subscriber's session in the reference
(apps/emqx/src/emqx_session.erl, EMQX 5.0.0-beta.3): ``ignore_local/3`` (:280-291) and
``enrich_fun/1`` / ``get_subopts/2`` / ``enrich_subopts/3`` (:554-598), and a helper that runs a
whole delivery CSR through it.  The checker of emqx_deliver.h; nothing here shares code with it.

A session is ``{"subscriptions": {filter: subopts dict}, "upgrade_qos": bool}``; a message is a
dict with ``from``, ``qos``, ``flags`` (``{"retain": bool}``, ``"nl"`` once set) and ``headers``
(``{"retained": True}`` on the retainer's dispatch path, ``"properties"``).
"""

NO_SENDER = 0xFFFFFFFF
SHARED_BIT, RETRY_BIT = 0x80000000, 0x40000000
OUT_RETAIN, OUT_NL, OUT_DROP, OUT_NO_SUBOPTS, OUT_BAD = 0x04, 0x08, 0x10, 0x20, 0x40


def dropwhile(pred, xs):
    """lists:dropwhile/2."""
    i = 0
    while i < len(xs) and pred(xs[i]):
        i += 1
    return xs[i:]


def no_local_hit(deliver, subscriber, session):
    """The fun of ignore_local/3, emqx_session.erl:282-290."""
    topic, msg = deliver                       # :282 {deliver, Topic, #message{from = Publisher}}
    subs = session["subscriptions"]            # :281 Subs = info(subscriptions, Session)
    found = subs.get(topic)                    # :283 maps:find(Topic, Subs)
    if found is not None and found.get("nl") == 1 and subscriber == msg["from"]:  # :284
        return True                            # :285-287 the two metrics, true
    return False                               # :288-289 _ -> false


def ignore_local(delivers, subscriber, session):
    """emqx_session.erl:280-291, with its literal lists:dropwhile: only the LEADING run of hits goes."""
    return dropwhile(lambda d: no_local_hit(d, subscriber, session), delivers)


def get_subopts(topic, submap):
    """emqx_session.erl:569-576."""
    found = submap.get(topic)                  # :570 maps:find(Topic, SubMap)
    if found is not None and "subid" in found:  # :571-572
        return [("nl", found["nl"]), ("qos", found["qos"]), ("rap", found["rap"]), ("subid", found["subid"])]
    if found is not None:                      # :573-574
        return [("nl", found["nl"]), ("qos", found["qos"]), ("rap", found["rap"])]
    return []                                  # :575 error -> []


def enrich_subopts(opts, msg, session):
    """emqx_session.erl:578-598 (the recursion as a loop over the list, clause for clause)."""
    msg = dict(msg, flags=dict(msg["flags"]), headers=dict(msg["headers"]))  # terms are immutable there
    for key, val in opts:
        if key == "nl" and val == 1:           # :579-580
            msg["flags"]["nl"] = True
        elif key == "nl" and val == 0:         # :581-582
            pass
        elif key == "qos" and session["upgrade_qos"] is True:   # :583-585
            msg["qos"] = max(val, msg["qos"])
        elif key == "qos" and session["upgrade_qos"] is False:  # :586-588
            msg["qos"] = min(val, msg["qos"])
        elif key == "rap" and val == 1:        # :589-590
            pass
        elif key == "rap" and val == 0 and msg["headers"].get("retained") is True:  # :591-592
            pass
        elif key == "rap" and val == 0:        # :593-594 set_flag(retain, false, Msg)
            msg["flags"]["retain"] = False
        elif key == "subid":                   # :595-598
            props = dict(msg["headers"].get("properties", {}))
            props["Subscription-Identifier"] = val
            msg["headers"]["properties"] = props
        else:
            raise ValueError("function_clause: %r" % ((key, val),))
    return msg                                 # :578 [] -> Msg


def enrich(deliver, session):
    """enrich_fun/1, emqx_session.erl:554-557."""
    topic, msg = deliver
    return enrich_subopts(get_subopts(topic, session["subscriptions"]), msg, session)


# ---- the C ABI's encoding of the above ------------------------------------------------------

def message(qos, flags, frm):
    """A #message{} from the per-message inputs of emqx_deliver.h."""
    return {"from": frm, "qos": qos, "flags": {"retain": bool(flags & 1)},
            "headers": {"retained": True} if flags & 2 else {}}


def output(deliver, subscriber, session):
    """(options byte, subid) of one delivery: ignore_local of the one-element list, then enrich."""
    topic, msg = deliver
    dropped = ignore_local([deliver], subscriber, session) == []
    out = enrich(deliver, session)
    byte = out["qos"] | (OUT_RETAIN if out["flags"].get("retain") else 0) | (OUT_NL if out["flags"].get("nl") else 0)
    if dropped:
        byte |= OUT_DROP
    if topic not in session["subscriptions"]:
        byte |= OUT_NO_SUBOPTS
    return byte, out["headers"].get("properties", {}).get("Subscription-Identifier", 0)


class Sessions:
    """subscriber id -> session, filled as emqx_session:subscribe/4 does (maps:put, :300-309)."""

    def __init__(self):
        self.sessions = {}

    def set(self, filt, sub, qos=0, nl=0, rap=0, upgrade_qos=False, subid=None):
        s = self.sessions.setdefault(sub, {"subscriptions": {}, "upgrade_qos": False})
        s["upgrade_qos"] = bool(upgrade_qos)
        opts = {"qos": int(qos), "nl": int(nl), "rap": int(rap)}
        if subid:
            opts["subid"] = int(subid)
        s["subscriptions"][filt] = opts

    def remove(self, filt, sub):
        self.sessions.get(sub, {"subscriptions": {}})["subscriptions"].pop(filt, None)

    def drop_subscriber(self, sub):
        self.sessions.pop(sub, None)

    def session(self, sub):
        return self.sessions.get(sub, {"subscriptions": {}, "upgrade_qos": False})


def run_csr(sessions, offsets, subs, filters, qos, flags, frm=None):
    """Every delivery of a CSR through output(): dict with ``opts``, ``subids``, the compacted CSR
    ``kept`` = (offsets, subs, filters, opts, subids) and ``summary`` (the 8 words, flags 0)."""
    n = len(offsets) - 1
    opts, subids = [], []
    k_off, k_subs, k_fil, k_opts, k_ids = [0], [], [], [], []
    dropped = no_subopts = 0
    by_qos = [0, 0, 0]
    for i in range(n):
        q, fl = int(qos[i]), int(flags[i])
        sender = NO_SENDER if frm is None else int(frm[i])
        bad = q > 2 or (fl & ~3)
        for d in range(int(offsets[i]), int(offsets[i + 1])):
            s, word = int(subs[d]), int(filters[d])
            if bad:
                byte, sid = OUT_BAD, 0
            else:
                f = word & ~(SHARED_BIT | RETRY_BIT)
                msg = message(q, fl, None if sender == NO_SENDER else sender)
                byte, sid = output((f, msg), s, sessions.session(s))
            opts.append(byte)
            subids.append(sid)
            no_subopts += bool(byte & OUT_NO_SUBOPTS)
            if byte & OUT_DROP:
                dropped += 1
                continue
            k_subs.append(s)
            k_fil.append(word)
            k_opts.append(byte)
            k_ids.append(sid)
            if not bad:
                by_qos[byte & 3] += 1
        k_off.append(len(k_subs))
    total = int(offsets[n]) if n else 0
    return {"opts": opts, "subids": subids, "kept": (k_off, k_subs, k_fil, k_opts, k_ids),
            "summary": [0, total, len(k_subs), dropped, no_subopts] + by_qos}
