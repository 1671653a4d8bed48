"""The inbox stage restated in numpy (include/emqx_inbox.h): the stable sort of the delivery
positions by subscriber, the message of each position by a search over the offsets, the inboxes
from np.unique.  Nothing here shares code with the library."""

import numpy as np

SUMMARY_WORDS = 8
F_BOX_OVERFLOW, F_INPUT_REFUSED, F_BAD_SUB = 1, 2, 4
SHARED_BIT, RETRY_BIT = 0x80000000, 0x40000000


def group(offsets, subs, filters, sub_limit, opts=None, subids=None, cap_boxes=None, cap_in=None):
    """A dict of lists: inbox_subs, inbox_offsets, msgs, filters, opts, subids, src, summary.
    ``cap_boxes`` None: min(cap_in, sub_limit), which never overflows."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    subs = np.asarray(subs, dtype=np.uint32)
    filters = np.asarray(filters, dtype=np.uint32)
    n = offsets.size - 1
    total = int(offsets[n])
    cap_in = subs.size if cap_in is None else cap_in
    if cap_boxes is None:
        cap_boxes = min(cap_in, sub_limit)
    out = {"inbox_subs": [], "inbox_offsets": [], "msgs": [], "filters": [], "opts": [], "subids": [], "src": []}
    if total > cap_in or total >= 1 << 32 or n >= 1 << 32:
        out["summary"] = [F_INPUT_REFUSED, total, 0, 0, 0, 0, 0, 0]
        return out
    subs, filters = subs[:total], filters[:total]
    messages = int(np.count_nonzero(np.diff(offsets.astype(np.int64)) > 0))
    if total and int(subs.max()) >= sub_limit:
        out["summary"] = [F_BAD_SUB, total, 0, 0, messages, 0, 0, 0]
        return out
    perm = np.argsort(subs, kind="stable")
    out["src"] = perm.tolist()
    out["msgs"] = (np.searchsorted(offsets, perm.astype(np.uint64), side="right") - 1).tolist()
    out["filters"] = filters[perm].tolist()
    if opts is not None:
        out["opts"] = np.asarray(opts, dtype=np.uint8)[:total][perm].tolist()
    if subids is not None:
        out["subids"] = np.asarray(subids, dtype=np.uint32)[:total][perm].tolist()
    ids, counts = np.unique(subs, return_counts=True)
    m = int(ids.size)
    ends = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    flags = 0
    if m > cap_boxes:
        flags = F_BOX_OVERFLOW
        out["inbox_subs"], out["inbox_offsets"] = ids[:cap_boxes].tolist(), ends[:cap_boxes + 1].tolist()
    else:
        out["inbox_subs"], out["inbox_offsets"] = ids.tolist(), ends.tolist()
    out["summary"] = [flags, total, m, int(counts.max()) if m else 0, messages, 0, 0, 0]
    return out
