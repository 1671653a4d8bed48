"""The fast path's slab entries (GPU): the 4-byte and the 8-byte format, and the walk's own
resolution of fids[] ids.

The engine picks the entry format per full build from the ids the table reports: the narrow
one when they all lie below 2^26 - 1, else the wide one.  The tests steer that choice the way
a deployment would — through the reported ids (emqx_insert_filters_ext) — and compare every
topic id-for-id with the brute-force oracle, the two formats with each other, and the walk
order and the async entry point with the synchronous batch-order call.  The batched kernels are
the subject, so the one-launch small-batch path is switched off unless a test says otherwise."""

import numpy as np
import pytest

from oracle import emqx_ref as R

pytestmark = pytest.mark.gpu

NARROW_IDS = (1 << 26) - 1  # the narrow format takes ids below this (layout.h SLAB_NARROW_IDS)
NEVER = b"\x01never/\x01matched"


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (shares the HIP runtime with the engine)
    from emqx_amd.engine import Engine as E
    from emqx_amd import _lib
    _lib.lib()
    return E


def oracle_rows(filters, topics, mode):
    """Per topic, the indices of the matching filters (the brute-force oracle)."""
    if mode == 0:
        return [R.brute_force_routes(filters, t) for t in topics]
    if mode == 1:
        return [R.brute_force_trie(filters, t) for t in topics]
    wild = [f if R.wildcard(f) else b"\x00never" for f in filters]
    return [R.brute_force_trie(wild, t) for t in topics]


def reported(rows, ext):
    return [sorted(int(ext[i]) for i in row) for row in rows]


def expected(filters, ext, topics, mode):
    return reported(oracle_rows(filters, topics, mode), ext)


def engine_ext(Engine, filters, ext, small=0):
    from emqx_amd.engine import pack
    e = Engine()
    ids = e.insert_packed_ext(*pack(list(filters)), np.asarray(ext, dtype=np.uint32))
    assert list(ids) == list(range(len(filters)))
    e.commit()
    e.set_tuning("small_batch", small)
    return e


def mixed_table():
    """All three kinds of found child: edgeless leaves (ids inline in the slot), children with
    edges and one id (META_XFID), children with edges, a '#' and a terminal filter (ids in fids[],
    loaded by the walk) — below the root, below a literal and below '+'."""
    f = [b"#", b"+/#", b"$SYS/#", b"+", b"+/m", b"d/+", b"d/+/#", b"d/+/k/+"]
    for i in range(24):
        f += [b"a/b%d" % i, b"a/c%d/#" % i]                             # edgeless leaves
        f += [b"x%d" % i, b"x%d/y" % i, b"h%d/#" % i, b"h%d/z" % i]      # one id + edges
        f += [b"r%d" % i, b"r%d/#" % i, b"r%d/k" % i]                    # '#' + terminal + edges
        f += [b"d/r%d" % i, b"d/r%d/#" % i, b"d/r%d/k/l" % i]
    return f


def mixed_topics():
    t = []
    for i in range(24):
        t += [b"r%d" % i, b"r%d/k" % i, b"x%d" % i, b"d/r%d" % i, b"d/r%d/k/l" % i]
    t += [b"a/b3", b"a/c5/q/w", b"h2/z", b"h7", b"x9/y", b"$SYS/x", b"$SYS", b"", b"/", b"nope", b"d/zz/k/q",
          b"+/m", b"r1/#", b"d/+"]
    t = (t * 2)[:130]  # two full tiles and a partial one
    assert len(t) == 130
    return t


def wide_ext(n):
    """Reported ids that force the wide format and put large ids on matching filters."""
    return [i if i % 2 == 0 else (1 << 26) + 7 * i for i in range(n)]


@pytest.fixture(scope="module")
def mixed(Engine):
    f, t = mixed_table(), mixed_topics()
    ext = {"narrow": list(range(len(f))), "wide": wide_ext(len(f))}
    rows = {m: oracle_rows(f, t, m) for m in (0, 1, 2)}  # computed once, shared by the tests below
    exp = {(k, m): reported(rows[m], ext[k]) for k in ext for m in (0, 1, 2)}
    return f, t, ext, exp, rows[0]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("fmt", ["narrow", "wide"])
def test_mixed_table_every_mode(Engine, mixed, fmt, mode):
    f, t, ext, exp, _ = mixed
    e = engine_ext(Engine, f, ext[fmt])
    got = e.match(t, mode=mode)
    for topic, g, x in zip(t, got, exp[(fmt, mode)]):
        assert g == x, (fmt, mode, topic, g, x)
    if mode == 0:  # ids the walk reads from fids[]: a child with a '#', a terminal filter and edges
        assert {ext[fmt][f.index(b"r5")], ext[fmt][f.index(b"r5/#")]} <= set(got[t.index(b"r5")])


def test_mixed_table_small_batch_kernel(Engine, mixed):
    """The one-launch kernel shares the walk and keeps the wide entry on a table whose batched
    calls use the narrow one."""
    f, t, ext, exp, _ = mixed
    e = engine_ext(Engine, f, ext["narrow"], small=1)
    assert e.match(t, mode=0) == exp[("narrow", 0)]


def device_csr(e, topics, mode=0, order=None, asynchronous=False):
    import torch
    from emqx_amd.engine import pack
    dev = torch.device("cuda:0")
    tb_np, to_np = pack(list(topics))
    tb = torch.from_numpy(np.array(tb_np)).to(dev)
    to = torch.from_numpy(to_np.view(np.int64)).to(dev)
    n = len(topics)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(1 << 20, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    if order is not None:
        e.set_tuning("order", order)
    try:
        if asynchronous:
            summ = torch.zeros(8, dtype=torch.int64, device=dev)
            e.match_device_async(tb.data_ptr(), to.data_ptr(), n, d_off.data_ptr(), d_ids.data_ptr(), d_ids.numel(),
                                 summ.data_ptr(), mode=mode, stream=s)
            torch.cuda.synchronize()
            assert int(summ[0]) == 0, summ.tolist()
            total = int(summ[1])
        else:
            total = e.match_device(tb.data_ptr(), to.data_ptr(), n, d_off.data_ptr(), d_ids.data_ptr(), d_ids.numel(),
                                   mode=mode, stream=s)
    finally:
        if order is not None:
            e.set_tuning("order", -1)
    off = d_off.cpu().numpy().view(np.uint64)
    ids = d_ids[:total].cpu().numpy().view(np.uint32)
    assert int(off[-1]) == total
    return off, [sorted(ids[off[i]:off[i + 1]].tolist()) for i in range(n)]


@pytest.mark.parametrize("fmt", ["narrow", "wide"])
def test_walk_order_and_async_give_the_sync_csr(Engine, mixed, fmt):
    f, t, ext, exp, _ = mixed
    e = engine_ext(Engine, f, ext[fmt])
    off0, rows0 = device_csr(e, t, order=0)
    assert rows0 == exp[(fmt, 0)]
    off1, rows1 = device_csr(e, t, order=1)            # the a.perm path
    off2, rows2 = device_csr(e, t, asynchronous=True)  # no rerun, no host read of the summary
    assert np.array_equal(off1, off0) and rows1 == rows0
    assert np.array_equal(off2, off0) and rows2 == rows0


def test_formats_agree_at_the_boundary(Engine, mixed):
    """Ids up to the narrow format's last one (2^26 - 2, owner 63: the entry next to the
    padding marker) on one engine; the same table plus one filter nothing matches whose id no
    longer fits (2^26 - 1, the marker's id bits) on another, which must take the wide format.
    Same input, same CSR, and both equal the oracle."""
    f, t, _, _, rows0 = mixed
    n = len(f)
    ext = [NARROW_IDS - 1 - i for i in range(n)]  # 2^26 - 2 downwards: '#' (every topic, lane 63 too)
    assert max(ext) == NARROW_IDS - 1 and f[0] == b"#"
    exp = reported(rows0, ext)
    a = engine_ext(Engine, f, ext)
    b = engine_ext(Engine, f + [NEVER], ext + [NARROW_IDS])
    off_a, rows_a = device_csr(a, t)
    off_b, rows_b = device_csr(b, t)
    assert rows_a == exp
    assert np.array_equal(off_a, off_b) and rows_a == rows_b
    assert NARROW_IDS - 1 in rows_a[63]


@pytest.mark.parametrize("big", [NARROW_IDS, 1 << 26, (1 << 32) - 2])
def test_ids_past_the_boundary_are_reported_whole(Engine, mixed, big):
    """A matching filter whose id is the first that does not fit, the first with bit 26 set, and
    the largest id there is: packed into a narrow entry each would come out wrong or vanish (the
    first is the padding marker on lane 63, the others spill into the owner bits)."""
    f, t, _, _, rows0 = mixed
    ext = list(range(len(f)))
    ext[0] = big  # '#': on every topic that is not a '$' topic, lanes 0 and 63 included
    e = engine_ext(Engine, f, ext)
    _, rows = device_csr(e, t)
    assert rows == reported(rows0, ext)
    assert big in rows[0] and big in rows[63]


def test_ids_pushed_past_the_boundary_by_later_commits(Engine, mixed):
    """A table that starts within the narrow format and grows out of it: each commit's calls
    report every id whole (a commit that brings in an id the committed tables' format cannot
    hold builds fresh tables, which choose their format anew), deletes included."""
    from emqx_amd.engine import pack
    f, t, _, _, _ = mixed
    f, ext = list(f), list(range(len(f)))
    e = engine_ext(Engine, f, ext)
    for filt, fid in ((b"r1/new/+", NARROW_IDS - 1), (b"r1/+/+", NARROW_IDS), (b"r1/new/#", 1 << 30), (b"r2/+", 5000)):
        f.append(filt)
        ext.append(fid)
        e.insert_packed_ext(*pack([filt]), np.asarray([fid], dtype=np.uint32))
        e.commit()
        topics = t + [b"r1/new/x", b"r2/k"]
        _, rows = device_csr(e, topics)
        assert rows == expected(f, ext, topics, 0)
    e.delete([len(f) - 3, len(f) - 2])  # the two ids that do not fit
    e.commit()
    live = f[:-3] + [NEVER + b"1", NEVER + b"2"] + f[-1:]
    _, rows = device_csr(e, topics)
    assert rows == expected(live, ext, topics, 0)


def test_owner_field_and_slab_growth(Engine):
    """One tile whose first and last topic (owners 0 and 63) both have matches and one of whose
    topics is matched by thousands of filters: the slab grows and the call reruns, in the narrow
    format (ids from 0) and in the wide one."""
    words = [b"w%d" % i for i in range(10)]
    filters = [b"first", b"last/#"]
    for n in range(11):  # every literal / '+' pattern of the hot topic and of its prefixes + '#': 2047 matches
        for m in range(1 << n):
            lv = [b"+" if (m >> i) & 1 else words[i] for i in range(n)]
            filters.append(b"/".join(lv + [b"#"]) if n < 10 else b"/".join(lv))
    hot = b"/".join(words)
    topics = [b"first"] + [b"/".join(words[:1 + i % 9]) for i in range(30)] + [hot] + [b"q/%d" % i for i in range(31)]
    topics += [b"last/one"]
    assert len(topics) == 64
    rows = oracle_rows(filters, topics, 0)
    assert rows[0] and rows[63] and len(rows[31]) > 2000
    for ext in (list(range(len(filters))), wide_ext(len(filters))):
        exp = reported(rows, ext)
        e = engine_ext(Engine, filters, ext)
        assert e.match(topics, mode=0) == exp  # host batch: async call, then the rerun
        e2 = engine_ext(Engine, filters, ext)
        _, got = device_csr(e2, topics)        # synchronous call: rerun in place
        assert got == exp
