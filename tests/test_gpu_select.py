"""The select stage on the device (include/emqx_select.h): every entry point against sets
computed from the contract (tests/select_cases.py) and against the host evaluator, the wave and
tile boundaries of the look-back and of the compaction, overflow and refusal, snapshot lifetime
across a commit, and the match -> select chain on one stream against the restatement
(tests/select_ref.py)."""

import os
import subprocess

import numpy as np
import pytest

from tests import select_cases as C
from tests import select_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S32, S64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
TAIL = 64  # sentinel words behind out_owners[cap_out]


@pytest.fixture(scope="module")
def S():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from emqx_amd import select
    return select


def dev(a, dtype):
    import torch
    view = {np.uint64: np.int64, np.uint32: np.int32}.get(dtype, dtype)
    a = np.array(a, dtype=dtype)  # a writable copy
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)
    return torch.from_numpy(a.view(view)).to(DEV)


class DeviceBatch:
    """A case's batch in device memory with sentinel-filled outputs."""

    def __init__(self, S, case, cap_out=None, cap_in=None):
        import torch
        off, fils, classes = case.batch
        self.n, self.total = len(off) - 1, len(fils)
        self.cap_in = self.total if cap_in is None else cap_in
        self.cap_out = case.reference()["summary"][3] if cap_out is None else cap_out
        self.ins = [dev(off, np.uint64), dev(fils, np.uint32), None if classes is None else dev(classes, np.uint32)]
        self.ooff = torch.full((self.n + 1,), S64, dtype=torch.int64, device=DEV)
        self.owners = torch.full((self.cap_out + TAIL,), S32, dtype=torch.int32, device=DEV)
        self.summary = torch.full((8,), S64, dtype=torch.int64, device=DEV)
        i = self.ins
        self.args = S.OwnerTable.batch(i[0].data_ptr(), i[1].data_ptr(), self.n, self.cap_in,
                                       0 if i[2] is None else i[2].data_ptr(), self.ooff.data_ptr(),
                                       self.owners.data_ptr(), self.cap_out)

    def summary_dict(self, S):
        return dict(zip(S.SUMMARY, self.summary.cpu().numpy().view(np.uint64).tolist()))

    def owners_host(self):
        return self.owners.cpu().numpy().view(np.uint32)

    def result(self, S, summary=None):
        summary = self.summary_dict(S) if summary is None else summary
        own = self.owners_host()
        assert (own[self.cap_out:] == S32).all(), "nothing behind out_owners[cap_out]"
        return S.Selected(self.ooff.cpu().numpy().view(np.uint64), own[:summary["selected"]], summary)


def run_sync(S, t, case, **kw):
    b = DeviceBatch(S, case, **kw)
    return b.result(S, t.select_device(b.args))


def run_async(S, t, case, **kw):
    import torch
    b = DeviceBatch(S, case, **kw)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())  # the buffers were filled there
    with torch.cuda.stream(stream):
        t.select_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return b.result(S)


def all_forms(S, t, case):
    """Every entry point, exact against the contract's sets and identical to the host evaluator;
    the device forms with cap_out exactly enough."""
    host = t.select_host(*case.batch)
    C.check(case, host)
    for got in (t.select_packed(*case.batch), t.select_packed(*case.batch, cap_out=host.summary["selected"]),
                run_sync(S, t, case), run_async(S, t, case)):
        C.check(case, got)
        assert got.rows() == host.rows() and got.summary == host.summary


@pytest.mark.parametrize("name, match_all, masked", C.SHAPE_CASES)
def test_shapes(S, name, match_all, masked):
    """n = 0 and 1; 0, 1, 63..65, 255..257 and 10 002 entries with empty messages before, between
    and after; with and without match-all owners; masks of 0, one class and all classes; disabled
    owners, repeated, unheld and unknown filter ids, a posting list of 65."""
    case = C.shape(name, match_all, masked)
    all_forms(S, case.load(S.OwnerTable(0)), case)


@pytest.mark.parametrize("blocks", [1, 3])
def test_blocks_stride_over_the_tiles(S, blocks):
    case = C.shape("e10002")
    t = S.OwnerTable(0)
    t.set_tuning("max_blocks", blocks)
    all_forms(S, case.load(t), case)


@pytest.mark.parametrize("match_all", [True, False])
@pytest.mark.parametrize("start", [0, 3])
def test_straddle(S, start, match_all):
    """The same owner behind entries 63 and 64, and behind entries 255 and 256, of one message."""
    case = C.straddle(start, match_all)
    all_forms(S, case.load(S.OwnerTable(0)), case)


@pytest.mark.parametrize("match_all", [True, False])
@pytest.mark.parametrize("form", ["packed", "sync", "async"])
def test_out_overflow(S, form, match_all):
    """cap_out one short: summary bit 0, complete out_offsets, out_owners untouched."""
    from emqx_amd import _lib
    import torch
    case = C.shape("e257", match_all, True)
    t = case.load(S.OwnerTable(0))
    ref = case.reference()
    need = ref["summary"][3]
    if form == "packed":
        with pytest.raises(_lib.EngineError) as e:
            t.select_packed(*case.batch, cap_out=need - 1)
        assert e.value.code == _lib.EMQX_EOVERFLOW and e.value.needed == need and e.value.summary["flags"] == 1
        assert e.value.out_offsets.tolist() == ref["offsets"] and not e.value.out_owners.any()
        return
    b = DeviceBatch(S, case, cap_out=need - 1)
    if form == "sync":
        with pytest.raises(_lib.EngineError) as e:
            t.select_device(b.args)
        assert e.value.code == _lib.EMQX_EOVERFLOW and e.value.needed == need
        summary = e.value.summary
    else:
        t.select_device_async(b.args, b.summary.data_ptr())
        torch.cuda.synchronize()
        summary = b.summary_dict(S)
    assert [summary[k] for k in S.SUMMARY] == [1] + ref["summary"][1:]
    assert b.ooff.cpu().numpy().view(np.uint64).tolist() == ref["offsets"]
    assert (b.owners_host() == S32).all()


@pytest.mark.parametrize("form", ["sync", "async"])
def test_input_refused(S, form):
    """offsets[n] > cap_in (the match in front overflowed): summary bit 1, nothing else written."""
    from emqx_amd import _lib
    import torch
    case = C.shape("e257")
    t = case.load(S.OwnerTable(0))
    b = DeviceBatch(S, case, cap_in=256)
    if form == "sync":
        with pytest.raises(_lib.EngineError) as e:
            t.select_device(b.args)
        assert e.value.code == _lib.EMQX_EINVAL
        summary = e.value.summary
    else:
        t.select_device_async(b.args, b.summary.data_ptr())
        torch.cuda.synchronize()
        summary = b.summary_dict(S)
    assert [summary[k] for k in S.SUMMARY] == [2, 257, 0, 0, 0, 0, 0, 0]
    assert (b.owners_host() == S32).all()
    assert (b.ooff.cpu().numpy().view(np.uint64) == S64).all()


def test_wild_device_offsets_stay_in_bounds(S):
    """Offsets that decrease and exceed the count (only their last entry is within cap_in): the
    call completes, reads 200 entries, and writes nothing behind out_owners[cap_out]."""
    import torch
    case = C.shape("e257")
    t = case.load(S.OwnerTable(0))
    b = DeviceBatch(S, case, cap_out=300)
    b.ins[0].copy_(dev([0, 900, 5, 1 << 40, 2, 200], np.uint64))
    t.select_device_async(b.args, b.summary.data_ptr())
    torch.cuda.synchronize()
    s = b.summary_dict(S)
    assert s["flags"] in (0, 1) and s["entries"] == 200
    assert (b.owners_host()[300:] == S32).all()


def test_async_call_keeps_its_snapshot_across_a_commit(S):
    import torch
    case = C.shape("e10002")
    t = case.load(S.OwnerTable(0))
    stream = torch.cuda.Stream(device=DEV)
    calls = [DeviceBatch(S, case) for _ in range(3)]
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for b in calls:
            t.select_device_async(b.args, b.summary.data_ptr(), stream=stream.cuda_stream)
    # remove half of the owners while the calls may still be running: they answer from the old snapshot
    gone = [o[0] for o in case.owners[::2]]
    t.remove(gone)
    t.commit()
    stream.synchronize()
    for b in calls:
        C.check(case, b.result(S))
    after = C.Case("e10002_half", case.owners[1::2], *case.batch)
    got = run_async(S, t, after)
    C.check(after, got)
    assert 0 < got.summary["selected"] < case.reference()["summary"][3]
    assert t.stats()["n_owners"] == len(case.owners) - len(gone) and t.stats()["epoch"] == 2


def test_known_answers_on_the_device(S):
    import json
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "select_kats.json")))["cases"]
    for kat in kats:
        index = R.load(kat["world"], S.HookIndex(0))
        assert R.selected(index, kat["world"], kat["messages"]) == kat["expect"], kat["name"]
        index.close()


def test_match_then_select_on_one_stream(S):
    """emqx_match_batch_device_async -> emqx_select_batch_device_async on one stream, no host read
    in between: 300 rules, bridges and exhook entries, 2 000 messages over 150 topics with
    $SYS/... (some flagged sys) and $events/... names; the owners equal the restatement computed
    from the strings."""
    import torch
    from emqx_amd.engine import pack
    w = C.world(300, 80, seed=5)
    index = R.load(w, S.HookIndex(0))
    n = 2000
    msgs = C.messages(n, 150, seed=8)
    want = C.world_expected(w, msgs)
    assert any(m["sys"] for m in msgs) and any(m["topic"].startswith("$events/") for m in msgs)
    assert sum(map(len, want)) > 20000
    # the synchronous path of the same index first: it sizes the engine's match scratch for this batch, as
    # include/emqx_match.h asks of a caller of the asynchronous match (summary flag 1 otherwise)
    assert R.selected(index, w, msgs) == want
    buf, offs = pack([m["topic"].encode() for m in msgs])
    d_buf, d_off = dev(buf, np.uint8), dev(offs, np.uint64)
    d_cls = dev([index.message_classes(m["sys"], w["ignore_sys_message"]) for m in msgs], np.uint32)
    cap_match, cap_out = 128 * n, 300 * n
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    d_moff, d_mids, d_ms = z(n + 1, torch.int64), z(cap_match, torch.int32), z(8, torch.int64)
    d_ooff, d_own, d_sum = z(n + 1, torch.int64), z(cap_out, torch.int32), z(8, torch.int64)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        index.select_device_async(d_buf.data_ptr(), d_off.data_ptr(), n, d_moff.data_ptr(), d_mids.data_ptr(),
                                  cap_match, d_ms.data_ptr(), d_cls.data_ptr(), d_ooff.data_ptr(), d_own.data_ptr(),
                                  cap_out, d_sum.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert int(d_ms[0]) == 0, "the match completed in one pass"
    s = d_sum.cpu().numpy().view(np.uint64).tolist()
    assert s[0] == 0 and s[1] == int(d_ms[1]) and s[3] == sum(map(len, want))
    off, own = d_ooff.cpu().numpy(), d_own.cpu().numpy().view(np.uint32)
    for i in range(n):
        got = sorted("%s:%s" % index.owner_key(int(o)) for o in own[int(off[i]):int(off[i + 1])])
        assert got == want[i], msgs[i]
