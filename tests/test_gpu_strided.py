"""The loops no other GPU test takes a second trip through: the tile-strided and row-strided
loops of the select, route, deliver, inbox, window and ack stages and the carry of their one-block
scans.  Tuning key "max_blocks" caps the grid, so that one block takes several tiles or groups of
rows (1: every one of them; 2: 4 + 3 of 7 tiles; 3: 3 + 2 + 2); "scan_chunk" shortens the carry
step of the scans (1 and 3: 7 and 3 steps over 7 tiles).  The barriers between two trips of a
block and the carry are what these shapes exercise; at the default settings both need inputs of
millions of deliveries.

Every comparison is exact: against the sequential restatements (tests/*_ref.py) and byte for byte
against the stage's host evaluator, through the helpers of the stage's own GPU test module, with
their sentinel checks behind every output."""

import functools
import os
import subprocess

import numpy as np
import pytest

from tests import ack_cases as AC
from tests import ack_ref as AR
from tests import deliver_cases as DC
from tests import inbox_cases as IC
from tests import inbox_ref as IR
from tests import route_cases as RC
from tests import select_cases as SC
from tests import window_cases as WC
from tests import window_ref as WR
from tests import test_gpu_ack as TA
from tests import test_gpu_deliver as TD
from tests import test_gpu_inbox as TI
from tests import test_gpu_route as TR
from tests import test_gpu_select as TS
from tests import test_gpu_window as TW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CAPS, CHUNKS = (1, 2, 3), (1, 3, None)  # None: the default
SETTINGS = [(cap, chunk) for cap in CAPS for chunk in CHUNKS]
THIN = [(1, 1), (2, 3), (3, None)]  # for the one case that is not small: the deliver fuzz batch


def setting_id(s):
    return "blocks_%s-chunk_%s" % tuple("default" if x is None else x for x in s)


def tune(h, setting):
    cap, chunk = setting
    if cap is not None:
        h.set_tuning("max_blocks", cap)
    if chunk is not None:
        h.set_tuning("scan_chunk", chunk)
    return h


class Stages:
    """The stage modules, and one handle per stage (and path) for one setting."""

    def __init__(self, setting):
        from emqx_amd import ack, deliver, inbox, route, select, window
        self.setting = setting
        self.A, self.D, self.I, self.M, self.S, self.W = ack, deliver, inbox, route, select, window
        self.ack = tune(ack.Ack(0), setting)
        self.windows = {path: tune(window.Window(0), setting) for path in (0, 1)}
        self.inboxes = {path: tune(inbox.Inbox(0), setting) for path in TI.PATHS}
        for path in (0, 1):
            self.windows[path].set_tuning("path", path)
            self.inboxes[path].set_tuning("path", path)

    def subopts(self):
        return tune(self.D.SubOpts(0), self.setting)


@pytest.fixture(scope="module")
def gpu():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True, capture_output=True)
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)


@pytest.fixture(scope="module", params=SETTINGS, ids=setting_id)
def stages(gpu, request):
    return Stages(request.param)


# the cases are built, and their restatements computed, once for all settings
@functools.lru_cache(maxsize=None)
def ack_run_case(w):
    return AC.strided_run(w)


@functools.lru_cache(maxsize=None)
def ack_record_case(refs):
    return AC.strided_record(refs)


@functools.lru_cache(maxsize=None)
def window_cases():
    return (WC.strided(),) + WC.strided_chained()


@functools.lru_cache(maxsize=None)
def inbox_case(name):
    if name == "fuzz_wide":
        return IC.fuzz_wide()
    return IC.shape(7 * IC.T + 5, name)


# ---- ack ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rematch", [0, 1], ids=["carry_slot", "rematch"])
@pytest.mark.parametrize("w", [16, 64])
def test_ack_run(stages, w, rematch):
    """7 T + 5 acks over 121 sessions (ack_cases.strided_run): every device form with update_table,
    then with buffers larger than what is written."""
    A, h, case = stages.A, stages.ack, ack_run_case(w)
    h.set_tuning("rematch", rematch)
    ref = TA.all_forms(A, h, case, update_table=True)
    for run in (TA.run_sync, TA.run_async):
        got, slots, table = run(A, h, case, cap_in=case.total + 3 * AC.T + 5, cap_boxes=case.m + 77, update_table=True,
                                count_on_device=True)
        AC.check_run(ref, got, slots, table)


@pytest.mark.parametrize("refs", [False, True], ids=["refs_null", "refs"])
def test_ack_record(stages, refs):
    """7 T + 5 positions over 107 inboxes (ack_cases.strided_record)."""
    case = ack_record_case(refs)
    assert case.reference()["summary"][0] == AR.F_BAD_SUB | AR.F_ROW_FULL
    TA.rec_all_forms(stages.A, stages.ack, case)


# ---- window ------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", [0, 1], ids=["tile_scan", "wave_per_inbox"])
def test_window(stages, path):
    """7 T + 5 deliveries over 997 inboxes (window_cases.strided): every device form, then two such
    batches chained through the table on one stream."""
    W, h = stages.W, stages.windows[path]
    case, a, b = window_cases()
    TW.all_forms(W, h, case)
    TW.chain_two_batches(W, h, a, b)


# ---- inbox -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fuzz_wide", "one_sub", "distinct_desc"])
def test_inbox(stages, name):
    """Both paths.  fuzz_wide: 8 T + 37 deliveries, three passes; one_sub: 7 T + 5 deliveries that
    must keep their order across the tiles one block takes; distinct_desc: 7 T + 5 inboxes, so the
    head scan carries and the longest pass strides."""
    TI.all_forms(stages.I, stages.inboxes, inbox_case(name))


# ---- deliver -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["mixed", "all", "none"])
def test_deliver_40_tiles(stages, mode):
    """The 10 000-delivery message between empty ones: 40 tiles, annotate-only and compacting."""
    case = DC.shape("10002", mode)
    TD.all_forms(stages.D, case.load(stages.subopts()), case)


@pytest.mark.parametrize("setting", THIN, ids=setting_id)
def test_deliver_fuzz(gpu, setting):
    """About 150 K deliveries, 574 tiles: 574, 192 and 1 carry steps of the scan."""
    from emqx_amd import deliver as D
    case = DC.fuzz()
    TD.all_forms(D, case.load(tune(D.SubOpts(0), setting)), case)


# ---- route and select: the scans' carry --------------------------------------------------------

@pytest.mark.parametrize("max_blocks", [None, 2], ids=["default_grid", "2_blocks"])
@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("path, stored_mask", TR.VARIANTS)
@pytest.mark.parametrize("name", ["total_2049_n_7", "total_6149_n_7", "one_message", "fuzz_1"])
def test_route_scan_carry(gpu, name, path, stored_mask, chunk, max_blocks):
    """The cases of 2, 3 and 4 tiles: 64 node rows a tile make the histogram scan carry hundreds of
    times at these chunks."""
    from emqx_amd import route as M
    case = RC.BY_NAME[name]
    t = tune(TR.table_of(M, case, path, max_blocks, stored_mask), (None, chunk))
    ref = t.route_host(case.offsets, case.filters)
    RC.check(case, ref)
    need = ref.summary["forwards"]
    for got in (t.route_packed(case.offsets, case.filters), TR.run_sync(M, t, case, need), TR.run_async(M, t, case, need + 3)):
        RC.check(case, got)
        assert TR.same_bytes(got, ref)
    t.close()


@pytest.mark.parametrize("max_blocks", [None, 2], ids=["default_grid", "2_blocks"])
@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("match_all, masked", [(True, True), (False, False)])
def test_select_scan_carry(gpu, match_all, masked, chunk, max_blocks):
    """10 002 entries, 40 tiles."""
    from emqx_amd import select as S
    case = SC.shape("e10002", match_all, masked)
    TS.all_forms(S, case.load(tune(S.OwnerTable(0), (max_blocks, chunk))), case)


# ---- the chain ---------------------------------------------------------------------------------

def test_chain_window_record_group_ack_window_on_one_stream(gpu):
    """tests/test_gpu_ack.py's chain at 3 T + 1 deliveries (T: the window stage's tile) over 40
    sessions, every handle at max_blocks 1 and scan_chunk 1: emqx_window_run_batch_device_async ->
    emqx_ack_record_batch_device_async -> emqx_inbox_group_batch_device_async over 3 T + 1 raw acks
    -> emqx_ack_run_batch_device_async with update_table -> emqx_window_run_batch_device_async of a
    second batch.  One stream, no host read in between; each step against the restatements."""
    import torch
    from emqx_amd import ack as A
    from emqx_amd import inbox as I
    from emqx_amd import window as W
    dev, dev_raw = TA.dev, TA.dev_raw
    T = W.TILE
    total, n_sessions, sub_limit, w = 3 * T + 1, 40, 48, 16
    rng = np.random.default_rng(77)
    subs = np.arange(3, 3 + n_sessions)
    cuts = np.sort(rng.choice(np.arange(1, total), size=n_sessions - 1, replace=False))
    off = np.concatenate([[0], cuts, [total]])
    opts = [rng.choice([0, 1, 1, 2, 5, 6], size=total).astype(np.uint8) for _ in range(2)]
    table = W.pack_sessions(sub_limit, inflight_max=rng.choice([4, 8, 12], sub_limit), mq_max=rng.choice([5, 1000], sub_limit),
                            next_pkt_id=rng.integers(1, 65536, sub_limit))
    rows = A.empty_slots(sub_limit, w)
    refs = (np.arange(total, dtype=np.uint32) * 2654435761 + 5).astype(np.uint32)
    recs = [{f: int(table[f][i]) for f in WR.FIELDS} for i in range(sub_limit)]
    # the restatement of batch 1 first: the raw acks name the ids it sends
    x1 = WR.run(subs, off, opts[0], recs, update_table=True)
    sent = [(int(subs[k]), x1["pkt_ids"][d]) for k in range(n_sessions) for d in range(int(off[k]), int(off[k + 1]))
            if x1["verdicts"][d] == W.W_SEND]
    assert len(sent) > 200
    n_raw = total
    pick = rng.integers(0, len(sent), size=n_raw)
    raw_subs = np.array([sent[i][0] for i in pick], dtype=np.uint32)
    raw_ids = np.array([sent[i][1] for i in pick], dtype=np.uint32)
    stray = rng.random(n_raw) < 0.2
    raw_subs[stray] = rng.integers(0, sub_limit, size=int(stray.sum()))  # other sessions, among them ones without a row entry
    raw_acks = A.pack_acks(rng.choice([AR.PUBACK, AR.PUBREC, AR.PUBCOMP], size=n_raw, p=[0.5, 0.3, 0.2]), raw_ids)
    raw_off = np.arange(n_raw + 1)  # one "message" each

    z = lambda k, dt: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    d_table, d_rows = dev_raw(table), dev_raw(rows)
    d_subs, d_off, d_refs = dev(subs, np.uint32), dev(off, np.uint64), dev(refs, np.uint32)
    d_opts = [dev(o, np.uint8) for o in opts]
    ver = [z(total, torch.uint8) for _ in range(2)]
    ids = [z(total, torch.int16) for _ in range(2)]
    wrec = [z(4 * n_sessions, torch.int64) for _ in range(2)]
    wcnt = [z(4 * n_sessions, torch.int32) for _ in range(2)]
    wsum = [z(8, torch.int64) for _ in range(2)]
    unrec, rsum = z(n_sessions, torch.int32), z(8, torch.int64)
    d_raw_subs, d_raw_acks, d_raw_off = dev(raw_subs, np.uint32), dev(raw_acks, np.uint32), dev(raw_off, np.uint64)
    box_msgs, box_acks = z(n_raw, torch.int32), z(n_raw, torch.int32)
    ack_subs, ack_off, isum = z(sub_limit, torch.int32), z(sub_limit + 1, torch.int64), z(8, torch.int64)
    aver, arefs, acnt, asum = z(n_raw, torch.uint8), z(n_raw, torch.int32), z(4 * sub_limit, torch.int32), z(8, torch.int64)
    setting = (1, 1)
    win, ack, box = tune(W.Window(0), setting), tune(A.Ack(0), setting), tune(I.Inbox(0), setting)
    win.reserve(total, n_sessions)
    ack.reserve(max(total, n_raw), sub_limit, w)
    box.reserve(n_raw, sub_limit)
    wargs = [W.Window.batch(d_subs.data_ptr(), d_off.data_ptr(), d_opts[i].data_ptr(), n_sessions, total, n_sessions,
                            d_table.data_ptr(), sub_limit, ver[i].data_ptr(), ids[i].data_ptr(), wrec[i].data_ptr(),
                            wcnt[i].data_ptr(), update_table=True) for i in range(2)]
    r1 = A.Ack.record_args(d_subs.data_ptr(), d_off.data_ptr(), d_opts[0].data_ptr(), n_sessions, total, n_sessions,
                           ver[0].data_ptr(), ids[0].data_ptr(), d_rows.data_ptr(), w, sub_limit, unrec.data_ptr(),
                           d_refs=d_refs.data_ptr())
    g1 = I.Inbox.batch(d_raw_off.data_ptr(), d_raw_subs.data_ptr(), d_raw_acks.data_ptr(), n_raw, n_raw, sub_limit,
                       box_msgs.data_ptr(), box_acks.data_ptr(), ack_subs.data_ptr(), ack_off.data_ptr(), sub_limit)
    a1 = A.Ack.run_args(ack_subs.data_ptr(), ack_off.data_ptr(), box_acks.data_ptr(), 0, n_raw, sub_limit, d_table.data_ptr(),
                        sub_limit, d_rows.data_ptr(), w, aver.data_ptr(), arefs.data_ptr(), acnt.data_ptr(), update_table=True,
                        d_n_boxes=isum.data_ptr() + 16)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        win.run_device_async(wargs[0], wsum[0].data_ptr(), stream=stream.cuda_stream)
        ack.record_device_async(r1, rsum.data_ptr(), stream=stream.cuda_stream)
        box.group_device_async(g1, isum.data_ptr(), stream=stream.cuda_stream)
        ack.run_device_async(a1, asum.data_ptr(), stream=stream.cuda_stream)
        win.run_device_async(wargs[1], wsum[1].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()

    u = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    # batch 1 of the window
    assert u(ver[0], np.uint8).tolist() == x1["verdicts"] and u(ids[0], np.uint16).tolist() == x1["pkt_ids"]
    assert u(wsum[0], np.uint64).tolist() == x1["summary"] and u(wcnt[0], np.uint32).reshape(-1, 4).tolist() == x1["counts"]
    assert min(x1["summary"][3:6]) > 0, "sends, QoS 0 sends and queued all occur"
    # record
    ref_rows = AC.rows_of(rows)
    xr = AR.record(subs, off, opts[0], x1["verdicts"], x1["pkt_ids"], refs, ref_rows)
    assert u(rsum, np.uint64).tolist() == xr["summary"] and u(unrec, np.uint32).tolist() == xr["unrecorded"]
    assert xr["summary"][4] == len(sent), "every send found a slot"
    # the grouping of the raw acks
    xg = IR.group(raw_off, raw_subs, raw_acks, sub_limit)
    m = xg["summary"][2]
    assert u(isum, np.uint64).tolist() == xg["summary"] and m > n_sessions
    assert u(ack_subs, np.uint32)[:m].tolist() == xg["inbox_subs"] and u(ack_off, np.uint64)[:m + 1].tolist() == xg["inbox_offsets"]
    assert u(box_acks, np.uint32).tolist() == xg["filters"] and u(box_msgs, np.uint32).tolist() == xg["msgs"]
    # the acks
    xa = AR.run(xg["inbox_subs"], xg["inbox_offsets"], xg["filters"], recs, ref_rows, update_table=True)
    assert u(aver, np.uint8).tolist() == xa["verdicts"] and u(arefs, np.uint32).tolist() == xa["refs"]
    assert u(acnt, np.uint32)[:4 * m].reshape(-1, 4).tolist() == xa["counts"] and u(asum, np.uint64).tolist() == xa["summary"]
    assert xa["summary"][3] > 100 and xa["summary"][4] > 50, "acks were answered OK and slots released"
    got_rows = np.frombuffer(d_rows.cpu().numpy().tobytes(), dtype=A.SLOT).reshape(sub_limit, w)
    assert AC.rows_of(got_rows) == ref_rows
    # batch 2 of the window: the windows the acks reopened
    x2 = WR.run(subs, off, opts[1], recs, update_table=True)
    assert u(ver[1], np.uint8).tolist() == x2["verdicts"] and u(ids[1], np.uint16).tolist() == x2["pkt_ids"]
    assert u(wsum[1], np.uint64).tolist() == x2["summary"] and x2["summary"][3] > 50
    got_table = np.frombuffer(d_table.cpu().numpy().tobytes(), dtype=W.SESSION)
    assert [{f: int(got_table[f][i]) for f in WR.FIELDS} for i in range(sub_limit)] == recs
