"""The HIP engine's device flow loop (tgsim_flow_init / tgsim_gen_flow / tgsim_flow_report /
tgsim_flow_rows) against the same loop driven from the host over the CPU oracle
(workloads.flow_reference), bit for bit: the verdict bytes and drained records of every window, and
the flow rows, summary and FCT histogram at three points of each run (before the first ACK, mid-run
with ACKs waiting in the calendar, and at the end).  What the cases exercise is asserted on the model
alone in tests/test_flow_model.py."""
import errno

import numpy as np
import pytest

import flow_cases as fc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl
from testground_amd.engine import CABIEngine, Engine, EngineError

pytestmark = pytest.mark.gpu
MS = nw.Millisecond
GROUPS = 4


def mesh_groups():
    return (np.arange(fc.MESH["n"]) % GROUPS).astype(np.uint16)


@pytest.fixture(scope="module")
def mesh_ref(oracle_lib):
    """The lossy mesh's host model over the oracle, once for the tests that compare with it, folded
    into a GroupMatrix on the way."""
    gm = wl.GroupMatrix(mesh_groups(), GROUPS)
    eng = CABIEngine(oracle_lib, "tgo_", fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"])
    out = fc.run_mesh(fc.Folding(eng, gm), device=False)
    out["groups"] = gm.m
    return out


# -- 1, 3, 4, 5: the small cases ---------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [1, 3])
def test_rounds(make_oracle, rounds):
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    dev = fc.run_rounds(Engine(2, **kw), device=True, rounds=rounds)
    fc.assert_same_run(dev, fc.run_rounds(make_oracle(2, **kw), device=False, rounds=rounds))
    assert (dev["rows"]["state"] == abi.FLOW_DONE).all() and dev["summary"]["retransmits"] == 0


def test_ping_disarm_leaves_flows(make_oracle):
    """The flow driver holds the reply calendar: disarming ping (not its owner) while flows are
    armed, mid-run with ACKs in the calendar, frees nothing, and the run goes on as the reference does."""
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    eng = Engine(2, **kw)
    dev = fc.run_rounds(eng, device=True, rounds=3, before=lambda w: eng.ping_init(None) if w in (1, 4) else None)
    fc.assert_same_run(dev, fc.run_rounds(make_oracle(2, **kw), device=False, rounds=3))
    assert (dev["rows"]["state"] == abi.FLOW_DONE).all() and dev["probes"][2][1]["segs_acked"] > 0
    eng.ping_init(None)
    assert eng.flow_report()["done"] == 2  # still armed, still readable


def test_netem_limit(make_oracle):
    kw = dict(lookahead_ns=fc.LIMIT["lookahead_ns"])
    dev = fc.run_limit(Engine(fc.LIMIT["n"], **kw), device=True)
    fc.assert_same_run(dev, fc.run_limit(make_oracle(fc.LIMIT["n"], **kw), device=False))
    assert dev["summary"]["retransmits"] == 24 and dev["summary"]["done"] == 16


@pytest.mark.parametrize("window", [fc.CUT["window"], fc.CUT["window"] // 2])
def test_unreachable(make_oracle, window):
    kw = dict(lookahead_ns=fc.CUT["lookahead_ns"])
    dev = fc.run_cut(Engine(fc.CUT["n"], **kw), device=True, window=window)
    fc.assert_same_run(dev, fc.run_cut(make_oracle(fc.CUT["n"], **kw), device=False, window=window))
    assert dev["rows"]["state"].tolist() == [abi.FLOW_FAILED, abi.FLOW_DONE, abi.FLOW_DONE, abi.FLOW_DONE]


def test_partition_heals(make_oracle):
    kw = dict(lookahead_ns=fc.HEAL["lookahead_ns"])
    dev = fc.run_heal(Engine(fc.HEAL["n"], **kw), device=True)
    fc.assert_same_run(dev, fc.run_heal(make_oracle(fc.HEAL["n"], **kw), device=False))
    assert (dev["rows"]["state"] == abi.FLOW_DONE).all() and dev["rows"]["retransmits"][0] > 0


# -- 6. lossy mesh ---------------------------------------------------------------------------------------------
def test_mesh_parity(mesh_ref):
    dev = fc.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), device=True)
    fc.assert_same_run(dev, mesh_ref)
    m = mesh_ref["model"]
    assert m.max_row > 64 and m.max_ack_row > 64 and m.carried_max >= 2 and m.max_attempt >= 2 and m.ring_wraps > 0


@pytest.mark.parametrize("flags", [abi.OPT_DISCARD_DELIVERIES, abi.OPT_METRICS])
def test_mesh_reports_with_flags(mesh_ref, flags):
    """Nothing reaches the host / the metrics fold beside it: identical reports."""
    dev = fc.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"], flags=flags), device=True)
    fc.assert_same_run(dev, mesh_ref, windows=flags == abi.OPT_METRICS)
    if flags == abi.OPT_DISCARD_DELIVERIES:
        assert all(len(d) == 0 for _, d in dev["windows"])
        for (dv, _), (rv, _) in zip(dev["windows"], mesh_ref["windows"]):
            assert dv.tobytes() == rv.tobytes()


def test_mesh_window_length(make_oracle, mesh_ref):
    """The mesh at a second window length, against the model at that length: the rows and the histogram
    are identical.  They are NOT those of the first length, on either engine: a generation knows every
    record up to the lookahead beyond its window's start, so an ACK delivered just after its segment's
    timer ran out suppresses the retransmission when a window happens to start before that tick, and
    not otherwise (with rto_ticks below some round trips the mesh is full of such ACKs).  Only the
    failure rule is by tick alone (test_unreachable)."""
    kw = dict(lookahead_ns=fc.MESH["lookahead_ns"])
    dev = fc.run_mesh(Engine(fc.MESH["n"], **kw), device=True, window=2_000, probe_at=())
    ref = fc.run_mesh(make_oracle(fc.MESH["n"], **kw), device=False, window=2_000, probe_at=())
    assert dev["rows"].tobytes() == ref["rows"].tobytes()
    assert (dev["summary"]["hist"] == ref["summary"]["hist"]).all()
    fc.assert_same_run(dev, ref)
    assert dev["summary"]["pending_acks"] == 0 and dev["summary"]["done"] == len(dev["rows"])
    assert (ref["rows"]["acked"] == mesh_ref["rows"]["acked"]).all()  # every flow completes either way


def test_mesh_group_matrix(mesh_ref):
    eng = Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"])
    eng.groups_init(mesh_groups(), GROUPS)
    dev = fc.run_mesh(eng, device=True)
    fc.assert_same_run(dev, mesh_ref)  # the flow reports and every window are what they are unarmed
    got = eng.group_matrix()
    assert got.shape == mesh_ref["groups"].shape and (got == mesh_ref["groups"]).all()
    assert got[:, :, 12].sum() > 0 and got[:, :, 2 + abi.V_LOSS].sum() > 0


# -- parameter corners on 4 peers --------------------------------------------------------------------------------
@pytest.mark.parametrize("window,n_seg,max_attempts", [(1, 1, 2), (1, 65, 2), (64, 1, 2), (64, 65, 2), (64, 130, 16),
                                                       (7, 65, 16)])
def test_corners(make_oracle, window, n_seg, max_attempts):
    """window 1 and 64 (a shift of the whole bitmap), n_seg 1 and 65 (no multiple of the window, a ring
    that wraps), max_attempts 16 (attempt 15 is the last one a seq encodes) behind a Drop rule."""
    def run(eng, device):
        fc.plain(eng, 4, 5 * MS, Loss=20.0)
        eng.configure(3, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=5 * MS),
                                   Rules=[fc.rule(0, nw.FilterAction.Drop)]))
        now = eng.stats()["now_tick"]
        flows = fc.table([(0, 1, n_seg, now), (1, 2, n_seg, now + 3), (2, 3, n_seg, now), (3, 0, n_seg, now)])
        flow = dict(seg_len=300, ack_len=40, window=window, rto_ticks=11_000, max_attempts=max_attempts, bin_ns=MS, n_bins=8)
        n_windows = 40 if max_attempts == 16 else 12
        return fc.drive(eng, device, flow, flows, n_windows, 5_000, probe_at=(0, 3, n_windows - 2))

    kw = dict(lookahead_ns=5 * MS)
    dev, ref = run(Engine(4, **kw), True), run(make_oracle(4, **kw), False)
    fc.assert_same_run(dev, ref)
    assert ref["rows"]["acked"].sum() > 0
    if max_attempts == 16:
        assert ref["rows"]["state"][3] == abi.FLOW_FAILED and ref["model"].max_attempt == 15
        assert ref["rows"]["offered"][3] == 16 * min(window, n_seg)


# -- late receipt ------------------------------------------------------------------------------------------------
def test_late_receipt():
    n, win = fc.LATE["n"], fc.LATE["window"]
    eng = Engine(n, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=50.0)
    eng.flow_init(fc.late_flows(0), **fc.LATE_FLOW)
    eng.gen_flow(win)
    eng.step(win)
    rows = eng.flow_rows()
    for _ in range(2):  # sticky
        with pytest.raises(EngineError, match="flow: a receipt due at tick") as ei:
            eng.gen_flow(win)
        assert ei.value.code == -errno.EINVAL
    rep = eng.flow_report()  # still readable
    assert rep["flows"] == n and rep["data_offered"] == 8 * n and rep["pending_acks"] > 0
    assert eng.flow_rows().tobytes() == rows.tobytes()  # unchanged by the failed generation
    for _ in range(4):  # empty windows: what is in flight drains
        eng.step(win)
    fc.configure_late(eng, reorder=0.0)
    eng.flow_init(fc.late_flows(eng.stats()["now_tick"], n_seg=20), **fc.LATE_FLOW)
    wl.flow_run(eng, 8, win)
    rep = eng.flow_report()
    assert rep["done"] == n and rep["segs_acked"] == 20 * n and rep["retransmits"] == 0 and rep["pending_acks"] == 0


# -- arming rules --------------------------------------------------------------------------------------------------
def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


def test_arming_rules(make_oracle):
    import torch

    n = 8
    ok = dict(seg_len=500, ack_len=64, window=4, rto_ticks=20_000, max_attempts=4)
    t = wl.flow_table_mesh(n, 2, 6, seed=1)
    _raises(errno.EINVAL, "one engine for every peer", Engine(n, shard=(0, 4)).flow_init, t, **ok)
    _raises(errno.ENOSYS, "tgo_flow_init is not exported", make_oracle(n).flow_init, t, **ok)
    eng = Engine(n, lookahead_ns=5 * MS)
    fc.plain(eng, n, 5 * MS)
    _raises(errno.EINVAL, "not armed", eng.flow_report)
    _raises(errno.EINVAL, "not armed", eng.flow_rows)
    _raises(errno.EINVAL, "not armed", eng.gen_flow, 100)
    for bad, match in ((dict(seg_len=0), "seg_len 0"), (dict(seg_len=65536), "seg_len 65536"), (dict(ack_len=0), "ack_len 0"),
                       (dict(ack_len=65536), "ack_len 65536"), (dict(window=0), "window 0"), (dict(window=65), "window 65"),
                       (dict(rto_ticks=0), "rto_ticks 0"), (dict(max_attempts=0), "max_attempts 0"),
                       (dict(max_attempts=17), "max_attempts 17"), (dict(n_bins=257, bin_ns=1), "n_bins 257"),
                       (dict(n_bins=4, bin_ns=0), "bin_ns 0")):
        _raises(errno.EINVAL, match, eng.flow_init, t, **dict(ok, **bad))

    def entry(i, **kw):
        bad = t.copy()
        for k, v in kw.items():
            bad[k][i] = v
        return bad

    _raises(errno.EINVAL, r"flows\[5\]\.src = 1 after src 2", eng.flow_init, entry(5, src=1), **ok)
    _raises(errno.EINVAL, r"flows\[3\]\.dst = 1 is the source itself", eng.flow_init, entry(3, dst=1), **ok)
    _raises(errno.EINVAL, r"flows\[3\]\.dst = 8 is out of range", eng.flow_init, entry(3, dst=n), **ok)
    _raises(errno.EINVAL, r"flows\[3\]\.dst = 4294967295 is out of range", eng.flow_init, entry(3, dst=abi.EXTERNAL), **ok)
    _raises(errno.EINVAL, r"flows\[15\]\.src = 8 is out of range", eng.flow_init, entry(15, src=n), **ok)
    _raises(errno.EINVAL, r"flows\[2\]\.n_seg = 0", eng.flow_init, entry(2, n_seg=0), **ok)
    _raises(errno.EINVAL, r"flows\[2\]\.n_seg = 8388609", eng.flow_init, entry(2, n_seg=(1 << 23) + 1), **ok)
    many = fc.table([(2, (3 + k) % n if (3 + k) % n != 2 else 0, 4, 0) for k in range(17)])
    _raises(errno.EINVAL, r"flows\[16\] is flow 17 of source 2", eng.flow_init, many, **ok)
    pkt = np.array([(0, 1, 0, 64, 0)], dtype=abi.PKT_DTYPE)
    eng.submit(pkt)
    _raises(errno.EBUSY, "host packets", eng.flow_init, t, **ok)
    eng.step(10)
    eng.gen_storm(0.01, 10)
    _raises(errno.EBUSY, "generated windows", eng.flow_init, t, **ok)
    eng.step(10)
    buf = torch.empty(max(1, eng.sim_capacity(), 64) * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    eng.step_sim_launch(10, [0, n], buf.data_ptr(), buf.numel() // 24)
    _raises(errno.EBUSY, "launched steps", eng.flow_init, t, **ok)
    eng.step_sim_finish()
    _raises(errno.EINVAL, r"flows\[0\]\.start_tick 0 in the past", eng.flow_init, t, **ok)
    eng.step(10_000)  # (nothing of the earlier traffic is left in flight)
    eng.drain()
    # armed: the other sources of traffic and the sharded steps refuse; step_n runs window by window
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, **ok)
    _raises(errno.EBUSY, "flow driver is armed", eng.submit, pkt)
    _raises(errno.EBUSY, "flow driver is armed", eng.gen_storm, 0.01, 10)
    _raises(errno.EBUSY, "flow driver is armed", eng.gossip_init, n_floods=1, degree=2)
    _raises(errno.EBUSY, "flow driver is armed", eng.ping_init, wl.ping_targets_mesh(n, 2, seed=1), count=1)
    _raises(errno.EBUSY, "flow driver is armed", eng.step_sim, 10, [0, n], 0, 0)
    _raises(errno.EBUSY, "step_sim_launch: the flow driver is armed", eng.step_sim_launch, 10, [0, n], 0, 0)
    _raises(errno.EBUSY, "step_sim_launch_slotted: the flow driver is armed", eng.step_sim_launch_slotted, 10, [0, n],
            buf.data_ptr(), 16)
    _raises(errno.EBUSY, "step_sim_launch_slotted_n: the flow driver is armed", eng.step_sim_launch_slotted_n, 10, 2,
            [0, n], buf.data_ptr(), 16)
    eng.ping_init(None)  # disarming the ping driver leaves the armed flow driver (and the calendar they share) alone
    _raises(errno.EINVAL, "longer than rto_ticks", eng.gen_flow, ok["rto_ticks"] + 1)
    eng.gen_flow(5_000)
    _raises(errno.EBUSY, "one window at a time", eng.gen_flow, 5_000)
    eng.step_n(5_000, 1)
    wl.flow_run(eng, 5, 5_000)
    rep = eng.flow_report()
    assert rep["done"] == rep["flows"] == 2 * n and rep["segs_acked"] == 12 * n and rep["pending_acks"] == 0
    assert rep["bytes_acked"] == 12 * n * ok["seg_len"]
    assert len(eng.flow_rows(3, 5)) == 5 and (eng.flow_rows(3, 5)["acked"] == 6).all()
    _raises(errno.EINVAL, "outside", eng.flow_rows, 10, 7)
    # disarm: the host's traffic is back, the reports are gone; re-arm
    eng.flow_init(None)
    _raises(errno.EINVAL, "not armed", eng.flow_rows)
    eng.submit(pkt)
    eng.step(10)
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, **ok)
    assert eng.flow_report()["segs_acked"] == 0
    # ping or gossip armed: no flows
    p = Engine(n, lookahead_ns=5 * MS)
    p.ping_init(wl.ping_targets_mesh(n, 2, seed=1), count=1)
    _raises(errno.EBUSY, "ping driver is armed", p.flow_init, t, **ok)
    p.flow_init(None)  # (disarming the flow driver leaves the ping driver alone)
    assert p.ping_report()["pairs"] == 2 * n
    g = Engine(n, lookahead_ns=5 * MS)
    g.gossip_init(n_floods=1, degree=2)
    _raises(errno.EBUSY, "gossip driver is armed", g.flow_init, t, **ok)


def test_exchange_refuses_while_armed():
    """tgsim_comm_launch and tgsim_comm_run (and tgsim_comm_step, which is their sum) on an engine joined
    to a one-rank exchange: -EBUSY while flows are armed, back to work once disarmed."""
    from testground_amd.engine import comm_id

    n = 8
    eng = Engine(n, lookahead_ns=5 * MS)
    fc.plain(eng, n, 5 * MS)
    eng.comm_init(comm_id(), 0, 1)
    eng.flow_init(wl.flow_table_mesh(n, 2, 6, seed=1), seg_len=500, ack_len=64, window=4, rto_ticks=20_000)
    _raises(errno.EBUSY, "comm_launch: the flow driver is armed", eng.comm_launch, 100)
    _raises(errno.EBUSY, "comm_launch: the flow driver is armed", eng.comm_step, 100)
    _raises(errno.EBUSY, "comm_run: the flow driver is armed", eng.comm_run, 100, 2)
    wl.flow_run(eng, 6, 5_000)  # the single-engine steps run the transfer
    assert eng.flow_report()["done"] == 2 * n
    eng.flow_init(None)
    eng.comm_step(100)
