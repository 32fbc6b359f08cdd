"""The device flow loop armed with congestion control (tgsim_flow_init_cc / tgsim_flow_cc_rows /
tgsim_flow_cc_report) against the host model over the CPU oracle (workloads.FlowCCModel), bit for bit:
the verdict bytes and drained records of every window, and the flow rows, cc rows, both summaries and
the FCT histogram at three probes and at the end.  The closed forms, and what the parity inputs
exercise, are asserted on the model alone in tests/test_flow_cc_model.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import flow_cases as fc
import flow_cc_cases as cc
from testground_amd import abi
from testground_amd import workloads as wl
from testground_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
MS = fc.MS


# -- 1, 2. slow start and congestion avoidance ---------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(cc.RAMPS)))
def test_ramp(make_oracle, case):
    ccp, n_seg, rounds = cc.RAMPS[case]
    kw = dict(lookahead_ns=cc.RAMP["lookahead_ns"])
    dev = cc.run_ramp(Engine(2, **kw), True, ccp, n_seg, rounds)
    cc.assert_same_run(dev, cc.run_ramp(make_oracle(2, **kw), False, ccp, n_seg, rounds))
    rtt, fct = 2 * cc.RAMP["latency_ns"], int(fc.fct(dev)[0])
    assert dev["rows"]["state"][0] == abi.FLOW_DONE and rounds * rtt <= fct <= rounds * (rtt + cc.RAMP_SLACK_NS)
    assert dev["summary"]["retransmits"] == 0 and dev["cc_summary"]["loss_events"] == 0
    if ccp is cc.SLOW_START:
        assert dev["cc_rows"]["cwnd"][0] == min(1 + n_seg, cc.RAMP_FLOW["window"])
    elif n_seg == 22:
        assert dev["cc_rows"]["cwnd"][0] == 8


# -- 3. degenerate equivalence: the cc kernels give the answers of the kernels without ------------------------------
@pytest.mark.parametrize("rounds,dupthresh", [(1, 0), (3, 3)])
def test_degenerate_rounds(make_oracle, rounds, dupthresh):
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    ccp = cc.degenerate(fc.ROUNDS_FLOW["window"], dupthresh)
    dev = cc.run_rounds(Engine(2, **kw), True, rounds, ccp)
    cc.same_plain_run(dev, fc.run_rounds(Engine(2, **kw), device=True, rounds=rounds))
    cc.assert_same_run(dev, cc.run_rounds(make_oracle(2, **kw), False, rounds, ccp))


def test_degenerate_bandwidth(make_oracle):
    kw = dict(lookahead_ns=fc.BW["lookahead_ns"])
    ccp = cc.degenerate(fc.BW_FLOW["window"], 63)
    dev = cc.run_bandwidth(Engine(2, **kw), True, ccp)
    cc.same_plain_run(dev, fc.run_bandwidth(Engine(2, **kw), device=True))
    cc.assert_same_run(dev, cc.run_bandwidth(make_oracle(2, **kw), False, ccp))


# -- 4. unreachable -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [fc.CUT["window"], fc.CUT["window"] // 2])
def test_unreachable(make_oracle, window):
    kw = dict(lookahead_ns=fc.CUT["lookahead_ns"])
    dev = cc.run_cut(Engine(fc.CUT["n"], **kw), True, window=window)
    cc.assert_same_run(dev, cc.run_cut(make_oracle(fc.CUT["n"], **kw), False, window=window))
    p, c, crow = fc.CUT_FLOW, cc.CUT_CC, dev["cc_rows"][0]
    assert dev["rows"]["state"].tolist() == [abi.FLOW_FAILED, abi.FLOW_DONE, abi.FLOW_DONE, abi.FLOW_DONE]
    assert dev["rows"]["done_ns"][0] == (int(dev["flows"]["start_tick"][0]) + p["max_attempts"] * p["rto_ticks"]) * fc.TICK
    assert dev["rows"]["offered"][0] == c["init_cwnd"] * p["max_attempts"]
    assert crow["timeouts"] == c["init_cwnd"] * (p["max_attempts"] - 1) and crow["loss_events"] == 1
    assert crow["cwnd"] == 1 and crow["ssthresh"] == max(c["init_cwnd"] // 2, 2)


# -- 5. cc == NULL through tgsim_flow_init_cc ------------------------------------------------------------------------
class NullCC:
    """An Engine whose flow_init arms through tgsim_flow_init_cc with cc == NULL."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def flow_init(self, flows, seg_len, ack_len, window, rto_ticks, max_attempts, bin_ns=0, n_bins=0):
        e = self._inner
        t = np.ascontiguousarray(flows, dtype=abi.FLOW_SPEC_DTYPE)
        p = abi.Flow(seg_len, ack_len, window, rto_ticks, max_attempts, n_bins, bin_ns)
        e._check(e._fn("flow_init_cc")(e._h, C.byref(p), None, t.ctypes.data, len(t)), "flow_init_cc")
        e._n_flows = len(t)


def test_null_cc_is_flow_init():
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    eng = Engine(2, **kw)
    got = fc.run_rounds(NullCC(eng), device=True, rounds=3)
    fc.assert_same_run(got, fc.run_rounds(Engine(2, **kw), device=True, rounds=3))
    assert got["rows"].tobytes() != b"" and (got["rows"]["state"] == abi.FLOW_DONE).all()
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_rows)
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_report)


# -- 6. netem limit ---------------------------------------------------------------------------------------------------
def test_netem_limit(make_oracle):
    kw = dict(lookahead_ns=fc.LIMIT["lookahead_ns"])
    dev = cc.run_limit(Engine(fc.LIMIT["n"], **kw), True)
    cc.assert_same_run(dev, cc.run_limit(make_oracle(fc.LIMIT["n"], **kw), False))
    assert dev["summary"]["done"] == 16 and dev["cc_summary"]["loss_events"] > 0


# -- 7. lossy mesh ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_ref(oracle_lib):
    from testground_amd.engine import CABIEngine

    return cc.run_mesh(CABIEngine(oracle_lib, "tgo_", fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), False)


def test_mesh_parity(mesh_ref):
    dev = cc.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), True)
    cc.assert_same_run(dev, mesh_ref)
    assert fc.mesh_tie_sources_have_jitter(mesh_ref["model"])
    assert dev["cc_summary"]["fast_retransmits"] > 0 and dev["cc_summary"]["timeouts"] > 0


def test_mesh_discard_deliveries(mesh_ref):
    dev = cc.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"], flags=abi.OPT_DISCARD_DELIVERIES), True)
    cc.assert_same_run(dev, mesh_ref, windows=False)
    assert all(len(d) == 0 for _, d in dev["windows"])
    for (dv, _), (rv, _) in zip(dev["windows"], mesh_ref["windows"]):
        assert dv.tobytes() == rv.tobytes()


def test_mesh_window_length(make_oracle):
    """At a second window length, against the model at that length (the counters depend on the step
    length, test_gpu_flow.test_mesh_window_length says why)."""
    kw = dict(lookahead_ns=fc.MESH["lookahead_ns"])
    dev = cc.run_mesh(Engine(fc.MESH["n"], **kw), True, window=2_000, probe_at=())
    ref = cc.run_mesh(make_oracle(fc.MESH["n"], **kw), False, window=2_000, probe_at=())
    cc.assert_same_run(dev, ref)
    assert dev["cc_rows"].tobytes() == ref["cc_rows"].tobytes() and dev["summary"]["done"] == len(dev["rows"])


# -- 8. corners -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,init_cwnd,dupthresh,n_seg", cc.CORNERS)
def test_corners(make_oracle, window, init_cwnd, dupthresh, n_seg):
    kw = dict(lookahead_ns=5 * MS)
    dev = cc.run_corner(Engine(4, **kw), True, window, init_cwnd, dupthresh, n_seg)
    ref = cc.run_corner(make_oracle(4, **kw), False, window, init_cwnd, dupthresh, n_seg)
    cc.assert_same_run(dev, ref)
    assert ref["rows"]["acked"].sum() > 0 and ref["rows"]["state"][3] == abi.FLOW_FAILED  # (behind the Drop rule)
    assert ref["model"].max_attempt == 15 and ref["rows"]["offered"][3] == 16 * min(init_cwnd, n_seg)


# -- 9. arming and validation ---------------------------------------------------------------------------------------
def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


def test_arming_and_validation():
    n = 8
    ok = dict(seg_len=500, ack_len=64, window=4, rto_ticks=20_000, max_attempts=4)
    good = dict(init_cwnd=2, init_ssthresh=0, dupthresh=3)
    t = wl.flow_table_mesh(n, 2, 6, seed=1)
    eng = Engine(n, lookahead_ns=5 * MS)
    fc.plain(eng, n, 5 * MS)
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_rows)
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_report)
    for bad, match in ((dict(init_cwnd=0), "init_cwnd 0"), (dict(init_cwnd=5), "init_cwnd 5"),
                       (dict(init_ssthresh=1), "init_ssthresh 1"), (dict(init_ssthresh=5), "init_ssthresh 5"),
                       (dict(dupthresh=64), "dupthresh 64")):
        _raises(errno.EINVAL, match, eng.flow_init, t, cc=dict(good, **bad), **ok)
    _raises(errno.EINVAL, "window 65", eng.flow_init, t, cc=good, **dict(ok, window=65))  # tgsim_flow_init's own rules
    _raises(errno.EINVAL, "one engine for every peer", Engine(n, shard=(0, 4)).flow_init, t, cc=good, **ok)
    pkt = np.array([(0, 1, 0, 64, 0)], dtype=abi.PKT_DTYPE)
    eng.submit(pkt)
    _raises(errno.EBUSY, "host packets", eng.flow_init, t, cc=good, **ok)
    eng.step(10_000)
    eng.drain()
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, cc=good, **ok)
    _raises(errno.EBUSY, "flow driver is armed", eng.submit, pkt)
    rows = eng.flow_cc_rows()
    assert (rows["cwnd"] == 2).all() and (rows["ssthresh"] == 4).all() and (rows["next"] == 2).all()
    assert eng.flow_cc_report() == dict(loss_events=0, fast_retransmits=0, timeouts=0, active=2 * n, cwnd_sum=4 * n,
                                        cwnd_min=2, cwnd_max=2)
    wl.flow_run(eng, 8, 5_000)
    rep, crep = eng.flow_report(), eng.flow_cc_report()
    assert rep["done"] == rep["flows"] == 2 * n and rep["segs_acked"] == 12 * n and crep["active"] == 0
    assert len(eng.flow_cc_rows(3, 5)) == 5 and (eng.flow_cc_rows(3, 5)["next"] == 6).all()
    _raises(errno.EINVAL, "outside", eng.flow_cc_rows, 10, 7)
    # armed without cc: the flow reports answer, the cc readers do not; disarmed: none does
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, **ok)
    assert eng.flow_report()["segs_acked"] == 0
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_rows)
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_report)
    wl.flow_run(eng, 6, 5_000)
    assert eng.flow_report()["done"] == 2 * n
    eng.flow_init(None)
    _raises(errno.EINVAL, "not armed", eng.flow_rows)
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_report)
    eng.submit(pkt)
    eng.step(10)


def test_late_receipt_keeps_cc_rows():
    n, win = fc.LATE["n"], fc.LATE["window"]
    eng = Engine(n, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=50.0)
    eng.flow_init(fc.late_flows(0), cc=dict(init_cwnd=4, init_ssthresh=0, dupthresh=3), **fc.LATE_FLOW)
    eng.gen_flow(win)
    eng.step(win)
    rows, crows = eng.flow_rows(), eng.flow_cc_rows()
    for _ in range(2):  # sticky
        _raises(errno.EINVAL, "flow: a receipt due at tick", eng.gen_flow, win)
    rep, crep = eng.flow_report(), eng.flow_cc_report()  # still readable
    assert rep["flows"] == n and rep["data_offered"] == 4 * n and rep["pending_acks"] > 0 and crep["active"] == n
    assert eng.flow_rows().tobytes() == rows.tobytes() and eng.flow_cc_rows().tobytes() == crows.tobytes()
    for _ in range(4):  # empty windows: what is in flight drains
        eng.step(win)
    fc.configure_late(eng, reorder=0.0)
    eng.flow_init(fc.late_flows(eng.stats()["now_tick"], n_seg=20), **fc.LATE_FLOW)  # re-armed without cc
    wl.flow_run(eng, 8, win)
    rep = eng.flow_report()
    assert rep["done"] == n and rep["segs_acked"] == 20 * n and rep["retransmits"] == 0
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_rows)
