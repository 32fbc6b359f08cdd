"""The device flow loop armed with the RTT estimator (tgsim_flow_init_rto / tgsim_flow_rto_rows /
tgsim_flow_rto_report) against the host model over the CPU oracle (workloads.FlowRtoModel and
FlowCCRtoModel), bit for bit: the verdict bytes and drained records of every window, and the flow rows,
cc rows where armed, rto rows, all summaries and the FCT histogram at three probes and at the end.  The
closed forms, and what the parity inputs exercise, are asserted on the model alone in
tests/test_flow_rto_model.py."""
import ctypes as C
import errno
import gc

import numpy as np
import pytest

import flow_cases as fc
import flow_cc_cases as cc
import flow_rto_cases as rc
from testground_amd import abi
from testground_amd import workloads as wl
from testground_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
MS, TICK = fc.MS, fc.TICK


@pytest.fixture(autouse=True)
def _release_engines():
    """Every engine of a test is destroyed, and its streams released, before the next test starts: one
    caught in a reference cycle (pytest.raises keeps the traceback, and with it the frame that holds the
    engine) would otherwise live until some later collection."""
    yield
    gc.collect()


def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


# -- 1. the estimator on a constant link -------------------------------------------------------------------------------
def test_constant_link(make_oracle):
    kw = dict(lookahead_ns=rc.CONST["lookahead_ns"])
    dev = rc.run_const(Engine(2, **kw), True)
    ref = rc.run_const(make_oracle(2, **kw), False)
    rc.assert_same_run(dev, ref)
    p, row = rc.CONST_RTO, dev["rto_rows"][0]
    assert rc.row_tuple(row) == rc.restate(ref["model"].sample_log[0], rc.CONST_FLOW["rto_ticks"], p["min_rto_ticks"],
                                           p["max_rto_ticks"])
    rtt = 2 * rc.CONST["latency_ns"]
    assert row["samples"] == 12 and rtt <= row["rtt_min"] * TICK and row["rtt_max"] * TICK <= rtt + rc.CONST_SLACK_NS
    assert dev["summary"]["retransmits"] == 0 and dev["summary"]["done"] == 1


# -- 2. spurious retransmissions stop ----------------------------------------------------------------------------------
def test_spurious_retransmissions_stop(make_oracle):
    kw = dict(lookahead_ns=rc.SPUR["lookahead_ns"])
    dev = rc.run_spur(Engine(2, **kw), True, rc.SPUR_RTO)
    rc.assert_same_run(dev, rc.run_spur(make_oracle(2, **kw), False, rc.SPUR_RTO))
    fixed = rc.run_spur(Engine(2, **kw), True, None)
    fc.assert_same_run(fixed, rc.run_spur(make_oracle(2, **kw), False, None))
    assert fixed["summary"]["retransmits"] == 120 and fixed["summary"]["stale_acks"] == 120
    assert dev["summary"]["retransmits"] == 12 and dev["summary"]["stale_acks"] == 12
    assert dev["rto_rows"]["rto"][0] >= 2 * rc.SPUR["latency_ns"] // TICK and fc.fct(dev)[0] <= fc.fct(fixed)[0]


# -- 3. the backoff in closed form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [fc.CUT["window"], fc.CUT["window"] // 2])
@pytest.mark.parametrize("ccp", [None, cc.CUT_CC], ids=["plain", "cc"])
def test_backoff_closed_form(make_oracle, ccp, window):
    kw = dict(lookahead_ns=fc.CUT["lookahead_ns"])
    dev = rc.run_cut(Engine(fc.CUT["n"], **kw), True, window=window, ccp=ccp)
    rc.assert_same_run(dev, rc.run_cut(make_oracle(fc.CUT["n"], **kw), False, window=window, ccp=ccp))
    first = fc.CUT_FLOW["window"] if ccp is None else ccp["init_cwnd"]
    assert dev["rows"]["state"].tolist() == [abi.FLOW_FAILED, abi.FLOW_DONE, abi.FLOW_DONE, abi.FLOW_DONE]
    assert dev["rows"]["done_ns"][0] == (int(dev["flows"]["start_tick"][0]) + rc.CUT_FAIL_AFTER) * TICK
    assert dev["rows"]["offered"][0] == first * rc.CUT_FLOW["max_attempts"]
    assert dev["rto_rows"]["samples"][0] == 0 and dev["rto_rows"]["rto"][0] == rc.CUT_FLOW["rto_ticks"]


# -- 4. degenerate equivalence: the rto kernels give the answers of the kernels without ----------------------------------
@pytest.mark.parametrize("rounds", [1, 3])
def test_degenerate_rounds(make_oracle, rounds):
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    rto = rc.degenerate(fc.ROUNDS_FLOW)
    dev = rc.run_rounds(Engine(2, **kw), True, rounds, rto)
    rc.same_but_rto(dev, fc.run_rounds(Engine(2, **kw), device=True, rounds=rounds))
    rc.assert_same_run(dev, rc.run_rounds(make_oracle(2, **kw), False, rounds, rto))


def test_degenerate_mesh(make_oracle):
    kw = dict(lookahead_ns=fc.MESH["lookahead_ns"])
    rto = rc.degenerate(cc.MESH_FLOW)
    dev = rc.run_mesh(Engine(fc.MESH["n"], **kw), True, rto=rto)
    rc.same_but_rto(dev, cc.run_mesh(Engine(fc.MESH["n"], **kw), True))
    rc.assert_same_run(dev, rc.run_mesh(make_oracle(fc.MESH["n"], **kw), False, rto=rto))


# -- 5. lossy mesh with cc and rto, backoff on ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_ref(oracle_lib):
    from testground_amd.engine import CABIEngine

    return rc.run_mesh(CABIEngine(oracle_lib, "tgo_", fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), False)


def test_mesh_parity(mesh_ref):
    dev = rc.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), True)
    rc.assert_same_run(dev, mesh_ref)
    assert fc.mesh_tie_sources_have_jitter(mesh_ref["model"])
    s, p = dev["rto_summary"], rc.MESH_RTO
    assert s["sampled_flows"] == len(dev["rows"]) and s["rto_min"] == p["min_rto_ticks"] and s["rto_max"] <= p["max_rto_ticks"]


def test_mesh_discard_deliveries(mesh_ref):
    dev = rc.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"], flags=abi.OPT_DISCARD_DELIVERIES), True)
    rc.assert_same_run(dev, mesh_ref, windows=False)
    assert all(len(d) == 0 for _, d in dev["windows"])
    for (dv, _), (rv, _) in zip(dev["windows"], mesh_ref["windows"]):
        assert dv.tobytes() == rv.tobytes()


def test_mesh_window_length(make_oracle):
    """At a second window length, against the model at that length (the counters and the samples depend
    on the step length)."""
    kw = dict(lookahead_ns=fc.MESH["lookahead_ns"])
    dev = rc.run_mesh(Engine(fc.MESH["n"], **kw), True, window=2_000, probe_at=())
    ref = rc.run_mesh(make_oracle(fc.MESH["n"], **kw), False, window=2_000, probe_at=())
    rc.assert_same_run(dev, ref)
    assert dev["rto_rows"].tobytes() == ref["rto_rows"].tobytes() and dev["summary"]["done"] == len(dev["rows"])


# -- 6. corners -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(rc.CORNERS)))
def test_corners(make_oracle, case):
    kw = dict(lookahead_ns=5 * MS)
    dev = rc.run_corner(Engine(4, **kw), True, *rc.CORNERS[case])
    ref = rc.run_corner(make_oracle(4, **kw), False, *rc.CORNERS[case])
    rc.assert_same_run(dev, ref)
    assert ref["rto_summary"]["samples"] > 0 and ref["rows"]["acked"].sum() > 0


# -- 7. rto == NULL through tgsim_flow_init_rto --------------------------------------------------------------------------
class NullRto:
    """An Engine whose flow_init arms through tgsim_flow_init_rto with rto == NULL."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def flow_init(self, flows, seg_len, ack_len, window, rto_ticks, max_attempts, bin_ns=0, n_bins=0, cc=None, rto=None):
        e = self._inner
        assert rto is None
        t = np.ascontiguousarray(flows, dtype=abi.FLOW_SPEC_DTYPE)
        p = abi.Flow(seg_len, ack_len, window, rto_ticks, max_attempts, n_bins, bin_ns)
        c = None if cc is None else C.byref(abi.FlowCC(cc["init_cwnd"], cc["init_ssthresh"], cc["dupthresh"], 0))
        e._check(e._fn("flow_init_rto")(e._h, C.byref(p), c, None, t.ctypes.data, len(t)), "flow_init_rto")
        e._n_flows, e.flow_cc_armed, e.flow_rto_armed = len(t), cc is not None, False


def test_null_rto_is_flow_init_cc():
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    ccp = dict(init_cwnd=2, init_ssthresh=0, dupthresh=3)
    eng = Engine(2, **kw)
    got = cc.run_rounds(NullRto(eng), True, 3, ccp)
    cc.assert_same_run(got, cc.run_rounds(Engine(2, **kw), True, 3, ccp))
    assert (got["rows"]["acked"] > 8).all() and (got["cc_rows"]["cwnd"] == fc.ROUNDS_FLOW["window"]).all()
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_rows)
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_report)
    eng2 = Engine(2, **kw)
    plain = fc.run_rounds(NullRto(eng2), device=True, rounds=1)  # cc == NULL as well: tgsim_flow_init
    fc.assert_same_run(plain, fc.run_rounds(Engine(2, **kw), device=True, rounds=1))
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng2.flow_rto_report)


# -- 8. arming, validation and readers ---------------------------------------------------------------------------------
def test_arming_and_validation():
    n = 8
    ok = dict(seg_len=500, ack_len=64, window=4, rto_ticks=20_000, max_attempts=4)
    good = dict(min_rto_ticks=5_000, max_rto_ticks=100_000, backoff=1)
    t = wl.flow_table_mesh(n, 2, 6, seed=1)
    eng = Engine(n, lookahead_ns=5 * MS)
    fc.plain(eng, n, 5 * MS)
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_rows)
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_report)
    for ccp in (None, dict(init_cwnd=2)):
        for bad, match in ((dict(min_rto_ticks=0), "min_rto_ticks 0"), (dict(max_rto_ticks=4_999), "max_rto_ticks 4999"),
                           (dict(max_rto_ticks=2**27 + 1), f"max_rto_ticks {2**27 + 1}"), (dict(backoff=2), "backoff 2"),
                           (dict(min_rto_ticks=20_001), "rto_ticks 20000"), (dict(max_rto_ticks=19_999), "rto_ticks 20000")):
            _raises(errno.EINVAL, match, eng.flow_init, t, cc=ccp, rto=dict(good, **bad), **ok)
    _raises(errno.EINVAL, "window 65", eng.flow_init, t, rto=good, **dict(ok, window=65))  # tgsim_flow_init's own rules
    _raises(errno.EINVAL, "init_cwnd 5", eng.flow_init, t, cc=dict(init_cwnd=5), rto=good, **ok)
    _raises(errno.EINVAL, "one engine for every peer", Engine(n, shard=(0, 4)).flow_init, t, rto=good, **ok)
    pkt = np.array([(0, 1, 0, 64, 0)], dtype=abi.PKT_DTYPE)
    eng.submit(pkt)
    _raises(errno.EBUSY, "host packets", eng.flow_init, t, rto=good, **ok)
    eng.step(10_000)
    eng.drain()
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, rto=good, **ok)
    assert eng.flow_rto_armed and not eng.flow_cc_armed
    _raises(errno.EBUSY, "flow driver is armed", eng.submit, pkt)
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_rows)
    rows = eng.flow_rto_rows()
    assert len(rows) == 2 * n and (rows["rto"] == 20_000).all() and (rows["rtt_min"] == 0xFFFFFFFF).all()
    assert all((rows[k] == 0).all() for k in ("srtt8", "rttvar4", "samples", "rtt_max", "rtt_last", "_pad"))
    assert eng.flow_rto_report() == dict(samples=0, sampled_flows=0, srtt_sum=0, srtt_min=2**64 - 1, srtt_max=0, rto_sum=0,
                                         rto_min=2**64 - 1, rto_max=0)
    _raises(errno.EINVAL, "longer than min_rto_ticks 5000", eng.gen_flow, 5_001)
    wl.flow_run(eng, 8, 5_000)
    rep, rrep = eng.flow_report(), eng.flow_rto_report()
    assert rep["done"] == rep["flows"] == 2 * n and rrep["samples"] == rep["segs_acked"] == 12 * n and rrep["sampled_flows"] == 2 * n
    # a round trip: 2 x 5 ms, two tick quantisations, and at most every packet of one round (2 n flows x
    # 4 segments and their ACKs, under 0.25 ns per byte) ahead in a queue: under 10 ticks
    slack = 2 + -(-(2 * n * ok["window"] * (ok["seg_len"] + ok["ack_len"]) // 4) // fc.TICK)
    assert 10_000 <= rrep["srtt_min"] <= rrep["srtt_max"] <= 10_000 + slack
    assert 5_000 <= rrep["rto_min"] <= rrep["rto_max"] <= 100_000
    assert len(eng.flow_rto_rows(3, 5)) == 5 and (eng.flow_rto_rows(3, 5)["samples"] == 6).all()
    assert len(eng.flow_rto_rows(2 * n, 0)) == 0
    _raises(errno.EINVAL, "outside", eng.flow_rto_rows, 10, 7)
    _raises(errno.EINVAL, "outside", eng.flow_rto_rows, 2 * n + 1, 0)
    out = np.zeros(2, dtype=abi.FLOW_RTO_ROW_DTYPE)
    assert eng._fn("flow_rto_rows")(eng._h, 0, 3, out.ctypes.data, 2) == -errno.ENOSPC  # cap below n
    assert eng._fn("flow_rto_rows")(eng._h, 0, 3, None, 3) == -errno.EINVAL
    assert eng._fn("flow_rto_report")(eng._h, None) == -errno.EINVAL
    # armed without rto: the flow reports answer, the rto readers do not; disarmed: none does
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, cc=dict(init_cwnd=2), **ok)
    assert not eng.flow_rto_armed and eng.flow_report()["segs_acked"] == 0
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_rows)
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_report)
    _raises(errno.EINVAL, "longer than rto_ticks 20000", eng.gen_flow, 20_001)
    wl.flow_run(eng, 8, 5_000)
    assert eng.flow_report()["done"] == 2 * n
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, cc=dict(init_cwnd=2), rto=good, **ok)  # both
    assert eng.flow_rto_armed and eng.flow_cc_armed and (eng.flow_cc_rows()["cwnd"] == 2).all()
    eng.flow_init(None)
    _raises(errno.EINVAL, "not armed", eng.flow_rows)
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_rows)
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng.flow_rto_report)
    eng.submit(pkt)
    eng.step(10)


def test_late_receipt_keeps_rto_rows():
    n, win = fc.LATE["n"], fc.LATE["window"]
    good = dict(min_rto_ticks=5_000, max_rto_ticks=100_000, backoff=1)
    eng = Engine(n, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=50.0)
    eng.flow_init(fc.late_flows(0), cc=dict(init_cwnd=4, init_ssthresh=0, dupthresh=3), rto=good, **fc.LATE_FLOW)
    eng.gen_flow(win)
    eng.step(win)
    rows, crows, rrows = eng.flow_rows(), eng.flow_cc_rows(), eng.flow_rto_rows()
    for _ in range(2):  # sticky
        _raises(errno.EINVAL, "flow: a receipt due at tick", eng.gen_flow, win)
    rep, rrep = eng.flow_report(), eng.flow_rto_report()  # still readable
    assert rep["flows"] == n and rep["data_offered"] == 4 * n and rep["pending_acks"] > 0
    assert rrep["samples"] == int(rrows["samples"].sum())
    assert eng.flow_rows().tobytes() == rows.tobytes() and eng.flow_cc_rows().tobytes() == crows.tobytes()
    assert eng.flow_rto_rows().tobytes() == rrows.tobytes()
    for _ in range(4):  # empty windows: what is in flight drains
        eng.step(win)
    fc.configure_late(eng, reorder=0.0)
    eng.flow_init(fc.late_flows(eng.stats()["now_tick"], n_seg=20), rto=good, **fc.LATE_FLOW)  # re-armed, without cc
    wl.flow_run(eng, 8, win)
    rep = eng.flow_report()
    assert rep["done"] == n and rep["segs_acked"] == 20 * n and rep["retransmits"] == 0
    assert eng.flow_rto_report()["samples"] == 20 * n
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_rows)


def test_struct_sizes():
    assert C.sizeof(abi.FlowRto) == 16 and abi.FLOW_RTO_ROW_DTYPE.itemsize == 32 and C.sizeof(abi.FlowRtoSummary) == 64
