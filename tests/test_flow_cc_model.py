"""The congestion-control host model (workloads.FlowCCModel) over the CPU oracle: the closed forms of
slow start, congestion avoidance, the degenerate window and an unreachable peer, and the conditions the
parity inputs of tests/test_gpu_flow_cc.py (netem limit, lossy mesh, corners) have to meet for a green
device run to mean something."""
import numpy as np
import pytest

import flow_cases as fc
import flow_cc_cases as cc
from testground_amd import abi
from testground_amd import workloads as wl

MS = fc.MS


# -- 1, 2. slow start and congestion avoidance -----------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(cc.RAMPS)))
def test_ramp(make_oracle, case):
    """Slow start from 1: round r carries 2^(r-1) segments, so 31 segments take 5 round trips and 32
    take 6.  Avoidance from cwnd = ssthresh = 4: round r carries 3 + r, so 22 take 4 and 23 take 5.  Per
    round 2 L <= time <= 2 L + slack (flow_cc_cases.RAMP_SLACK_NS)."""
    ccp, n_seg, rounds = cc.RAMPS[case]
    out = cc.run_ramp(make_oracle(2, lookahead_ns=cc.RAMP["lookahead_ns"]), False, ccp, n_seg, rounds)
    row, crow, rtt = out["rows"][0], out["cc_rows"][0], 2 * cc.RAMP["latency_ns"]
    fct = int(fc.fct(out)[0])
    print("FCT", fct, "bounds", rounds * rtt, rounds * (rtt + cc.RAMP_SLACK_NS), "cc row", crow)
    assert row["state"] == abi.FLOW_DONE and row["acked"] == row["offered"] == n_seg and row["retransmits"] == 0
    assert rounds * rtt <= fct <= rounds * (rtt + cc.RAMP_SLACK_NS)
    assert crow["loss_events"] == 0 and crow["fast_retransmits"] == 0 and crow["timeouts"] == 0
    assert crow["next"] == n_seg and crow["recover"] == 0
    if ccp is cc.SLOW_START:
        assert crow["cwnd"] == min(1 + n_seg, cc.RAMP_FLOW["window"]) and crow["ssthresh"] == cc.RAMP_FLOW["window"]
    elif n_seg == 22:
        assert crow["cwnd"] == 8 and crow["ssthresh"] == 4
    s = out["cc_summary"]
    assert s["active"] == 0 and s["cwnd_sum"] == 0 and s["cwnd_min"] == 2**64 - 1 and s["cwnd_max"] == 0
    first = out["probes"][0]  # before the first ACK: the initial window, and the flow ACTIVE
    assert first[0]["offered"][0] == ccp["init_cwnd"] and first[3]["active"] == 1
    assert first[3]["cwnd_sum"] == first[3]["cwnd_min"] == first[3]["cwnd_max"] == ccp["init_cwnd"]


# -- 3. degenerate equivalence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds,dupthresh", [(1, 0), (3, 3)])
def test_degenerate_rounds(make_oracle, rounds, dupthresh):
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    ccp = cc.degenerate(fc.ROUNDS_FLOW["window"], dupthresh)
    got = cc.run_rounds(make_oracle(2, **kw), False, rounds, ccp)
    cc.same_plain_run(got, fc.run_rounds(make_oracle(2, **kw), device=False, rounds=rounds))
    assert (got["cc_rows"]["cwnd"] == fc.ROUNDS_FLOW["window"]).all() and got["cc_summary"]["loss_events"] == 0


def test_degenerate_bandwidth(make_oracle):
    kw = dict(lookahead_ns=fc.BW["lookahead_ns"])
    got = cc.run_bandwidth(make_oracle(2, **kw), False, cc.degenerate(fc.BW_FLOW["window"], 63))
    cc.same_plain_run(got, fc.run_bandwidth(make_oracle(2, **kw), device=False))
    assert got["cc_rows"]["cwnd"][0] == fc.BW_FLOW["window"] and got["cc_summary"]["fast_retransmits"] == 0


# -- 4. unreachable ---------------------------------------------------------------------------------------------------
def test_unreachable(make_oracle):
    kw = dict(lookahead_ns=fc.CUT["lookahead_ns"])
    out = cc.run_cut(make_oracle(fc.CUT["n"], **kw), False)
    none = fc.run_cut(make_oracle(fc.CUT["n"], **kw), device=False)
    rows, crow, p, c = out["rows"], out["cc_rows"][0], fc.CUT_FLOW, cc.CUT_CC
    assert rows["state"].tolist() == [abi.FLOW_FAILED, abi.FLOW_DONE, abi.FLOW_DONE, abi.FLOW_DONE]
    assert rows["done_ns"][0] == none["rows"]["done_ns"][0]  # the fail tick of the run without cc
    assert rows["offered"][0] == c["init_cwnd"] * p["max_attempts"] and rows["acked"][0] == 0
    assert crow["timeouts"] == c["init_cwnd"] * (p["max_attempts"] - 1)
    assert crow["loss_events"] == 1 and crow["cwnd"] == 1 and crow["ssthresh"] == max(c["init_cwnd"] // 2, 2)
    assert crow["next"] == crow["recover"] == c["init_cwnd"]
    half = cc.run_cut(make_oracle(fc.CUT["n"], **kw), False, window=fc.CUT["window"] // 2)
    assert half["rows"]["done_ns"][0] == rows["done_ns"][0]  # by tick, not by window
    assert half["cc_rows"][0].tobytes() == crow.tobytes()


# -- 6 to 8: the conditions of the parity inputs, on the model alone ---------------------------------------------------
@pytest.fixture(scope="module")
def parity_runs(oracle_lib):
    from testground_amd.engine import CABIEngine

    mk = (lambda n, **kw: CABIEngine(oracle_lib, "tgo_", n, **kw))
    runs = {"limit": cc.run_limit(mk(fc.LIMIT["n"], lookahead_ns=fc.LIMIT["lookahead_ns"]), False),
            "mesh": cc.run_mesh(mk(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), False)}
    for row in cc.CORNERS:
        runs[row] = cc.run_corner(mk(4, lookahead_ns=5 * MS), False, *row)
    return runs


def test_limit_conditions(parity_runs):
    out = parity_runs["limit"]
    v = np.concatenate([w[0] for w in out["windows"]])
    assert ((v & 15) == abi.V_QUEUE_FULL).sum() > 0 and out["model"].max_row > 1000
    assert out["cc_summary"]["loss_events"] > 0 and out["summary"]["done"] == out["summary"]["flows"] == 16
    assert (out["cc_rows"]["cwnd"] <= cc.LIMIT_FLOW["window"]).all()


def test_mesh_conditions(parity_runs):
    out = parity_runs["mesh"]
    m, s = out["model"], out["summary"]
    lat, jit, _ = fc.mesh_shapes()
    assert (jit > 0).all() and fc.mesh_tie_sources_have_jitter(m) and (lat - jit).min() >= fc.MESH["lookahead_ns"]
    assert s["done"] == s["flows"] == len(out["flows"]) and s["pending_acks"] == 0 and s["stale_acks"] > 0
    mid = out["probes"][max(out["probes"])]
    assert mid[1]["pending_acks"] > 0 and 0 < mid[1]["done"] < s["flows"] and mid[3]["active"] > 0
    assert 1 <= mid[3]["cwnd_min"] <= mid[3]["cwnd_max"] <= cc.MESH_FLOW["window"]


def test_corner_rows():
    rows = cc.CORNERS
    assert (64, 64, 63, 130) in rows and any(r[0] == 1 for r in rows) and 7 <= len(rows) <= 10
    assert {r[0] for r in rows} == {1, 2, 64} and {r[2] for r in rows} == {0, 1, 3, 63} and {r[3] for r in rows} == {1, 65, 130}
    assert all(r[1] in (1, r[0]) for r in rows)


def test_parity_inputs_exercise_every_path(parity_runs):
    """Over the netem limit, the mesh and the corners together (flow_cc_cases.exercised)."""
    tot = cc.exercised(parity_runs.values())
    print(tot)
    assert tot["fast_retransmits"] > 0 and tot["timeouts"] > 0
    assert tot["loss_fast"] > 0 and tot["loss_timeout"] > 0  # a loss event from each cause
    assert tot["draining"] > 0  # next - base > cwnd: a reduced window draining
    assert tot["fast_acked_early"] > 0  # a fast-marked segment acknowledged before its re-offer
    assert tot["fast_lost"] > 0  # a fast retransmission lost and recovered by its timer (attempt >= 2)
    assert tot["cwnd_at_cap"] > 0 and tot["grow_ss"] > 0 and tot["grow_ca"] > 0
    assert tot["suppressed"] > 0 and tot["ring_wraps"] > 0
    for out in parity_runs.values():  # the invariant, and the counters' sums
        r, c, f, w = out["rows"], out["cc_rows"], out["flows"], out["model"].flow["window"]
        assert (r["base"] <= c["next"]).all() and (c["next"] <= np.minimum(r["base"].astype(np.int64) + w, f["n_seg"])).all()
        assert (c["cwnd"] >= 1).all() and (c["cwnd"] <= w).all()
        assert (r["retransmits"] == c["timeouts"].astype(np.int64) + c["fast_retransmits"] - _unsent_fast(out)).all()


def _unsent_fast(out):
    """Per flow, the segments marked FAST whose retransmission was never offered: acknowledged first,
    or still waiting when the run (or the flow) ended."""
    m = out["model"]
    sent = np.array([len(s) for s in m._was_fast])
    # a segment is marked at most once (attempt 1 exactly), and _was_fast holds each one offered
    return m.fast_retransmits - sent


# -- the model's rules -----------------------------------------------------------------------------------------------
def test_model_validation(make_oracle):
    eng = make_oracle(4, lookahead_ns=fc.LATE["lookahead_ns"])
    flows, w = fc.late_flows(0), fc.LATE_FLOW["window"]
    for bad, match in ((dict(init_cwnd=0), "init_cwnd 0"), (dict(init_cwnd=w + 1), f"init_cwnd {w + 1}"),
                       (dict(init_ssthresh=1), "init_ssthresh 1"), (dict(init_ssthresh=w + 1), f"init_ssthresh {w + 1}"),
                       (dict(dupthresh=64), "dupthresh 64")):
        with pytest.raises(ValueError, match=match):
            wl.FlowCCModel(eng, fc.LATE_FLOW, flows, bad)
    assert wl.flow_reference(eng, fc.LATE_FLOW, flows, 0, 1000)["model"].__class__ is wl.FlowModel  # cc=None: as before


def test_model_late_receipt_keeps_cc_rows(make_oracle):
    eng = make_oracle(4, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=50.0)
    m = wl.FlowCCModel(eng, fc.LATE_FLOW, fc.late_flows(0), dict(init_cwnd=4))
    m.step(fc.LATE["window"])
    rows, crows = m.rows().copy(), m.cc_rows().copy()
    with pytest.raises(wl.FlowLate, match="a receipt due at tick"):
        m.step(fc.LATE["window"])
    assert m.rows().tobytes() == rows.tobytes() and m.cc_rows().tobytes() == crows.tobytes()


def test_flow_cc_lines(make_oracle):
    from testground_amd import metrics

    out = cc.run_cut(make_oracle(fc.CUT["n"], lookahead_ns=fc.CUT["lookahead_ns"]), False)
    plain = metrics.flow_lines(out["summary"], MS, "transfer", "r1", 7)
    assert not any(".flow.cc." in ln for ln in plain)
    lines = metrics.flow_lines(dict(out["summary"], cc=out["cc_summary"]), MS, "transfer", "r1", 7)
    assert [ln for ln in lines if ".flow.cc." not in ln] == plain
    vals = {ln.split(",")[0]: int(ln.split("value=")[1].split("i ")[0]) for ln in lines if ".flow.cc." in ln}
    assert vals["results.transfer.flow.cc.loss_events"] == 1 and vals["results.transfer.flow.cc.timeouts"] == 6
    assert vals["results.transfer.flow.cc.active"] == 0 and "results.transfer.flow.cc.cwnd_min" not in vals
