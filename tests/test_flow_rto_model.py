"""The RTT-estimator host model (workloads.FlowRtoModel / FlowCCRtoModel) over the CPU oracle: the
estimator on a constant link, the end of spurious retransmissions, the closed form of the backoff, the
degenerate timer, and the conditions the parity inputs of tests/test_gpu_flow_rto.py (lossy mesh,
corners) have to meet for a green device run to mean something."""
import numpy as np
import pytest

import flow_cases as fc
import flow_cc_cases as cc
import flow_rto_cases as rc
from testground_amd import abi
from testground_amd import workloads as wl

MS, TICK = fc.MS, fc.TICK


# -- 1. the estimator on a constant link -------------------------------------------------------------------------------
def test_constant_link(make_oracle):
    out = rc.run_const(make_oracle(2, lookahead_ns=rc.CONST["lookahead_ns"]), False)
    m, row, rtt = out["model"], out["rows"][0], 2 * rc.CONST["latency_ns"]
    log = m.sample_log[0]
    print("samples", log, "slack ns", rc.CONST_SLACK_NS, "row", out["rto_rows"][0])
    assert len(log) == rc.CONST["n_seg"] == 12 and out["rto_rows"]["samples"][0] == 12
    assert all(rtt <= s * TICK <= rtt + rc.CONST_SLACK_NS for s in log)
    p = rc.CONST_RTO
    assert rc.row_tuple(out["rto_rows"][0]) == rc.restate(log, rc.CONST_FLOW["rto_ticks"], p["min_rto_ticks"], p["max_rto_ticks"])
    assert row["state"] == abi.FLOW_DONE and row["retransmits"] == 0 and row["offered"] == 12
    s = out["rto_summary"]
    assert s["samples"] == 12 and s["sampled_flows"] == 1
    assert s["srtt_sum"] == s["srtt_min"] == s["srtt_max"] == out["rto_rows"]["srtt8"][0] >> 3
    assert s["rto_sum"] == s["rto_min"] == s["rto_max"] == out["rto_rows"]["rto"][0]
    first = out["probes"][0]  # before the first ACK: the initial timer, no sample
    assert rc.row_tuple(first[2][0]) == (0, 0, rc.CONST_FLOW["rto_ticks"], 0, 0xFFFFFFFF, 0, 0)
    assert first[3] == dict(samples=0, sampled_flows=0, srtt_sum=0, srtt_min=2**64 - 1, srtt_max=0, rto_sum=0,
                            rto_min=2**64 - 1, rto_max=0)


# -- 2. spurious retransmissions stop ----------------------------------------------------------------------------------
def test_spurious_retransmissions_stop(make_oracle):
    kw = dict(lookahead_ns=rc.SPUR["lookahead_ns"])
    fixed = rc.run_spur(make_oracle(2, **kw), False, None)
    out = rc.run_spur(make_oracle(2, **kw), False, rc.SPUR_RTO)
    print("fixed", fixed["summary"], "adaptive", out["summary"], out["rto_rows"][0])
    assert fixed["summary"]["retransmits"] == 120 and fixed["summary"]["stale_acks"] == 120
    assert out["summary"]["retransmits"] == 12 and out["summary"]["stale_acks"] == 12
    # all from the first four segments: after the probe behind their ACKs nothing is retransmitted again
    assert out["probes"][11][1]["retransmits"] == 12 and out["probes"][11][0]["base"][0] >= 4
    assert out["rto_rows"]["rto"][0] >= 2 * rc.SPUR["latency_ns"] // TICK
    assert out["rows"]["state"][0] == fixed["rows"]["state"][0] == abi.FLOW_DONE
    assert fc.fct(out)[0] <= fc.fct(fixed)[0]
    assert out["model"].sampled_after_retransmit == 4


# -- 3. the backoff in closed form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ccp", [None, cc.CUT_CC], ids=["plain", "cc"])
def test_backoff_closed_form(make_oracle, ccp):
    kw = dict(lookahead_ns=fc.CUT["lookahead_ns"])
    out = rc.run_cut(make_oracle(fc.CUT["n"], **kw), False, ccp=ccp)
    half = rc.run_cut(make_oracle(fc.CUT["n"], **kw), False, window=fc.CUT["window"] // 2, ccp=ccp)
    first = fc.CUT_FLOW["window"] if ccp is None else ccp["init_cwnd"]
    for o in (out, half):
        assert o["rows"]["state"].tolist() == [abi.FLOW_FAILED, abi.FLOW_DONE, abi.FLOW_DONE, abi.FLOW_DONE]
        assert o["rows"]["done_ns"][0] == (int(o["flows"]["start_tick"][0]) + rc.CUT_FAIL_AFTER) * TICK
        assert o["rows"]["offered"][0] == first * rc.CUT_FLOW["max_attempts"] and o["rows"]["acked"][0] == 0
        assert o["rto_rows"]["samples"][0] == 0 and o["rto_rows"]["rto"][0] == rc.CUT_FLOW["rto_ticks"]
        assert (o["rto_rows"]["samples"][1:] > 0).all() and o["rto_summary"]["sampled_flows"] == 3
    assert out["model"].shifted_twice > 0 and out["model"].shift_capped > 0


# -- 4. degenerate equivalence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [1, 3])
def test_degenerate_rounds(make_oracle, rounds):
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])
    got = rc.run_rounds(make_oracle(2, **kw), False, rounds, rc.degenerate(fc.ROUNDS_FLOW))
    rc.same_but_rto(got, fc.run_rounds(make_oracle(2, **kw), device=False, rounds=rounds))
    assert (got["rto_rows"]["rto"] == fc.ROUNDS_FLOW["rto_ticks"]).all() and (got["rto_rows"]["samples"] > 0).all()


@pytest.fixture(scope="module")
def parity_runs(oracle_lib):
    from testground_amd.engine import CABIEngine

    mk = (lambda n, **kw: CABIEngine(oracle_lib, "tgo_", n, **kw))
    runs = {"mesh": rc.run_mesh(mk(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), False)}
    for i, row in enumerate(rc.CORNERS):
        runs[i] = rc.run_corner(mk(4, lookahead_ns=5 * MS), False, *row)
    return runs


def test_degenerate_mesh(oracle_lib):
    from testground_amd.engine import CABIEngine

    mk = (lambda: CABIEngine(oracle_lib, "tgo_", fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]))
    got = rc.run_mesh(mk(), False, rto=rc.degenerate(cc.MESH_FLOW))
    rc.same_but_rto(got, cc.run_mesh(mk(), False))
    assert (got["rto_rows"]["rto"] == cc.MESH_FLOW["rto_ticks"]).all() and got["rto_summary"]["samples"] > 0


# -- 5. what the parity inputs exercise --------------------------------------------------------------------------------------
def test_mesh_conditions(parity_runs):
    out = parity_runs["mesh"]
    m, s = out["model"], out["summary"]
    assert fc.mesh_tie_sources_have_jitter(m)
    assert s["done"] == s["flows"] == len(out["flows"]) and s["pending_acks"] == 0
    r, p = out["rto_rows"], rc.MESH_RTO
    assert (r["samples"] > 0).all() and r["rto"].min() == p["min_rto_ticks"] and (r["rto"] <= p["max_rto_ticks"]).all()
    assert m.clamped_min > 0 and m.clamped_max > 0 and m.sampled_after_retransmit > 0 and m.unsampled_attempts > 0
    mid = out["probes"][max(out["probes"])]
    assert mid[1]["pending_acks"] > 0 and 0 < mid[1]["done"] < s["flows"] and 0 < mid[5]["sampled_flows"]


def test_corner_rows():
    rows = rc.CORNERS
    assert {r[0] for r in rows} == {1, 64} and {r[1] is None for r in rows} == {True, False}
    assert any(r[0] == w and (r[1] is None) == plain for w in (1, 64) for plain in (True, False) for r in rows)
    assert any(r[2] == 1 and r[4] == 12_000 for r in rows) and any(r[4] == rc.MAX_RTO for r in rows)
    assert any(r[3] == r[4] and r[2] == 1 for r in rows)


def test_parity_inputs_exercise_every_path(parity_runs):
    """Over the mesh and the corners together (flow_rto_cases.exercised)."""
    tot = rc.exercised(parity_runs.values())
    print(tot)
    assert tot["samples"] > 0
    assert tot["sampled_after_retransmit"] > 0  # a sample from a segment that had been retransmitted since
    assert tot["clamped_min"] > 0 and tot["clamped_max"] > 0
    assert tot["shifted_twice"] > 0 and tot["shift_capped"] > 0
    assert tot["unsampled_attempts"] > 0  # a non-stale ACK of a later attempt: no sample
    assert tot["ring_wraps"] > 0
    for i, row in enumerate(rc.CORNERS):  # each corner on its own
        out = parity_runs[i]
        m, r = out["model"], out["rto_rows"]
        assert out["rto_summary"]["samples"] > 0 and (r["rto"] >= row[3]).all() and (r["rto"] <= row[4]).all()
        assert r["samples"][3] == 0 and r["rto"][3] == row[5]  # (behind the Drop rule)
        if row[2] == 1 and row[4] == 12_000:  # the flow behind the Drop rule runs out of attempts: shift 15, capped
            assert m.max_attempt == 15 and out["rows"]["state"][3] == abi.FLOW_FAILED and m.shift_capped > 0
            fail = row[5] + 15 * row[4]
            assert out["rows"]["done_ns"][3] == (int(out["flows"]["start_tick"][3]) + fail) * TICK
        if row[3] == row[4]:
            assert (r["rto"] == row[3]).all() and m.shift_capped > 0


# -- the model's rules ---------------------------------------------------------------------------------------------------------
def test_model_validation(make_oracle):
    eng = make_oracle(4, lookahead_ns=fc.LATE["lookahead_ns"])
    flows, p = fc.late_flows(0), fc.LATE_FLOW
    good = dict(min_rto_ticks=5_000, max_rto_ticks=100_000, backoff=1)
    for bad, match in ((dict(min_rto_ticks=0), "min_rto_ticks 0"), (dict(max_rto_ticks=4_999), "max_rto_ticks 4999"),
                       (dict(max_rto_ticks=2**27 + 1), f"max_rto_ticks {2**27 + 1}"), (dict(backoff=2), "backoff 2"),
                       (dict(min_rto_ticks=50_001), "rto_ticks 50000"), (dict(max_rto_ticks=49_999), "rto_ticks 50000")):
        with pytest.raises(ValueError, match=match):
            wl.FlowRtoModel(eng, p, flows, rto=dict(good, **bad))
    with pytest.raises(ValueError, match="longer than min_rto_ticks 5000"):
        wl.FlowRtoModel(eng, p, flows, rto=good).window_packets(5_001)
    assert wl.flow_reference(eng, p, flows, 0, 1000)["model"].__class__ is wl.FlowModel  # rto=None: as before
    assert wl.flow_reference(eng, p, flows, 0, 1000, cc=dict(init_cwnd=2))["model"].__class__ is wl.FlowCCModel
    assert isinstance(wl.flow_reference(eng, p, flows, 0, 1000, cc=dict(init_cwnd=2), rto=good)["model"], wl.FlowCCModel)


def test_model_late_receipt_keeps_rto_rows(make_oracle):
    eng = make_oracle(4, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=50.0)
    m = wl.FlowCCRtoModel(eng, fc.LATE_FLOW, fc.late_flows(0), dict(init_cwnd=4),
                          rto=dict(min_rto_ticks=5_000, max_rto_ticks=100_000, backoff=1))
    m.step(fc.LATE["window"])
    rows, rrows, sent = m.rows().copy(), m.rto_rows().copy(), m.sent.copy()
    with pytest.raises(wl.FlowLate, match="a receipt due at tick"):
        m.step(fc.LATE["window"])
    assert m.rows().tobytes() == rows.tobytes() and m.rto_rows().tobytes() == rrows.tobytes() and (m.sent == sent).all()


def test_flow_rto_lines(make_oracle):
    from testground_amd import metrics

    out = rc.run_const(make_oracle(2, lookahead_ns=rc.CONST["lookahead_ns"]), False)
    plain = metrics.flow_lines(out["summary"], MS, "transfer", "r1", 7)
    assert not any(".flow.rto." in ln for ln in plain)
    lines = metrics.flow_lines(dict(out["summary"], rto=out["rto_summary"]), MS, "transfer", "r1", 7)
    assert [ln for ln in lines if ".flow.rto." not in ln] == plain
    vals = {ln.split(",")[0]: int(ln.split("value=")[1].split("i ")[0]) for ln in lines if ".flow.rto." in ln}
    assert vals["results.transfer.flow.rto.samples"] == 12 and vals["results.transfer.flow.rto.sampled_flows"] == 1
    assert vals["results.transfer.flow.rto.rto_max"] == out["rto_rows"]["rto"][0]
    none = metrics.flow_lines(dict(out["summary"], rto=out["probes"][0][3]), MS, "transfer", "r1", 7)
    assert not any("rto.srtt_min" in ln or "rto.rto_max" in ln for ln in none)


def test_struct_sizes():
    import ctypes as C

    assert C.sizeof(abi.FlowRto) == 16 and abi.FLOW_RTO_ROW_DTYPE.itemsize == 32 and C.sizeof(abi.FlowRtoSummary) == 64
