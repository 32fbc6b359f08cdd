"""The flow driver's host model (workloads.FlowModel) over the CPU oracle, against answers known in
closed form: round trips, the HTB wire time, the netem limit, an unreachable peer, a partition that
heals, and the conditions the lossy mesh has to exercise for tests/test_gpu_flow.py to mean something."""
import numpy as np
import pytest

import flow_cases as fc
from testground_amd import abi
from testground_amd import workloads as wl

MS = fc.MS


# -- 1. one round and k rounds ------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [1, 3])
def test_rounds(make_oracle, rounds):
    """n_seg <= window: one round trip, 2 L <= FCT <= 2 L + slack; n_seg = 3 windows: three of them.
    The slack (flow_cases.ROUNDS_SLACK_NS) is two ticks of quantisation and the serialisation of a
    window's segments and ACKs at the unlimited link's HTB rate, per round."""
    out = fc.run_rounds(make_oracle(2, lookahead_ns=fc.ROUNDS["lookahead_ns"]), device=False, rounds=rounds)
    rows, rtt = out["rows"], 2 * fc.ROUNDS["latency_ns"]
    assert (rows["state"] == abi.FLOW_DONE).all() and (rows["retransmits"] == 0).all()
    assert (rows["acked"] == out["flows"]["n_seg"]).all() and (rows["offered"] == rows["acked"]).all()
    fct = fc.fct(out)
    print("FCT", fct, "bounds", rounds * rtt, rounds * (rtt + fc.ROUNDS_SLACK_NS))
    assert (fct >= rounds * rtt).all() and (fct <= rounds * (rtt + fc.ROUNDS_SLACK_NS)).all()
    s = out["summary"]
    assert s["done"] == 2 and s["fct_min_ns"] == fct.min() and s["fct_max_ns"] == fct.max() and s["fct_sum_ns"] == fct.sum()
    assert s["hist"].sum() == 2 and s["hist"][fct[0] // MS] >= 1
    assert out["probes"][0][1]["segs_acked"] == 0  # before the first ACK


# -- 2. bandwidth-bound ---------------------------------------------------------------------------------------
# FCT - wire time of the model's run over the CPU oracle (this test's own run; 8,833,000 ns when this was
# written): the segment's and the ACK's 5-ms hops, less what the burst and the first segment save.  The
# bound is that run's figure rounded up to the two hops, 2 L.
BW_UPPER_SLACK_NS = 2 * fc.BW["latency_ns"]


def test_bandwidth_bound(make_oracle):
    out = fc.run_bandwidth(make_oracle(2, lookahead_ns=fc.BW["lookahead_ns"]), device=False)
    row = out["rows"][0]
    assert row["state"] == abi.FLOW_DONE and row["retransmits"] == 0 and row["acked"] == fc.BW["n_seg"]
    wire_ns = (fc.BW["n_seg"] * fc.BW_FLOW["seg_len"] - fc.BW_BURST_BYTES) * 8 * 10**9 // fc.BW["rate_bps"]
    fct = int(fc.fct(out)[0])
    print("FCT", fct, "wire", wire_ns, "over", fct - wire_ns)
    assert wire_ns <= fct <= wire_ns + BW_UPPER_SLACK_NS
    goodput = out["summary"]["bytes_acked"] * 8 * 10**9 / fct
    assert 0.95 * fc.BW["rate_bps"] <= goodput <= fc.BW["rate_bps"] * 1.01  # the window covers the BDP: the link is full


# -- 3. netem limit ---------------------------------------------------------------------------------------------
def test_netem_limit(make_oracle):
    out = fc.run_limit(make_oracle(fc.LIMIT["n"], lookahead_ns=fc.LIMIT["lookahead_ns"]), device=False)
    v0 = out["windows"][0][0]
    assert len(v0) == 1024 and ((v0 & 15) == abi.V_QUEUE_FULL).sum() == 24  # 1,024 packets, a queue of 1,000
    s = out["summary"]
    assert s["retransmits"] == 24 and s["done"] == 16 and s["failed"] == 0 and s["segs_acked"] == 1024
    assert out["model"].max_row == 1024


# -- 4. unreachable -----------------------------------------------------------------------------------------------
def test_unreachable(make_oracle):
    kw = dict(lookahead_ns=fc.CUT["lookahead_ns"])
    out = fc.run_cut(make_oracle(fc.CUT["n"], **kw), device=False)
    rows, p, flows = out["rows"], fc.CUT_FLOW, out["flows"]
    assert rows["state"].tolist() == [abi.FLOW_FAILED, abi.FLOW_DONE, abi.FLOW_DONE, abi.FLOW_DONE]
    assert rows["offered"][0] == p["max_attempts"] * min(p["window"], flows["n_seg"][0]) and rows["acked"][0] == 0
    assert rows["done_ns"][0] == (int(flows["start_tick"][0]) + p["max_attempts"] * p["rto_ticks"]) * fc.TICK
    assert (rows["retransmits"][1:] == 0).all() and (rows["acked"][1:] == flows["n_seg"][1:]).all()  # the others: unaffected
    v = np.concatenate([w[0] for w in out["windows"]])
    assert ((v & 15) == abi.V_BLACKHOLE).sum() == rows["offered"][0]
    half = fc.run_cut(make_oracle(fc.CUT["n"], **kw), device=False, window=fc.CUT["window"] // 2)
    assert half["rows"].tobytes() == rows.tobytes()  # by tick, not by window
    assert (half["summary"]["hist"] == out["summary"]["hist"]).all()


# -- 5. partition that heals ----------------------------------------------------------------------------------------
def test_partition_heals(make_oracle):
    out = fc.run_heal(make_oracle(fc.HEAL["n"], lookahead_ns=fc.HEAL["lookahead_ns"]), device=False)
    rows = out["rows"]
    assert (rows["state"] == abi.FLOW_DONE).all() and (rows["acked"] == out["flows"]["n_seg"]).all()
    heal_ns = fc.HEAL["w2"] * fc.HEAL["window"] * fc.TICK
    assert fc.fct(out)[0] >= heal_ns and rows["retransmits"][0] > 0  # 0 -> 1 stalled until the rule went
    assert (rows["retransmits"][1:] == 0).all()
    assert out["probes"][6][0]["state"][0] == abi.FLOW_ACTIVE


# -- 6. lossy mesh: the conditions of the GPU comparison, on the model alone ------------------------------------------
def test_mesh_conditions(make_oracle):
    out = fc.run_mesh(make_oracle(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), device=False)
    m, s, flows = out["model"], out["summary"], out["flows"]
    assert 380 <= len(flows) <= 420 and np.bincount(flows["src"]).max() == abi.FLOW_SLOTS and flows["n_seg"].max() > 64
    lat, jit, _ = fc.mesh_shapes()
    assert (jit > 0).all() and fc.mesh_tie_sources_have_jitter(m)
    assert (lat - jit).min() >= fc.MESH["lookahead_ns"]
    assert fc.MESH_FLOW["rto_ticks"] * fc.TICK < 2 * lat.max()  # a timer shorter than some round trips
    assert s["stale_acks"] > 0 and m.max_attempt >= 2
    assert m.max_row > 64 and m.max_ack_row > 64
    assert m.carried_max >= 2 and m.ring_wraps > 0
    assert s["dup_ignored"] > 0 and s["corrupt_ignored"] > 0
    assert s["done"] == s["flows"] == len(flows) and s["pending_acks"] == 0
    mid = out["probes"][fc.MESH["n_windows"] // 2][1]
    assert mid["pending_acks"] > 0 and 0 < mid["done"] < s["flows"]


# -- 7. the model's rules ---------------------------------------------------------------------------------------------
def test_model_rules(make_oracle):
    eng = make_oracle(4, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=0.0)
    with pytest.raises(ValueError, match="not sorted"):
        wl.FlowModel(eng, fc.LATE_FLOW, fc.late_flows(0)[::-1])
    with pytest.raises(ValueError, match="more than 16 flows of source 2"):
        wl.FlowModel(eng, fc.LATE_FLOW, fc.table([(2, 1, 4, 0)] * 17))
    m = wl.FlowModel(eng, fc.LATE_FLOW, fc.late_flows(0))
    with pytest.raises(ValueError, match="longer than rto_ticks"):
        m.window_packets(fc.LATE_FLOW["rto_ticks"] + 1)
    assert m.offered.sum() == 0  # (nothing was generated)


def test_model_late_receipt(make_oracle):
    eng = make_oracle(4, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=50.0)  # half of peer 1's segments skip the netem delay
    m = wl.FlowModel(eng, fc.LATE_FLOW, fc.late_flows(0))
    m.step(fc.LATE["window"])
    rows = m.rows().copy()
    with pytest.raises(wl.FlowLate, match="a receipt due at tick"):
        m.step(fc.LATE["window"])
    assert m.rows().tobytes() == rows.tobytes() and len(m.cal) > 0


def test_flow_table_mesh():
    t = wl.flow_table_mesh(50, 4, 7, seed=2)
    assert len(t) == 200 and (np.diff(t["src"].astype(np.int64)) >= 0).all() and (t["dst"] != t["src"]).all()
    assert (np.bincount(t["src"]) == 4).all() and (t["n_seg"] == 7).all()


def test_flow_lines(make_oracle):
    from testground_amd import metrics

    out = fc.run_bandwidth(make_oracle(2, lookahead_ns=fc.BW["lookahead_ns"]), device=False)
    s = out["summary"]
    lines = metrics.flow_lines(s, fc.BW_FLOW["bin_ns"], "transfer", "r1", 7)
    vals = {ln.split(",")[0]: int(ln.split("value=")[1].split("i ")[0]) for ln in lines if ",bin=" not in ln}
    assert vals["results.transfer.flow.done"] == 1 and vals["results.transfer.flow.bytes_acked"] == 200 * 1460
    assert vals["results.transfer.flow.goodput_bps"] == 200 * 1460 * 8 * 10**9 // s["fct_sum_ns"]
    assert 0.95 * fc.BW["rate_bps"] <= vals["results.transfer.flow.goodput_bps"] <= fc.BW["rate_bps"]
    bins = [ln for ln in lines if ",bin=" in ln]
    assert bins == [f"results.transfer.flow.fct_hist,run=r1,bin={s['fct_sum_ns'] // (10 * MS) * 10 * MS} value=1i 7"]
    idle = dict(s, done=0, fct_sum_ns=0, hist=np.zeros(4, dtype=np.uint64))
    names = [ln.split(",")[0] for ln in metrics.flow_lines(idle, MS, "transfer", "r1", 7)]
    assert "results.transfer.flow.fct_min_ns" not in names and "results.transfer.flow.goodput_bps" not in names
    part = dict(s, flows=2, active=1)  # a flow still running: its bytes are in bytes_acked, its FCT is not
    names = [ln.split(",")[0] for ln in metrics.flow_lines(part, MS, "transfer", "r1", 7)]
    assert "results.transfer.flow.fct_min_ns" in names and "results.transfer.flow.goodput_bps" not in names
