"""The device flow loop armed with the verdict feedback (tgsim_flow_init_fb / tgsim_flow_fb_rows /
tgsim_flow_fb_report) against the host model over the CPU oracle (workloads.FlowFbMixin), bit for bit:
the verdict bytes and drained records of every window, and the flow rows, the cc and rto rows where
armed, the fb rows, all summaries and the FCT histogram at three probes and at the end.  The closed
forms, and what the parity inputs exercise, are asserted on the model alone in
tests/test_flow_fb_model.py."""
import ctypes as C
import errno
import gc

import numpy as np
import pytest

import flow_cases as fc
import flow_cc_cases as cc
import flow_fb_cases as fb
import flow_rto_cases as rc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl
from testground_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
MS, TICK = fc.MS, fc.TICK
CUT_KW = dict(lookahead_ns=fc.CUT["lookahead_ns"])
DONE, FAILED = abi.FLOW_DONE, abi.FLOW_FAILED
NOT_ARMED = "verdict feedback is not armed"


@pytest.fixture(autouse=True)
def _release_engines():
    """Every engine of a test is destroyed, and its streams released, before the next test starts (see
    tests/test_gpu_flow_rto.py)."""
    yield
    gc.collect()


def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


def _fb(out, f):
    return {k: int(out["fb_rows"][k][f]) for k in abi.FLOW_FB_ROW_DTYPE.names}


# -- 1. cut at arming -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [fc.CUT["window"], fc.CUT["window"] // 2])
@pytest.mark.parametrize("variant", list(fb.CUT_VARIANTS))
def test_cut_at_arming(make_oracle, variant, window):
    dev = fb.run_cut(Engine(fc.CUT["n"], **CUT_KW), True, variant, fb.BLACKHOLE, window=window)
    fb.assert_same_run(dev, fb.run_cut(make_oracle(fc.CUT["n"], **CUT_KW), False, variant, fb.BLACKHOLE, window=window))
    rows, row = dev["rows"], _fb(dev, 0)
    assert rows["state"].tolist() == [FAILED, DONE, DONE, DONE]
    assert rows["done_ns"][0] == int(dev["flows"]["start_tick"][0]) * TICK  # the same at both step lengths
    assert (row["fail_verdict"], row["fail_seg"], row["fail_attempt"]) == (abi.V_BLACKHOLE, 0, 0)
    assert row["refused"] == rows["offered"][0] == fb.cut_first(variant)
    assert dev["fb_summary"]["failed_blackhole"] == 1 and fb.identity_everywhere(dev)


@pytest.mark.parametrize("variant", list(fb.CUT_VARIANTS))
def test_cut_without_mask_fails_by_timer(make_oracle, variant):
    dev = fb.run_cut(Engine(fc.CUT["n"], **CUT_KW), True, variant, 0)
    fb.assert_same_run(dev, fb.run_cut(make_oracle(fc.CUT["n"], **CUT_KW), False, variant, 0))
    flow, _, _, fail_after, _ = fb.CUT_VARIANTS[variant]
    rows, row = dev["rows"], _fb(dev, 0)
    assert rows["state"].tolist() == [FAILED, DONE, DONE, DONE]
    assert rows["done_ns"][0] == (int(dev["flows"]["start_tick"][0]) + fail_after) * TICK
    assert (row["fail_verdict"], row["fail_seg"], row["fail_attempt"]) == (0, 0, 0)
    assert row["refused"] == rows["offered"][0] == fb.cut_first(variant) * flow["max_attempts"]
    assert dev["fb_summary"]["failed_timer"] == 1


# -- 2. the mask selects -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [fb.BLACKHOLE, fb.PROHIBIT], ids=["other", "mine"])
def test_mask_selects(make_oracle, mask):
    reject = nw.FilterAction.Reject
    dev = fb.run_cut(Engine(fc.CUT["n"], **CUT_KW), True, "plain", mask, action=reject)
    ref = fb.run_cut(make_oracle(fc.CUT["n"], **CUT_KW), False, "plain", mask, action=reject)
    fb.assert_same_run(dev, ref)
    p, t0 = fc.CUT_FLOW, int(dev["flows"]["start_tick"][0])
    if mask == fb.PROHIBIT:
        assert _fb(dev, 0)["fail_verdict"] == abi.V_PROHIBIT and dev["rows"]["done_ns"][0] == t0 * TICK
    else:
        assert ref["model"].refused_unmasked > 0 and _fb(dev, 0)["fail_verdict"] == 0
        assert dev["rows"]["done_ns"][0] == (t0 + p["max_attempts"] * p["rto_ticks"]) * TICK and dev["fb_summary"]["failed_timer"] == 1


# -- 3. partition mid-transfer ---------------------------------------------------------------------------------------------------
def test_partition_mid_transfer(make_oracle):
    kw = dict(lookahead_ns=fc.HEAL["lookahead_ns"])
    ticks = []
    for window in (5_000, 2_500):
        dev = fb.run_partition(Engine(fc.HEAL["n"], **kw), True, window=window)
        fb.assert_same_run(dev, fb.run_partition(make_oracle(fc.HEAL["n"], **kw), False, window=window))
        assert dev["rows"]["state"].tolist() == [FAILED, DONE, DONE, DONE] and _fb(dev, 0)["fail_verdict"] == abi.V_BLACKHOLE
        assert dev["rows"]["retransmits"][3] == 0
        ticks.append(fb.fail_tick(dev, 0))
    assert ticks[0] == ticks[1] >= fb.PART["tick"]


def test_partition_of_the_ack_leg_fails_by_timer(make_oracle):
    kw = dict(lookahead_ns=fc.HEAL["lookahead_ns"])
    dev = fb.run_partition(Engine(fc.HEAL["n"], **kw), True, ack_leg=True)
    fb.assert_same_run(dev, fb.run_partition(make_oracle(fc.HEAL["n"], **kw), False, ack_leg=True))
    assert dev["rows"]["state"][0] == FAILED and _fb(dev, 0)["fail_verdict"] == 0 and dev["fb_summary"]["refused"] == 0


# -- 4. disconnect -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [5_000, 2_500])
def test_disconnect(make_oracle, window):
    kw = dict(lookahead_ns=fc.BW["lookahead_ns"])
    dev = fb.run_disconnect(Engine(4, **kw), True, window=window)
    fb.assert_same_run(dev, fb.run_disconnect(make_oracle(4, **kw), False, window=window))
    assert dev["rows"]["state"].tolist() == [FAILED, FAILED, DONE] and dev["fb_summary"]["failed_disconnected"] == 2
    assert dev["rows"]["stale_acks"][0] > 0


# -- 5. a timer failure and a refusal in one window -----------------------------------------------------------------------------------
def test_timer_failure_and_refusal_in_one_window(make_oracle):
    rows = []
    for window in (5_000, 2_500):
        dev = fb.run_both(Engine(fb.BOTH["n"], **fb.both_kw()), True, window=window)
        ref = fb.run_both(make_oracle(fb.BOTH["n"], **fb.both_kw()), False, window=window)
        fb.assert_same_run(dev, ref)
        assert ref["model"].fail_replaced >= (window == 5_000)
        row = _fb(dev, 0)
        assert (row["fail_verdict"], row["fail_seg"], row["fail_attempt"], row["queue_full"]) == (abi.V_PROHIBIT, 2, 1, 3)
        rows.append(dev["rows"][0].tobytes() + dev["fb_rows"][0].tobytes())
    assert rows[0] == rows[1]


# -- 6. lossy mesh with cc, rto and fb ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_ref(oracle_lib):
    from testground_amd.engine import CABIEngine

    return fb.run_mesh(CABIEngine(oracle_lib, "tgo_", fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), False)


def test_mesh_parity(mesh_ref):
    dev = fb.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"]), True)
    fb.assert_same_run(dev, mesh_ref)
    s = dev["fb_summary"]
    assert s["failed_blackhole"] >= 10 and s["lost"] > 0 and s["cloned"] > 0 and fb.identity_everywhere(dev)
    assert mesh_ref["model"].stale_after_fail > 0


def test_mesh_discard_deliveries(mesh_ref):
    dev = fb.run_mesh(Engine(fc.MESH["n"], lookahead_ns=fc.MESH["lookahead_ns"], flags=abi.OPT_DISCARD_DELIVERIES), True)
    fb.assert_same_run(dev, mesh_ref, windows=False)
    assert all(len(d) == 0 for _, d in dev["windows"])
    for (dv, _), (rv, _) in zip(dev["windows"], mesh_ref["windows"]):
        assert dv.tobytes() == rv.tobytes()


def test_mesh_window_length(make_oracle):
    kw = dict(lookahead_ns=fc.MESH["lookahead_ns"])
    dev = fb.run_mesh(Engine(fc.MESH["n"], **kw), True, window=2_000)
    fb.assert_same_run(dev, fb.run_mesh(make_oracle(fc.MESH["n"], **kw), False, window=2_000))
    assert dev["fb_summary"]["failed_blackhole"] >= 10


def test_queue_full_corner(make_oracle):
    dev = fb.run_qfull(Engine(fb.QFULL["n"], **fb.qfull_kw()), True)
    fb.assert_same_run(dev, fb.run_qfull(make_oracle(fb.QFULL["n"], **fb.qfull_kw()), False))
    assert dev["fb_summary"]["queue_full"] > 0 and fb.identity_everywhere(dev)


# -- 7. degenerate equivalence: fail_mask 0 against the same arming without fb, device against device ------------------------------
@pytest.mark.parametrize("rounds", [1, 3])
def test_degenerate_rounds(rounds):
    kw = dict(lookahead_ns=fc.ROUNDS["lookahead_ns"])

    def run(fbp):
        eng = Engine(2, **kw)
        fc.plain(eng, 2, fc.ROUNDS["latency_ns"])
        w, now = fc.ROUNDS_FLOW["window"], eng.stats()["now_tick"]
        flows = fc.table([(0, 1, w * rounds - (rounds == 1) * 3, now), (1, 0, w * rounds, now + 500)])
        n_windows = 2 * rounds + 2
        return fb.drive(eng, True, fc.ROUNDS_FLOW, None, None, fbp, flows, n_windows, fc.ROUNDS["window"],
                        probe_at=(0, 2, n_windows - 2))

    armed, plain = run(dict(fail_mask=0)), run(None)
    fb.assert_same_run(armed, plain, fb=False)
    assert (armed["fb_rows"]["scheduled"] == armed["rows"]["offered"]).all() and armed["summary"]["done"] == 2


def test_degenerate_mesh():
    kw = dict(lookahead_ns=fc.MESH["lookahead_ns"])
    armed = fb.run_mesh(Engine(fc.MESH["n"], **kw), True, fb=dict(fail_mask=0), cut=False)
    plain = fb.run_mesh(Engine(fc.MESH["n"], **kw), True, fb=None, cut=False)
    fb.assert_same_run(armed, plain, fb=False)
    assert fb.identity_everywhere(armed) and armed["fb_summary"]["lost"] > 0 and armed["fb_summary"]["refused"] == 0


# -- 8. fb == NULL through tgsim_flow_init_fb ----------------------------------------------------------------------------------------
class NullFb:
    """An Engine whose flow_init arms through tgsim_flow_init_fb with fb == NULL."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def flow_init(self, flows, seg_len, ack_len, window, rto_ticks, max_attempts, bin_ns=0, n_bins=0, cc=None, rto=None, fb=None):
        e = self._inner
        assert fb is None
        t = np.ascontiguousarray(flows, dtype=abi.FLOW_SPEC_DTYPE)
        p = abi.Flow(seg_len, ack_len, window, rto_ticks, max_attempts, n_bins, bin_ns)
        c = None if cc is None else C.byref(abi.FlowCC(cc["init_cwnd"], cc["init_ssthresh"], cc["dupthresh"], 0))
        r = None if rto is None else C.byref(abi.FlowRto(rto["min_rto_ticks"], rto["max_rto_ticks"], rto["backoff"], 0))
        e._check(e._fn("flow_init_fb")(e._h, C.byref(p), c, r, None, t.ctypes.data, len(t)), "flow_init_fb")
        e._n_flows, e.flow_cc_armed, e.flow_rto_armed, e.flow_fb_armed = len(t), cc is not None, rto is not None, False


def test_null_fb_is_flow_init_rto():
    kw = dict(lookahead_ns=rc.CONST["lookahead_ns"])
    eng = Engine(2, **kw)
    got = rc.run_const(NullFb(eng), True)
    rc.assert_same_run(got, rc.run_const(Engine(2, **kw), True))
    assert got["rto_rows"]["samples"][0] == rc.CONST["n_seg"]
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_rows)
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_report)
    eng2 = Engine(2, lookahead_ns=fc.ROUNDS["lookahead_ns"])
    plain = fc.run_rounds(NullFb(eng2), device=True, rounds=1)  # cc and rto NULL as well: tgsim_flow_init
    fc.assert_same_run(plain, fc.run_rounds(Engine(2, lookahead_ns=fc.ROUNDS["lookahead_ns"]), device=True, rounds=1))
    _raises(errno.EINVAL, NOT_ARMED, eng2.flow_fb_report)
    _raises(errno.EINVAL, "the RTT estimator is not armed", eng2.flow_rto_report)


# -- 9. arming, validation and readers ---------------------------------------------------------------------------------------------
def test_arming_and_validation():
    n = 8
    ok = dict(seg_len=500, ack_len=64, window=4, rto_ticks=20_000, max_attempts=4)
    t = wl.flow_table_mesh(n, 2, 6, seed=1)
    eng = Engine(n, lookahead_ns=5 * MS)
    fc.plain(eng, n, 5 * MS)
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_rows)
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_report)
    for ccp, rto in ((None, None), (dict(init_cwnd=2), None), (dict(init_cwnd=2), dict(min_rto_ticks=5_000, max_rto_ticks=100_000))):
        for bad in (1, 0x20, 0x1F):
            _raises(errno.EINVAL, f"fail_mask {bad:#x}", eng.flow_init, t, cc=ccp, rto=rto, fb=dict(fail_mask=bad), **ok)
    _raises(errno.EINVAL, "window 65", eng.flow_init, t, fb=dict(fail_mask=0), **dict(ok, window=65))  # tgsim_flow_init's own rules
    _raises(errno.EINVAL, "one engine for every peer", Engine(n, shard=(0, 4)).flow_init, t, fb=dict(fail_mask=0), **ok)
    assert not eng.flow_fb_armed
    eng.flow_init(t, fb=dict(fail_mask=abi.FLOW_FB_REFUSALS), **ok)
    assert eng.flow_fb_armed and not eng.flow_cc_armed and not eng.flow_rto_armed
    _raises(errno.EINVAL, "congestion control is not armed", eng.flow_cc_rows)
    rows = eng.flow_fb_rows()
    assert len(rows) == 2 * n and rows.tobytes() == bytes(32 * 2 * n)  # fresh rows: all zero
    assert eng.flow_fb_report() == dict.fromkeys(abi.FLOW_FB_SUMMARY_FIELDS, 0)
    wl.flow_run(eng, 8, 5_000)
    rep, frep = eng.flow_report(), eng.flow_fb_report()
    assert rep["done"] == rep["flows"] == 2 * n and frep["scheduled"] == rep["data_offered"] == 12 * n
    assert frep == dict(dict.fromkeys(abi.FLOW_FB_SUMMARY_FIELDS, 0), scheduled=12 * n)
    assert len(eng.flow_fb_rows(3, 5)) == 5 and (eng.flow_fb_rows(3, 5)["scheduled"] == 6).all()
    assert len(eng.flow_fb_rows(2 * n, 0)) == 0
    _raises(errno.EINVAL, "outside", eng.flow_fb_rows, 10, 7)
    _raises(errno.EINVAL, "outside", eng.flow_fb_rows, 2 * n + 1, 0)
    out = np.zeros(2, dtype=abi.FLOW_FB_ROW_DTYPE)
    assert eng._fn("flow_fb_rows")(eng._h, 0, 3, out.ctypes.data, 2) == -errno.ENOSPC  # cap below n
    assert eng._fn("flow_fb_rows")(eng._h, 0, 3, None, 3) == -errno.EINVAL
    assert eng._fn("flow_fb_report")(eng._h, None) == -errno.EINVAL
    # armed without fb: the flow reports answer, the fb readers do not; disarmed: none does
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, cc=dict(init_cwnd=2), **ok)
    assert not eng.flow_fb_armed and eng.flow_report()["segs_acked"] == 0
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_rows)
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_report)
    wl.flow_run(eng, 8, 5_000)
    assert eng.flow_report()["done"] == 2 * n
    t["start_tick"] = eng.stats()["now_tick"]
    eng.flow_init(t, cc=dict(init_cwnd=2), rto=dict(min_rto_ticks=5_000, max_rto_ticks=100_000), fb=dict(fail_mask=0), **ok)  # all three
    assert eng.flow_fb_armed and eng.flow_rto_armed and eng.flow_cc_armed and eng.flow_fb_rows().tobytes() == bytes(32 * 2 * n)
    eng.flow_init(None)
    assert not eng.flow_fb_armed
    _raises(errno.EINVAL, "not armed", eng.flow_rows)
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_rows)
    _raises(errno.EINVAL, NOT_ARMED, eng.flow_fb_report)


def test_late_receipt_keeps_fb_rows():
    n, win = fc.LATE["n"], fc.LATE["window"]
    eng = Engine(n, lookahead_ns=fc.LATE["lookahead_ns"])
    fc.configure_late(eng, reorder=50.0)
    eng.flow_init(fc.late_flows(0), fb=dict(fail_mask=abi.FLOW_FB_REFUSALS), **fc.LATE_FLOW)
    eng.gen_flow(win)
    eng.step(win)
    rows, frows = eng.flow_rows(), eng.flow_fb_rows()
    assert (frows["scheduled"] == rows["offered"]).all() and frows["scheduled"].sum() == 8 * n
    for _ in range(2):  # sticky
        _raises(errno.EINVAL, "flow: a receipt due at tick", eng.gen_flow, win)
    rep, frep = eng.flow_report(), eng.flow_fb_report()  # still readable
    assert rep["flows"] == n and frep["scheduled"] == rep["data_offered"] == 8 * n
    assert eng.flow_rows().tobytes() == rows.tobytes() and eng.flow_fb_rows().tobytes() == frows.tobytes()


def test_struct_sizes():
    assert C.sizeof(abi.FlowFb) == 16 and abi.FLOW_FB_ROW_DTYPE.itemsize == 32 and C.sizeof(abi.FlowFbSummary) == 96
