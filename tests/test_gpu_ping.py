"""The HIP engine's device ping loop (tgsim_ping_init / tgsim_gen_ping / tgsim_ping_report /
tgsim_ping_pairs) against the same loop driven from the host over the CPU oracle
(workloads.ping_reference), bit for bit: the verdict bytes and drained records of every window, and
the pair table, summary and RTT histogram at three or more points of each run (before the first
reply, mid-run with replies waiting in the calendar, and at the end)."""
import errno

import numpy as np
import pytest

import ping_cases as pc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl
from testground_amd.engine import CABIEngine, Engine, EngineError

pytestmark = pytest.mark.gpu
MS = nw.Millisecond


@pytest.fixture(scope="module")
def mesh_ref(oracle_lib):
    """The lossy mesh's host model over the oracle, once for the tests that compare with it."""
    return pc.run_mesh(CABIEngine(oracle_lib, "tgo_", pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"]), device=False)


# -- A. the known-answer cases ------------------------------------------------------------------------
def test_pingpong(make_oracle):
    kw = dict(lookahead_ns=pc.PINGPONG["lookahead_ns"])
    dev = pc.run_pingpong(Engine(2, **kw), device=True)
    ref = pc.run_pingpong(make_oracle(2, **kw), device=False)
    for d, r, lo, hi in zip(dev, ref, (200 * MS, 20 * MS), (215 * MS, 35 * MS)):
        pc.assert_same_run(d, r)
        assert (d["pairs"]["received"] == 3).all()
        assert (d["pairs"]["min_ns"] >= lo).all() and (d["pairs"]["max_ns"] <= hi).all()


@pytest.mark.parametrize("allow_all", [False, True])
def test_verify(make_oracle, allow_all):
    kw = dict(lookahead_ns=pc.VERIFY["lookahead_ns"])
    dev = pc.run_verify(Engine(pc.VERIFY["n"], **kw), device=True, allow_all=allow_all)
    pc.assert_same_run(dev, pc.run_verify(make_oracle(pc.VERIFY["n"], **kw), device=False, allow_all=allow_all))
    assert dev["summary"]["pairs_all"] == 4 and dev["summary"]["pairs_none"] == 4
    assert (dev["pairs"]["received"][:, 1] == 0).all() and (dev["pairs"]["received"][:, 0] == 3).all()


@pytest.mark.parametrize("case", ["drop", "reject", "accept"])
def test_splitbrain(make_oracle, case):
    n, kw = pc.SPLIT["n"], dict(lookahead_ns=pc.SPLIT["lookahead_ns"])
    dev = pc.run_splitbrain(Engine(n, **kw), device=True, case=case)
    pc.assert_same_run(dev, pc.run_splitbrain(make_oracle(n, **kw), device=False, case=case))
    assert (pc.splitbrain_reached(dev["pairs"], n) == wl.splitbrain_expected(n, case)).all()


# -- B. lossy mesh with a hot responder (its conditions: tests/test_ping_model.py) ------------------------
def test_mesh_parity(mesh_ref):
    dev = pc.run_mesh(Engine(pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"]), device=True)
    pc.assert_same_run(dev, mesh_ref)
    assert mesh_ref["model"].max_row > 64 and mesh_ref["model"].ties > 0 and mesh_ref["model"].carried_max >= 2


# -- C. nothing reaches the host / the metrics fold beside it: identical reports -------------------------
@pytest.mark.parametrize("flags", [abi.OPT_DISCARD_DELIVERIES, abi.OPT_METRICS])
def test_mesh_reports_with_flags(mesh_ref, flags):
    eng = Engine(pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"], flags=flags)
    dev = pc.run_mesh(eng, device=True)
    pc.assert_same_run(dev, mesh_ref, windows=flags == abi.OPT_METRICS)
    if flags == abi.OPT_DISCARD_DELIVERIES:
        assert all(len(d) == 0 for _, d in dev["windows"])
        for (dv, _), (rv, _) in zip(dev["windows"], mesh_ref["windows"]):
            assert dv.tobytes() == rv.tobytes()


# -- D. the result does not depend on the step length --------------------------------------------------
def test_mesh_window_length(mesh_ref):
    dev = pc.run_mesh(Engine(pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"]), device=True, window=2_000, probe_at=())
    for key in abi.PING_PAIR_DTYPE.names:
        assert (dev["pairs"][key] == mesh_ref["pairs"][key]).all(), key
    assert (dev["summary"]["hist"] == mesh_ref["summary"]["hist"]).all()
    assert dev["summary"]["pending_replies"] == 0


# -- E. late receipt --------------------------------------------------------------------------------------
def test_late_receipt():
    n, win = pc.LATE["n"], pc.LATE["window"]
    eng = Engine(n, lookahead_ns=pc.LATE["lookahead_ns"])
    pc.configure_late(eng, reorder=50.0)
    eng.ping_init(wl.ping_targets_all(n), count=8, interval_ticks=500, length=64, start_tick=0, bin_ns=MS, n_bins=8)
    eng.gen_ping(win)
    eng.step(win)
    for _ in range(2):  # sticky
        with pytest.raises(EngineError, match="ping: a reply due at tick") as ei:
            eng.gen_ping(win)
        assert ei.value.code == -errno.EINVAL
    rep = eng.ping_report()  # still readable
    assert rep["pairs"] == n * (n - 1) and rep["sent"] == rep["pairs"] * 8 and rep["pending_replies"] > 0
    assert eng.ping_pairs().shape == (n, n - 1)
    for _ in range(4):  # empty windows: what is in flight drains
        eng.step(win)
    pc.configure_late(eng, reorder=0.0)
    eng.ping_init(wl.ping_targets_all(n), count=2, interval_ticks=500, length=64, bin_ns=MS, n_bins=8)
    wl.ping_run(eng, 4, win)
    rep = eng.ping_report()
    assert rep["received"] == rep["sent"] == rep["pairs"] * 2 and rep["pairs_all"] == rep["pairs"]


# -- F. arming rules --------------------------------------------------------------------------------------
def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


def test_arming_rules(make_oracle):
    n = 8
    t = wl.ping_targets_mesh(n, 2, seed=1)
    ok = dict(count=2, interval_ticks=100, length=64, start_tick=0)
    _raises(errno.EINVAL, "one engine for every peer", Engine(n, shard=(0, 4)).ping_init, t, **ok)
    _raises(errno.ENOSYS, "tgo_ping_init is not exported", make_oracle(n).ping_init, t, **ok)
    eng = Engine(n, lookahead_ns=5 * MS)
    for i in range(n):
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=5 * MS)))
    _raises(errno.EINVAL, "not armed", eng.ping_report)
    _raises(errno.EINVAL, "not armed", eng.gen_ping, 100)
    for bad, match in ((dict(count=0), "count 0"), (dict(count=65536), "count 65536"), (dict(interval_ticks=0), "interval"),
                       (dict(length=0), "len 0"), (dict(length=65536), "len 65536"), (dict(n_bins=257, bin_ns=1), "n_bins 257"),
                       (dict(n_bins=4, bin_ns=0), "bin_ns 0")):
        _raises(errno.EINVAL, match, eng.ping_init, t, **dict(ok, **bad))
    _raises(errno.EINVAL, "fanout 65", eng.ping_init, np.full((n, 65), abi.PING_NONE, dtype=np.uint32), **ok)
    self_t, far_t = t.copy(), t.copy()
    self_t[2, 1], far_t[3, 0] = 2, n
    _raises(errno.EINVAL, r"targets\[2\]\[1\] = 2 is the peer itself", eng.ping_init, self_t, **ok)
    _raises(errno.EINVAL, r"targets\[3\]\[0\] = 8 is out of range", eng.ping_init, far_t, **ok)
    pkt = np.array([(0, 1, 0, 64, 0)], dtype=abi.PKT_DTYPE)
    eng.submit(pkt)
    _raises(errno.EBUSY, "host packets", eng.ping_init, t, **ok)
    eng.step(10)
    eng.gen_storm(0.01, 10)
    _raises(errno.EBUSY, "generated windows", eng.ping_init, t, **ok)
    eng.step(10)
    _raises(errno.EINVAL, "in the past", eng.ping_init, t, **ok)
    eng.step(10_000)  # (nothing of the earlier traffic is left in flight)
    eng.drain()
    # armed: the other sources of traffic and the sharded steps refuse; step_n runs window by window
    eng.ping_init(t, **dict(ok, start_tick=None))
    _raises(errno.EBUSY, "ping driver is armed", eng.submit, pkt)
    _raises(errno.EBUSY, "ping driver is armed", eng.gen_storm, 0.01, 10)
    _raises(errno.EBUSY, "ping driver is armed", eng.gossip_init, n_floods=1, degree=2)
    _raises(errno.EBUSY, "ping driver is armed", eng.step_sim, 10, [0, n], 0, 0)
    eng.gen_ping(5_000)
    _raises(errno.EBUSY, "one window at a time", eng.gen_ping, 5_000)
    eng.step_n(5_000, 1)
    wl.ping_run(eng, 3, 5_000)
    rep = eng.ping_report()
    assert rep["received"] == rep["sent"] == 2 * 2 * n and rep["pending_replies"] == 0
    # disarm: the host's traffic is back, the reports are gone; re-arm
    eng.ping_init(None)
    _raises(errno.EINVAL, "not armed", eng.ping_pairs)
    eng.submit(pkt)
    eng.step(10)
    eng.ping_init(t, **dict(ok, start_tick=None))
    assert eng.ping_report()["received"] == 0
    # gossip armed: no ping
    g = Engine(n, lookahead_ns=5 * MS)
    g.gossip_init(n_floods=1, degree=2)
    _raises(errno.EBUSY, "gossip driver is armed", g.ping_init, t, **ok)


# -- G. a responder disconnected between two windows --------------------------------------------------------
def test_responder_disconnected(make_oracle):
    def run(eng, device):
        def before(w):
            if w == 2:
                eng.configure(0, nw.Config(Network="default", Enable=False))
        return pc.run_mesh(eng, device, ticks=60_000, probe_at=(1, 3), before=before)

    kw = dict(lookahead_ns=pc.MESH["lookahead_ns"])
    ref = run(make_oracle(pc.MESH["n"], **kw), False)
    pc.assert_same_run(run(Engine(pc.MESH["n"], **kw), True), ref)
    assert ref["probes"][1][1]["pending_replies"] > 0
    # peer 0's row comes first, and in it the replies to the probes of tick 3,000, due from tick 8,001
    # on, ahead of its own probes of tick 9,000
    v2 = ref["windows"][2][0] & 15
    assert (v2[:4] == abi.V_DISCONNECTED).all()


# -- H. size: 100,000 peers against the closed form ---------------------------------------------------------
def test_size_closed_form():
    """No host model: received == sent, every pair complete, every RTT == 2 L + tick_ns, one histogram
    bin.  The probes are 4 bytes long: HTB at the rate an unlimited link gets (2^32 - 1 bytes/s) charges
    whole nanoseconds, 0 for a packet under 5 bytes, so the eight probes a peer offers in one tick and
    the replies a responder offers in one tick leave at the same instant.  Longer packets add their
    serialization (15 ns per 64 bytes) to the round trips: 2 L + tick_ns would then be the minimum only."""
    n, lat, win = 100_000, 5 * MS, 5_000
    eng = Engine(n, lookahead_ns=lat, flags=abi.OPT_DISCARD_DELIVERIES)
    eng.configure_batch(np.arange(n), nw.configs_array(np.full(n, lat)))
    eng.ping_init(wl.ping_targets_mesh(n, 8, seed=9), count=2, interval_ticks=1_000, length=4, start_tick=0,
                  bin_ns=MS, n_bins=32)
    wl.ping_run(eng, 4, win)
    rep, rtt = eng.ping_report(), 2 * lat + eng.tick_ns
    assert rep["pairs"] == 8 * n and rep["sent"] == rep["received"] == 16 * n
    assert rep["pairs_all"] == rep["pairs"] and rep["pairs_none"] == 0 and rep["pending_replies"] == 0
    assert rep["min_ns"] == rep["max_ns"] == rtt and rep["sum_ns"] == 16 * n * rtt
    assert rep["hist"][rtt // MS] == 16 * n and rep["hist"].sum() == 16 * n
    rows = eng.ping_pairs(n - 1000, 1000)
    assert (rows["sent"] == 2).all() and (rows["received"] == 2).all()
    assert (rows["min_ns"] == rtt).all() and (rows["max_ns"] == rtt).all() and (rows["sum_ns"] == 2 * rtt).all()
