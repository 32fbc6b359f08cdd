"""The ping mesh loop of include/tgsim.h, driven from the host (workloads.ping_reference) over the CPU
oracle, against the reference's known answers about a shaped network.  None of these depends on the
model's own arithmetic: the round-trip windows of plans/network/pingpong.go:185, :195, the loss rates
of plans/verify/main.go:101-107 and the reachability matrix of plans/splitbrain/main.go:50-58."""
import numpy as np
import pytest

import ping_cases as pc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

MS = nw.Millisecond


def test_targets():
    t = wl.ping_targets_all(5)
    assert t.shape == (5, 4) and all(sorted(t[s]) == [p for p in range(5) if p != s] for s in range(5))
    m = wl.ping_targets_mesh(50, 7, seed=3)
    assert m.shape == (50, 7) and (m != np.arange(50)[:, None]).all() and m.max() < 50
    assert all(len(set(row)) == 7 for row in m.tolist())
    assert (m == wl.ping_targets_mesh(50, 7, seed=3)).all()


def test_pingpong_rtt_windows(make_oracle):
    """pingpong.go:185: every RTT in [200, 215] ms at 100 ms; :195: in [20, 35] ms after the reshape."""
    e = make_oracle(pc.PINGPONG["n"], lookahead_ns=pc.PINGPONG["lookahead_ns"])
    slow, fast = pc.run_pingpong(e, device=False)
    for res, lo, hi in ((slow, 200 * MS, 215 * MS), (fast, 20 * MS, 35 * MS)):
        p, s = res["pairs"], res["summary"]
        assert (p["sent"] == 3).all() and (p["received"] == 3).all()
        assert (p["min_ns"] >= lo).all() and (p["max_ns"] <= hi).all(), (p["min_ns"], p["max_ns"])
        assert s["pairs"] == 2 and s["received"] == 6 and s["pairs_all"] == 2 and s["pending_replies"] == 0
        assert lo <= s["min_ns"] <= s["max_ns"] <= hi and s["hist"].sum() == 6
    # the first probe: before any reply (the request is still in flight)
    assert slow["probes"][0][1]["received"] == 0 and slow["probes"][0][1]["sent"] == 2


@pytest.mark.parametrize("allow_all", [False, True])
def test_verify_loss(make_oracle, allow_all):
    """verify/main.go:101-107: 0 % loss on the data network, 100 % towards addresses outside it,
    whatever the routing policy (with AllowAll the packet leaves the data network)."""
    e = make_oracle(pc.VERIFY["n"], lookahead_ns=pc.VERIFY["lookahead_ns"])
    res = pc.run_verify(e, device=False, allow_all=allow_all)
    p, s = res["pairs"], res["summary"]
    assert (p["sent"] == 3).all()
    assert (p["received"][:, 0] == 3).all() and (p["received"][:, 1] == 0).all()
    assert s["pairs"] == 8 and s["pairs_all"] == 4 and s["pairs_none"] == 4
    want = abi.V_EXTERNAL if allow_all else abi.V_NO_ROUTE
    v0 = res["windows"][0][0] & 15  # rows are (tick, seq): slot 0 then slot 1 of every probe
    assert (v0[0::2] == abi.V_SCHEDULED).all() and (v0[1::2] == want).all()


@pytest.mark.parametrize("case", ["drop", "reject", "accept"])
def test_splitbrain_matrix(make_oracle, case):
    """splitbrain/main.go:50-58: who can reach whom."""
    n = pc.SPLIT["n"]
    e = make_oracle(n, lookahead_ns=pc.SPLIT["lookahead_ns"])
    res = pc.run_splitbrain(e, device=False, case=case)
    exp = wl.splitbrain_expected(n, case)
    assert (pc.splitbrain_reached(res["pairs"], n) == exp).all()
    assert res["model"].ties == 0
    assert res["summary"]["pairs_none"] == (~exp).sum() - n  # (the diagonal is no pair)


def test_mesh_conditions(make_oracle):
    """The lossy mesh of tests/test_gpu_ping.py exercises what it is there for, shown by the model alone."""
    e = make_oracle(pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"])
    res = pc.run_mesh(e, device=False)
    m, s = res["model"], res["summary"]
    assert s["pending_replies"] == 0 and s["sent"] == s["pairs"] * pc.MESH_PING["count"]  # quiescent
    assert s["received"] < s["sent"]                    # a lost probe
    assert m.dup_requests > 0 and m.dup_replies > 0     # a clone ignored on each leg
    assert s["corrupt_ignored"] > 0                     # a corrupted copy ignored
    assert m.carried_max >= 2                           # a calendar entry carried over two or more windows
    assert m.max_row > 64                               # one source's row longer than 64 packets
    assert m.ties > 0 and 0 in m.tie_sources            # equal (tick, seq), different dst
    assert pc.mesh_tie_sources_have_jitter(m)           # ... only where the responder's jitter orders them
    assert 0 < res["probes"][4][1]["pending_replies"]   # mid-run, a non-empty calendar
    assert res["probes"][0][1]["received"] == 0         # before the first reply


def test_late_receipt_is_detected(make_oracle):
    """A peer that reorders (sends without delay) answers inside the window: the model refuses."""
    e = make_oracle(pc.LATE["n"], lookahead_ns=pc.LATE["lookahead_ns"])
    pc.configure_late(e, reorder=50.0)
    ping = dict(count=8, interval_ticks=500, length=64, start_tick=0)
    with pytest.raises(wl.PingLate, match="precedes the window"):
        wl.ping_reference(e, ping, wl.ping_targets_all(pc.LATE["n"]), 4, pc.LATE["window"])


def test_ping_lines():
    from testground_amd.metrics import ping_lines
    rep = dict.fromkeys(abi.PING_SUMMARY_FIELDS, 0)
    rep.update(pairs=2, sent=6, received=5, min_ns=7, max_ns=9, hist=np.array([0, 5, 0], dtype=np.uint64))
    out = ping_lines(rep, 1000, "plan", "run", 42)
    assert "results.plan.ping.received,run=run value=5i 42" in out
    assert "results.plan.ping.rtt_hist,run=run,bin=1000 value=5i 42" in out and len(out) == 12
