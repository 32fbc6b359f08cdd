"""GPU parity away from t = 0 (tests/late_clock_cases.py): the HIP engine against the CPU oracle, bit
for bit (verdict bytes, the drain in order, the statistics), with the clock at the places where the
kernels' time arithmetic could truncate -- t_ns across 2^32, ticks across 2^31 and 2^32, just below
the 2^46-ns time field -- across that field's end, where the engine must fail with -EOVERFLOW and
never hand out a record, and with tick lengths other than 1000 ns.  The oracle side of every
scenario is pinned in tests/test_late_clock_model.py."""
import errno

import numpy as np
import pytest

import flow_cases as fc
import group_cases as gc
import late_clock_cases as lc
import ping_cases as pc
from testground_amd import abi
from testground_amd import workloads as wl
from testground_amd.engine import Engine, EngineError

from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None


def _fused(e):
    return int(e._fn("debug_fused_windows")(e._h))


def both(make_oracle, n, **kw):
    return Engine(n, **kw), make_oracle(n, **kw)


def edge_pair(make_oracle, start, tick_ns=1000, **kw):
    g, c = both(make_oracle, lc.EDGE["n"], **lc.edge_kwargs(tick_ns), **kw)
    for e in (g, c):
        lc.configure_edge(e)
        lc.advance(e, start)
    return g, c


def run_same(g, c, plan, what):
    """The plan on both engines, every window compared; returns the engine's drains."""
    out = []
    for w, (pk, ticks) in enumerate(plan):
        for e in (g, c):
            if pk is not None:
                e.submit(pk)
            e.step(ticks)
        out.append(assert_same(g, c, f"{what} window {w}")[1])
    return out


# -- late clocks -------------------------------------------------------------------------------------------
_gpu_base = {}


def gpu_base_drains(mode):
    """The engine's own edge run at BASE (per TGSIM_SPARSE mode, which the caller has set), once."""
    if mode not in _gpu_base:
        g = Engine(lc.EDGE["n"], **lc.edge_kwargs())
        lc.configure_edge(g)
        lc.advance(g, lc.POS["BASE"])
        _gpu_base[mode] = [d for _, d in lc.run_plan(g, lc.edge_plan())]
    return _gpu_base[mode]


@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("name", ["BASE", "NS32", "T31", "T32", "NEAR"])
def test_edge_at_late_clocks(make_oracle, monkeypatch, name, mode):
    """The edge scenario through the dense k_sim (TGSIM_SPARSE=0) and through k_sim_sparse + k_sim_list
    (=1) with the windows across t_ns = 2^32, tick 2^31, tick 2^32, and 3 s below 2^46 ns, where no
    call may fail and the flushing step empties every queue."""
    monkeypatch.setenv("TGSIM_SPARSE", mode)
    start = lc.POS[name]
    g, c = edge_pair(make_oracle, start)
    drains = run_same(g, c, lc.edge_plan(lc.EDGE_FLUSH if name == "NEAR" else 0), f"edge at {name}, sparse {mode}")
    if name == "NEAR":
        assert g.pending() == 0 and len(drains[3]) > 0
        assert max(int(d["t_ns"].max()) for d in drains) < lc.NS_LIMIT
    # not through the oracle: the engine's run is its own BASE run, shifted
    off = (start - lc.POS["BASE"]) * 1000
    for w, bd in enumerate(gpu_base_drains(mode)):
        assert lc.shifted(drains[w], off).tobytes() == bd.tobytes(), f"window {w} against the engine's BASE run"


@pytest.mark.parametrize("name", ["T32", "STORM_NEAR"])
def test_storm_at_late_clocks(make_oracle, name):
    """The device generator with the 32-bit wrap of its Philox tick counter inside a window (T32), and
    20 s below 2^46 ns; three windows through tgsim_step, eight through tgsim_step_n (fused)."""
    n = lc.STORM["n"]
    g, c = both(make_oracle, n)
    for e in (g, c):
        wl.configure_storm(e, n)
        lc.advance(e, lc.STORM_POS[name])
    for w in range(lc.STORM["windows"]):
        for e in (g, c):
            lc.storm_step(e)
        v, _ = assert_same(g, c, f"storm at {name}, window {w}")
        assert len(v) > 100_000
    for e in (g, c):
        lc.storm_step_n(e)
    assert_same(g, c, f"storm at {name}, step_n")
    assert _fused(g) > 0
    if name == "T32":
        assert g.stats()["now_tick"] > 1 << 32


def test_edge_at_t32_with_groups_and_metrics(make_oracle):
    """The per-group matrix against the host model folded over the oracle, and the metrics tables
    against the oracle's, with the windows across tick 2^32."""
    n, ng = lc.EDGE["n"], 5
    group_of = (np.arange(n) * 7 % ng).astype(np.uint16)
    g, c = edge_pair(make_oracle, lc.POS["T32"], flags=abi.OPT_METRICS)
    g.groups_init(group_of, ng)
    plan = lc.edge_plan()
    model = gc.model_series(c, group_of, ng, plan)
    for w, (d, m) in enumerate(zip(gc.device_series(g, plan), model)):
        gc.assert_same(d, m, f"after window {w}")
    assert g.stats() == c.stats()
    mg, mc = g.metrics(), c.metrics()
    for k in ("src", "dst", "hist"):
        assert (mg[k] == mc[k]).all(), k


# -- the overflow guard --------------------------------------------------------------------------------
def host_driver(pk, ticks):
    return lambda e: lc.run_window(e, pk, ticks)


def guard_run(g, c, drivers, what):
    """Window by window (a driver runs one window on an engine and returns its verdicts and drain):
    the engine's window equals the oracle's, or a call fails with -EOVERFLOW, no later than the reader
    of the first window in which the oracle's drain holds a t_ns >= 2^46; no drain returns such a
    record; after the failure every step and reader keeps failing.  Returns (the window that raised or
    None, the oracle's first window past the limit or None)."""
    first = raised = None
    for w, drive in enumerate(drivers):
        cv, cd = drive(c)
        if first is None and len(cd) and int(cd["t_ns"].max()) >= lc.NS_LIMIT:
            first = w
        try:
            gv, gd = drive(g)
            gs = g.stats()
        except EngineError as err:
            assert err.code == -errno.EOVERFLOW, (what, w, err)
            raised = w
            break
        assert not len(gd) or int(gd["t_ns"].max()) < lc.NS_LIMIT, f"{what}: window {w} drained a time past 2^46 ns"
        assert first is None, f"{what}: window {w} passed although the oracle's times pass 2^46 ns"
        assert gv.tobytes() == cv.tobytes(), f"{what}: verdicts of window {w}"
        assert gd.tobytes() == cd.tobytes(), f"{what}: deliveries of window {w}"
        assert gs == c.stats(), f"{what}: statistics after window {w}"
    if raised is not None:
        for call in (lambda: g.step(100), g.drain, g.verdicts, g.stats, lambda: g.step(100), g.drain):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == -errno.EOVERFLOW, what
    return raised, first


@pytest.mark.parametrize("mode", ["0", "1"])
def test_eligibility_times_cross_the_limit(make_oracle, monkeypatch, mode):
    """10 ms below 2^46 ns the 20-ms links enqueue items beyond it in the first window."""
    monkeypatch.setenv("TGSIM_SPARSE", mode)
    g, c = edge_pair(make_oracle, lc.POS["CROSS_E"])
    raised, first = guard_run(g, c, [host_driver(pk, t) for pk, t in lc.edge_plan()], f"CROSS_E sparse {mode}")
    assert (raised, first) == (0, 0)


@pytest.mark.parametrize("mode", ["0", "1"])
def test_departure_times_cross_the_limit(make_oracle, monkeypatch, mode):
    """1 s below 2^46 ns every packet is eligible when offered (zero latency) and a slow link's backlog
    carries the departures across: the first burst's window matches the oracle, the second's fails."""
    monkeypatch.setenv("TGSIM_SPARSE", mode)
    g, c = both(make_oracle, lc.BACKLOG["n"], **lc.backlog_kwargs())
    for e in (g, c):
        lc.configure_backlog(e)
        lc.advance(e, lc.POS["CROSS_D"])
    raised, first = guard_run(g, c, [host_driver(pk, t) for pk, t in lc.backlog_plan()], f"CROSS_D sparse {mode}")
    assert (raised, first) == (1, 1)


def test_storm_crosses_the_limit(make_oracle):
    """The storm 3 s below 2^46 ns: its slow links' departures cross (tests/test_late_clock_model.py)."""
    n = lc.STORM["n"]
    g, c = both(make_oracle, n)
    for e in (g, c):
        wl.configure_storm(e, n)
        lc.advance(e, lc.STORM_POS["NEAR"])

    def one(e):
        lc.storm_step(e)
        return e.verdicts(), e.drain()

    def fused(e):
        lc.storm_step_n(e)
        return e.verdicts(), e.drain()

    raised, first = guard_run(g, c, [one] * lc.STORM["windows"] + [fused], "storm at NEAR")
    assert first is not None and raised is not None and raised <= first


def _refused(fn, *a):
    with pytest.raises(EngineError) as ei:
        fn(*a)
    return ei.value


def test_ping_stops_at_tick_2_31(make_oracle):
    """A window that ends at tick 2^31 is refused by the engine and by the model alike and changes
    nothing; the window one tick shorter runs and matches."""
    n, kw = pc.VERIFY["n"], dict(lookahead_ns=pc.VERIFY["lookahead_ns"])
    g, c = both(make_oracle, n, **kw)
    for e in (g, c):
        fc.plain(e, n, 5 * pc.MS)
        lc.advance(e, lc.POS["T31"])
    ping, targets = lc.ping_at_t31(g), pc.verify_targets()
    g.ping_init(targets, **ping)
    m = wl.PingModel(c, ping, targets)
    for err in (_refused(g.gen_ping, 3000), _refused(m.step, 3000)):
        assert err.code == -errno.EOVERFLOW and "ping: the window ends beyond tick 2^31" in str(err)
    g.gen_ping(2999)
    g.step(2999)
    v, d = m.step(2999)
    assert g.verdicts().tobytes() == v.tobytes() and len(v) == 2 * n
    assert g.drain().tobytes() == d.tobytes()
    pc.assert_same_report((g.ping_pairs(), g.ping_report()), (m.pairs(), m.report()))


def test_flow_stops_at_tick_2_31(make_oracle):
    n, kw = fc.CUT["n"], dict(lookahead_ns=fc.CUT["lookahead_ns"])
    g, c = both(make_oracle, n, **kw)
    for e in (g, c):
        fc.plain(e, n, fc.CUT["latency_ns"])
        lc.advance(e, lc.POS["T31"])
    flows = fc.cut_flows(lc.POS["T31"])
    g.flow_init(flows, **fc.CUT_FLOW)
    m = wl.FlowModel(c, fc.CUT_FLOW, flows)
    for err in (_refused(g.gen_flow, 3000), _refused(m.step, 3000)):
        assert err.code == -errno.EOVERFLOW and "flow: the window ends beyond tick 2^31" in str(err)
    g.gen_flow(2999)
    g.step(2999)
    v, d = m.step(2999)
    assert g.verdicts().tobytes() == v.tobytes() and len(v) > 0
    assert g.drain().tobytes() == d.tobytes()
    fc.assert_same_report((g.flow_rows(), g.flow_report()), (m.rows(), m.report()))


def test_ping_mesh_ends_below_tick_2_31(make_oracle):
    """The 9-peer full mesh (splitbrain, accept) started so that its last window ends at T31."""
    n, kw = pc.SPLIT["n"], dict(lookahead_ns=pc.SPLIT["lookahead_ns"])
    g, c = both(make_oracle, n, **kw)
    for e in (g, c):
        lc.advance(e, lc.POS["T31"] - 5 * pc.SPLIT["window"])
    dev = pc.run_splitbrain(g, device=True, case="accept")
    pc.assert_same_run(dev, pc.run_splitbrain(c, device=False, case="accept"))
    assert g.stats()["now_tick"] == lc.POS["T31"] and dev["summary"]["received"] > 0


def test_flow_mesh_ends_below_tick_2_31(make_oracle):
    n, kw = fc.CUT["n"], dict(lookahead_ns=fc.CUT["lookahead_ns"])
    g, c = both(make_oracle, n, **kw)
    for e in (g, c):
        lc.advance(e, lc.POS["T31"] - fc.CUT["ticks"])
    dev = fc.run_cut(g, device=True)
    fc.assert_same_run(dev, fc.run_cut(c, device=False))
    assert g.stats()["now_tick"] == lc.POS["T31"]
    assert dev["rows"]["state"].tolist() == [abi.FLOW_FAILED, abi.FLOW_DONE, abi.FLOW_DONE, abi.FLOW_DONE]


# -- tick lengths ------------------------------------------------------------------------------------------
TICKS = [100, 768, 3000, 10**6]


@pytest.mark.parametrize("tick_ns", TICKS)
def test_edge_at_other_tick_lengths(make_oracle, tick_ns):
    g, c = edge_pair(make_oracle, lc.POS["BASE"], tick_ns=tick_ns)
    run_same(g, c, lc.edge_plan(), f"edge at {tick_ns}-ns ticks")
    assert g.stats()["scheduled"] > 10_000


@pytest.mark.parametrize("tick_ns", TICKS)
def test_storm_at_other_tick_lengths(make_oracle, tick_ns):
    n = lc.STORM["n"]
    g, c = both(make_oracle, n, tick_ns=tick_ns)
    for e in (g, c):
        wl.configure_storm(e, n)
        lc.advance(e, lc.POS["BASE"])
    for w in range(lc.STORM["windows"]):
        for e in (g, c):
            lc.storm_step(e)
        assert_same(g, c, f"storm at {tick_ns}-ns ticks, window {w}")
    for e in (g, c):
        lc.storm_step_n(e)
    assert_same(g, c, f"storm at {tick_ns}-ns ticks, step_n")
    assert _fused(g) > 0


def gossip_same(make_oracle, tick_ns, start):
    n = lc.GOSSIP["n"]
    g, c = both(make_oracle, n, lookahead_ns=wl.GOSSIP_MIN_LAT, tick_ns=tick_ns)
    w = wl.gossip_window_ticks(g)
    start = start(w)
    for e in (g, c):
        lc.advance(e, start)
        lc.gossip_arm(e, start)
    total = 0
    for k in range(lc.GOSSIP["windows"]):
        for e in (g, c):
            e.gen_gossip(w)
            e.step(w)
        total += len(assert_same(g, c, f"gossip at {tick_ns}-ns ticks, window {k}")[0])
    rg, rc = g.gossip_reached(), c.gossip_reached()
    assert (rg == rc).all() and (rg > 0.9 * n).all() and total > 0
    return g


@pytest.mark.parametrize("tick_ns", [768, 3000])
def test_gossip_at_tick_lengths_that_divide_no_latency(make_oracle, tick_ns):
    """The receipt's tick is floor(d / tick_ns) + 1 with latencies in whole microseconds: neither tick
    length divides them."""
    gossip_same(make_oracle, tick_ns, lambda w: lc.POS["BASE"])


def test_gossip_ends_below_tick_2_32(make_oracle):
    g = gossip_same(make_oracle, 1000, lambda w: lc.POS["T32"] - 40 * w)
    assert (1 << 32) - 60_000 < g.stats()["now_tick"] < 0xFFFFFFFE


def test_gossip_refuses_ticks_beyond_32_bits():
    """The oracle's guard (tests/test_late_clock_model.py), on the engine."""
    n = 50
    g = Engine(n, lookahead_ns=wl.GOSSIP_MIN_LAT)
    wl.configure_gossip(g, n)
    w, last = wl.gossip_window_ticks(g), 0xFFFFFFFE
    lc.advance(g, last - 3 * w)
    now = g.stats()["now_tick"]
    err = _refused(lambda: g.gossip_init(n_floods=4, degree=4, start_gap_ticks=w, start_tick=now + 1))
    assert err.code == -errno.EINVAL and "beyond tick 2^32" in str(err)
    g.gossip_init(n_floods=4, degree=4, start_gap_ticks=w, start_tick=now)
    for _ in range(3):
        g.gen_gossip(w)
        g.step(w)
        g.drain()
    err = _refused(g.gen_gossip, 1)
    assert err.code == -errno.EOVERFLOW and "gossip: the window ends beyond tick 2^32" in str(err)
    g.step(1)


def test_ping_mesh_at_768_ns_ticks(make_oracle):
    n, kw = pc.SPLIT["n"], dict(lookahead_ns=pc.SPLIT["lookahead_ns"], tick_ns=768)
    g, c = both(make_oracle, n, **kw)
    for e in (g, c):
        lc.advance(e, lc.POS["BASE"])
    dev = pc.run_splitbrain(g, device=True, case="accept")
    pc.assert_same_run(dev, pc.run_splitbrain(c, device=False, case="accept"))
    assert dev["summary"]["received"] > 0


def test_flow_mesh_at_768_ns_ticks(make_oracle):
    n, kw = fc.CUT["n"], dict(lookahead_ns=fc.CUT["lookahead_ns"], tick_ns=768)
    g, c = both(make_oracle, n, **kw)
    for e in (g, c):
        lc.advance(e, lc.POS["BASE"])
    dev = fc.run_cut(g, device=True)
    fc.assert_same_run(dev, fc.run_cut(c, device=False))
    assert (dev["rows"]["state"] != abi.FLOW_ACTIVE).any()


@pytest.mark.parametrize("name", ["NEAR", "CROSS_E"])
def test_edge_at_millisecond_ticks_near_the_limit(make_oracle, name):
    """tick_ns = 10^6: one empty step reaches 2^46 ns, and a 2,000-tick window is 2 s long, so both
    positions cross it (NEAR in its second window on the oracle, CROSS_E in its first)."""
    tick_ns = 10**6
    g, c = edge_pair(make_oracle, lc.positions(tick_ns)[name], tick_ns=tick_ns)
    raised, first = guard_run(g, c, [host_driver(pk, t) for pk, t in lc.edge_plan()], f"{name} at 10^6-ns ticks")
    assert first == (1 if name == "NEAR" else 0) and raised is not None and raised <= first
