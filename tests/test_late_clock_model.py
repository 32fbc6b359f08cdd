"""The late-clock scenarios on the CPU oracle alone (tests/late_clock_cases.py): the reference the GPU
tests compare with is itself pinned.  For host traffic the oracle is shift-invariant once the clock is
past the HTB warm-up: a run started at any later tick gives the BASE run's verdicts, and its deliveries
with the offset added, at and beyond 2^46 ns too (the oracle has no time limit).  One time of the
oracle narrowed to 32 bits breaks that at the positions beyond 2^32 ns."""
import errno

import numpy as np
import pytest

import flow_cases as fc
import late_clock_cases as lc
import ping_cases as pc
from testground_amd import workloads as wl
from testground_amd.engine import EngineError


def edge_run(make_oracle, start, flush=0, tick_ns=1000):
    e = make_oracle(lc.EDGE["n"], **lc.edge_kwargs(tick_ns))
    lc.configure_edge(e)
    lc.advance(e, start)
    assert e.stats()["now_tick"] == start
    return e, lc.run_plan(e, lc.edge_plan(flush))


@pytest.fixture(scope="module")
def edge_base(oracle_lib):
    from testground_amd.engine import CABIEngine

    _, out = edge_run(lambda n, **kw: CABIEngine(oracle_lib, "tgo_", n, **kw), lc.POS["BASE"])
    v = np.concatenate([v for v, _ in out])
    # the scenario still holds what it is for: a full netem queue, clones, losses, deliveries
    assert len(set(v.tolist())) >= 3 and all(len(d) > 1000 for _, d in out)
    return out


@pytest.mark.parametrize("name", [k for k in {**lc.POS, **lc.PAST} if k != "BASE"])
def test_oracle_edge_is_shift_invariant(make_oracle, edge_base, name):
    start = {**lc.POS, **lc.PAST}[name]
    _, out = edge_run(make_oracle, start)
    off = (start - lc.POS["BASE"]) * 1000
    for w, ((v, d), (bv, bd)) in enumerate(zip(out, edge_base)):
        assert v.tobytes() == bv.tobytes(), f"{name}: verdicts of window {w}"
        assert len(d) == len(bd) and lc.shifted(d, off).tobytes() == bd.tobytes(), f"{name}: deliveries of window {w}"
    if name in lc.PAST:
        assert lc.first_overflow_window(out) == 0  # the oracle itself goes on beyond 2^46 ns


def test_near_run_stays_below_the_limit(make_oracle):
    """The precondition of the GPU test at NEAR: the three windows and the flushing step end below
    2^46 ns with nothing left in flight (3 s of margin against a worst backlog of 200 x 12,000 bit at
    2^20 bit/s plus 25 ms of delay)."""
    e, out = edge_run(make_oracle, lc.POS["NEAR"], flush=lc.EDGE_FLUSH)
    assert e.pending() == 0
    assert lc.first_overflow_window(out) is None
    assert max(int(d["t_ns"].max()) for _, d in out if len(d)) < lc.NS_LIMIT
    assert (e.stats()["now_tick"] + 1) * 1000 < lc.NS_LIMIT
    # nothing is queued any more: a further window delivers nothing
    e.step(1000)
    assert len(e.drain()) == 0


def test_crossing_runs_cross_where_the_gpu_tests_expect(make_oracle):
    """CROSS_E: the first window's records already pass 2^46 ns (the 20-ms links).  CROSS_D: the first
    burst departs below it, the second burst's backlog crosses it (eligible at once, departing up to
    2.3 s later), so one window matches before the engine's guard must fire."""
    _, out = edge_run(make_oracle, lc.POS["CROSS_E"])
    assert lc.first_overflow_window(out) == 0
    e = make_oracle(lc.BACKLOG["n"], **lc.backlog_kwargs())
    lc.configure_backlog(e)
    lc.advance(e, lc.POS["CROSS_D"])
    out = lc.run_plan(e, lc.backlog_plan())
    assert lc.first_overflow_window(out) == 1
    assert len(out[0][1]) == lc.BACKLOG["n"] * lc.BACKLOG["first"]
    # e < 2^46 <= d: every packet of the crossing burst was offered a second below the limit
    assert (lc.POS["CROSS_D"] + 2 * lc.BACKLOG["window"]) * 1000 < lc.NS_LIMIT - 900_000_000
    d1 = out[1][1]
    assert 0 < int((d1["t_ns"] >= lc.NS_LIMIT).sum()) < len(d1)


def test_storm_positions(make_oracle):
    """The storm's slow links hold seconds of backlog: at NEAR its departures cross 2^46 ns (the GPU test
    there checks the guard), at STORM_NEAR they stay below (the GPU test there checks parity)."""
    for name, crosses in (("NEAR", True), ("STORM_NEAR", False)):
        e = make_oracle(lc.STORM["n"])
        wl.configure_storm(e, lc.STORM["n"])
        lc.advance(e, lc.STORM_POS[name])
        top = 0
        for _ in range(lc.STORM["windows"]):
            lc.storm_step(e)
            top = max(top, int(e.drain()["t_ns"].max()))
        lc.storm_step_n(e)
        top = max(top, int(e.drain()["t_ns"].max()))
        assert (top >= lc.NS_LIMIT) == crosses, (name, top - lc.NS_LIMIT)


@pytest.mark.parametrize("tick_ns", [100, 768, 3000, 10**6])
def test_oracle_takes_other_tick_lengths(make_oracle, tick_ns):
    """The edge scenario at another tick length still fills queues and delivers; the offered packets'
    times scale with the tick, the link delays do not, so the runs differ from the 1000-ns one."""
    e, out = edge_run(make_oracle, lc.POS["BASE"], tick_ns=tick_ns)
    s = e.stats()
    assert s["offered"] == lc.EDGE["windows"] * lc.EDGE["per_window"] and s["scheduled"] > 10_000
    t0 = lc.POS["BASE"] * tick_ns
    assert all(int(d["t_ns"].min()) >= t0 for _, d in out)


# -- the gossip guard ------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    with pytest.raises(EngineError) as ei:
        fn(*a, **kw)
    return ei.value


def test_gossip_refuses_ticks_beyond_32_bits(make_oracle):
    n = 50
    e = make_oracle(n, lookahead_ns=wl.GOSSIP_MIN_LAT)
    wl.configure_gossip(e, n)
    w = wl.gossip_window_ticks(e)
    last = 0xFFFFFFFE
    lc.advance(e, last - 3 * w)
    now = e.stats()["now_tick"]
    # the last flood's start tick: 0xFFFFFFFE is the last one a receipt can hold
    err = _code(e.gossip_init, n_floods=4, degree=4, start_gap_ticks=w, start_tick=now + 1)
    assert err.code == -errno.EINVAL and "beyond tick 2^32" in str(err)
    err = _code(e.gossip_init, n_floods=1, degree=4, start_gap_ticks=0, start_tick=last + 1)
    assert err.code == -errno.EINVAL
    e.gossip_init(n_floods=4, degree=4, start_gap_ticks=w, start_tick=now)  # the last flood at 0xFFFFFFFE
    for _ in range(3):  # the third window ends at tick 0xFFFFFFFE
        e.gen_gossip(w)
        e.step(w)
        e.drain()
    assert e.stats()["now_tick"] == last
    err = _code(e.gen_gossip, 1)
    assert err.code == -errno.EOVERFLOW and "gossip: the window ends beyond tick 2^32" in str(err)
    e.step(1)  # the refused window changed nothing: the engine steps on without it


# -- ping and flow models at tick 2^31 -------------------------------------------------------------------
def test_ping_and_flow_models_refuse_tick_2_31(make_oracle):
    e = make_oracle(pc.VERIFY["n"], lookahead_ns=pc.VERIFY["lookahead_ns"])
    lc.advance(e, lc.POS["T31"])
    m = wl.PingModel(e, lc.ping_at_t31(e), pc.verify_targets())
    err = _code(m.step, 3000)  # ends at tick 2^31
    assert err.code == -errno.EOVERFLOW and "ping: the window ends beyond tick 2^31" in str(err)
    e = make_oracle(fc.CUT["n"], lookahead_ns=fc.CUT["lookahead_ns"])
    lc.advance(e, lc.POS["T31"])
    m = wl.FlowModel(e, fc.CUT_FLOW, fc.cut_flows(lc.POS["T31"]))
    err = _code(m.step, 3000)
    assert err.code == -errno.EOVERFLOW and "flow: the window ends beyond tick 2^31" in str(err)
