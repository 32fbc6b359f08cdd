"""The reply calendar's hand-over between its two holders on ONE engine: a ping
run of two armed phases (so the calendar's buffers have flipped), a flow run, a ping run again, each
phase against the same chain on one oracle engine, bit for bit.  The clock is carried through (ticks
500,000 -> 580,000 -> 1,080,000) and every phase ends with nothing pending.  Then the four C entry points
that arm the flow driver, and which of the optional tables each leaves readable."""
import ctypes as C
import errno

import pytest

import flow_cases as fc
import ping_cases as pc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
MS = nw.Millisecond


def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


def _ping_complete(phases):
    for out in phases:
        s = out["summary"]
        assert (s["sent"], s["received"], s["pending_replies"]) == (6, 6, 0), s


def test_ping_flow_ping(make_oracle):
    kw = dict(lookahead_ns=10 * MS)
    eng, ref = Engine(2, **kw), make_oracle(2, **kw)

    # 1. ping holds the calendar, twice over
    dev1, ref1 = pc.run_pingpong(eng, device=True), pc.run_pingpong(ref, device=False)
    for d, r in zip(dev1, ref1):
        pc.assert_same_run(d, r)
    _ping_complete(dev1)
    assert eng.stats()["now_tick"] == ref.stats()["now_tick"] == 500_000
    _raises(errno.EBUSY, "flow: the ping driver is armed", eng.flow_init, fc.table([(0, 1, 1, 500_000)]), **fc.ROUNDS_FLOW)
    eng.ping_init(None)

    # 2. flow takes it; disarming ping meanwhile is not its owner's business
    def ping_disarm(w):
        if w in (1, 4):
            eng.ping_init(None)
            assert eng.flow_report()["flows"] == 2

    dev2 = fc.run_rounds(eng, device=True, rounds=3, before=ping_disarm)
    fc.assert_same_run(dev2, fc.run_rounds(ref, device=False, rounds=3))
    s = dev2["summary"]
    assert (s["done"], s["flows"], s["segs_acked"], s["pending_acks"]) == (2, 2, 48, 0), s
    assert eng.stats()["now_tick"] == ref.stats()["now_tick"] == 580_000
    _raises(errno.EBUSY, "ping: the flow driver is armed", eng.ping_init, pc.PINGPONG_TARGETS, start_tick=580_000)
    eng.flow_init(None)
    _raises(errno.EINVAL, "not armed", eng.flow_report)

    # 3. and ping again, on a calendar reset from the flow driver's state
    dev3, ref3 = pc.run_pingpong(eng, device=True), pc.run_pingpong(ref, device=False)
    for d, r in zip(dev3, ref3):
        pc.assert_same_run(d, r)
    _ping_complete(dev3)
    assert eng.stats()["now_tick"] == ref.stats()["now_tick"] == 1_080_000


def test_flow_entry_points():
    """tgsim_flow_init, _cc, _rto and _fb, called as C: each arms its own optional tables and no other."""
    eng = Engine(2, lookahead_ns=10 * MS)
    fc.plain(eng, 2, 10 * MS)
    t = fc.table([(0, 1, 4, 0)])
    f = fc.ROUNDS_FLOW
    p = C.byref(abi.Flow(f["seg_len"], f["ack_len"], f["window"], f["rto_ticks"], f["max_attempts"], f["n_bins"], f["bin_ns"]))
    cc = C.byref(abi.FlowCC(1, 0, 3, 0))
    rto = C.byref(abi.FlowRto(1_000, abi.FLOW_MAX_RTO, 1, 0))
    fb = C.byref(abi.FlowFb(0))
    for name, parts, armed in (("flow_init", (), ()), ("flow_init_cc", (cc,), ("cc",)), ("flow_init_rto", (cc, rto), ("cc", "rto")),
                               ("flow_init_fb", (cc, rto, fb), ("cc", "rto", "fb"))):
        assert eng._fn(name)(eng._h, p, *parts, t.ctypes.data, len(t)) == 0, name
        eng._n_flows = len(t)
        assert len(eng.flow_rows()) == 1
        for part in ("cc", "rto", "fb"):
            rows = getattr(eng, f"flow_{part}_rows")
            if part in armed:
                assert len(rows()) == 1, (name, part)
            else:
                _raises(errno.EINVAL, "not armed", rows)
