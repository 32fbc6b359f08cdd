"""Long fused groups (tgsim_step_n with TGSIM_FUSE up to 32): the windows' descriptors live in a
device buffer instead of the kernel-argument segment, a call is split into near-equal groups and, where it pays,
a short last one (_groups), and the memory rule (TGSIM_FUSE_MEM_MB) may cut the groups shorter.

Every case runs the engine under test beside an engine at TGSIM_FUSE=1 (tgsim_step per window) and the
CPU oracle on the same inputs, and compares after every call what tgsim_step_n leaves: the verdict
bytes (a call keeps its last window's; the earlier windows' verdicts are in the statistics'
by_verdict counts), every delivery in drain order, and stats().  The calls' lengths differ from case
to case, so the compared verdicts are those of windows 9, 15, 16, 17, 22, 30, 32, 33 and 38.

The shapes are small on purpose: 96 sources with the C3 storm shapes, 200-tick windows at
lambda = 0.5 (100 packets per source and window, above the 64 a window needs to fuse) and a netem
limit of 64, so every queue is full and the hand-off between a source's windows carries it."""
import numpy as np
import pytest

from testground_amd import workloads as wl
from testground_amd.engine import Engine

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None

N, TICKS, LAM, QLIM = 96, 200, 0.5, 64


def _fused(e):
    return int(e._fn("debug_fused_windows")(e._h))


def _launches(e):
    return int(e._fn("debug_fused_launches")(e._h))


def _groups(n, cap):
    """The split rule the engine documents (caps of 8 and more): the fewest groups of at
    most cap windows, of near-equal size; the call ends with a short group of 6 where 25 us per window
    that the last group gets shorter by outweigh 180 us per launch that this adds."""
    k_plain, k_tail = -(-n // cap), -(-(n - 6) // cap) + 1
    last_plain = n // k_plain
    tail = 6 if n > 6 and last_plain > 6 and 25 * (last_plain - 6) > 180 * (k_tail - k_plain) else 0
    out = []
    while n:
        body = n - tail if n > tail else n
        k = -(-body // cap)
        g = -(-body // k)
        out.append(g)
        n -= g
    return out


assert _groups(30, 32) == [24, 6] and _groups(30, 16) == [12, 12, 6] and _groups(30, 8) == [8, 8, 8, 6]
assert _groups(9, 16) == [9] and _groups(16, 8) == [8, 8] and _groups(22, 8) == [8, 8, 6] and _groups(22, 16) == [16, 6]
assert _groups(38, 32) == [32, 6] and _groups(33, 16) == [14, 13, 6] and _groups(13, 32) == [13] and _groups(14, 32) == [8, 6]


def _trio(make_oracle, monkeypatch, fuse, env=None, **kw):
    """(engine under test, engine at TGSIM_FUSE=1, oracle), configured alike (the knobs are read at
    engine creation)."""
    monkeypatch.setenv("TGSIM_FUSE", "1")
    ref = Engine(N, queue_limit=QLIM, **kw)
    monkeypatch.setenv("TGSIM_FUSE", str(fuse))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    g = Engine(N, queue_limit=QLIM, **kw)
    for k in env or {}:
        monkeypatch.delenv(k)
    c = make_oracle(N, queue_limit=QLIM, **kw)
    es = (g, ref, c)
    for e in es:
        wl.configure_storm(e, N)
    return es


def _call(es, n, what, lam=LAM, ticks=TICKS):
    """n generated windows through one step_n call on every engine, then the comparison."""
    g, ref, c = es
    for e in es:
        for _ in range(n):
            e.gen_storm(lam, ticks)
        e.step_n(ticks, n)
    vg, vr = g.verdicts(), ref.verdicts()
    assert len(vg) == len(vr) and (vg == vr).all(), f"{what}: verdicts differ from TGSIM_FUSE=1"
    dg, dr = g.drain(), ref.drain()
    assert len(dg) == len(dr) and (dg == dr).all(), f"{what}: deliveries differ from TGSIM_FUSE=1"
    sg, sr, sc = g.stats(), ref.stats(), c.stats()
    assert sg == sr, f"{what}: stats differ from TGSIM_FUSE=1"
    vc, dc = c.verdicts(), c.drain()
    assert len(vg) == len(vc) and (vg == vc).all(), f"{what}: verdicts differ from the oracle"
    assert len(dg) == len(dc) and (dg == dc).all(), f"{what}: deliveries differ from the oracle"
    assert sg == sc, f"{what}: stats differ from the oracle"
    return dg


@pytest.mark.parametrize("n", [9, 16, 17, 22, 30, 32, 33, 38])
@pytest.mark.parametrize("fuse", [16, 32])
def test_long_groups_equal_unfused(make_oracle, monkeypatch, fuse, n):
    """One group, a call of exactly the cap and of cap + 1 windows, a group of exactly the cap (22 at 16,
    38 at 32) and more than 32 windows."""
    es = _trio(make_oracle, monkeypatch, fuse)
    d = _call(es, n, f"TGSIM_FUSE={fuse}, {n} windows")
    assert len(d) > 0  # 1-100 ms latencies: few records are due within the call's few milliseconds
    g, ref, _ = es
    assert _fused(g) == n and _fused(ref) == 0
    assert _launches(g) == len(_groups(n, fuse))
    s = g.stats()
    assert s["scheduled"] > 0 and s["offered"] > s["scheduled"]


def test_two_calls_reuse_parities(make_oracle, monkeypatch):
    """Two consecutive calls of 15 windows: call 2's launch runs beside the delivery of call 1's
    group, and a third call comes back to the first parity's buffer sets and descriptors."""
    es = _trio(make_oracle, monkeypatch, 16)
    for k in range(3):
        _call(es, 15, f"call {k}")
    assert _fused(es[0]) == 45 and _launches(es[0]) == 3 * len(_groups(15, 16)) == 6


def test_reshape_between_calls(make_oracle, monkeypatch):
    """A configure_batch reshape of 10 % of the sources between two calls applies from the next
    call's first window."""
    es = _trio(make_oracle, monkeypatch, 32)
    _call(es, 17, "before the reshape")
    sel = np.arange(3, N, 10)
    assert len(sel) == 10
    for e in es:
        e.configure_batch(sel, wl.storm_configs(len(sel), 0x5EED))
    _call(es, 18, "after the reshape")
    assert _fused(es[0]) == 35


def test_long_group_after_sparse_fifo_windows(make_oracle, monkeypatch):
    """Sparse FIFO windows leave queues in place (head slot != 0); the long group behind them reads
    every queue from slot 0 (k_unrotate compacts them first)."""
    from testground_amd.network import configs_array

    es = _trio(make_oracle, monkeypatch, 16)
    for e in es:
        e.configure_batch(np.arange(N), configs_array(np.full(N, 3_000_000), routing_policy=2))
    for k in range(4):  # ~20 packets per source and window: sparse, FIFO
        _call(es, 1, f"sparse FIFO window {k}", lam=0.02, ticks=1000)
    assert _fused(es[0]) == 0
    _call(es, 16, "16 fused windows after in-place queues")
    assert _fused(es[0]) == 16 and _launches(es[0]) == len(_groups(16, 16)) == 2


def test_lookahead(make_oracle, monkeypatch):
    """A nonzero lookahead moves every window's horizon (a per-window descriptor field).  At 110 ms
    it is past every storm latency and jitter, so each window delivers what its sources' HTB rates let
    through in the call's 4 ms (the netem limit of 64 refuses most of the rest): a 1 Gbit/s source sends
    some hundred packets in that time, and about a quarter of the 96 sources have such a link."""
    es = _trio(make_oracle, monkeypatch, 32, lookahead_ns=110_000_000)
    d = _call(es, 20, "lookahead 110 ms")
    assert len(d) > 1000
    _call(es, 9, "lookahead 110 ms, second call")
    assert _fused(es[0]) == 29


def test_memory_budget_splits_groups(make_oracle, monkeypatch):
    """TGSIM_FUSE_MEM_MB too low for more than 8 buffer sets: a 16-window request runs at a cap of 8
    (never below what fit before the cap was raised) as 8 + 8 instead of 10 + 6, a 22-window request
    as 8 + 8 + 6 instead of 16 + 6, with the same results and no error."""
    es = _trio(make_oracle, monkeypatch, 16, env={"TGSIM_FUSE_MEM_MB": "1"})
    _call(es, 16, "16 windows under a 1-MB budget")
    assert _fused(es[0]) == 16 and _launches(es[0]) == len(_groups(16, 8)) == 2
    _call(es, 22, "22 windows under a 1-MB budget")
    assert _fused(es[0]) == 38 and _launches(es[0]) == 2 + len(_groups(22, 8)) == 5 != 2 + len(_groups(22, 16))


def test_stamps_on(make_oracle, monkeypatch):
    """Diagnostics on (TGSIM_STAMPS): 17 windows at a cap of 32 still equal the reference."""
    es = _trio(make_oracle, monkeypatch, 32, env={"TGSIM_STAMPS": "1"})
    _call(es, 17, "17 windows with stamps")
    assert _fused(es[0]) == 17 and _launches(es[0]) == len(_groups(17, 32)) == 2
