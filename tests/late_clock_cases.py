"""Scenarios and clock positions shared by tests/test_late_clock_model.py (the CPU oracle against
itself, shifted in time) and tests/test_gpu_late_clock.py (the HIP engine against the oracle): the
engine's time arithmetic away from t = 0.  Queued items keep their eligibility time in 46 bits,
sparse windows carry a record's destination slot above bit 46 of t_ns, the timing wheel keeps 32-bit
bucket ids, gossip receipts and the storm generator's Philox counter are 32-bit ticks, ping and flow
stop at tick 2^31: none of that shows in a run that starts at tick 0 with 1000-ns ticks.

A scenario is configured on any engine-shaped object (Engine or the oracle's CABIEngine), the clock
is moved by empty steps (advance), and the windows are driven one by one."""
import functools

import numpy as np

from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

NS_LIMIT = 1 << 46     # the engine's time field: eligibility and departure times stay below it
SECOND = 1_000_000_000
MAX_STEP = (1 << 32) - 1


def advance(e, ticks):
    """Moves e's clock forward by empty steps (no traffic pending) of at most 2^32 - 1 ticks each."""
    while ticks > 0:
        k = min(ticks, MAX_STEP)
        e.step(k)
        ticks -= k


def positions(tick_ns=1000):
    """Start ticks of a scenario.  BASE: past the HTB warm-up (a bucket that is not yet full at tick 0
    or 1 makes those starts differ), the reference every other position is compared with.  NS32: the
    windows straddle t_ns = 2^32.  T31, T32: they straddle tick 2^31 and tick 2^32.  NEAR: 3 s below
    2^46 ns, the run still fits.  CROSS_E: 10 ms below, the 20-ms links' eligibility times cross it.
    CROSS_D: 1 s below, only a slow link's departure times cross it."""
    return dict(BASE=10**7,
                NS32=4_294_000_000 // tick_ns,
                T31=(1 << 31) - 3000,
                T32=(1 << 32) - 3000,
                NEAR=(NS_LIMIT - 3 * SECOND) // tick_ns,
                CROSS_E=(NS_LIMIT - 10_000_000) // tick_ns,
                CROSS_D=(NS_LIMIT - SECOND) // tick_ns)


POS = positions()
# oracle only: starts at and beyond the engine's limit (the oracle has none)
PAST = dict(AT46=NS_LIMIT // 1000 + 10, T40=1 << 40)


# -- edge: tests/test_gpu_parity.py::test_window_edge_shapes, with correlated sources -----------------
EDGE = dict(n=128, queue_limit=200, lookahead_ns=300_000, window=2000, windows=3, per_window=20_000)
EDGE_FLUSH = 2_400_000  # ticks of 1000 ns: longer than the worst backlog (200 x 12,000 bit at 2^20 bit/s + 25 ms)


def edge_kwargs(tick_ns=1000):
    return dict(queue_limit=EDGE["queue_limit"], lookahead_ns=EDGE["lookahead_ns"], tick_ns=tick_ns)


def configure_edge(e):
    """Zero, sub-tick, 1-ms and 20-ms latency (sources at <= 1 ms park their far items in a wheel of
    2^14-ns buckets), jitter beyond the latency, every bandwidth class (1 Mbit/s among them: departures
    seconds behind the eligibility times), reorder, duplication, loss, corruption; every seventh source
    correlated (the i % 7 sources of test_sparse_and_dense_kernels_agree)."""
    n = EDGE["n"]
    lat = [0, 50 * nw.Microsecond, 1 * nw.Millisecond, 20 * nw.Millisecond]
    for i in range(n):
        L = lat[i % 4]
        J = [0, L // 2, 2 * L, 5 * nw.Millisecond][(i // 4) % 4]
        s = nw.LinkShape(Latency=L, Jitter=J,
                         Bandwidth=int([0, 1 << 20, 10**7, 10**8, 10**9][(i // 16) % 5]),
                         Reorder=float([0, 5, 50][(i // 3) % 3]), Duplicate=float([0, 20][(i // 7) % 2]),
                         Loss=float([0, 5][(i // 11) % 2]), Corrupt=float([0, 10][(i // 5) % 2]))
        if i % 7 == 0:
            s.DuplicateCorr, s.CorruptCorr = 30.0, 20.0
        e.configure(i, nw.Config(Network="default", Enable=True, Default=s))


@functools.lru_cache(maxsize=None)
def edge_windows():
    """The host packets of the three windows (tick relative to the window): a third of them on 20
    ticks, sequence numbers unique and not monotone across ticks."""
    n, m = EDGE["n"], EDGE["per_window"]
    rng = np.random.default_rng(211)
    out = []
    for step in range(EDGE["windows"]):
        src = rng.integers(0, n, m)
        pk = np.zeros(m, dtype=abi.PKT_DTYPE)
        pk["src"] = src
        pk["dst"] = (src + 1 + rng.integers(0, n - 1, m)) % n
        pk["len"] = rng.integers(40, 1500, m)
        tick = rng.integers(0, EDGE["window"], m)
        burst = rng.random(m) < 0.33
        tick[burst] = rng.choice(rng.integers(0, EDGE["window"], 20), burst.sum())
        pk["tick"] = tick
        pk["seq"] = rng.permutation(m).astype(np.uint32) + np.uint32(step * m)
        pk.setflags(write=False)
        out.append(pk)
    return tuple(out)


def edge_plan(flush=0):
    """[(packets or None, ticks)]: the three windows, then an empty step of `flush` ticks."""
    plan = [(pk, EDGE["window"]) for pk in edge_windows()]
    return plan + [(None, flush)] if flush else plan


# -- backlog: a slow link's departures run seconds behind its eligibility times -------------------------
BACKLOG = dict(n=16, queue_limit=200, first=60, burst=300, length=1500, window=2000, idle=400_000, idle_windows=3)


def backlog_kwargs(tick_ns=1000):
    return dict(queue_limit=BACKLOG["queue_limit"], tick_ns=tick_ns)


def configure_backlog(e):
    for i in range(BACKLOG["n"]):
        e.configure(i, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=0, Bandwidth=1 << 20)))


def _burst(count, seq0):
    n = BACKLOG["n"]
    pk = np.zeros(n * count, dtype=abi.PKT_DTYPE)
    pk["src"] = np.repeat(np.arange(n), count)
    pk["dst"] = (pk["src"] + 1) % n
    pk["len"] = BACKLOG["length"]
    pk["tick"] = 0
    pk["seq"] = np.tile(np.arange(seq0, seq0 + count), n)
    return pk


def backlog_plan():
    """Zero latency, so every admitted packet is eligible at once and served in its own window, with a
    departure time as far ahead as the backlog is long (1500 B at 2^20 bit/s: 11.4 ms each).  A first
    burst of 60 x 1500 B per source at tick 0 of window 0 (0.7 s of service), a burst of 300 per source
    at tick 0 of window 1 (the queue of 200 fills: 2.3 s of service from the first burst's start), then
    empty windows of 0.4 s."""
    return ([(_burst(BACKLOG["first"], 0), BACKLOG["window"]), (_burst(BACKLOG["burst"], BACKLOG["first"]), BACKLOG["window"])]
            + [(None, BACKLOG["idle"])] * BACKLOG["idle_windows"])


# -- storm: the device generator (Philox keyed by the 32-bit tick) ------------------------------------
STORM = dict(n=257, lam=0.5, window=1500, windows=3, fused=8)


# The storm's slowest links hold more than 3 s of backlog: its departures cross 2^46 ns from NEAR.
# STORM_NEAR leaves 20 s (tests/test_late_clock_model.py pins both on the oracle).
STORM_POS = dict(T32=POS["T32"], NEAR=POS["NEAR"], STORM_NEAR=(NS_LIMIT - 20 * SECOND) // 1000)


def storm_step(e):
    e.gen_storm(STORM["lam"], STORM["window"])
    e.step(STORM["window"])


def storm_step_n(e):
    for _ in range(STORM["fused"]):
        e.gen_storm(STORM["lam"], STORM["window"])
    e.step_n(STORM["window"], STORM["fused"])


# -- gossip ---------------------------------------------------------------------------------------------
GOSSIP = dict(n=600, floods=8, degree=8, windows=30, start_gap_ticks=500)


def gossip_arm(e, start_tick):
    wl.configure_gossip(e, GOSSIP["n"])
    e.gossip_init(n_floods=GOSSIP["floods"], degree=GOSSIP["degree"], msg_len=1024,
                  start_gap_ticks=GOSSIP["start_gap_ticks"], start_tick=start_tick)


# -- ping and flow at tick 2^31 ---------------------------------------------------------------------------
def ping_at_t31(e):
    """One probe per slot at the engine's current tick (T31: a schedule that ends below tick 2^31)."""
    return dict(count=1, interval_ticks=1, length=64, start_tick=e.stats()["now_tick"], bin_ns=nw.Millisecond, n_bins=16)


# -- driving a plan -------------------------------------------------------------------------------------
def run_window(e, pk, ticks):
    """One window; returns (verdict bytes, drained records)."""
    have = pk is not None and len(pk)
    if have:
        e.submit(pk)
    e.step(ticks)
    return (e.verdicts() if have else np.zeros(0, dtype=np.uint8)), e.drain()


def run_plan(e, plan):
    return [run_window(e, pk, ticks) for pk, ticks in plan]


def shifted(drained, offset_ns):
    """The records with offset_ns taken off their delivery times."""
    d = drained.copy()
    d["t_ns"] = (d["t_ns"].astype(np.int64) - np.int64(offset_ns)).astype(np.uint64)  # (either sign)
    return d


def first_overflow_window(windows):
    """Index of the first window whose drain holds a t_ns >= 2^46, or None."""
    for w, (_, d) in enumerate(windows):
        if len(d) and int(d["t_ns"].max()) >= NS_LIMIT:
            return w
    return None
