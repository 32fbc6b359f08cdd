"""The propagation report of the gossip flood (tgsim_gossip_spread, tgsim_gossip_times) against
the oracle.

The expected values come from the oracle alone: it exposes the offered packets of every generated
window (tgo_offered), and every `degree`-th of them names one (peer, flood, absolute forward tick).
The table of those ticks is the expected gossip_times; the expected spread follows from it with
numpy (hold = tick - the flood's start tick).  The HIP engine runs the same windows in lockstep and
both of its reports are compared exactly, at probes where floods are untouched, partly spread (with
receipts still pending for a later window, which the report must not count) and complete.
"""
import ctypes as C
import errno

import numpy as np
import pytest

from testground_amd import abi
from testground_amd import workloads as wl
from testground_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None

NONE = 0xFFFFFFFF
PAIRS = [(5000, 32), (1000, 64), (777, 256), (1, 256), (5000, 1), (0, 0)]


class Lockstep:
    """The oracle and any number of HIP engines (whole or shards) driven window by window; `table`
    is the oracle-derived [n, floods] forward tick of every (peer, flood) offered so far."""

    def __init__(self, make_oracle, n, floods, degree, gap, shards=()):
        kw = dict(lookahead_ns=wl.GOSSIP_MIN_LAT)
        self.n, self.floods, self.degree, self.gap = n, floods, degree, gap
        self.cpu = make_oracle(n, **kw)
        self.gpu = Engine(n, **kw)
        self.bounds = [0] + [b for _, b in shards]
        self.shards = [Engine(n, shard=s, **kw) for s in shards]
        for e in self.engines():
            wl.configure_gossip(e, n)
        self.W = wl.gossip_window_ticks(self.cpu)
        self.arm(0)

    def engines(self):
        return [self.cpu, self.gpu] + self.shards

    def arm(self, start_tick):
        self.start = start_tick
        for e in self.engines():
            e.gossip_init(n_floods=self.floods, degree=self.degree, msg_len=1024, start_gap_ticks=self.gap,
                          start_tick=start_tick)
        self.table = np.full((self.n, self.floods), NONE, dtype=np.uint32)

    def window(self):
        now = self.cpu.stats()["now_tick"]
        self.cpu.gen_gossip(self.W)
        pk = np.zeros(1 << 20, dtype=abi.PKT_DTYPE)
        m = self.cpu._lib.tgo_offered(self.cpu._h, pk.ctypes.data, len(pk))
        assert 0 <= m < len(pk) and m % self.degree == 0
        one = pk[:m:self.degree]  # a forward is `degree` consecutive packets: its first names it
        assert (self.table[one["src"], one["seq"] // self.degree] == NONE).all()  # forwarded once
        self.table[one["src"], one["seq"] // self.degree] = one["tick"].astype(np.int64) + now
        self.cpu.step(self.W)
        self.cpu.drain()
        self.gpu.gen_gossip(self.W)
        self.gpu.step(self.W)
        self.gpu.drain()
        if self.shards:
            for s in self.shards:
                s.gen_gossip(self.W)
            _manual_sharded_step(self.shards, self.bounds, self.W)
            for s in self.shards:
                s.drain()

    def expected(self, bin_ticks, n_bins, rows=slice(None)):
        """The spread of the table's rows, by numpy."""
        t = self.table[rows].astype(np.int64)
        have = t != NONE
        hold = t - (self.start + self.gap * np.arange(self.floods, dtype=np.int64))[None, :]
        assert (hold[have] >= 0).all()
        hist = np.zeros((self.floods, n_bins), dtype=np.uint64)
        for f in range(self.floods if n_bins else 0):
            b = np.minimum(hold[have[:, f], f] // bin_ticks, n_bins - 1)
            hist[f] = np.bincount(b, minlength=n_bins)
        return {"reached": have.sum(0).astype(np.uint64),
                "sum_ticks": np.where(have, hold, 0).sum(0).astype(np.uint64),
                "min_ticks": np.where(have, hold, NONE).min(0).astype(np.uint32),
                "max_ticks": np.where(have, hold, 0).max(0).astype(np.uint32),
                "hist": hist}

    def close(self):
        for e in self.engines():
            e.close()


def _manual_sharded_step(shards, bounds, window):
    """step_sim on every shard, exchange through device buffers, deliver (one GPU, no collective)."""
    outs = []
    torch.cuda.current_stream().synchronize()  # the engines run on their own streams (shard.py)
    for s in shards:
        buf = torch.empty(max(1, s.sim_capacity()) * 24, dtype=torch.uint8, device="cuda")
        cnt = s.step_sim(window, bounds, buf.data_ptr(), s.sim_capacity())
        outs.append((buf, cnt))
    for k, s in enumerate(shards):
        parts = [buf[int(cnt[:k].sum()) * 24: int(cnt[:k + 1].sum()) * 24] for buf, cnt in outs]
        inbound = torch.cat(parts)
        torch.cuda.current_stream().synchronize()  # torch.cat ran on torch's stream
        s.deliver(inbound.data_ptr(), inbound.numel() // 24)


def assert_spread(got, want, what):
    assert set(got) == set(want), what
    for k in wl.SPREAD_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, f"{what}: {k}"
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {k} differs at {bad[:4].tolist()}: {got[k][tuple(bad[0])]} vs {want[k][tuple(bad[0])]}"


def assert_empty(e, n, floods, peer0=0):
    """No peer has forwarded anything: the neutral report, and no forward tick."""
    s = e.gossip_spread(1000, 16)
    assert (s["reached"] == 0).all() and (s["sum_ticks"] == 0).all() and len(s["reached"]) == floods
    assert (s["min_ticks"] == NONE).all() and (s["max_ticks"] == 0).all()
    assert s["hist"].shape == (floods, 16) and (s["hist"] == 0).all()
    t = e.gossip_times(peer0, n)
    assert t.shape == (n, floods) and t.dtype == np.uint32 and (t == NONE).all()


def probe(run, what):
    """gossip_times of the whole shard and gossip_spread for every (bin_ticks, n_bins) pair."""
    times = run.gpu.gossip_times(0, run.n)
    bad = np.argwhere(times != run.table)
    assert len(bad) == 0, f"{what}: gossip_times differs at {bad[:4].tolist()}"
    for bin_ticks, n_bins in PAIRS:
        got = run.gpu.gossip_spread(bin_ticks, n_bins)
        assert_spread(got, run.expected(bin_ticks, n_bins), f"{what} bins {bin_ticks} x {n_bins}")
    got = run.gpu.gossip_spread()
    assert (got["reached"] == run.cpu.gossip_reached()).all(), what
    assert (got["reached"] == run.gpu.gossip_reached()).all(), what
    return got


def test_spread_601_peers_64_floods(make_oracle):
    """Case 1: 601 peers (no multiple of 8 or 64), every lane a flood, probes with floods untouched,
    partly spread (receipts pending: first[] set, fwd bit not) and complete."""
    run = Lockstep(make_oracle, 601, 64, 8, 1000)
    seen = {}
    for k in range(60):
        run.window()
        if k in (5, 12, 20, 59):
            seen[k] = probe(run, f"window {k}")["reached"]
    # the states the probes are there for
    assert (seen[5] == 0).sum() == 34 and ((seen[5] > 0) & (seen[5] < 601)).sum() == 30
    assert ((seen[12] > 0) & (seen[12] < 601)).all()
    assert (seen[20] == 601).sum() > 0 and (seen[20] < 601).sum() > 0
    end = run.expected(5000, 32)
    assert (seen[59] == 601).all() and end["max_ticks"].max() == 152_905
    assert (end["hist"][:, -1] == 0).all()                       # (5000, 32): no overflow
    assert (run.expected(1000, 64)["hist"][:, -1] > 0).all()     # (1000, 64): the last bin collects
    run.close()


def test_spread_one_flood_then_rearm(make_oracle):
    """Cases 2 and 5: one flood (63 lanes carry none) that never reaches 8 of 130 peers (empty rows);
    then a re-armed driver reports the empty state, and its floods, which start at a tick other
    than 0, report their hold times from that start."""
    run = Lockstep(make_oracle, 130, 1, 3, 0)
    for k in range(40):
        run.window()
        if k in (3, 39):
            got = probe(run, f"window {k}")
    assert got["reached"][0] == 122
    now = run.cpu.stats()["now_tick"]
    assert now == 40 * run.W
    run.arm(now + 1)
    assert_empty(run.gpu, 130, 1)
    for k in range(12):
        run.window()
    got = probe(run, "re-armed, window 11")
    assert 1 < got["reached"][0] <= 130 and got["min_ticks"][0] == 0
    run.close()


def test_spread_before_any_window(make_oracle):
    """Case 3: the origins' entries are set but not yet forwarded."""
    run = Lockstep(make_oracle, 601, 64, 8, 1000)
    assert_empty(run.gpu, 601, 64)
    assert (run.cpu.gossip_reached() == 0).all()
    run.close()


def test_spread_two_shards_merge(make_oracle):
    """Case 4: the reports of two shards merge into the single engine's and the oracle-derived one."""
    n, half = 2000, 1000
    run = Lockstep(make_oracle, n, 8, 8, 300, shards=[(0, half), (half, n)])
    for k in range(30):
        run.window()
        if k not in (6, 29):
            continue
        for bin_ticks, n_bins in ((2000, 48), (0, 0)):
            parts = [s.gossip_spread(bin_ticks, n_bins) for s in run.shards]
            assert_spread(parts[0], run.expected(bin_ticks, n_bins, slice(0, half)), f"window {k} shard 0")
            assert_spread(parts[1], run.expected(bin_ticks, n_bins, slice(half, n)), f"window {k} shard 1")
            merged = wl.merge_spread(parts)
            assert_spread(merged, run.gpu.gossip_spread(bin_ticks, n_bins), f"window {k} merged vs single")
            assert_spread(merged, run.expected(bin_ticks, n_bins), f"window {k} merged vs oracle")
        assert (merged["reached"] == run.cpu.gossip_reached()).all()
        assert (run.shards[1].gossip_times(half, half) == run.table[half:]).all()
        assert (run.shards[0].gossip_times(3, 500) == run.table[3:503]).all()
        assert (run.gpu.gossip_times(997, 7) == run.table[997:1004]).all()
    with pytest.raises(EngineError) as ei:
        run.shards[1].gossip_times(0, 1)
    assert ei.value.code == -errno.EINVAL and "outside the shard" in ei.value.msg
    with pytest.raises(EngineError) as ei:
        run.shards[0].gossip_times(half - 1, 2)
    assert ei.value.code == -errno.EINVAL
    run.close()


def test_spread_contract():
    """Case 6: the error returns of both calls, each with a tgsim_last_error text."""
    e = Engine(100, lookahead_ns=wl.GOSSIP_MIN_LAT)
    spread, times = e._fn("gossip_spread"), e._fn("gossip_times")
    floods = np.zeros(64, dtype=abi.GOSSIP_FLOOD_DTYPE)
    hist = np.zeros(64 * 256, dtype=np.uint64)
    out = np.zeros(100 * 64, dtype=np.uint32)

    def text():
        return e._fn("last_error")(e._h).decode()

    # the gossip driver was never armed
    assert spread(e._h, 10, 4, floods.ctypes.data, hist.ctypes.data, 64) == -errno.EINVAL and "not armed" in text()
    assert times(e._h, 0, 1, out.ctypes.data, len(out)) == -errno.EINVAL and "not armed" in text()
    with pytest.raises(EngineError) as ei:
        e.gossip_spread(10, 4)
    assert ei.value.code == -errno.EINVAL
    with pytest.raises(EngineError) as ei:
        e.gossip_times(0, 1)
    assert ei.value.code == -errno.EINVAL

    wl.configure_gossip(e, 100)
    e.gossip_init(n_floods=5, degree=4, msg_len=512, start_tick=0)
    assert spread(e._h, 10, 257, floods.ctypes.data, hist.ctypes.data, 64) == -errno.EINVAL and "n_bins" in text()
    assert spread(e._h, 0, 4, floods.ctypes.data, hist.ctypes.data, 64) == -errno.EINVAL and "bin_ticks" in text()
    assert spread(e._h, 10, 4, floods.ctypes.data, None, 64) == -errno.EINVAL and "histogram" in text()
    assert spread(e._h, 10, 4, None, hist.ctypes.data, 64) == -errno.EINVAL and "flood buffer" in text()
    # the allowed corners: no histogram at all, no flood entries at all, fewer entries than floods
    assert spread(e._h, 0, 0, floods.ctypes.data, None, 64) == 5
    assert spread(e._h, 10, 256, None, hist.ctypes.data, 0) == 5
    e.gen_gossip(wl.gossip_window_ticks(e))
    e.step(wl.gossip_window_ticks(e))
    floods["reached"] = 77
    assert spread(e._h, 0, 0, floods.ctypes.data, None, 2) == 5
    assert (floods["reached"][:2] == 1).all() and (floods["reached"][2:] == 77).all()  # cap entries written

    assert times(e._h, 0, 100, out.ctypes.data, 100 * 5) == 500
    assert times(e._h, 0, 100, out.ctypes.data, 100 * 5 - 1) == -errno.ENOSPC and text()
    assert times(e._h, 100, 0, None, 0) == 0                      # the empty range at the shard's end
    assert times(e._h, 99, 2, out.ctypes.data, len(out)) == -errno.EINVAL and "outside the shard" in text()
    assert times(e._h, 101, 0, out.ctypes.data, len(out)) == -errno.EINVAL
    assert times(e._h, 1, 0xFFFFFFFF, out.ctypes.data, len(out)) == -errno.EINVAL
    e.close()


def test_spread_after_late_receipt():
    """A sticky late-receipt state does not block the report: the flood state is still valid, as
    it is for tgsim_gossip_reached."""
    e = Engine(200, lookahead_ns=wl.GOSSIP_MIN_LAT)
    wl.configure_gossip(e, 200)
    e.gossip_init(n_floods=2, degree=4, msg_len=512, start_tick=0)
    W = 2 * wl.gossip_window_ticks(e)  # receipts land inside windows already simulated
    with pytest.raises(EngineError, match="precedes the window"):
        for _ in range(20):
            e.gen_gossip(W)
            e.step(W)
    with pytest.raises(EngineError, match="preceded an earlier window"):
        e.gen_gossip(W)
    s = e.gossip_spread(1000, 8)
    assert (s["reached"] == e.gossip_reached()).all() and s["reached"].sum() > 0
    t = e.gossip_times(0, 200)
    assert ((t != NONE).sum(0) == s["reached"]).all()
    assert (s["hist"].sum(1) == s["reached"]).all()
    e.close()
