"""The per-group traffic matrix reduced on the device (tgsim_groups_init / tgsim_group_matrix) against
the host model (workloads.GroupMatrix) folded over the CPU oracle's offered packets, verdict bytes and
drained records: exact, word for word, after every window.  The cases are in tests/group_cases.py;
that the base case exercises every verdict, clones and corrupted copies is asserted on the oracle in
tests/test_group_model.py and again here."""
import errno

import numpy as np
import pytest

import group_cases as gc
import ping_cases as pc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl
from testground_amd.engine import CABIEngine, Engine, EngineError

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None


@pytest.fixture(scope="module")
def base(oracle_lib):
    """The base case's model over the oracle, once: the matrix after each of the four windows and
    every window's (packets, verdicts, drained records)."""
    cpu = CABIEngine(oracle_lib, "tgo_", gc.N)
    gc.configure_base(cpu)
    group_of, g = gc.base_groups()
    windows, art = gc.base_windows(), []
    series = gc.model_series(cpu, group_of, g, windows, artifacts=art)
    t = gc.class_totals(series[-1])
    assert all(t[k] > 0 for k in abi.VERDICT_NAMES + ["clones_delivered", "corrupt_delivered"]), t
    return dict(group_of=group_of, g=g, windows=windows, series=series, art=art)


def armed_base(base, **kw):
    eng = Engine(gc.N, **kw)
    gc.configure_base(eng)
    eng.groups_init(base["group_of"], base["g"])
    return eng


# -- 1. base case parity ---------------------------------------------------------------------------------
def test_base_parity(base):
    dev = gc.device_series(armed_base(base), base["windows"])
    assert dev[0].shape == (3, 4, abi.GROUP_WORDS)
    for w, (d, m) in enumerate(zip(dev, base["series"])):
        gc.assert_same(d, m, f"after window {w}")


def test_base_parity_intervals(base):
    """reset=True after every window: each read is the model's difference, the reads sum to the total."""
    dev = gc.device_series(armed_base(base), base["windows"], reset=True)
    prev = np.zeros_like(base["series"][0])
    for w, (d, m) in enumerate(zip(dev, base["series"])):
        gc.assert_same(d, m - prev, f"interval {w}")
        prev = m
    gc.assert_same(np.sum(dev, axis=0, dtype=np.uint64), base["series"][-1], "sum of the intervals")


# -- 2. layouts ------------------------------------------------------------------------------------------
def _random37(n):
    g = np.random.default_rng(3).integers(0, 37, n)
    g[:37] = np.arange(37)  # every group occurs
    return g.astype(np.uint16)


# (peers, groups, assignment, packets per window): the row/column form (more than 16 groups) with a
# wavefront per source (dense windows) and with a lane per source (fewer than 16 packets per source)
LAYOUTS = {
    "contiguous64": (192, 64, lambda n: (np.arange(n) // 3).astype(np.uint16), 20_000),
    "contiguous64_sparse": (192, 64, lambda n: (np.arange(n) // 3).astype(np.uint16), 1_000),
    "one_group": (96, 1, lambda n: np.zeros(n, dtype=np.uint16), 20_000),
    "random37": (333, 37, _random37, 20_000),
    "random37_sparse": (333, 37, _random37, 2_000),
    "sixteen_interleaved": (100, 16, lambda n: (np.arange(n) % 16).astype(np.uint16), 20_000),
    "seventeen_interleaved": (100, 17, lambda n: (np.arange(n) % 17).astype(np.uint16), 20_000),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_layouts(make_oracle, layout):
    n, g, assign, per_window = LAYOUTS[layout]
    group_of = assign(n)
    assert group_of.max() == g - 1
    windows = gc.base_windows(n, n_windows=2, per_window=per_window)
    cpu, eng = make_oracle(n), Engine(n)
    for e in (cpu, eng):
        gc.configure_plain(e, n)
    eng.groups_init(group_of, g)
    ref = gc.model_series(cpu, group_of, g, windows)
    assert ref[-1][:, :, 10].sum() > 0 and ref[-1][:, g, 0].sum() > 0
    for w, (d, m) in enumerate(zip(gc.device_series(eng, windows), ref)):
        assert d.shape == (g, g + 1, abi.GROUP_WORDS)
        gc.assert_same(d, m, f"{layout}, after window {w}")


# -- 3. tiles --------------------------------------------------------------------------------------------
def test_hot_destination(make_oracle, base):
    """30 % of the packets go to peer 0: one destination segment passes 1,024 records in a window; every
    source offers more than 64 packets a window."""
    windows, art = gc.base_windows(n_windows=2, hot=0.3), []
    cpu = make_oracle(gc.N)
    gc.configure_base(cpu)
    ref = gc.model_series(cpu, base["group_of"], base["g"], windows, artifacts=art)
    assert max(int((d["dst"] == 0).sum()) for _, _, d in art) > 1024
    assert min(np.bincount(windows[0][0]["src"], minlength=gc.N)) > 64
    for w, (d, m) in enumerate(zip(gc.device_series(armed_base(base), windows), ref)):
        gc.assert_same(d, m, f"after window {w}")


# -- 4. partial-sum width --------------------------------------------------------------------------------
def test_bytes_beyond_32_bits(make_oracle):
    """One source offers 70,000 packets of 65,535 B in one window to one group: 4.59e9 offered bytes."""
    n, k, ticks = 4, 70_000, 60_000
    group_of = np.array([0, 1, 1, 0], dtype=np.uint16)
    pk = np.zeros(k, dtype=abi.PKT_DTYPE)
    pk["src"], pk["dst"], pk["len"] = 0, 1 + (np.arange(k) & 1), 65_535
    pk["seq"], pk["tick"] = np.arange(k), np.arange(k) * ticks // k
    cpu, eng = make_oracle(n), Engine(n)
    for e in (cpu, eng):
        e.configure_batch(np.arange(n), nw.configs_array(np.full(n, 100 * nw.Millisecond)))
    eng.groups_init(group_of, 2)
    ref = gc.model_series(cpu, group_of, 2, [(pk, ticks)])[0]
    dev = gc.device_series(eng, [(pk, ticks)])[0]
    assert int(ref[0, 1, 1]) == k * 65_535 > 1 << 32 and int(ref[0, 1, 0]) == k
    assert int(ref[0, 1, 2 + abi.V_QUEUE_FULL]) == k - 1000  # the netem limit
    for word in (0, 1, 2 + abi.V_QUEUE_FULL):
        assert dev[0, 1, word] == ref[0, 1, word], word
    gc.assert_same(dev, ref, "one window")


# -- 5. generated traffic, dense and sparse (bucketed) windows -----------------------------------------------
def test_generated_windows_keep_the_bucket_path(make_oracle):
    """gen_storm windows of ~4 packets per source (the sparse kernels, whose records go straight into
    the destinations' buckets) and of ~100 (k_sim): parity through tgo_offered, and the armed engine
    takes the sparse kernels and the bucket path exactly where an unarmed one does."""
    n, window = 600, 2000
    group_of = (np.arange(n) % 3).astype(np.uint16)
    sparse = lambda e: int(e._fn("debug_sparse_windows")(e._h))  # noqa: E731
    cpu, eng, plain = make_oracle(n), Engine(n), Engine(n)
    for e in (cpu, eng, plain):
        wl.configure_gossip(e, n)  # L~U[5,50] ms, loss 1 %: open FIFO queues
    eng.groups_init(group_of, 3)
    gm = wl.GroupMatrix(group_of, 3)
    plan = [(0.002, window)] * 6 + [(0.05, window)] + [(0.002, window)] * 2 + [(0.0, 60_000)]
    for w, (lam, ticks) in enumerate(plan):
        sp0, bk0 = sparse(eng), eng.bucket_records()
        for e in (cpu, eng, plain):
            if lam:
                e.gen_storm(lam, ticks)
        gc.fold_step(gm, cpu, ticks)
        for e in (eng, plain):
            e.step(ticks)
            e.drain()
        gc.assert_same(eng.group_matrix(), gm.m, f"after window {w} (lambda {lam})")
        assert (sparse(eng), eng.bucket_records()) == (sparse(plain), plain.bucket_records()), w
        if w == 5:  # sparse windows so far, the last ones with deliveries: both counters advanced while armed
            assert sparse(eng) == sp0 + 1 == 6 and eng.bucket_records() > bk0 > 0, (sp0, bk0)
        if lam == 0.05:
            assert sparse(eng) == sp0
    assert gm.m[:, :, 10].sum() > 0 and (gm.m[:, :, 2] == gm.m[:, :, 10]).all()


# -- 6. drivers armed ----------------------------------------------------------------------------------------
def test_gossip_armed(make_oracle):
    n, floods, degree = 200, 4, 4
    group_of = (np.arange(n) * 5 // n).astype(np.uint16)
    kw = dict(lookahead_ns=wl.GOSSIP_MIN_LAT)
    cpu, eng, plain = make_oracle(n, **kw), Engine(n, **kw), Engine(n, **kw)
    for e in (cpu, eng, plain):
        wl.configure_gossip(e, n)
        e.gossip_init(n_floods=floods, degree=degree, msg_len=1024, start_gap_ticks=0, start_tick=0)
    eng.groups_init(group_of, 5)
    gm = wl.GroupMatrix(group_of, 5)
    W = wl.gossip_window_ticks(cpu)
    for w in range(20):
        cpu.gen_gossip(W)
        gc.fold_step(gm, cpu, W)
        for e in (eng, plain):
            e.gen_gossip(W)
            e.step(W)
            e.drain()
        gc.assert_same(eng.group_matrix(), gm.m, f"after window {w}")
    assert gm.m[:, :, 10].sum() > floods * n // 2 and gm.m[:, :, 2 + abi.V_LOSS].sum() > 0
    # the gossip reports do not change with the matrix armed
    assert (eng.gossip_reached() == cpu.gossip_reached()).all()
    assert eng.bucket_records() == plain.bucket_records() > 0  # armed, the sparse windows keep their buckets
    a, b = eng.gossip_spread(1000, 16), plain.gossip_spread(1000, 16)
    for key in wl.SPREAD_KEYS:
        assert (a[key] == b[key]).all(), key


class _Folding:
    """An engine-shaped wrapper that folds every window it is driven through into a GroupMatrix (the
    window's packets are the array submitted for it; drain() closes the window)."""

    def __init__(self, inner, gm):
        self._inner, self._gm, self._pk = inner, gm, None

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def submit(self, pk):
        assert self._pk is None
        self._pk = np.array(pk, dtype=abi.PKT_DTYPE)
        self._inner.submit(pk)

    def drain(self):
        d = self._inner.drain()
        self._gm.fold(self._pk, self._inner.verdicts() if self._pk is not None else None, d)
        self._pk = None
        return d


def test_ping_mesh_armed(make_oracle):
    n, kw = pc.MESH["n"], dict(lookahead_ns=pc.MESH["lookahead_ns"])
    group_of = (np.arange(n) % 4).astype(np.uint16)
    gm = wl.GroupMatrix(group_of, 4)
    snaps = {"ref": [], "dev": []}
    ref = pc.run_mesh(_Folding(make_oracle(n, **kw), gm), device=False, ticks=60_000,
                      before=lambda w: snaps["ref"].append(gm.m.copy()))
    eng = Engine(n, **kw)
    eng.groups_init(group_of, 4)
    dev = pc.run_mesh(eng, device=True, ticks=60_000, before=lambda w: snaps["dev"].append(eng.group_matrix()))
    pc.assert_same_run(dev, ref)  # the ping reports and every window are what they are unarmed
    assert len(snaps["dev"]) == len(snaps["ref"]) == 15
    for w, (d, m) in enumerate(zip(snaps["dev"], snaps["ref"])):
        gc.assert_same(d, m, f"before window {w}")
    gc.assert_same(eng.group_matrix(), gm.m, "end of run")
    assert gm.m[:, :, 12].sum() > 0 and gm.m[:, :, 13].sum() > 0 and gm.m[:, :, 2 + abi.V_LOSS].sum() > 0


# -- 7. shards -----------------------------------------------------------------------------------------------
def _sharded_step(shards, bounds, ticks):
    """step_sim on every shard, regroup through device buffers, deliver (one GPU, no collective)."""
    outs = []
    torch.cuda.current_stream().synchronize()
    for s in shards:
        cap = max(1, s.sim_capacity())
        buf = torch.empty(cap * 24, dtype=torch.uint8, device="cuda")
        outs.append((buf, s.step_sim(ticks, bounds, buf.data_ptr(), cap)))
    for k, s in enumerate(shards):
        inbound = torch.cat([buf[int(cnt[:k].sum()) * 24: int(cnt[:k + 1].sum()) * 24] for buf, cnt in outs])
        torch.cuda.current_stream().synchronize()  # torch.cat ran on torch's stream
        s.deliver(inbound.data_ptr(), inbound.numel() // 24)


def test_three_shards(base):
    bounds = [0, 20, 71, gc.N]
    shards = [Engine(gc.N, shard=(lo, hi)) for lo, hi in zip(bounds, bounds[1:])]
    for s in shards:
        gc.configure_base(s)
        s.groups_init(base["group_of"], base["g"])
    single = armed_base(base)
    own = [wl.GroupMatrix(base["group_of"], base["g"]) for _ in shards]  # what each shard must hold
    for w, ((pk, ticks), (apk, v, d)) in enumerate(zip(base["windows"], base["art"])):
        for (lo, hi), s, gm in zip(zip(bounds, bounds[1:]), shards, own):
            sel = (apk["src"] >= lo) & (apk["src"] < hi)
            if sel.any():
                s.submit(apk[sel])
            gm.fold(apk[sel], v[sel], d[(d["dst"] >= lo) & (d["dst"] < hi)])
        _sharded_step(shards, bounds, ticks)
        if pk is not None:
            single.submit(pk)
        single.step(ticks)
        single.drain()
        ms = [s.group_matrix() for s in shards]
        for k, (m, gm) in enumerate(zip(ms, own)):
            s_ = shards[k].drain()
            assert len(s_) == int(((d["dst"] >= bounds[k]) & (d["dst"] < bounds[k + 1])).sum())
            gc.assert_same(m, gm.m, f"shard {k} after window {w}")
        merged = wl.merge_group_matrices(ms)
        gc.assert_same(merged, base["series"][w], f"sum of the shards after window {w}")
        gc.assert_same(single.group_matrix(), merged, f"single engine after window {w}")
    # shard 0 owns peers 0..19 of every region; a shard of one region's peers has only that row
    one = Engine(gc.N, shard=(2, 3))
    gc.configure_base(one)
    one.groups_init(base["group_of"], base["g"])
    pk = base["windows"][0][0]
    one.submit(pk[pk["src"] == 2])
    buf = torch.empty(max(1, one.sim_capacity()) * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    one.step_sim(gc.WINDOW, [0, gc.N], buf.data_ptr(), buf.numel() // 24)
    m = one.group_matrix()
    row = int(base["group_of"][2])
    assert m[row, :, :10].sum() > 0 and np.delete(m, row, axis=0)[:, :, :10].sum() == 0


# -- 8. flags ------------------------------------------------------------------------------------------------
def test_discard_deliveries(base):
    eng = armed_base(base, flags=abi.OPT_DISCARD_DELIVERIES)
    for w, (d, m) in enumerate(zip(gc.device_series(eng, base["windows"]), base["series"])):
        gc.assert_same(d, m, f"after window {w}")
    assert eng.pending() == 0


def test_with_metrics(base):
    eng = armed_base(base, flags=abi.OPT_METRICS)
    for w, (d, m) in enumerate(zip(gc.device_series(eng, base["windows"]), base["series"])):
        gc.assert_same(d, m, f"after window {w}")
    m, g, group_of = base["series"][-1], base["g"], base["group_of"].astype(np.int64)
    tab = eng.metrics()
    rows, cols = np.zeros((g, 10), dtype=np.uint64), np.zeros((g, 2), dtype=np.uint64)
    np.add.at(rows, group_of, tab["src"][:, :10])
    np.add.at(cols, group_of, tab["dst"])
    assert (m[:, :, :10].sum(axis=1, dtype=np.uint64) == rows).all()
    assert (m[:, :g, 10:12].sum(axis=0, dtype=np.uint64) == cols).all()


# -- 9. reconfiguration --------------------------------------------------------------------------------------
def test_destination_disconnected(make_oracle, base):
    """Peer 20 is disconnected between windows 1 and 2: what is in flight towards it is purged, so its
    column ends with fewer records delivered than scheduled."""
    def before(eng, w):
        if w == 2:
            eng.configure(20, nw.Config(Network="default", Enable=False))

    cpu = make_oracle(gc.N)
    gc.configure_base(cpu)
    ref = gc.model_series(cpu, base["group_of"], base["g"], base["windows"], before=before)
    assert cpu.stats()["lost_in_flight"] > 0
    col = int(base["group_of"][20])
    assert ref[-1][:, col, 10].sum() < ref[-1][:, col, 2].sum()
    assert all((ref[-1][:, c, 10] == ref[-1][:, c, 2]).all() for c in range(base["g"]) if c != col)
    for w, (d, m) in enumerate(zip(gc.device_series(armed_base(base), base["windows"], before=before), ref)):
        gc.assert_same(d, m, f"after window {w}")


# -- 10. fusing ----------------------------------------------------------------------------------------------
def test_armed_windows_are_not_fused(make_oracle):
    n, window, lam = 256, 2000, 0.05
    group_of = (np.arange(n) % 3).astype(np.uint16)
    fused = lambda e: int(e._fn("debug_fused_windows")(e._h))  # noqa: E731
    cpu, a, b = make_oracle(n), Engine(n, flags=abi.OPT_DISCARD_DELIVERIES), Engine(n, flags=abi.OPT_DISCARD_DELIVERIES)
    for e in (cpu, a, b):
        wl.configure_storm(e, n)
    gm = wl.GroupMatrix(group_of, 3)
    for e in (a, b):
        e.groups_init(group_of, 3)
    for _ in range(8):
        a.gen_storm(lam, window)
    a.step_n(window, 8)
    assert fused(a) == 0
    for _ in range(8):
        b.gen_storm(lam, window)
        b.step(window)
        cpu.gen_storm(lam, window)
        gc.fold_step(gm, cpu, window)
    gc.assert_same(a.group_matrix(), b.group_matrix(), "step_n against eight steps")
    gc.assert_same(a.group_matrix(), gm.m, "step_n against the model")
    a.groups_init(None)
    for _ in range(8):
        a.gen_storm(lam, window)
    a.step_n(window, 8)
    assert fused(a) == 8
    assert a.stats()["offered"] > 0


# -- 11. arming rules ----------------------------------------------------------------------------------------
def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


def test_arming_rules(make_oracle):
    n = 8
    g = np.array([0, 1, 2, 0, 1, 2, 0, 1], dtype=np.uint16)
    _raises(errno.ENOSYS, "tgo_groups_init is not exported", make_oracle(n).groups_init, g, 3)
    _raises(errno.ENOSYS, "tgo_group_matrix is not exported", make_oracle(n).group_matrix)
    eng = Engine(n)
    for i in range(n):
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=nw.Millisecond)))
    _raises(errno.EINVAL, "not armed", eng.group_matrix)
    _raises(errno.EINVAL, "n_groups 0", eng.groups_init, g, 0)
    _raises(errno.EINVAL, "n_groups 65", eng.groups_init, g, 65)
    _raises(errno.EINVAL, "no group table for n_groups 3", eng.groups_init, None, 3)
    _raises(errno.EINVAL, r"group_of\[2\] = 2 .*peer 2", eng.groups_init, g, 2)
    far = g.copy()
    far[5] = 64
    _raises(errno.EINVAL, r"group_of\[5\] = 64 .*peer 5", eng.groups_init, far, 64)
    _raises(errno.EINVAL, "not armed", eng.group_matrix)  # a refused call arms nothing
    pkt = np.array([(0, 1, 0, 64, 0)], dtype=abi.PKT_DTYPE)
    eng.submit(pkt)
    _raises(errno.EBUSY, "host packets", eng.groups_init, g, 3)
    eng.step(10)
    eng.gen_storm(0.01, 10)
    _raises(errno.EBUSY, "generated windows", eng.groups_init, g, 3)
    eng.step(10)
    buf = torch.empty(max(1, eng.sim_capacity()) * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    eng.step_sim_launch(10, [0, n], buf.data_ptr(), buf.numel() // 24)
    _raises(errno.EBUSY, "launched steps", eng.groups_init, g, 3)
    eng.step_sim_finish()
    eng.step(5_000)  # (the packet of tick 0 is delivered unarmed)
    eng.drain()
    # armed: every source of traffic stays usable; too small a buffer is refused
    eng.groups_init(g, 3)
    assert eng.group_matrix().shape == (3, 4, 14) and eng.group_matrix().sum() == 0
    out = np.zeros(3 * 4 * 14 - 1, dtype=np.uint64)
    assert eng._fn("group_matrix")(eng._h, out.ctypes.data, len(out), 0) == -errno.ENOSPC
    eng.submit(pkt)
    eng.step(5_000)
    m = eng.group_matrix()
    assert m[0, 1].tolist() == [1, 64, 1, 0, 0, 0, 0, 0, 0, 0, 1, 64, 0, 0] and m.sum() == m[0, 1].sum()
    # re-arming replaces the table and zeroes; disarming frees
    eng.groups_init(np.zeros(n, dtype=np.uint16))
    assert eng.group_matrix().shape == (1, 2, 14) and eng.group_matrix().sum() == 0
    eng.groups_init(None)
    _raises(errno.EINVAL, "not armed", eng.group_matrix)
    eng.groups_init(None)  # (disarming an unarmed engine is not an error)
