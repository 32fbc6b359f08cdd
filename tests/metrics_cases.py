"""The TGSIM_OPT_METRICS cases shared by tests/test_metrics_model.py (the CPU oracle's tables against
ArtifactModel, an independent numpy model of them, and against closed forms) and
tests/test_gpu_metrics_paths.py (the HIP engine's k_metrics_src / k_metrics_dst against the oracle, bit
for bit after every window, on every simulate kernel, emit layout, delivery routine and driver).

A scenario is a generator over any engine-shaped object (engine.CABIEngine): it configures the engine,
then feeds and steps one window at a time and yields after each step: the packets it submitted (host
traffic), or, for a generated window, the packets the engine reports it will simulate where the
library exports `offered` (the oracle does), else None.  Whoever drives the generator reads verdicts,
drain and tables between two yields.  Nothing here imports a GPU library."""
import ipaddress

import numpy as np

import group_cases as gc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

MS = nw.Millisecond
NO_PACKETS = np.zeros(0, dtype=abi.PKT_DTYPE)
TABLES = ("src", "dst", "hist")


# -- comparing tables ------------------------------------------------------------------------------------------
def tables_of(x):
    """Engine.metrics() of an engine, or the dict itself."""
    return x if isinstance(x, dict) else x.metrics()


def _where(key, idx):
    if key == "src":
        return f"instance {idx[0]}, column {idx[1]} ({abi.METRICS_SRC_COLUMNS[idx[1]]})"
    if key == "dst":
        return f"instance {idx[0]}, column {idx[1]} ({('records', 'bytes')[idx[1]]})"
    return f"row {idx[0]} ({('backlog', 'delivered')[idx[0]]}), bin {idx[1]}"


def assert_tables_same(g, c, what=""):
    """`src`, `dst` and `hist` of Engine.metrics() (engines or their tables), bit for bit; a mismatch
    names the table, the first differing instance (or histogram row) and column, and both values."""
    tg, tc = tables_of(g), tables_of(c)
    for key in TABLES:
        a, b = np.asarray(tg[key]), np.asarray(tc[key])
        assert a.shape == b.shape and a.dtype == b.dtype == np.uint64, (what, key, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (f"{what}: table {key}: {len(bad)} words differ, first at {_where(key, bad[0].tolist())}: "
                               f"{a[tuple(bad[0])]} vs {b[tuple(bad[0])]}")


def assert_window_same(g, c, what=""):
    """The window's verdict bytes and drained records, so that a table mismatch can be told from a
    simulation mismatch; returns them."""
    vg, vc = g.verdicts(), c.verdicts()
    assert len(vg) == len(vc) and vg.tobytes() == vc.tobytes(), f"{what}: verdicts differ"
    dg, dc = g.drain(), c.drain()
    assert len(dg) == len(dc) and dg.tobytes() == dc.tobytes(), f"{what}: deliveries differ ({len(dg)} vs {len(dc)})"
    return vc, dc


def merged(tables):
    """The tables of a run's shards, in rank order, as the whole run's: src and dst rows concatenated,
    both histogram rows summed."""
    tables = [tables_of(t) for t in tables]
    return {"src": np.concatenate([t["src"] for t in tables]), "dst": np.concatenate([t["dst"] for t in tables]),
            "hist": np.sum([t["hist"] for t in tables], axis=0, dtype=np.uint64)}


def bin_of(x):
    """include/tgsim.h TGSIM_METRICS_HIST: 0 for none, b for 2^(b-1) <= x < 2^b, the last bin beyond."""
    return min(int(x).bit_length(), abi.METRICS_BINS - 1)


# -- the independent model -------------------------------------------------------------------------------------
class ArtifactModel:
    """The tables of an engine that owns every peer, from what a host sees per window and nothing else:
    the packets offered, their verdict bytes and the records drained after the step.  Columns 0..9 from
    the packets and both verdict nibbles (the high one only where it is not V_NONE); columns 10/11 and
    `dst` from the drained records (on such an engine a step's served records are exactly what it makes
    drainable; records lost in flight are in neither); hist[1] from the window's drained records per
    destination.  The backlog row hist[0] is no function of the artifacts: check() only holds it to one
    entry per instance and step."""

    def __init__(self, n):
        self.n, self.steps = n, 0
        self.src = np.zeros((n, abi.METRICS_SRC_WORDS), dtype=np.uint64)
        self.dst = np.zeros((n, abi.METRICS_DST_WORDS), dtype=np.uint64)
        self.delivered = np.zeros(abi.METRICS_BINS, dtype=np.uint64)

    def fold(self, pkts, verdicts, drained):
        one = np.uint64(1)
        if pkts is not None and len(pkts):
            v = np.asarray(verdicts, dtype=np.uint8)
            assert len(v) == len(pkts), "one verdict byte per offered packet"
            s = pkts["src"].astype(np.int64)
            np.add.at(self.src, (s, 0), one)
            np.add.at(self.src, (s, 1), pkts["len"].astype(np.uint64))
            lo, hi = (v & 15).astype(np.int64), (v >> 4).astype(np.int64)
            np.add.at(self.src, (s, 2 + lo), one)
            clone = hi != abi.V_NONE
            np.add.at(self.src, (s[clone], 2 + hi[clone]), one)
        per_dst = np.zeros(self.n, dtype=np.int64)
        if drained is not None and len(drained):
            s, d = drained["src"].astype(np.int64), drained["dst"].astype(np.int64)
            length = drained["len"].astype(np.uint64)
            np.add.at(self.src, (s, 10), one)
            np.add.at(self.src, (s, 11), length)
            np.add.at(self.dst, (d, 0), one)
            np.add.at(self.dst, (d, 1), length)
            per_dst = np.bincount(d, minlength=self.n)
        np.add.at(self.delivered, [bin_of(x) for x in per_dst], one)
        self.steps += 1
        return self

    def check(self, tables, what=""):
        t = tables_of(tables)
        want = {"src": self.src, "dst": self.dst, "hist": np.stack([t["hist"][0], self.delivered])}
        assert_tables_same(t, want, f"{what} (tables against the artifact model)")
        assert int(t["hist"][0].sum()) == self.n * self.steps, (what, "backlog entries", int(t["hist"][0].sum()))


def assert_stats_sums(tables, stats, what=""):
    """The table sums an engine's own statistics fix: offered, by_verdict, scheduled, bytes_scheduled."""
    src = tables_of(tables)["src"]
    assert int(src[:, 0].sum()) == stats["offered"], (what, "offered")
    for k, name in enumerate(abi.VERDICT_NAMES):
        assert int(src[:, 2 + k].sum()) == stats["by_verdict"][name], (what, name)
    assert int(src[:, 10].sum()) == stats["scheduled"], (what, "scheduled")
    assert int(src[:, 11].sum()) == stats["bytes_scheduled"], (what, "bytes_scheduled")


class Recording:
    """An engine-shaped wrapper for the host-driven loops (workloads.ping_reference, flow_reference):
    drain() closes a window; per window it keeps (packets, verdicts, drained records) and the tables."""

    def __init__(self, inner):
        self._inner, self._pk, self.windows, self.tables = inner, None, [], []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def submit(self, pk):
        assert self._pk is None
        self._pk = np.array(pk, dtype=abi.PKT_DTYPE)
        self._inner.submit(pk)

    def drain(self):
        d = self._inner.drain()
        v = self._inner.verdicts() if self._pk is not None else np.zeros(0, dtype=np.uint8)
        self.windows.append((self._pk if self._pk is not None else NO_PACKETS, v, d))
        self.tables.append(self._inner.metrics())
        self._pk = None
        return d


def deltas(series, key="src"):
    """Per-window differences of a series of tables (the first against zero)."""
    out, prev = [], None
    for t in series:
        a = t[key].astype(np.int64)
        out.append(a if prev is None else a - prev)
        prev = a
    return out


# -- traffic helpers -------------------------------------------------------------------------------------------
def _offered(eng):
    """The generated window the next step will simulate, where the library exports it (the oracle)."""
    if not hasattr(eng._lib, eng._p + "offered"):
        return None
    return gc.offered(eng)


def _sequenced(pk, seq):
    """Per-source running sequence numbers in (src, tick) order, carried in `seq` (updated)."""
    src, n = pk["src"].astype(np.int64), len(seq)
    order = np.lexsort((pk["tick"], src))
    counts = np.bincount(src, minlength=n)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    sq = np.empty(len(pk), dtype=np.uint32)
    sq[order] = np.arange(len(pk)) - starts[src[order]] + seq[src[order]]
    seq += counts.astype(np.uint32)
    pk["seq"] = sq
    return pk


def _submit_step(eng, pk, ticks):
    if len(pk):
        eng.submit(pk)
    eng.step(ticks)
    return pk


# -- A. dense and sparse kernels, mixed senders (the traffic of test_sparse_and_dense_kernels_agree) -----------
A = dict(n=201, kw=dict(queue_limit=300, lookahead_ns=200_000), steps=5, ticks=3000)
# what this traffic can produce: no rules, no disconnects, no external destinations
A_VERDICTS = (abi.V_SCHEDULED, abi.V_LOSS, abi.V_QUEUE_FULL)


def scenario_a(eng):
    n = A["n"]
    rng = np.random.default_rng(41)
    shapes = wl.storm_shapes(n, 3)
    for i, s in enumerate(shapes):
        if i % 7 == 0:
            s.DuplicateCorr, s.CorruptCorr = 30.0, 20.0
        s.Latency = int(rng.integers(0, 8)) * MS
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=s))
    seq = np.zeros(n, dtype=np.uint32)
    for _ in range(A["steps"]):
        heavy = rng.random(n) < 0.1  # a few heavy senders, many light ones
        m = 20_000
        src = np.where(rng.random(m) < 0.7, rng.choice(np.nonzero(heavy)[0], m), rng.integers(0, n, m))
        pk = np.zeros(m, dtype=abi.PKT_DTYPE)
        pk["src"] = src
        pk["dst"] = (src + 1 + rng.integers(0, n - 1, m)) % n
        pk["len"] = rng.integers(40, 1500, m)
        pk["tick"] = rng.integers(0, A["ticks"], m)
        yield _submit_step(eng, _sequenced(pk, seq), A["ticks"])


# -- B. compact emit layout and its pool (the traffic of test_compact_emit_layout) -----------------------------
B = dict(n=80, kw=dict(queue_limit=1024), steps=14, ticks=2000)


def scenario_b(eng):
    n = B["n"]
    rng = np.random.default_rng(31)
    for i in range(n):
        # latency longer than a window: old queue items are served next to a few new ones; every 8th
        # source offers > 64 packets (k_sim_multi), every 10th + 3 duplicates (k_sim_list)
        s = nw.LinkShape(Latency=int(rng.integers(3, 9)) * MS, Bandwidth=1 << 30, Loss=1.0,
                         Duplicate=3.0 if i % 10 == 3 else 0.0)
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=s))
    seq = np.zeros(n, dtype=np.uint32)
    for step in range(B["steps"]):
        burst = step % 4 == 0  # bursts, then quiet windows that serve the queued items
        per = np.where(np.arange(n) % 8 == 0, rng.integers(100, 200, n), rng.integers(20, 60, n)) if burst \
            else rng.integers(0, 4, n)
        src = np.repeat(np.arange(n), per)
        m = len(src)
        pk = np.zeros(m, dtype=abi.PKT_DTYPE)
        pk["src"] = src
        pk["dst"] = (src + 1 + rng.integers(0, n - 1, m)) % n
        pk["len"] = rng.integers(40, 1500, m)
        pk["tick"] = rng.integers(0, B["ticks"], m)
        yield _submit_step(eng, _sequenced(pk, seq), B["ticks"])


def pool_reached(series, reserve):
    """Some source in some window served more than 2 x its offered packets + reserve records: the
    condition under which k_metrics_src reads that source's pool index."""
    return any(((d[:, 10] > 2 * d[:, 0] + reserve)).any() for d in deltas(series))


# -- C. parked queues, closed form -----------------------------------------------------------------------------
C = dict(kw=dict(queue_limit=1024), ticks=1000, latency_ns=50 * MS, length=100, idle=60)
C_VARIANTS = {  # variant -> (peers, packets source i offers at tick 0)
    "ramp": (300, lambda i: i),            # bins 0..9: [1, 1, 2, 4, 8, 16, 32, 64, 128, 44]
    "ramp64": (300, lambda i: i % 64),     # every source below 64 packets: a sparse window by the engine's own rule
    "deep": (101, lambda i: 600 + 5 * i),  # 600..1,100 against a netem limit of 1,024: bins 10 and 11, QUEUE_FULL
}


def c_offers(variant):
    n, f = C_VARIANTS[variant]
    return n, f(np.arange(n, dtype=np.int64))


def c_expected(variant):
    """(n, offered per source, queued per source, backlog bins after the first step)."""
    n, k = c_offers(variant)
    queued = np.minimum(k, C["kw"]["queue_limit"])
    bins = np.bincount([bin_of(q) for q in queued], minlength=abi.METRICS_BINS).astype(np.uint64)
    return n, k, queued, bins


def scenario_c(variant):
    def run(eng):
        n, k = c_offers(variant)
        eng.configure_batch(np.arange(n), nw.configs_array(np.full(n, C["latency_ns"])))  # Bandwidth = 0
        src = np.repeat(np.arange(n), k)
        pk = np.zeros(len(src), dtype=abi.PKT_DTYPE)
        pk["src"], pk["dst"], pk["len"], pk["tick"] = src, (src + 1) % n, C["length"], 0
        pk["seq"] = np.arange(len(src)) - np.repeat(np.cumsum(k) - k, k)
        yield _submit_step(eng, pk, C["ticks"])
        for _ in range(C["idle"]):
            yield _submit_step(eng, NO_PACKETS, C["ticks"])
    return run


# -- D. gossip: sparse generated windows -----------------------------------------------------------------------
D = dict(n=600, kw=dict(lookahead_ns=wl.GOSSIP_MIN_LAT), floods=8, degree=8, windows=25)


def scenario_d(eng, n=D["n"], step=None):
    step = eng.step if step is None else step
    wl.configure_gossip(eng, n)
    eng.gossip_init(n_floods=D["floods"], degree=D["degree"], msg_len=1024, start_gap_ticks=0, start_tick=0)
    w = wl.gossip_window_ticks(eng)
    for _ in range(D["windows"]):
        eng.gen_gossip(w)
        pk = _offered(eng)
        step(w)
        yield pk


# -- E, F. the ping mesh and the flow driver armed -------------------------------------------------------------
# Links for the closed loops: latencies from {5, 7, 12} ms, jitter of 0.2 to 1 ms on EVERY peer (the
# engines leave the order of two originals of one source with equal eligibility time and equal seq open;
# with jitter everywhere the responder's draw tells such replies apart, see ping_cases.mesh_shapes), loss
# 4 %, duplicate 2 %, corrupt 1 %.  The minimum netem delay is 5 ms - 1 ms = the 4 ms lookahead.
LOOP = dict(kw=dict(lookahead_ns=4 * MS), window=4_000)


def configure_loop(eng, n, seed):
    rng = np.random.default_rng(seed)
    lat = rng.choice(np.array([5, 7, 12]) * MS, n, p=[0.6, 0.2, 0.2])
    jit = rng.integers(200_000, MS + 1, n)
    pct = (lambda v: np.full(n, v, dtype=np.float32))
    eng.configure_batch(np.arange(n), nw.configs_array(lat, jitter_ns=jit, loss=pct(4.0), duplicate=pct(2.0), corrupt=pct(1.0)))


E = dict(n=200, fanout=4, windows=12, ping=dict(count=4, interval_ticks=3_000, length=200, bin_ns=2 * MS, n_bins=48))


def e_setup(eng):
    configure_loop(eng, E["n"], 17)
    return dict(E["ping"], start_tick=eng.stats()["now_tick"]), wl.ping_targets_mesh(E["n"], E["fanout"])


F = dict(n=64, per_source=2, n_seg=16, windows=40, cut=(3, 0),
         flow=dict(seg_len=1000, ack_len=64, window=8, rto_ticks=30_000, max_attempts=16, bin_ns=20 * MS, n_bins=64),
         fb=dict(fail_mask=abi.FLOW_FB_REFUSALS))


def f_setup(eng):
    """The loop links; peer 3 drops what it sends towards its first flow's destination (a refusal the
    verdict feedback fails that flow with).  Returns the flow table."""
    configure_loop(eng, F["n"], 19)
    flows = wl.flow_table_mesh(F["n"], F["per_source"], F["n_seg"], start_tick=eng.stats()["now_tick"])
    s = F["cut"][0]
    dst = int(flows["dst"][flows["src"] == s][F["cut"][1]])
    eng.configure(s, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=5 * MS, Jitter=MS // 2),
                               Rules=[nw.LinkRule(Subnet=(str(ipaddress.IPv4Address(wl.peer_ip(dst))), 32),
                                                  LinkShape=nw.LinkShape(Filter=nw.FilterAction.Drop))]))
    return flows


# -- G. reconfiguration on the group tests' base case ----------------------------------------------------------
def _g_plain(n):
    """The peers the base case leaves plain: no rule of their own, not disconnected, not AllowAll."""
    region = wl.splitbrain_regions(n)
    return [i for i in range(21, n) if region[i] != wl.REGION_A]


def g_gone(n=gc.N):
    """The peer that is disconnected: the plain peer with the longest latency, whose own queue holds
    everything it has been offered so far."""
    lat = wl.storm_shape_arrays(n)["latency_ns"]
    return max(_g_plain(n), key=lambda i: int(lat[i]))


G = dict(n=gc.N, kw={}, gone=g_gone(), at=2, back=3)


def g_reshaped(n=gc.N):
    """The peer that is reshaped to a much faster link: the first plain 1 Mbit/s peer."""
    bw = wl.storm_shape_arrays(n)["bandwidth_bps"]
    return next(i for i in _g_plain(n) if bw[i] == 1_000_000 and i != g_gone(n))


def scenario_g(eng):
    """group_cases.configure_base and its windows.  Ahead of window 2 peer G["gone"] is disconnected (its
    own queue is flushed, what waits towards it is lost in flight) and a 1 Mbit/s peer is reshaped to an
    unlimited link (what it has served leaves its HTB at once: the departure ring empties); ahead of window 3 that peer is connected again."""
    n = G["n"]
    gc.configure_base(eng, n)
    fast, shapes = g_reshaped(n), wl.storm_shapes(n)
    for w, (pk, ticks) in enumerate(gc.base_windows(n)):
        if w == G["at"]:
            eng.configure(G["gone"], nw.Config(Network="default", Enable=False))
            s = shapes[fast]
            s.Bandwidth = 0
            eng.configure(fast, nw.Config(Network="default", Enable=True, Default=s))
        if w == G["back"]:
            eng.configure(G["gone"], nw.Config(Network="default", Enable=True, Default=shapes[G["gone"]]))
        yield _submit_step(eng, pk if pk is not None else NO_PACKETS, ticks)


# -- H, I. generated storm windows -----------------------------------------------------------------------------
H = dict(n=240, lam=0.5, ticks=1000, windows=4)
I = dict(n=128, lam=0.1, ticks=1000, windows=6)


def scenario_storm(n, lam, ticks, windows, step=None):
    def run(eng):
        do = eng.step if step is None else (lambda t: step(eng, t))
        wl.configure_storm(eng, n)
        for _ in range(windows):
            eng.gen_storm(lam, ticks)
            pk = _offered(eng)
            do(ticks)
            yield pk
    return run


# scenario name -> (peers, engine keywords, generator); every one runs on a single engine that owns every peer
SCENARIOS = {
    "A": (A["n"], A["kw"], scenario_a),
    "B": (B["n"], B["kw"], scenario_b),
    **{f"C-{v}": (C_VARIANTS[v][0], C["kw"], scenario_c(v)) for v in C_VARIANTS},
    "D": (D["n"], D["kw"], scenario_d),
    "G": (G["n"], G["kw"], scenario_g),
    "H": (H["n"], {}, scenario_storm(H["n"], H["lam"], H["ticks"], H["windows"])),
    "I": (I["n"], {}, scenario_storm(I["n"], I["lam"], I["ticks"], I["windows"])),
}


# -- the C ABI's edges (tgsim_metrics) -------------------------------------------------------------------------
def check_abi_edges(with_flag, without_flag):
    """On an engine created with TGSIM_OPT_METRICS that has stepped, and on one created without."""
    import errno

    e, fn = with_flag, with_flag._fn("metrics")
    full = e.metrics()["src"].ravel()
    assert len(full) == e.n_peers * abi.METRICS_SRC_WORDS and full.sum() > 0
    sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
    for cap in (1, 5, len(full) - 1):  # a cap below the table: the prefix, and still the full word count
        out = np.full(len(full), sentinel, dtype=np.uint64)
        assert fn(e._h, abi.METRICS_SRC, out.ctypes.data, cap) == len(full)
        assert (out[:cap] == full[:cap]).all() and (out[cap:] == sentinel).all(), cap
    out = np.full(4, sentinel, dtype=np.uint64)
    assert fn(e._h, abi.METRICS_HIST, out.ctypes.data, 4) == 2 * abi.METRICS_BINS
    assert (out == e.metrics()["hist"].ravel()[:4]).all()
    assert fn(e._h, 3, None, 0) == -errno.EINVAL
    assert fn(e._h, 3, out.ctypes.data, 4) == -errno.EINVAL
    assert without_flag._fn("metrics")(without_flag._h, abi.METRICS_SRC, None, 0) == -errno.ENODATA
