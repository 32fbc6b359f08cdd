"""The ping mesh cases shared by tests/test_ping_model.py (the host model over the CPU oracle, against
the reference's known answers) and tests/test_gpu_ping.py (the HIP engine's device loop against that
model, bit for bit).  A case configures an engine-shaped object and runs the loop on it: on the
device (Engine.ping_init + workloads.ping_run) or from the host (workloads.ping_reference)."""
import ipaddress

import numpy as np

from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

MS = nw.Millisecond


def drive(eng, device, ping, targets, n_windows, window, probe_at=(), before=None):
    """One armed run of n_windows on `eng`; the same result keys either way."""
    if not device:
        return wl.ping_reference(eng, ping, targets, n_windows, window, probe_at=probe_at, before=before)
    eng.ping_init(targets, **ping)
    out = wl.ping_run(eng, n_windows, window, collect=True, probe_at=probe_at, before=before)
    out["pairs"], out["summary"] = eng.ping_pairs(), eng.ping_report()
    return out


def assert_same_report(dev, ref, what=""):
    (dp, ds), (rp, rs) = dev, ref
    for key in abi.PING_PAIR_DTYPE.names:
        assert (dp[key] == rp[key]).all(), (what, key)
    for key in abi.PING_SUMMARY_FIELDS:
        assert ds[key] == rs[key], (what, key, ds[key], rs[key])
    assert (np.asarray(ds["hist"]) == np.asarray(rs["hist"])).all(), (what, "hist")


def assert_same_run(dev, ref, windows=True):
    """Verdict bytes and drained records of every window, the reports at every probe and at the end."""
    if windows:
        assert len(dev["windows"]) == len(ref["windows"])
        for w, ((dv, dd), (rv, rd)) in enumerate(zip(dev["windows"], ref["windows"])):
            assert dv.tobytes() == rv.tobytes(), f"verdicts of window {w}"
            assert dd.tobytes() == rd.tobytes(), f"deliveries of window {w}"
    assert sorted(dev["probes"]) == sorted(ref["probes"])
    for w in ref["probes"]:
        assert_same_report(dev["probes"][w], ref["probes"][w], f"probe after window {w}")
    assert_same_report((dev["pairs"], dev["summary"]), (ref["pairs"], ref["summary"]), "end of run")


# -- 1. ping-pong (plans/network/pingpong.go:116-195) ---------------------------------------------
PINGPONG = dict(n=2, lookahead_ns=10 * MS, window=10_000)
PINGPONG_TARGETS = np.array([[1], [0]], dtype=np.uint32)


def run_pingpong(eng, device):
    """100 ms, three probes 50 ms apart until every reply is in; then reshaped to 10 ms and armed
    again.  Returns the two phases' results."""
    out = []
    for lat, n_windows, bin_ns in ((100 * MS, 35, 5 * MS), (10 * MS, 15, MS)):
        for i in (0, 1):
            eng.configure(i, wl.pingpong_config(lat, "network-configured" if lat == 100 * MS else "latency-reduced"))
        ping = dict(count=3, interval_ticks=50_000, length=66, start_tick=eng.stats()["now_tick"], bin_ns=bin_ns,
                    n_bins=64)
        out.append(drive(eng, device, ping, PINGPONG_TARGETS, n_windows, PINGPONG["window"],
                         probe_at=(0, n_windows // 2)))
    return out


# -- 2. verify (plans/verify/main.go:43-117) --------------------------------------------------------
VERIFY = dict(n=4, lookahead_ns=5 * MS, window=5_000)


def verify_targets(n=4):
    t = np.empty((n, 2), dtype=np.uint32)
    t[:, 0] = (np.arange(n) + 1) % n
    t[:, 1] = abi.EXTERNAL
    return t


def run_verify(eng, device, allow_all):
    n = VERIFY["n"]
    policy = nw.RoutingPolicyType.AllowAll if allow_all else nw.RoutingPolicyType.DenyAll
    for i in range(n):
        cfg = nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=5 * MS))
        if allow_all:
            cfg.RoutingPolicy = policy
        eng.configure(i, cfg)
    ping = dict(count=3, interval_ticks=2_000, length=64, start_tick=eng.stats()["now_tick"], bin_ns=MS, n_bins=16)
    return drive(eng, device, ping, verify_targets(n), 5, VERIFY["window"], probe_at=(0, 1))


# -- 3. splitbrain (plans/splitbrain/main.go:50-58, 159-175) ---------------------------------------
SPLIT = dict(n=9, lookahead_ns=5 * MS, window=5_000)


def run_splitbrain(eng, device, case):
    n = SPLIT["n"]
    action = {"drop": nw.FilterAction.Drop, "reject": nw.FilterAction.Reject, "accept": nw.FilterAction.Accept}[case]
    region = wl.splitbrain_regions(n)
    # wl.configure_splitbrain's rules (region A filters region B), on links of 5 ms + 0.1 ms per peer id:
    # the requests of one probe reach a responder in different ticks, so no two of its replies share
    # (tick, seq) (see mesh_shapes for why that matters)
    for i in range(n):
        rules = [nw.LinkRule(Subnet=(str(ipaddress.IPv4Address(wl.peer_ip(int(p)))), 32),
                             LinkShape=nw.LinkShape(Filter=action))
                 for p in np.nonzero(region == wl.REGION_B)[0]] if region[i] == wl.REGION_A else []
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=5 * MS + 100_000 * i),
                                   Rules=rules))
    ping = dict(count=2, interval_ticks=3_000, length=66, start_tick=eng.stats()["now_tick"], bin_ns=MS, n_bins=16)
    return drive(eng, device, ping, wl.ping_targets_all(n), 5, SPLIT["window"], probe_at=(0, 2))


def splitbrain_reached(pairs, n):
    """ok[i, j] = pair i -> j has a counted reply."""
    ok = np.zeros((n, n), dtype=bool)
    t = wl.ping_targets_all(n)
    ok[np.repeat(np.arange(n), n - 1), t.ravel()] = (pairs["received"] > 0).ravel()
    return ok


# -- B. lossy mesh with a hot responder --------------------------------------------------------------
MESH = dict(n=130, lookahead_ns=4 * MS, window=4_000, seed=5)
MESH_PING = dict(count=4, interval_ticks=3_000, length=200, bin_ns=2 * MS, n_bins=48)


def mesh_targets(n=130, seed=MESH["seed"]):
    """Three mesh slots and one slot that is peer 0 for everyone (empty for peer 0 itself)."""
    t = np.empty((n, 4), dtype=np.uint32)
    t[:, :3] = wl.ping_targets_mesh(n, 3, seed)
    t[:, 3] = 0
    t[0, 3] = abi.PING_NONE
    return t


def mesh_shapes(n=130, seed=MESH["seed"]):
    """Latencies from {5, 7, 12, 23, 50} ms (most peers 5 ms, so that peer 0 answers more than 64
    requests in one window), jitter of 0.2 to 1 ms on most peers (peer 0 among them), 10 Mbit/s on
    some.  The minimum netem delay is 5 ms - 1 ms = the 4 ms lookahead.

    Why the jitter: the engine serves a source's queue in (e, seq, clone first) order and leaves the
    order of two originals with equal eligibility time e and equal seq open (the oracle's heap and the
    HIP engine's sorted queue then differ in which of them HTB serves first).  A responder answers two
    requesters whose slots coincide with the same reply seq; when the requests arrived in the same
    tick, only the responder's jitter tells the replies' e apart.  The mesh keeps such ties to
    responders with jitter (mesh_tie_sources_have_jitter, asserted on the model alone)."""
    rng = np.random.default_rng(seed)
    lat = rng.choice(np.array([5, 7, 12, 23, 50]) * MS, n, p=[0.6, 0.1, 0.1, 0.1, 0.1])
    jit = np.where(rng.random(n) < 0.8, rng.integers(200_000, MS + 1, n), 0)
    jit[0] = MS
    bw = np.where(rng.random(n) < 0.3, 10_000_000, 0)
    return lat, jit, bw


def mesh_tie_sources_have_jitter(model, n=130, seed=MESH["seed"]):
    jit = mesh_shapes(n, seed)[1]
    return all(jit[s] > 0 for s in model.tie_sources)


def configure_mesh(eng, n=130, seed=MESH["seed"], lossy=True):
    """mesh_shapes with loss 10 %, duplicate 10 %, corrupt 5 %."""
    lat, jit, bw = mesh_shapes(n, seed)
    pct = (lambda v: np.full(n, v if lossy else 0.0, dtype=np.float32))
    eng.configure_batch(np.arange(n), nw.configs_array(lat, jitter_ns=jit, bandwidth_bps=bw, loss=pct(10.0),
                                                       duplicate=pct(10.0), corrupt=pct(5.0)))


def run_mesh(eng, device, window=MESH["window"], ticks=120_000, probe_at=None, before=None, lossy=True):
    n = MESH["n"]
    configure_mesh(eng, n, lossy=lossy)
    ping = dict(MESH_PING, start_tick=eng.stats()["now_tick"])
    n_windows = ticks // window
    probe_at = (0, 4, n_windows // 2) if probe_at is None else probe_at
    return drive(eng, device, ping, mesh_targets(n), n_windows, window, probe_at=probe_at, before=before)


# -- E. late receipt ---------------------------------------------------------------------------------
LATE = dict(n=4, lookahead_ns=5 * MS, window=5_000)


def configure_late(eng, reorder):
    for i in range(LATE["n"]):
        eng.configure(i, nw.Config(Network="default", Enable=True,
                                   Default=nw.LinkShape(Latency=5 * MS, Reorder=reorder if i == 1 else 0.0)))
