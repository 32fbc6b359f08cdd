"""The flow driver's cases shared by tests/test_flow_model.py (the host model over the CPU oracle,
against answers known in closed form) and tests/test_gpu_flow.py (the HIP engine's device loop against
that model, bit for bit).  A case configures an engine-shaped object and runs the loop on it: on the
device (Engine.flow_init + workloads.flow_run) or from the host (workloads.flow_reference)."""
import ipaddress

import numpy as np

from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

MS = nw.Millisecond
TICK = 1_000  # ns: the engines' default tick


def table(entries):
    """[(src, dst, n_seg, start_tick)] sorted by src."""
    return np.array(sorted(entries, key=lambda e: e[0]), dtype=abi.FLOW_SPEC_DTYPE)


def drive(eng, device, flow, flows, n_windows, window, probe_at=(), before=None):
    """One armed run of n_windows on `eng`; the same result keys either way."""
    if not device:
        return wl.flow_reference(eng, flow, flows, n_windows, window, probe_at=probe_at, before=before)
    eng.flow_init(flows, **flow)
    out = wl.flow_run(eng, n_windows, window, collect=True, probe_at=probe_at, before=before)
    out["rows"], out["summary"] = eng.flow_rows(), eng.flow_report()
    return out


def assert_same_report(dev, ref, what=""):
    (dr, ds), (rr, rs) = dev, ref
    for key in abi.FLOW_ROW_DTYPE.names:
        assert (dr[key] == rr[key]).all(), (what, key, np.nonzero(dr[key] != rr[key])[0][:8])
    for key in abi.FLOW_SUMMARY_FIELDS:
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
    assert_same_report((dev["rows"], dev["summary"]), (ref["rows"], ref["summary"]), "end of run")


def fct(out):
    """FCT of every flow of a result (ns); only meaningful where the flow is DONE."""
    return out["rows"]["done_ns"].astype(np.int64) - out["flows"]["start_tick"].astype(np.int64) * TICK


def plain(eng, n, latency_ns, **shape):
    for i in range(n):
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=latency_ns, **shape)))


def rule(peer, action):
    return nw.LinkRule(Subnet=(str(ipaddress.IPv4Address(wl.peer_ip(int(peer)))), 32), LinkShape=nw.LinkShape(Filter=action))


# -- 1. one round and k rounds ------------------------------------------------------------------------
# 2 peers, L both ways, no jitter, no loss, unlimited bandwidth.
ROUNDS = dict(n=2, latency_ns=10 * MS, lookahead_ns=10 * MS, window=10_000)
ROUNDS_FLOW = dict(seg_len=1460, ack_len=64, window=8, rto_ticks=100_000, max_attempts=4, bin_ns=MS, n_bins=128)
# One round trip takes 2 L plus, at most:
#   - two tick quantisations: the ACK is offered at the tick after the segment's delivery, and a
#     segment an ACK releases at the tick after the ACK's delivery (each < 1 tick late, + the tick);
#   - the HTB serialisation of what shares a queue: an unlimited link is served at 2^32 - 1 bytes/s,
#     under 0.25 ns per byte, and at most `window` segments and `window` ACKs of one round queue
#     behind each other.
ROUNDS_SLACK_NS = 2 * TICK + ROUNDS_FLOW["window"] * (ROUNDS_FLOW["seg_len"] + ROUNDS_FLOW["ack_len"]) // 4


def run_rounds(eng, device, rounds, before=None):
    plain(eng, 2, ROUNDS["latency_ns"])
    w, now = ROUNDS_FLOW["window"], eng.stats()["now_tick"]
    flows = table([(0, 1, w * rounds - (rounds == 1) * 3, now), (1, 0, w * rounds, now + 500)])
    n_windows = 2 * rounds + 2
    out = drive(eng, device, ROUNDS_FLOW, flows, n_windows, ROUNDS["window"], probe_at=(0, 2, n_windows - 2),
                before=before)
    out["flows"] = flows
    return out


# -- 2. bandwidth-bound ---------------------------------------------------------------------------------
BW = dict(n=2, latency_ns=5 * MS, lookahead_ns=5 * MS, window=5_000, rate_bps=10_000_000, n_seg=200)
# the bandwidth-delay product is 10 Mbit/s x 10 ms = 12,500 bytes, under 9 segments: a window of 16 covers it
BW_FLOW = dict(seg_len=1460, ack_len=64, window=16, rto_ticks=60_000, max_attempts=4, bin_ns=10 * MS, n_bins=64)
BW_BURST_BYTES = 1_600  # the HTB burst of the shape (mtu 1600 at rates far below 1e9 bytes/s, link.go:156-167)


def run_bandwidth(eng, device):
    eng.configure(0, nw.Config(Network="default", Enable=True,
                               Default=nw.LinkShape(Latency=BW["latency_ns"], Bandwidth=BW["rate_bps"])))
    eng.configure(1, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=BW["latency_ns"])))
    flows = table([(0, 1, BW["n_seg"], eng.stats()["now_tick"])])
    out = drive(eng, device, BW_FLOW, flows, 60, BW["window"], probe_at=(0, 30))
    out["flows"] = flows
    return out


# -- 3. netem limit ----------------------------------------------------------------------------------------
# One source, 16 flows of window 64 to 16 peers, all starting in one tick: 1,024 packets into a netem
# queue of 1,000.
LIMIT = dict(n=17, latency_ns=5 * MS, lookahead_ns=5 * MS, window=5_000)
LIMIT_FLOW = dict(seg_len=200, ack_len=64, window=64, rto_ticks=20_000, max_attempts=4, bin_ns=MS, n_bins=64)


def run_limit(eng, device):
    plain(eng, LIMIT["n"], LIMIT["latency_ns"])
    now = eng.stats()["now_tick"]
    flows = table([(0, 1 + k, 64, now) for k in range(16)])
    out = drive(eng, device, LIMIT_FLOW, flows, 10, LIMIT["window"], probe_at=(0, 2, 5))
    out["flows"] = flows
    return out


# -- 4. unreachable -----------------------------------------------------------------------------------------
# Peer 0 has a Drop rule towards peer 1.  No responder answers two requesters (see mesh_shapes).
CUT = dict(n=4, latency_ns=5 * MS, lookahead_ns=5 * MS, window=5_000, ticks=50_000)
CUT_FLOW = dict(seg_len=500, ack_len=64, window=4, rto_ticks=12_000, max_attempts=3, bin_ns=MS, n_bins=64)


def cut_flows(now):
    return table([(0, 1, 9, now), (0, 2, 9, now), (2, 3, 3, now), (3, 0, 9, now + 7)])


def run_cut(eng, device, window=CUT["window"]):
    plain(eng, CUT["n"], CUT["latency_ns"])
    eng.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=CUT["latency_ns"]),
                               Rules=[rule(1, nw.FilterAction.Drop)]))
    flows = cut_flows(eng.stats()["now_tick"])
    n_windows = CUT["ticks"] // window
    out = drive(eng, device, CUT_FLOW, flows, n_windows, window, probe_at=(0, 2, n_windows // 2))
    out["flows"] = flows
    return out


# -- 5. partition that heals ----------------------------------------------------------------------------------
# The rule of case 4 is installed before window W1 and removed (an Accept rule on the subnet) before W2.
HEAL = dict(n=4, latency_ns=5 * MS, lookahead_ns=5 * MS, window=5_000, n_windows=40, w1=3, w2=12)
HEAL_FLOW = dict(seg_len=500, ack_len=64, window=4, rto_ticks=15_000, max_attempts=16, bin_ns=5 * MS, n_bins=64)


def run_heal(eng, device):
    plain(eng, HEAL["n"], HEAL["latency_ns"])
    now = eng.stats()["now_tick"]
    flows = table([(0, 1, 40, now), (0, 2, 40, now), (2, 3, 12, now), (3, 0, 40, now + 7)])

    def before(w):
        if w in (HEAL["w1"], HEAL["w2"]):
            action = nw.FilterAction.Drop if w == HEAL["w1"] else nw.FilterAction.Accept
            eng.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=HEAL["latency_ns"]),
                                       Rules=[rule(1, action)]))

    out = drive(eng, device, HEAL_FLOW, flows, HEAL["n_windows"], HEAL["window"], probe_at=(0, 6, 20), before=before)
    out["flows"] = flows
    return out


# -- 6. lossy mesh ------------------------------------------------------------------------------------------
MESH = dict(n=130, lookahead_ns=4 * MS, window=4_000, seed=3, n_windows=130)
# rto 30 ms: below the round trip of every pair with a 23- or 50-ms leg, so those flows retransmit
# segments whose ACK is still on its way, and the late ACK of the first attempt makes the second's stale
MESH_FLOW = dict(seg_len=1000, ack_len=64, window=8, rto_ticks=30_000, max_attempts=16, bin_ns=20 * MS, n_bins=64)


def mesh_shapes(n=MESH["n"], seed=MESH["seed"]):
    """Latencies from {5, 7, 12, 23, 50} ms (peers 0 and 1: 5 ms), jitter of 0.2 to 1 ms on EVERY peer,
    10 Mbit/s on some.  The minimum netem delay is 5 ms - 1 ms = the 4 ms lookahead.

    Why the jitter: the engines leave the order of two originals of one source with equal
    eligibility time and equal seq open.  A receiver acknowledges two senders whose (attempt, slot,
    segment) coincide with the same ACK seq; when the segments arrived in the same tick, only the
    receiver's jitter tells the ACKs' eligibility times apart (mesh_tie_sources_have_jitter, asserted
    on the model alone)."""
    rng = np.random.default_rng(seed)
    lat = rng.choice(np.array([5, 7, 12, 23, 50]) * MS, n, p=[0.5, 0.15, 0.15, 0.1, 0.1])
    lat[:2] = 5 * MS
    jit = rng.integers(200_000, MS + 1, n)
    bw = np.where(rng.random(n) < 0.3, 10_000_000, 0)
    bw[:2] = 0
    return lat, jit, bw


def mesh_tie_sources_have_jitter(model, n=MESH["n"], seed=MESH["seed"]):
    jit = mesh_shapes(n, seed)[1]
    return all(jit[s] > 0 for s in model.tie_sources)


def mesh_flows(now, n=MESH["n"], seed=MESH["seed"]):
    """Peer 0 sends 16 flows (one of 70 segments); every other peer sends three, the third of them to
    peer 1 (peer 1's third goes to peer 0): peer 1 acknowledges some 128 senders' windows at once."""
    rng = np.random.default_rng(seed + 1)
    t = wl.flow_table_mesh(n, 3, 1, seed)
    t["n_seg"] = rng.integers(3, 30, len(t))
    t["dst"][2::3] = 1
    t["dst"][1 * 3 + 2] = 0
    for s in range(n):  # a flow to peer 1 beside the mesh's own: keep a source's destinations distinct
        row = t[3 * s:3 * s + 3]
        for k in (0, 1):
            while row["dst"][k] in (s, row["dst"][2]) or row["dst"][k] == row["dst"][1 - k]:
                row["dst"][k] = (row["dst"][k] + 1) % n
    hot = np.zeros(16, dtype=abi.FLOW_SPEC_DTYPE)
    hot["src"], hot["dst"], hot["n_seg"] = 0, 1 + np.arange(16), rng.integers(3, 30, 16)
    hot["n_seg"][5] = 70
    t = np.concatenate([hot, t[3:]])
    t["start_tick"] = now + rng.integers(0, 3_000, len(t))
    t["start_tick"][:16] = now
    return t


def configure_mesh(eng, n=MESH["n"], seed=MESH["seed"]):
    """mesh_shapes with loss 4 %, duplicate 2 %, corrupt 1 %, reorder 0."""
    lat, jit, bw = mesh_shapes(n, seed)
    pct = (lambda v: np.full(n, v, dtype=np.float32))
    eng.configure_batch(np.arange(n), nw.configs_array(lat, jitter_ns=jit, bandwidth_bps=bw, loss=pct(4.0),
                                                       duplicate=pct(2.0), corrupt=pct(1.0)))


def run_mesh(eng, device, window=MESH["window"], probe_at=None, before=None):
    configure_mesh(eng)
    flows = mesh_flows(eng.stats()["now_tick"])
    n_windows = MESH["n_windows"] * MESH["window"] // window
    probe_at = (0, 6, n_windows // 2) if probe_at is None else probe_at
    out = drive(eng, device, MESH_FLOW, flows, n_windows, window, probe_at=probe_at, before=before)
    out["flows"] = flows
    return out


# -- 7. late receipt -----------------------------------------------------------------------------------------
LATE = dict(n=4, lookahead_ns=5 * MS, window=5_000)
LATE_FLOW = dict(seg_len=64, ack_len=64, window=8, rto_ticks=50_000, max_attempts=4)


def configure_late(eng, reorder):
    for i in range(LATE["n"]):
        eng.configure(i, nw.Config(Network="default", Enable=True,
                                   Default=nw.LinkShape(Latency=5 * MS, Reorder=reorder if i == 1 else 0.0)))


def late_flows(now, n_seg=8):
    return table([(0, 1, n_seg, now), (1, 2, n_seg, now), (2, 3, n_seg, now), (3, 0, n_seg, now)])


class Folding:
    """An engine-shaped wrapper that folds every window it is driven through into a wl.GroupMatrix (the
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
