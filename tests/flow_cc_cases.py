"""The cases of the flow driver's congestion control (tgsim_flow_init_cc) shared by
tests/test_flow_cc_model.py (the host model over the CPU oracle, against closed forms, and the
conditions the parity inputs have to meet) and tests/test_gpu_flow_cc.py (the device loop against that
model, bit for bit).  The topologies and helpers are those of tests/flow_cases.py."""
import numpy as np

import flow_cases as fc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

MS, TICK = fc.MS, fc.TICK


def drive(eng, device, flow, cc, flows, n_windows, window, probe_at=(), before=None):
    """flow_cases.drive with a `cc` dict (None: armed without congestion control); the result carries
    "cc_rows" and "cc_summary" when cc is given, and the table under "flows"."""
    if not device:
        out = wl.flow_reference(eng, flow, flows, n_windows, window, probe_at=probe_at, before=before, cc=cc)
    else:
        eng.flow_init(flows, cc=cc, **flow)
        out = wl.flow_run(eng, n_windows, window, collect=True, probe_at=probe_at, before=before)
        out["rows"], out["summary"] = eng.flow_rows(), eng.flow_report()
        if cc is not None:
            out["cc_rows"], out["cc_summary"] = eng.flow_cc_rows(), eng.flow_cc_report()
    out["flows"] = flows
    return out


def assert_same_cc(dev, ref, what=""):
    (dr, ds), (rr, rs) = dev, ref
    for key in abi.FLOW_CC_ROW_DTYPE.names:
        assert (dr[key] == rr[key]).all(), (what, key, np.nonzero(dr[key] != rr[key])[0][:8])
    assert dr.tobytes() == rr.tobytes(), what
    for key in abi.FLOW_CC_SUMMARY_FIELDS:
        assert ds[key] == rs[key], (what, key, ds[key], rs[key])


def assert_same_run(dev, ref, windows=True):
    """flow_cases.assert_same_run, and the cc rows and cc summary at every probe and at the end."""
    for w in ref["probes"]:
        assert len(dev["probes"][w]) == len(ref["probes"][w]) == 4
    plain = (lambda o: dict(o, probes={w: p[:2] for w, p in o["probes"].items()}))
    fc.assert_same_run(plain(dev), plain(ref), windows=windows)
    for w in ref["probes"]:
        assert_same_cc(dev["probes"][w][2:], ref["probes"][w][2:], f"probe after window {w}")
    assert_same_cc((dev["cc_rows"], dev["cc_summary"]), (ref["cc_rows"], ref["cc_summary"]), "end of run")


def same_plain_run(a, b):
    """Flow rows, summary, histogram, verdicts and deliveries of two runs are byte-identical (the cc
    rows, which only one of them may have, aside)."""
    plain = (lambda o: dict(o, probes={w: p[:2] for w, p in o["probes"].items()}))
    fc.assert_same_run(plain(a), plain(b))
    assert a["rows"].tobytes() == b["rows"].tobytes()


# -- 1, 2. slow start and congestion avoidance ------------------------------------------------------------
# flow_cases case 1's link (2 peers, L both ways, no jitter, no loss, unlimited bandwidth), window 64.
RAMP = dict(n=2, latency_ns=10 * MS, lookahead_ns=10 * MS, window=10_000)
RAMP_FLOW = dict(seg_len=1460, ack_len=64, window=64, rto_ticks=100_000, max_attempts=4, bin_ns=MS, n_bins=256)
# per round, as flow_cases.ROUNDS_SLACK_NS: two tick quantisations, and the serialisation of at most
# `window` segments and `window` ACKs at the unlimited link's HTB rate (under 0.25 ns per byte)
RAMP_SLACK_NS = 2 * TICK + RAMP_FLOW["window"] * (RAMP_FLOW["seg_len"] + RAMP_FLOW["ack_len"]) // 4
SLOW_START = dict(init_cwnd=1, init_ssthresh=0, dupthresh=3)
AVOIDANCE = dict(init_cwnd=4, init_ssthresh=4, dupthresh=3)
# (cc, n_seg, round trips): round r of slow start carries 2^(r-1) segments, of avoidance 3 + r
RAMPS = [(SLOW_START, 31, 5), (SLOW_START, 32, 6), (AVOIDANCE, 22, 4), (AVOIDANCE, 23, 5)]


def run_ramp(eng, device, cc, n_seg, rounds):
    fc.plain(eng, 2, RAMP["latency_ns"])
    flows = fc.table([(0, 1, n_seg, eng.stats()["now_tick"])])
    n_windows = 2 * rounds + 2
    return drive(eng, device, RAMP_FLOW, cc, flows, n_windows, RAMP["window"], probe_at=(0, 2, n_windows - 2))


# -- 3. degenerate equivalence --------------------------------------------------------------------------------
# init_cwnd = window and init_ssthresh = 0 on a lossless link: cwnd never moves, nothing is marked, and
# the run is the one armed without cc.  These restate flow_cases.run_rounds / run_bandwidth with a cc.
def degenerate(window, dupthresh):
    return dict(init_cwnd=window, init_ssthresh=0, dupthresh=dupthresh)


def run_rounds(eng, device, rounds, cc):
    fc.plain(eng, 2, fc.ROUNDS["latency_ns"])
    w, now = fc.ROUNDS_FLOW["window"], eng.stats()["now_tick"]
    flows = fc.table([(0, 1, w * rounds - (rounds == 1) * 3, now), (1, 0, w * rounds, now + 500)])
    n_windows = 2 * rounds + 2
    return drive(eng, device, fc.ROUNDS_FLOW, cc, flows, n_windows, fc.ROUNDS["window"], probe_at=(0, 2, n_windows - 2))


def run_bandwidth(eng, device, cc):
    eng.configure(0, nw.Config(Network="default", Enable=True,
                               Default=nw.LinkShape(Latency=fc.BW["latency_ns"], Bandwidth=fc.BW["rate_bps"])))
    eng.configure(1, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=fc.BW["latency_ns"])))
    flows = fc.table([(0, 1, fc.BW["n_seg"], eng.stats()["now_tick"])])
    return drive(eng, device, fc.BW_FLOW, cc, flows, 60, fc.BW["window"], probe_at=(0, 30))


# -- 4. unreachable ---------------------------------------------------------------------------------------------
CUT_CC = dict(init_cwnd=3, init_ssthresh=0, dupthresh=3)


def run_cut(eng, device, window=fc.CUT["window"], cc=CUT_CC):
    fc.plain(eng, fc.CUT["n"], fc.CUT["latency_ns"])
    eng.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=fc.CUT["latency_ns"]),
                               Rules=[fc.rule(1, nw.FilterAction.Drop)]))
    flows = fc.cut_flows(eng.stats()["now_tick"])
    n_windows = fc.CUT["ticks"] // window
    return drive(eng, device, fc.CUT_FLOW, cc, flows, n_windows, window, probe_at=(0, 2, n_windows // 2))


# -- 6. netem limit ------------------------------------------------------------------------------------------------
# flow_cases case 3's 17 peers and 16 flows of one source.  From 32 segments each the windows double
# within the first round trip: 16 x 64 = 1,024 packets are released into a netem queue of 1,000 while
# the 5-ms delay still holds all of them.
LIMIT_FLOW = dict(fc.LIMIT_FLOW, max_attempts=8)
LIMIT_CC = dict(init_cwnd=32, init_ssthresh=0, dupthresh=3)
LIMIT_SEGS, LIMIT_WINDOWS = 200, 24


def run_limit(eng, device):
    fc.plain(eng, fc.LIMIT["n"], fc.LIMIT["latency_ns"])
    now = eng.stats()["now_tick"]
    flows = fc.table([(0, 1 + k, LIMIT_SEGS, now) for k in range(16)])
    return drive(eng, device, LIMIT_FLOW, LIMIT_CC, flows, LIMIT_WINDOWS, fc.LIMIT["window"], probe_at=(0, 3, 8))


# -- 7. lossy mesh ---------------------------------------------------------------------------------------------------
# flow_cases' mesh (shapes, table, loss 4 %, duplicate 2 %, corrupt 1 %, jitter on every peer) with a
# cap of 16 segments, from 2.
MESH_FLOW = dict(fc.MESH_FLOW, window=16)
MESH_CC = dict(init_cwnd=2, init_ssthresh=8, dupthresh=3)
MESH_WINDOWS = 400


def run_mesh(eng, device, window=fc.MESH["window"], probe_at=None):
    fc.configure_mesh(eng)
    flows = fc.mesh_flows(eng.stats()["now_tick"])
    n_windows = MESH_WINDOWS * fc.MESH["window"] // window
    probe_at = (0, 6, n_windows // 10) if probe_at is None else probe_at  # (the last flows are stragglers)
    return drive(eng, device, MESH_FLOW, MESH_CC, flows, n_windows, window, probe_at=probe_at)


# -- 8. corners on 4 peers with 20 % loss and one Drop rule (test_gpu_flow.test_corners) ---------------------------
# (window, init_cwnd, dupthresh, n_seg), max_attempts 16
CORNERS = [(1, 1, 0, 1), (1, 1, 3, 65), (2, 1, 1, 65), (2, 2, 63, 130), (64, 1, 3, 130), (64, 64, 1, 65),
           (64, 64, 63, 130), (64, 1, 0, 65), (64, 64, 3, 1)]
CORNER_WINDOWS = 44


def run_corner(eng, device, window, init_cwnd, dupthresh, n_seg):
    fc.plain(eng, 4, 5 * MS, Loss=20.0)
    eng.configure(3, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=5 * MS),
                               Rules=[fc.rule(0, nw.FilterAction.Drop)]))
    now = eng.stats()["now_tick"]
    flows = fc.table([(0, 1, n_seg, now), (1, 2, n_seg, now + 3), (2, 3, n_seg, now), (3, 0, n_seg, now)])
    flow = dict(seg_len=300, ack_len=40, window=window, rto_ticks=11_000, max_attempts=16, bin_ns=MS, n_bins=8)
    cc = dict(init_cwnd=init_cwnd, init_ssthresh=0, dupthresh=dupthresh)
    return drive(eng, device, flow, cc, flows, CORNER_WINDOWS, 5_000, probe_at=(0, 3, CORNER_WINDOWS - 2))


# What cases 6 to 8 have to exercise together, as counters of workloads.FlowCCModel and of its cc summary.
def exercised(outs):
    tot = {}
    for o in outs:
        m = o["model"]
        for key in ("loss_fast", "loss_timeout", "suppressed", "grow_ss", "grow_ca", "cwnd_at_cap", "draining",
                    "fast_acked_early", "fast_lost", "ring_wraps"):
            tot[key] = tot.get(key, 0) + int(getattr(m, key))
        for key in ("fast_retransmits", "timeouts"):
            tot[key] = tot.get(key, 0) + o["cc_summary"][key]
    return tot
