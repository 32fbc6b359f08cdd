"""The cases of the flow driver's RTT estimator and timer backoff (tgsim_flow_init_rto) shared by
tests/test_flow_rto_model.py (the host model over the CPU oracle, against closed forms, and the
conditions the parity inputs have to meet) and tests/test_gpu_flow_rto.py (the device loop against that
model, bit for bit).  The topologies and helpers are those of tests/flow_cases.py and
tests/flow_cc_cases.py."""
import numpy as np

import flow_cases as fc
import flow_cc_cases as cc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

MS, TICK = fc.MS, fc.TICK
MAX_RTO = abi.FLOW_MAX_RTO


def drive(eng, device, flow, ccp, rto, flows, n_windows, window, probe_at=(), before=None):
    """flow_cc_cases.drive with an `rto` dict (None: armed without the estimator); the result carries
    "rto_rows" and "rto_summary" when rto is given."""
    if not device:
        out = wl.flow_reference(eng, flow, flows, n_windows, window, probe_at=probe_at, before=before, cc=ccp, rto=rto)
    else:
        eng.flow_init(flows, cc=ccp, rto=rto, **flow)
        out = wl.flow_run(eng, n_windows, window, collect=True, probe_at=probe_at, before=before)
        out["rows"], out["summary"] = eng.flow_rows(), eng.flow_report()
        if ccp is not None:
            out["cc_rows"], out["cc_summary"] = eng.flow_cc_rows(), eng.flow_cc_report()
        if rto is not None:
            out["rto_rows"], out["rto_summary"] = eng.flow_rto_rows(), eng.flow_rto_report()
    out["flows"] = flows
    return out


def assert_same_rto(dev, ref, what=""):
    (dr, ds), (rr, rs) = dev, ref
    for key in abi.FLOW_RTO_ROW_DTYPE.names:
        assert (dr[key] == rr[key]).all(), (what, key, np.nonzero(dr[key] != rr[key])[0][:8])
    assert dr.tobytes() == rr.tobytes(), what
    for key in abi.FLOW_RTO_SUMMARY_FIELDS:
        assert ds[key] == rs[key], (what, key, ds[key], rs[key])


def assert_same_run(dev, ref, windows=True):
    """flow_cases.assert_same_run (verdicts, deliveries, flow rows, summary, histogram), the cc rows and
    cc summary where armed, and the rto rows and rto summary, at every probe and at the end."""
    with_cc = "cc_rows" in ref
    assert with_cc == ("cc_rows" in dev) and "rto_rows" in ref and "rto_rows" in dev
    n = 6 if with_cc else 4
    for w in ref["probes"]:
        assert len(dev["probes"][w]) == len(ref["probes"][w]) == n
    plain = (lambda o: dict(o, probes={w: p[:2] for w, p in o["probes"].items()}))
    fc.assert_same_run(plain(dev), plain(ref), windows=windows)
    for w in ref["probes"]:
        if with_cc:
            cc.assert_same_cc(dev["probes"][w][2:4], ref["probes"][w][2:4], f"probe after window {w}")
        assert_same_rto(dev["probes"][w][-2:], ref["probes"][w][-2:], f"probe after window {w}")
    if with_cc:
        cc.assert_same_cc((dev["cc_rows"], dev["cc_summary"]), (ref["cc_rows"], ref["cc_summary"]), "end of run")
    assert_same_rto((dev["rto_rows"], dev["rto_summary"]), (ref["rto_rows"], ref["rto_summary"]), "end of run")


def same_but_rto(a, b):
    """Verdicts, deliveries, flow rows, summary, histogram and (where both have them) cc rows and cc
    summary of two runs are byte-identical; the rto rows, which only one of them has, aside."""
    cc.same_plain_run(a, b)
    assert ("cc_rows" in a) == ("cc_rows" in b)
    if "cc_rows" in a:
        cc.assert_same_cc((a["cc_rows"], a["cc_summary"]), (b["cc_rows"], b["cc_summary"]), "end of run")
        for w in a["probes"]:
            cc.assert_same_cc(a["probes"][w][2:4], b["probes"][w][2:4], f"probe after window {w}")


def restate(samples, rto0, min_rto, max_rto):
    """The update rule of include/tgsim.h applied to a list of samples, written apart from the model:
    (srtt8, rttvar4, rto, samples, rtt_min, rtt_max, rtt_last)."""
    srtt8 = rttvar4 = 0
    rto = rto0
    for n, m in enumerate(samples):
        if n == 0:
            srtt8, rttvar4 = m << 3, m << 1
        else:
            err = m - srtt8 // 8
            rttvar4 += abs(err) - rttvar4 // 4
            srtt8 += err
        rto = sorted((min_rto, srtt8 // 8 + (rttvar4 or 1), max_rto))[1]
    return (srtt8, rttvar4, rto, len(samples), min(samples, default=0xFFFFFFFF), max(samples, default=0),
            samples[-1] if samples else 0)


def row_tuple(row):
    return tuple(int(row[k]) for k in ("srtt8", "rttvar4", "rto", "samples", "rtt_min", "rtt_max", "rtt_last"))


# -- 1. the estimator on a constant link ----------------------------------------------------------------------------
# flow_cases case 1's link (2 peers, 10 ms each way, no jitter, no loss), one segment in flight.
CONST = dict(n=2, latency_ns=10 * MS, lookahead_ns=10 * MS, window=10_000, n_seg=12, n_windows=30)
CONST_FLOW = dict(seg_len=1460, ack_len=64, window=1, rto_ticks=100_000, max_attempts=4, bin_ns=MS, n_bins=64)
CONST_RTO = dict(min_rto_ticks=10_000, max_rto_ticks=1_000_000, backoff=1)
# a sample is tick(ACK delivery) - tick(offer): 2 L plus, as flow_cases.ROUNDS_SLACK_NS, two tick
# quantisations (the ACK is offered at the tick after the segment's delivery, the sample taken at the
# tick after the ACK's) and the serialisation of one segment and one ACK at the unlimited link's HTB
# rate (under 0.25 ns per byte)
CONST_SLACK_NS = 2 * TICK + CONST_FLOW["window"] * (CONST_FLOW["seg_len"] + CONST_FLOW["ack_len"]) // 4


def run_const(eng, device):
    fc.plain(eng, 2, CONST["latency_ns"])
    flows = fc.table([(0, 1, CONST["n_seg"], eng.stats()["now_tick"])])
    return drive(eng, device, CONST_FLOW, None, CONST_RTO, flows, CONST["n_windows"], CONST["window"], probe_at=(0, 2, 12))


# -- 2. spurious retransmissions stop -------------------------------------------------------------------------------
# 50 ms each way: a round trip of 100,000 ticks against a timer of 30,000, and 3 x 30 ms < 100 ms < 4 x
# 30 ms: with the fixed timer every segment is offered at +0, +30, +60 and +90 ms before its ACK.
SPUR = dict(n=2, latency_ns=50 * MS, lookahead_ns=10 * MS, window=10_000, n_seg=40, n_windows=125)
SPUR_FLOW = dict(seg_len=1460, ack_len=64, window=4, rto_ticks=30_000, max_attempts=8, bin_ns=10 * MS, n_bins=128)
SPUR_RTO = dict(min_rto_ticks=30_000, max_rto_ticks=1_000_000, backoff=0)


def run_spur(eng, device, rto):
    fc.plain(eng, 2, SPUR["latency_ns"])
    flows = fc.table([(0, 1, SPUR["n_seg"], eng.stats()["now_tick"])])
    return drive(eng, device, SPUR_FLOW, None, rto, flows, SPUR["n_windows"], SPUR["window"], probe_at=(0, 11, 40))


# -- 3. backoff in closed form ------------------------------------------------------------------------------------------
# flow_cases.CUT: peer 0 has a Drop rule towards peer 1, so flow 0 never gets an ACK.
CUT_FLOW = dict(fc.CUT_FLOW, rto_ticks=20_000, max_attempts=6)
CUT_RTO = dict(min_rto_ticks=5_000, max_rto_ticks=200_000, backoff=1)
CUT_FAIL_AFTER = 20_000 + 40_000 + 80_000 + 160_000 + 200_000 + 200_000
CUT_TICKS = CUT_FAIL_AFTER + 10_000


def run_cut(eng, device, window=fc.CUT["window"], ccp=None):
    fc.plain(eng, fc.CUT["n"], fc.CUT["latency_ns"])
    eng.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=fc.CUT["latency_ns"]),
                               Rules=[fc.rule(1, nw.FilterAction.Drop)]))
    flows = fc.cut_flows(eng.stats()["now_tick"])
    n_windows = CUT_TICKS // window
    return drive(eng, device, CUT_FLOW, ccp, CUT_RTO, flows, n_windows, window, probe_at=(0, 2, n_windows // 2))


# -- 4. degenerate equivalence --------------------------------------------------------------------------------------------
# min = max = rto_ticks and no backoff: the flow's timer never moves, and the run is the one armed without rto.
def degenerate(flow):
    return dict(min_rto_ticks=flow["rto_ticks"], max_rto_ticks=flow["rto_ticks"], backoff=0)


def run_rounds(eng, device, rounds, rto):
    fc.plain(eng, 2, fc.ROUNDS["latency_ns"])
    w, now = fc.ROUNDS_FLOW["window"], eng.stats()["now_tick"]
    flows = fc.table([(0, 1, w * rounds - (rounds == 1) * 3, now), (1, 0, w * rounds, now + 500)])
    n_windows = 2 * rounds + 2
    return drive(eng, device, fc.ROUNDS_FLOW, None, rto, flows, n_windows, fc.ROUNDS["window"], probe_at=(0, 2, n_windows - 2))


# -- 5. lossy mesh ----------------------------------------------------------------------------------------------------------
# flow_cc_cases' mesh (jitter on every peer, loss 4 %, duplicate 2 %, corrupt 1 %, cap 16 from 2).  Round
# trips run from 10 to about 100 ms: from the initial 30,000 ticks the timers of the 5-ms pairs settle at
# the 12,000-tick floor, those of the 50-ms pairs start at three round trips, above the 120,000-tick cap.
MESH_RTO = dict(min_rto_ticks=12_000, max_rto_ticks=120_000, backoff=1)


def run_mesh(eng, device, window=fc.MESH["window"], probe_at=None, rto=MESH_RTO):
    fc.configure_mesh(eng)
    flows = fc.mesh_flows(eng.stats()["now_tick"])
    n_windows = cc.MESH_WINDOWS * fc.MESH["window"] // window
    probe_at = (0, 6, n_windows // 10) if probe_at is None else probe_at
    return drive(eng, device, cc.MESH_FLOW, cc.MESH_CC, rto, flows, n_windows, window, probe_at=probe_at)


# -- 6. corners on flow_cc_cases' 4 peers with 20 % loss and one Drop rule ----------------------------------------------
# (window, cc or None, backoff, min, max, rto_ticks, n_seg), max_attempts 16.  The round trip is 10,000 ticks.
_CC1, _CC64 = dict(init_cwnd=1, init_ssthresh=0, dupthresh=3), dict(init_cwnd=64, init_ssthresh=0, dupthresh=1)
CORNERS = [
    (1, None, 1, 5_000, 12_000, 6_000, 65),     # window 1; the timer below the round trip; shift 15 capped
    (1, _CC1, 0, 5_000, MAX_RTO, 11_000, 65),   # window 1 with cc; no backoff; max = 2^27
    (64, None, 1, 5_000, MAX_RTO, 11_000, 130),  # window 64 without cc; shifts towards 2^27
    (64, _CC1, 1, 5_000, 12_000, 6_000, 130),   # window 64 with cc from 1; shift 15 capped
    (64, _CC64, 1, 11_000, 11_000, 11_000, 65),  # min == max with backoff: every shift capped, rto pinned
]
CORNER_WINDOWS = 44


def run_corner(eng, device, window, ccp, backoff, min_rto, max_rto, rto_ticks, n_seg):
    fc.plain(eng, 4, 5 * MS, Loss=20.0)
    eng.configure(3, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=5 * MS),
                               Rules=[fc.rule(0, nw.FilterAction.Drop)]))
    now = eng.stats()["now_tick"]
    flows = fc.table([(0, 1, n_seg, now), (1, 2, n_seg, now + 3), (2, 3, n_seg, now), (3, 0, n_seg, now)])
    flow = dict(seg_len=300, ack_len=40, window=window, rto_ticks=rto_ticks, max_attempts=16, bin_ns=MS, n_bins=8)
    rto = dict(min_rto_ticks=min_rto, max_rto_ticks=max_rto, backoff=backoff)
    return drive(eng, device, flow, ccp, rto, flows, CORNER_WINDOWS, 5_000, probe_at=(0, 3, CORNER_WINDOWS - 2))


# What the mesh and the corners have to exercise together, as counters of workloads.FlowRtoMixin.
EXERCISED = ("sampled_after_retransmit", "clamped_min", "clamped_max", "shifted_twice", "shift_capped",
             "unsampled_attempts", "ring_wraps")


def exercised(outs):
    tot = {"samples": 0}
    for o in outs:
        tot["samples"] += o["rto_summary"]["samples"]
        for key in EXERCISED:
            tot[key] = tot.get(key, 0) + int(getattr(o["model"], key))
    return tot
