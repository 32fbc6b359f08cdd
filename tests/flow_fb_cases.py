"""The cases of the flow driver's verdict feedback (tgsim_flow_init_fb) shared by
tests/test_flow_fb_model.py (the host model over the CPU oracle, against closed forms, and the conditions
the parity inputs have to meet) and tests/test_gpu_flow_fb.py (the device loop against that model, bit
for bit).  The topologies and helpers are those of tests/flow_cases.py, tests/flow_cc_cases.py and
tests/flow_rto_cases.py."""
import numpy as np

import flow_cases as fc
import flow_cc_cases as cc
import flow_rto_cases as rc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

MS, TICK = fc.MS, fc.TICK
DISCONNECTED, NO_ROUTE, BLACKHOLE, PROHIBIT = (1 << v for v in (abi.V_DISCONNECTED, abi.V_NO_ROUTE, abi.V_BLACKHOLE,
                                                                abi.V_PROHIBIT))
ALL = abi.FLOW_FB_REFUSALS


def drive(eng, device, flow, ccp, rto, fb, flows, n_windows, window, probe_at=(), before=None):
    """flow_rto_cases.drive with an `fb` dict (None: armed without the feedback); the result carries
    "fb_rows" and "fb_summary" when fb is given."""
    if not device:
        out = wl.flow_reference(eng, flow, flows, n_windows, window, probe_at=probe_at, before=before, cc=ccp, rto=rto, fb=fb)
    else:
        eng.flow_init(flows, cc=ccp, rto=rto, fb=fb, **flow)
        out = wl.flow_run(eng, n_windows, window, collect=True, probe_at=probe_at, before=before)
        out["rows"], out["summary"] = eng.flow_rows(), eng.flow_report()
        if ccp is not None:
            out["cc_rows"], out["cc_summary"] = eng.flow_cc_rows(), eng.flow_cc_report()
        if rto is not None:
            out["rto_rows"], out["rto_summary"] = eng.flow_rto_rows(), eng.flow_rto_report()
        if fb is not None:
            out["fb_rows"], out["fb_summary"] = eng.flow_fb_rows(), eng.flow_fb_report()
    out["flows"] = flows
    return out


def assert_same_fb(dev, ref, what=""):
    (dr, ds), (rr, rs) = dev, ref
    for key in abi.FLOW_FB_ROW_DTYPE.names:
        assert (dr[key] == rr[key]).all(), (what, key, np.nonzero(dr[key] != rr[key])[0][:8])
    assert dr.tobytes() == rr.tobytes(), what
    for key in abi.FLOW_FB_SUMMARY_FIELDS:
        assert ds[key] == rs[key], (what, key, ds[key], rs[key])


def _parts(o):
    """(with cc, with rto, with fb) of a result, and its probes cut into (plain, cc, rto, fb) pairs."""
    has = tuple(k + "_rows" in o for k in ("cc", "rto", "fb"))
    cut = {}
    for w, p in o["probes"].items():
        assert len(p) == 2 + 2 * sum(has), (w, len(p), has)
        pairs, at = [p[:2]], 2
        for on in has:
            pairs.append(p[at:at + 2] if on else None)
            at += 2 * on
        cut[w] = pairs
    return has, cut


def assert_same_run(dev, ref, windows=True, fb=True):
    """flow_cases.assert_same_run (verdicts, deliveries, flow rows, summary, histogram), and the cc, rto
    and fb rows and summaries, each where armed, at every probe and at the end.  fb=False: the fb rows,
    which only one of the two runs may have, aside."""
    (dcc, drt, dfb), dcut = _parts(dev)
    (rcc, rrt, rfb), rcut = _parts(ref)
    assert (dcc, drt) == (rcc, rrt) and (not fb or (dfb and rfb))
    plain = (lambda o, cut: dict(o, probes={w: p[0] for w, p in cut.items()}))
    fc.assert_same_run(plain(dev, dcut), plain(ref, rcut), windows=windows)
    assert dev["rows"].tobytes() == ref["rows"].tobytes()
    ends = lambda o, k: (o[k + "_rows"], o[k + "_summary"])  # noqa: E731
    for k, (on, check) in enumerate(((rcc, cc.assert_same_cc), (rrt, rc.assert_same_rto), (fb, assert_same_fb))):
        if not on:
            continue
        for w in rcut:
            check(dcut[w][1 + k], rcut[w][1 + k], f"probe after window {w}")
        check(ends(dev, ("cc", "rto", "fb")[k]), ends(ref, ("cc", "rto", "fb")[k]), "end of run")


def sum_identity(rows, fb_rows):
    """scheduled + lost + queue_full + refused == offered, for every flow."""
    tot = sum(fb_rows[k].astype(np.int64) for k in ("scheduled", "lost", "queue_full", "refused"))
    return bool((tot == rows["offered"]).all())


def identity_everywhere(out):
    return sum_identity(out["rows"], out["fb_rows"]) and all(sum_identity(p[0], p[-2]) for p in out["probes"].values())


def fail_tick(out, f):
    return int(out["rows"]["done_ns"][f]) // TICK


# -- 1, 2. cut at arming ---------------------------------------------------------------------------------------------
# flow_cases.CUT: 4 peers, peer 0 has a Drop (or Reject) rule towards peer 1 from the start.
# variant -> (flow, cc, rto, ticks until the timer fails flow 0, ticks of the run without a mask)
CUT_VARIANTS = {
    "plain": (fc.CUT_FLOW, None, None, fc.CUT_FLOW["max_attempts"] * fc.CUT_FLOW["rto_ticks"], fc.CUT["ticks"]),
    "cc": (fc.CUT_FLOW, cc.CUT_CC, None, fc.CUT_FLOW["max_attempts"] * fc.CUT_FLOW["rto_ticks"], fc.CUT["ticks"]),
    "ccrto": (rc.CUT_FLOW, cc.CUT_CC, rc.CUT_RTO, rc.CUT_FAIL_AFTER, rc.CUT_TICKS),
}


def cut_first(variant):
    """The segments flow 0 releases at its start tick."""
    flow, ccp = CUT_VARIANTS[variant][:2]
    return flow["window"] if ccp is None else ccp["init_cwnd"]


def run_cut(eng, device, variant, mask, window=fc.CUT["window"], action=nw.FilterAction.Drop):
    flow, ccp, rto, _, ticks = CUT_VARIANTS[variant]
    fc.plain(eng, fc.CUT["n"], fc.CUT["latency_ns"])
    eng.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=fc.CUT["latency_ns"]),
                               Rules=[fc.rule(1, action)]))
    flows = fc.cut_flows(eng.stats()["now_tick"])
    refuses = mask & (BLACKHOLE if action == nw.FilterAction.Drop else PROHIBIT)
    n_windows = (fc.CUT["ticks"] if refuses else ticks) // window  # (the timer's run is the long one)
    return drive(eng, device, flow, ccp, rto, dict(fail_mask=mask), flows, n_windows, window, probe_at=(0, 2, n_windows // 2))


# -- 3. partition mid-transfer -----------------------------------------------------------------------------------------
# flow_cases.HEAL's topology and flows; the rule is installed at tick 15,000 and stays.
PART = dict(tick=15_000, ticks=200_000)
PART_ACK_FLOW = dict(fc.HEAL_FLOW, max_attempts=4)  # the ACK leg cut: the timer fails the flow inside the run


def heal_flows(now):
    return fc.table([(0, 1, 40, now), (0, 2, 40, now), (2, 3, 12, now), (3, 0, 40, now + 7)])


def run_partition(eng, device, window=fc.HEAL["window"], ack_leg=False, mask=BLACKHOLE):
    """Data leg: peer 0 gets a Drop rule towards peer 1.  ACK leg: peer 1 gets one towards peer 0, so
    flow 0 -> 1's segments arrive and their ACKs are refused."""
    lat = fc.HEAL["latency_ns"]
    fc.plain(eng, fc.HEAL["n"], lat)
    flows = heal_flows(eng.stats()["now_tick"])
    at = PART["tick"] // window
    assert at * window == PART["tick"]
    peer, towards = (1, 0) if ack_leg else (0, 1)

    def before(w):
        if w == at:
            eng.configure(peer, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=lat),
                                          Rules=[fc.rule(towards, nw.FilterAction.Drop)]))

    n_windows = PART["ticks"] // window
    return drive(eng, device, PART_ACK_FLOW if ack_leg else fc.HEAL_FLOW, None, None, dict(fail_mask=mask), flows, n_windows,
                 window, probe_at=(0, at, n_windows // 2), before=before)


# -- 4. disconnect -------------------------------------------------------------------------------------------------------
# 4 peers, 5 ms each way; peer 0 sends at 10 Mbit/s (flow_cases.BW), so its segments queue at its HTB
# and arrive one serialisation time apart, up to several windows after they were offered.  Peer 1 goes
# Enable=false at tick 15,000 and comes back one 5,000-tick window later.  Flow 0 -> 1 (to it) fails on
# the first segment an ACK released into that window, flow 1 -> 2 (from it; started 7,000 ticks late so
# that a round of it falls into the window) on its next round.  Both legs are refused while the peer is
# away, and records count when a step emits them, so no ACK can reach a flow in the step that failed
# it; the segments of flow 0 still queued at peer 0 arrive all the same, peer 1 acknowledges them once it
# is back, and those ACKs find the flow FAILED: stale_acks.  Flow 2 -> 3 is untouched.
DISC_FLOW = dict(fc.BW_FLOW, max_attempts=16)
DISC_TICKS = 5_000


def run_disconnect(eng, device, window=fc.HEAL["window"], mask=DISCONNECTED):
    lat = fc.BW["latency_ns"]
    fc.plain(eng, 4, lat)
    eng.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=lat, Bandwidth=fc.BW["rate_bps"])))
    now = eng.stats()["now_tick"]
    flows = fc.table([(0, 1, 200, now), (1, 2, 40, now + 7_000), (2, 3, 12, now)])
    at, back = PART["tick"] // window, (PART["tick"] + DISC_TICKS) // window

    def before(w):
        if w in (at, back):
            eng.configure(1, nw.Config(Network="default", Enable=w == back, Default=nw.LinkShape(Latency=lat)))

    n_windows = 100_000 // window
    return drive(eng, device, DISC_FLOW, None, None, dict(fail_mask=mask), flows, n_windows, window,
                 probe_at=(0, at, n_windows // 2), before=before)


# -- 5. a timer failure and a refusal in one window ---------------------------------------------------------------------
# 3 peers, 5 ms each way, a netem queue of ONE packet.  A = 0 -> 1 (3 segments, window 2), B = 0 -> 2 (1
# segment, 10,000 ticks later), max_attempts 2, timer 12,000.  Segment 1 of A finds the queue full behind
# segment 0 at tick 0 and behind B's segment at tick 12,000, so its timer fails the flow at tick 24,000.
# Segment 2 of A, released at tick 10,002, finds the queue full behind B too and is offered again at
# 22,002, where a Reject rule 0 -> 1 installed at tick 20,000 refuses it: at 5,000-tick steps in the
# window whose generation has already failed the flow by its timer.
BOTH = dict(n=3, latency_ns=5 * MS, lookahead_ns=5 * MS, queue_limit=1, rule_tick=20_000, ticks=40_000)
BOTH_FLOW = dict(seg_len=500, ack_len=64, window=2, rto_ticks=12_000, max_attempts=2, bin_ns=MS, n_bins=64)


def both_kw():
    return dict(lookahead_ns=BOTH["lookahead_ns"], queue_limit=BOTH["queue_limit"])


def run_both(eng, device, window=5_000, mask=PROHIBIT):
    lat = BOTH["latency_ns"]
    fc.plain(eng, BOTH["n"], lat)
    now = eng.stats()["now_tick"]
    flows = fc.table([(0, 1, 3, now), (0, 2, 1, now + 10_000)])
    at = BOTH["rule_tick"] // window

    def before(w):
        if w == at:
            eng.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=lat),
                                       Rules=[fc.rule(1, nw.FilterAction.Reject)]))

    n_windows = BOTH["ticks"] // window
    return drive(eng, device, BOTH_FLOW, None, None, dict(fail_mask=mask), flows, n_windows, window,
                 probe_at=(0, at, n_windows - 2), before=before)


# -- 6. lossy mesh with cc, rto and fb ------------------------------------------------------------------------------------
# flow_rto_cases' mesh; at tick 80,000 (window 20 of 4,000 ticks) every fifth source gets a Drop rule
# towards its first flow's destination, keeping its shape.
MESH_CUT_TICK = 20 * fc.MESH["window"]
MESH_WINDOWS = 150  # (of 4,000 ticks: the flows the rules leave alone are done well before)


def run_mesh(eng, device, window=fc.MESH["window"], probe_at=None, fb=dict(fail_mask=ALL), cut=True, n_windows=MESH_WINDOWS):
    fc.configure_mesh(eng)
    flows = fc.mesh_flows(eng.stats()["now_tick"])
    lat, jit, bw = fc.mesh_shapes()
    at = MESH_CUT_TICK // window
    first_dst = {int(f["src"]): int(f["dst"]) for f in flows[::-1]}  # (the first flow of a source wins)

    def before(w):
        if cut and w == at:
            for s in range(0, fc.MESH["n"], 5):
                shape = nw.LinkShape(Latency=int(lat[s]), Jitter=int(jit[s]), Bandwidth=int(bw[s]), Loss=4.0, Duplicate=2.0,
                                     Corrupt=1.0)
                eng.configure(s, nw.Config(Network="default", Enable=True, Default=shape,
                                           Rules=[fc.rule(first_dst[s], nw.FilterAction.Drop)]))

    n_windows = n_windows * fc.MESH["window"] // window
    probe_at = (0, at, n_windows // 2) if probe_at is None else probe_at
    return drive(eng, device, cc.MESH_FLOW, cc.MESH_CC, rc.MESH_RTO, fb, flows, n_windows, window, probe_at=probe_at,
                 before=before)


# One more corner under parity: two flows of one source, window 16, into a netem queue of 4.
QFULL = dict(n=3, latency_ns=5 * MS, lookahead_ns=5 * MS, queue_limit=4, window=5_000, n_windows=30)
QFULL_FLOW = dict(seg_len=300, ack_len=40, window=16, rto_ticks=11_000, max_attempts=16, bin_ns=MS, n_bins=8)


def qfull_kw():
    return dict(lookahead_ns=QFULL["lookahead_ns"], queue_limit=QFULL["queue_limit"])


def run_qfull(eng, device):
    fc.plain(eng, QFULL["n"], QFULL["latency_ns"])
    now = eng.stats()["now_tick"]
    flows = fc.table([(0, 1, 40, now), (0, 2, 40, now)])
    return drive(eng, device, QFULL_FLOW, None, None, dict(fail_mask=ALL), flows, QFULL["n_windows"], QFULL["window"],
                 probe_at=(0, 3, QFULL["n_windows"] - 2))
