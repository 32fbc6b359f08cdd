"""The flow driver at 100,000 peers, 8 flows per source (profiles/LOG.md).

  wall   wall time per steady window of the device loop (Engine.flow_init + workloads.flow_run) and
         of the same loop driven from the host over the same HIP engine (workloads.FlowModel; its
         first HOST_WINDOWS windows only: the model is plain Python)
  run    the device loop alone, for a kernel trace:
           rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/flow_measure.py run
  trace  per-kernel device time of the k_flow_* and the calendar's k_cal_* kernels in such a trace (max_us: the
         busy windows, see below), beside the HBM floor of a busy window
  steady the device loop alone: wall time per window and the median over the steady windows (the A/B
         figure: run it with TGSIM_LIB naming another build of the library)
  sharded  what a sharded window costs on one GPU: the device loop of the single engine (flow_init +
         step) against the sharded form at one rank on the routed path (TGSIM_COMM_ROUTE1=1:
         flow_init(sharded=True) + comm_step, the N > 1 step's own kernels, delivered in place), and
         the time of one comm_flow_report.  One process, no retries: run it under a time limit.
  curve  goodput per flow against link loss, with and without congestion control (the README's table)
  hetero 10,000 peers with latencies U[1,100] ms: a fixed timer of 60 ms, one above the largest round
         trip, and the RTT estimator from that same timer (the README's table)
  partition  the curve's 10,000 peers, links and flows with congestion control; at tick 100,000 every
         peer of region A (16.0.0.0/19: peers 0..8,189) gets a Drop rule for region B's prefix
         (16.0.32.0/19: the other 1,810).  Once with the verdict feedback failing flows on a refusal,
         once with fail_mask 0 (counted only: the timers fail them): flows failed and by what, the mean
         and largest fail tick - partition tick, the data packets offered after the partition
         (the README's table)

`--cc` arms run, steady and trace with congestion control (init_cwnd 2, dupthresh 3,
the cap `window` as without) and `--loss PCT` puts that loss on every link; with either the run takes
CC_WINDOWS windows, since the windows open from 2 segments and lost ones wait for a timer.  `--rto`
arms them with the RTT estimator as well (from the timer of 20 ms, a floor of one
window, backoff on), with or without `--cc`.  `--fb` arms them with the verdict feedback (DESIGN.md
§5.11, fail_mask = every refusal): nothing is refused in this workload, so it times the fold alone.

Every link 5 ms, lossless, unlimited, reorder off; 800,000 flows of 64 segments of 1,000 bytes, window
8, ACKs of 64 bytes, a timer of 20 ms that never fires; windows of 5,000 ticks.  Every flow starts at
tick 0, so the windows alternate: 6.4 M segments, then their 6.4 M ACKs.

Slot k of every source s goes to peer (s + OFFSETS[k]) mod N, so a receiver acknowledges exactly one
sender per slot and no two of its ACKs share (tick, seq): without jitter such a tie is where the HIP
engine and the oracle differ, and a random table makes millions of them."""
import csv
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from testground_amd import abi, network as nw, workloads as wl  # noqa: E402
from testground_amd.engine import Engine, comm_id  # noqa: E402

N, PER_SOURCE, N_SEG, WIN, LAT = 100_000, 8, 64, 5_000, 5 * nw.Millisecond
FLOW = dict(seg_len=1000, ack_len=64, window=8, rto_ticks=20_000, max_attempts=4, bin_ns=10 * nw.Millisecond, n_bins=32)
WINDOWS, STEADY = 18, range(2, 14)  # 8 round trips of two windows each, the last ACKs in window 15
HOST_WINDOWS, HOST_STEADY = 4, range(2, 4)
HBM_BPS = 6.3e12  # the measured rate DESIGN.md §5.5 uses
CC = dict(init_cwnd=2, init_ssthresh=0, dupthresh=3)
CC_WINDOWS, CC_STEADY = 44, range(8, 24)  # from 2 segments: 2, 4, then 8 a round trip; every flow ACTIVE in these windows
# curve: 10,000 peers, 8 flows each of 64 segments over links of 5 ms and 10 Mbit/s (a source's 8 flows share
# the link: 12.5 KB of bandwidth-delay product against 64 KB of fixed windows), a timer of 60 ms
CURVE = dict(n=10_000, rate_bps=10_000_000, rto_ticks=60_000, max_windows=1200, losses=(0.0, 0.5, 1.0, 2.0, 4.0))
OFFSETS = np.array([1, 17, 263, 4099, 9973, 31337, 54321, 77777])
RTO = dict(min_rto_ticks=WIN, max_rto_ticks=2_000_000, backoff=1)
# hetero: per-peer latency U[1,100] ms (round trips of 2 to 200 ms), jitter U[0.1,0.5] ms on every peer, 1 %
# loss; the minimum netem delay is 0.5 ms, which is the lookahead and the window.  Unlimited links.
FB = dict(fail_mask=abi.FLOW_FB_REFUSALS)
PARTITION = dict(at_window=20, prefix_b=("16.0.32.0", 19), first_b=(1 << 13) - 2, max_windows=1200)
HETERO = dict(n=10_000, win=500, lookahead_ns=nw.Millisecond // 2, loss=1.0, above_ticks=210_000, max_windows=16_000,
              bin_ns=20 * nw.Millisecond, n_bins=256, seed=11)


def flow_table(n=N):
    t = wl.flow_table_mesh(n, PER_SOURCE, N_SEG, seed=9)
    t["dst"] = (t["src"].astype(np.int64) + np.tile(OFFSETS % n, n)) % n
    return t


def engine(flags, loss=0.0, n=N, rate_bps=0):
    eng = Engine(n, lookahead_ns=LAT, flags=flags)
    eng.configure_batch(np.arange(n), nw.configs_array(np.full(n, LAT), loss=np.full(n, loss, dtype=np.float32),
                                                       bandwidth_bps=np.full(n, rate_bps)))
    return eng


def device_loop(windows=WINDOWS, cc=None, loss=0.0, rto=None, fb=None):
    eng, t = engine(abi.OPT_DISCARD_DELIVERIES, loss), []
    eng.flow_init(flow_table(), cc=cc, rto=rto, fb=fb, **FLOW)
    for w in range(windows):
        eng.sync()
        t0 = time.perf_counter()
        eng.gen_flow(WIN)
        eng.step(WIN)
        eng.sync()
        t.append(time.perf_counter() - t0)
    rep = eng.flow_report()
    if cc is not None:
        rep["cc"] = eng.flow_cc_report()
    if rto is not None:
        rep["rto"] = eng.flow_rto_report()
    if fb is not None:
        rep["fb"] = eng.flow_fb_report()
    return rep, t


def routed_loop(windows=WINDOWS, cc=None, loss=0.0, rto=None, fb=None):
    """The sharded form at one rank, routed (the environment is read by comm_init)."""
    os.environ["TGSIM_COMM_ROUTE1"] = "1"
    eng, t, rep_t = engine(abi.OPT_DISCARD_DELIVERIES, loss), [], []
    eng.comm_init(comm_id(), 0, 1)
    eng.flow_init(flow_table(), cc=cc, rto=rto, fb=fb, sharded=True, **FLOW)
    for w in range(windows):
        eng.sync()
        t0 = time.perf_counter()
        eng.gen_flow(WIN)
        eng.comm_step(WIN)
        eng.sync()
        t.append(time.perf_counter() - t0)
    for _ in range(5):
        eng.sync()
        t0 = time.perf_counter()
        rep = eng.comm_flow_report()
        rep_t.append(time.perf_counter() - t0)
    return rep, t, rep_t, eng.flow_report()


def hist_quantile_ms(hist, q, bin_ns):
    """The upper edge (ms) of the histogram bin that holds the q-quantile of the DONE flows."""
    c = np.cumsum(hist)
    return None if not c[-1] else round(float((np.searchsorted(c, q * c[-1]) + 1) * bin_ns) / 1e6, 1)


def hetero_point(name, rto_ticks, rto):
    """One row of the hetero table: run to the end (or max_windows)."""
    h = HETERO
    n, rng = h["n"], np.random.default_rng(h["seed"])
    lat = rng.integers(nw.Millisecond, 100 * nw.Millisecond + 1, n)
    jit = rng.integers(nw.Millisecond // 10, nw.Millisecond // 2 + 1, n)
    eng = Engine(n, lookahead_ns=h["lookahead_ns"], flags=abi.OPT_DISCARD_DELIVERIES)
    eng.configure_batch(np.arange(n), nw.configs_array(lat, jitter_ns=jit, loss=np.full(n, h["loss"], dtype=np.float32)))
    eng.flow_init(flow_table(n), cc=CC, rto=rto,
                  **dict(FLOW, rto_ticks=rto_ticks, max_attempts=16, n_bins=h["n_bins"], bin_ns=h["bin_ns"]))
    windows, t0 = 0, time.perf_counter()
    while windows < h["max_windows"]:
        wl.flow_run(eng, 500, h["win"])
        windows += 500
        if eng.flow_report()["active"] == 0:
            break
    eng.sync()
    wall = time.perf_counter() - t0
    rep, cc = eng.flow_report(), eng.flow_cc_report()
    out = {"row": name, "rto_ticks": rto_ticks, "rto": rto, "windows": windows, "wall_s": round(wall, 2),
           "done": rep["done"], "failed": rep["failed"], "active": rep["active"],
           "fct_ms_mean": round(rep["fct_sum_ns"] / rep["done"] / 1e6, 1) if rep["done"] else None,
           "fct_ms_p99_bin_edge": hist_quantile_ms(rep["hist"], 0.99, h["bin_ns"]),
           "retransmits": rep["retransmits"], "stale_acks": rep["stale_acks"], "timeouts": cc["timeouts"],
           "fast_retransmits": cc["fast_retransmits"], "loss_events": cc["loss_events"], "segs_acked": rep["segs_acked"]}
    if rto is not None:
        out["rto_report"] = eng.flow_rto_report()
    return out


def curve_point(loss, cc):
    """One run of the curve's table to the end (or max_windows): the mean over the DONE flows of their own
    goodput, bytes * 8 / FCT."""
    n = CURVE["n"]
    eng = engine(abi.OPT_DISCARD_DELIVERIES, loss, n, CURVE["rate_bps"])
    eng.flow_init(flow_table(n), cc=cc, **dict(FLOW, rto_ticks=CURVE["rto_ticks"], max_attempts=16, n_bins=0, bin_ns=0))
    windows = 0
    while windows < CURVE["max_windows"]:
        wl.flow_run(eng, 40, WIN)
        windows += 40
        if eng.flow_report()["active"] == 0:
            break
    rows, rep = eng.flow_rows(), eng.flow_report()
    done = rows[rows["state"] == abi.FLOW_DONE]
    goodput = N_SEG * FLOW["seg_len"] * 8e9 / done["done_ns"].astype(np.float64) if len(done) else np.zeros(1)
    out = {"loss_pct": loss, "cc": cc is not None, "windows": windows, "done": int(rep["done"]), "failed": int(rep["failed"]),
           "active": int(rep["active"]), "goodput_bps_per_flow_mean": round(float(goodput.mean())),
           "fct_ms_mean": round(float(done["done_ns"].mean()) / 1e6, 2) if len(done) else None,
           "retransmits_per_segment": round(rep["retransmits"] / max(rep["segs_acked"], 1), 4)}
    if cc is not None:
        out["cc"] = eng.flow_cc_report()
    return out


def partition_point(fail_mask):
    """One run of the partition to the end (or max_windows)."""
    n, p = CURVE["n"], PARTITION
    eng = engine(abi.OPT_DISCARD_DELIVERIES, 0.0, n, CURVE["rate_bps"])
    eng.flow_init(flow_table(n), cc=CC, fb=dict(fail_mask=fail_mask),
                  **dict(FLOW, rto_ticks=CURVE["rto_ticks"], max_attempts=16, n_bins=0, bin_ns=0))
    wl.flow_run(eng, p["at_window"], WIN)
    before, cut_tick = eng.flow_report(), eng.stats()["now_tick"]
    shape = nw.LinkShape(Latency=LAT, Bandwidth=CURVE["rate_bps"])
    for i in range(p["first_b"]):  # region A: every peer below 16.0.32.0
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=shape,
                                   Rules=[nw.LinkRule(Subnet=p["prefix_b"], LinkShape=nw.LinkShape(Filter=nw.FilterAction.Drop))]))
    windows, t0 = p["at_window"], time.perf_counter()
    while windows < p["max_windows"]:
        wl.flow_run(eng, 40, WIN)
        windows += 40
        if eng.flow_report()["active"] == 0:
            break
    eng.sync()
    wall = time.perf_counter() - t0
    rows, frows, rep, frep = eng.flow_rows(), eng.flow_fb_rows(), eng.flow_report(), eng.flow_fb_report()
    failed = rows["state"] == abi.FLOW_FAILED
    after = rows["done_ns"].astype(np.int64) // eng.tick_ns - cut_tick
    by = {"verdict": after[failed & (frows["fail_verdict"] > 0)], "timer": after[failed & (frows["fail_verdict"] == 0)]}
    t = flow_table(n)
    return {"fail_mask": fail_mask, "peers": n, "flows": len(t), "partition_tick": int(cut_tick),
            "flows_a_to_b": int(((t["src"] < p["first_b"]) & (t["dst"] >= p["first_b"])).sum()),
            "flows_b_to_a": int(((t["src"] >= p["first_b"]) & (t["dst"] < p["first_b"])).sum()),
            "windows": windows, "wall_s_after_partition": round(wall, 2), "done": rep["done"], "failed": rep["failed"],
            "active": rep["active"], "failed_by_verdict": int((failed & (frows["fail_verdict"] > 0)).sum()),
            "failed_by_timer": frep["failed_timer"],
            **{f"fail_after_partition_ticks_{stat}_by_{k}": (None if not len(v) else round(float(v.mean()), 1) if stat == "mean"
                                                             else int(v.max())) for k, v in by.items() for stat in ("mean", "max")},
            "data_offered_after_partition": rep["data_offered"] - before["data_offered"],
            "refused": frep["refused"], "retransmits": rep["retransmits"], "fb": frep}


def host_loop(windows=HOST_WINDOWS):
    eng, t = engine(0), []
    m = wl.FlowModel(eng, FLOW, flow_table())
    for w in range(windows):
        t0 = time.perf_counter()
        m.step(WIN)
        t.append(time.perf_counter() - t0)
    return m.report(), t


def main():
    mode = sys.argv[1]
    cc = CC if "--cc" in sys.argv else None
    rto = RTO if "--rto" in sys.argv else None
    fb = FB if "--fb" in sys.argv else None
    loss = float(sys.argv[sys.argv.index("--loss") + 1]) if "--loss" in sys.argv else 0.0
    windows, steady = (CC_WINDOWS, CC_STEADY) if cc is not None or loss else (WINDOWS, STEADY)
    if mode == "run":
        print(json.dumps({k: v for k, v in device_loop(windows, cc, loss, rto, fb)[0].items() if k != "hist"}))
    elif mode == "steady":
        rep, td = device_loop(windows, cc, loss, rto, fb)
        print(json.dumps({"cc": cc, "rto": rto, "fb": fb, "loss_pct": loss, "windows": windows, "steady": [steady[0], steady[-1]],
                          "report": {k: v for k, v in rep.items() if k != "hist"},
                          "device_ms_per_window": [round(1e3 * x, 3) for x in td],
                          "device_steady_ms": round(1e3 * statistics.median(td[w] for w in steady), 3),
                          "device_steady_min_max_ms": [round(1e3 * min(td[w] for w in steady), 3),
                                                       round(1e3 * max(td[w] for w in steady), 3)]}))
    elif mode == "sharded":
        dev, td = device_loop(windows, cc, loss, rto, fb)
        rep, tr, rep_t, local = routed_loop(windows, cc, loss, rto, fb)
        same = all(dev[k] == rep[k] == local[k] for k in abi.FLOW_SUMMARY_FIELDS) and (dev["hist"] == rep["hist"]).all()
        same = same and all(dev[k] == rep[k] for k in ("cc", "rto", "fb") if k in dev)
        print(json.dumps({"peers": N, "flows": N * PER_SOURCE, "cc": cc, "rto": rto, "fb": fb, "loss_pct": loss, "windows": windows,
                          "steady": [steady[0], steady[-1]], "reports_agree": bool(same), "done": int(rep["done"]),
                          "segs_acked": int(rep["segs_acked"]),
                          "single_ms_per_window": [round(1e3 * x, 3) for x in td],
                          "routed_ms_per_window": [round(1e3 * x, 3) for x in tr],
                          "single_steady_ms": round(1e3 * statistics.median(td[w] for w in steady), 3),
                          "routed_steady_ms": round(1e3 * statistics.median(tr[w] for w in steady), 3),
                          "comm_flow_report_ms": [round(1e3 * x, 3) for x in rep_t],
                          "comm_flow_report_median_ms": round(1e3 * statistics.median(rep_t), 3)}))
    elif mode == "curve":
        for loss_pct in CURVE["losses"]:
            for c in (None, CC):
                print(json.dumps(curve_point(loss_pct, c)), flush=True)
    elif mode == "partition":
        for mask in (FB["fail_mask"], 0):
            print(json.dumps(partition_point(mask)), flush=True)
    elif mode == "hetero":
        h = HETERO
        for row in (("fixed 60 ms", 60_000, None), ("fixed above the largest round trip", h["above_ticks"], None),
                    ("adaptive", h["above_ticks"], dict(min_rto_ticks=h["win"], max_rto_ticks=RTO["max_rto_ticks"], backoff=1))):
            print(json.dumps(hetero_point(*row)), flush=True)
    elif mode == "wall":
        dev, td = device_loop()
        short, _ = device_loop(HOST_WINDOWS)
        ref, th = host_loop()
        keys = ("segs_acked", "data_offered", "retransmits", "stale_acks", "pending_acks", "done")
        print(json.dumps({"peers": N, "flows": N * PER_SOURCE, "windows": WINDOWS, "host_windows": HOST_WINDOWS,
                          "reports_agree_after_host_windows": all(short[k] == ref[k] for k in keys),
                          "done": int(dev["done"]), "segs_acked": int(dev["segs_acked"]),
                          "retransmits": int(dev["retransmits"]), "fct_min_ns": int(dev["fct_min_ns"]),
                          "fct_max_ns": int(dev["fct_max_ns"]),
                          "device_ms_per_window": [round(1e3 * x, 3) for x in td],
                          "host_ms_per_window": [round(1e3 * x, 1) for x in th],
                          "device_steady_ms": round(1e3 * statistics.median(td[w] for w in STEADY), 3),
                          "host_steady_ms": round(1e3 * statistics.median(th[w] for w in HOST_STEADY), 1)}))
    elif mode == "trace":
        per = {}
        for r in csv.DictReader(open(sys.argv[2])):
            name = r["Kernel_Name"].split("(")[0].split("<")[0].split("::")[-1].split()[-1]  # (void k_flow_write<true, false>(...))
            if name.startswith(("k_flow_", "k_cal_")) or name in ("k_sim_sparse", "k_sim", "k_sim_list", "k_sim_multi"):
                per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        flows, w = N * PER_SOURCE, FLOW["window"]
        seg = flows * w  # the windows alternate: a busy window carries 6.4 M segments or their 6.4 M ACKs
        ccb = 32 if cc is not None else 0  # the cc row beside the flow row
        rtb, snt = (32, 4) if rto is not None else (0, 0)  # the rto row; a `sent` tick per ring slot
        state = flows * (16 + 32 + ccb + 8 + w * 5)  # spec, row, bitmap, timers
        floors = {"k_flow_recv_data": seg * 24 + seg * 16,          # a window of segments read, an entry each written
                  # ACKs once, state in and out, timers (rto: a `sent` tick read per ACK)
                  "k_flow_recv_ack": seg * 24 + flows * (16 + 2 * (32 + ccb + rtb) + 2 * 8) + seg * (5 + snt),
                  # (rto: the row's timer read, a `sent` tick written per first offer)
                  "k_flow_count": state, "k_flow_write": state + seg * 16 + seg * (5 + snt) + flows * (32 + ccb + rtb),
                  # (fb: the window's packets and verdict bytes, and in a window of segments the fb row in and out)
                  "k_flow_fb": seg * 17 + flows * 2 * 32,
                  "k_flow_rto_report": flows * 32,
                  "k_flow_cc_report": flows * (32 + 32),  # the cc row, and the flow row for its state
                  "k_cal_count": seg * 16, "k_cal_write": seg * 16 + seg * 16, "k_cal_order": seg * 16 * 2}
        out = {}
        for name, us in sorted(per.items()):
            out[name] = {"calls": len(us), "median_us": round(statistics.median(us), 1), "max_us": round(max(us), 1)}
            if name in floors:
                out[name]["floor_us_busy"] = round(floors[name] / HBM_BPS * 1e6, 1)
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
