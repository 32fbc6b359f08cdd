"""The ping mesh at 100,000 peers, fanout 8 (profiles/LOG.md).

  wall   wall time per steady window of the device loop (Engine.ping_init + workloads.ping_run) and
         of the same loop driven from the host over the same HIP engine (workloads.ping_reference)
  run    the device loop alone, for a kernel trace:
           rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/ping_measure.py run
  trace  per-kernel device time of the k_ping_* and k_cal_* kernels in such a trace, beside their HBM floors
  sharded  what a sharded window costs on one GPU: the device loop of the single engine (ping_init +
         step) against the sharded form at one rank on the routed path (TGSIM_COMM_ROUTE1=1:
         ping_init(sharded=True) + comm_step, the N > 1 step's own kernels, delivered in place), and
         the time of one comm_ping_report.  One process, no retries: run it under a time limit.

Every link 5 ms, lossless, unlimited; 16 probes per slot, one every 2,500 ticks; windows of 5,000
ticks: a steady window offers 1.6 M probes and 1.6 M replies."""
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

N, FANOUT, WIN, LAT = 100_000, 8, 5_000, 5 * nw.Millisecond
PING = dict(count=16, interval_ticks=2_500, length=64, start_tick=0, bin_ns=nw.Millisecond, n_bins=32)
WINDOWS, STEADY = 12, range(3, 8)  # windows 3..7 hold two probe rounds and the replies to two
HBM_BPS = 6.3e12  # the measured rate DESIGN.md §5.5 uses


def engine(flags):
    eng = Engine(N, lookahead_ns=LAT, flags=flags)
    eng.configure_batch(np.arange(N), nw.configs_array(np.full(N, LAT)))
    return eng


def device_loop():
    eng, t = engine(abi.OPT_DISCARD_DELIVERIES), []
    eng.ping_init(wl.ping_targets_mesh(N, FANOUT, seed=9), **PING)
    for w in range(WINDOWS):
        eng.sync()
        t0 = time.perf_counter()
        eng.gen_ping(WIN)
        eng.step(WIN)
        eng.sync()
        t.append(time.perf_counter() - t0)
    return eng.ping_report(), t


def routed_loop():
    """The sharded form at one rank, routed (the environment is read by comm_init)."""
    os.environ["TGSIM_COMM_ROUTE1"] = "1"
    eng, t, rep_t = engine(abi.OPT_DISCARD_DELIVERIES), [], []
    eng.comm_init(comm_id(), 0, 1)
    eng.ping_init(wl.ping_targets_mesh(N, FANOUT, seed=9), sharded=True, **PING)
    for w in range(WINDOWS):
        eng.sync()
        t0 = time.perf_counter()
        eng.gen_ping(WIN)
        eng.comm_step(WIN)
        eng.sync()
        t.append(time.perf_counter() - t0)
    for _ in range(5):
        eng.sync()
        t0 = time.perf_counter()
        rep = eng.comm_ping_report()
        rep_t.append(time.perf_counter() - t0)
    return rep, t, rep_t, eng.ping_report()


def host_loop():
    eng, t = engine(0), []
    m = wl.PingModel(eng, PING, wl.ping_targets_mesh(N, FANOUT, seed=9))
    for w in range(WINDOWS):
        t0 = time.perf_counter()
        m.step(WIN)
        t.append(time.perf_counter() - t0)
    return m.report(), t


def main():
    mode = sys.argv[1]
    if mode == "run":
        print(json.dumps({k: int(v) for k, v in device_loop()[0].items() if k != "hist"}))
    elif mode == "wall":
        dev, td = device_loop()
        ref, th = host_loop()
        same = all(dev[k] == ref[k] for k in ("sent", "received", "sum_ns", "pairs_all", "pending_replies"))
        print(json.dumps({"peers": N, "fanout": FANOUT, "windows": WINDOWS, "reports_agree": same,
                          "received": int(dev["received"]), "sent": int(dev["sent"]),
                          "device_ms_per_window": [round(1e3 * x, 3) for x in td],
                          "host_ms_per_window": [round(1e3 * x, 1) for x in th],
                          "device_steady_ms": round(1e3 * statistics.median(td[w] for w in STEADY), 3),
                          "host_steady_ms": round(1e3 * statistics.median(th[w] for w in STEADY), 1)}))
    elif mode == "sharded":
        dev, td = device_loop()
        rep, tr, rep_t, local = routed_loop()
        keys = ("pairs", "sent", "received", "sum_ns", "min_ns", "max_ns", "pairs_all", "pairs_none", "pending_replies")
        same = all(dev[k] == rep[k] == local[k] for k in keys) and (dev["hist"] == rep["hist"]).all()
        print(json.dumps({"peers": N, "fanout": FANOUT, "windows": WINDOWS, "reports_agree": bool(same),
                          "received": int(rep["received"]), "sent": int(rep["sent"]),
                          "single_ms_per_window": [round(1e3 * x, 3) for x in td],
                          "routed_ms_per_window": [round(1e3 * x, 3) for x in tr],
                          "single_steady_ms": round(1e3 * statistics.median(td[w] for w in STEADY), 3),
                          "routed_steady_ms": round(1e3 * statistics.median(tr[w] for w in STEADY), 3),
                          "comm_ping_report_ms": [round(1e3 * x, 3) for x in rep_t],
                          "comm_ping_report_median_ms": round(1e3 * statistics.median(rep_t), 3)}))
    elif mode == "trace":
        per = {}
        for r in csv.DictReader(open(sys.argv[2])):
            name = r["Kernel_Name"].split("(")[0].split("::")[-1]
            if name.startswith(("k_ping_", "k_cal_")) or name in ("k_sim_sparse", "k_sim", "k_sim_list", "k_sim_multi"):
                per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        pk = N * FANOUT * 2  # probes (= replies) a steady window offers
        floors = {"k_ping_recv": 2 * pk * 24 + pk * 16, "k_cal_count": pk * 16, "k_ping_write_sched": pk * 16,
                  "k_cal_write": pk * 16 + pk * 16, "k_cal_order": 2 * pk * 16 * 2}
        out = {}
        for name, us in sorted(per.items()):
            out[name] = {"calls": len(us), "median_us": round(statistics.median(us), 1), "max_us": round(max(us), 1)}
            if name in floors:
                out[name]["floor_us_steady"] = round(floors[name] / HBM_BPS * 1e6, 1)
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
