"""The ping mesh at 100,000 peers, fanout 8 (profiles/LOG.md).

  wall   wall time per steady window of the device loop (Engine.ping_init + workloads.ping_run) and
         of the same loop driven from the host over the same HIP engine (workloads.ping_reference)
  run    the device loop alone, for a kernel trace:
           rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/ping_measure.py run
  trace  per-kernel device time of the k_ping_* kernels in such a trace, beside their HBM floors

Every link 5 ms, lossless, unlimited; 16 probes per slot, one every 2,500 ticks; windows of 5,000
ticks: a steady window offers 1.6 M probes and 1.6 M replies."""
import csv
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from testground_amd import abi, network as nw, workloads as wl  # noqa: E402
from testground_amd.engine import Engine  # noqa: E402

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
    elif mode == "trace":
        per = {}
        for r in csv.DictReader(open(sys.argv[2])):
            name = r["Kernel_Name"].split("(")[0].split("::")[-1]
            if name.startswith("k_ping_") or name in ("k_sim_sparse", "k_sim", "k_sim_list", "k_sim_multi"):
                per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        pk = N * FANOUT * 2  # probes (= replies) a steady window offers
        floors = {"k_ping_recv": 2 * pk * 24 + pk * 16, "k_ping_count_cal": pk * 16, "k_ping_write_sched": pk * 16,
                  "k_ping_write_cal": pk * 16 + pk * 16, "k_ping_order": 2 * pk * 16 * 2}
        out = {}
        for name, us in sorted(per.items()):
            out[name] = {"calls": len(us), "median_us": round(statistics.median(us), 1), "max_us": round(max(us), 1)}
            if name in floors:
                out[name]["floor_us_steady"] = round(floors[name] / HBM_BPS * 1e6, 1)
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
