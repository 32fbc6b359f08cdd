"""The flow driver at 100,000 peers, 8 flows per source (profiles/LOG.md).

  wall   wall time per steady window of the device loop (Engine.flow_init + workloads.flow_run) and
         of the same loop driven from the host over the same HIP engine (workloads.FlowModel; its
         first HOST_WINDOWS windows only: the model is plain Python)
  run    the device loop alone, for a kernel trace:
           rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/flow_measure.py run
  trace  per-kernel device time of the k_flow_* and shared k_ping_* kernels in such a trace (max_us: the
         busy windows, see below), beside the HBM floor of a busy window

Every link 5 ms, lossless, unlimited, reorder off; 800,000 flows of 64 segments of 1,000 bytes, window
8, ACKs of 64 bytes, a timer of 20 ms that never fires; windows of 5,000 ticks.  Every flow starts at
tick 0, so the windows alternate: 6.4 M segments, then their 6.4 M ACKs.

Slot k of every source s goes to peer (s + OFFSETS[k]) mod N, so a receiver acknowledges exactly one
sender per slot and no two of its ACKs share (tick, seq): without jitter such a tie is where the HIP
engine and the oracle differ, and a random table makes millions of them."""
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

N, PER_SOURCE, N_SEG, WIN, LAT = 100_000, 8, 64, 5_000, 5 * nw.Millisecond
FLOW = dict(seg_len=1000, ack_len=64, window=8, rto_ticks=20_000, max_attempts=4, bin_ns=10 * nw.Millisecond, n_bins=32)
WINDOWS, STEADY = 18, range(2, 14)  # 8 round trips of two windows each, the last ACKs in window 15
HOST_WINDOWS, HOST_STEADY = 4, range(2, 4)
HBM_BPS = 6.3e12  # the measured rate DESIGN.md §5.5 uses
OFFSETS = np.array([1, 17, 263, 4099, 9973, 31337, 54321, 77777])


def flow_table():
    t = wl.flow_table_mesh(N, PER_SOURCE, N_SEG, seed=9)
    t["dst"] = (t["src"].astype(np.int64) + np.tile(OFFSETS, N)) % N
    return t


def engine(flags):
    eng = Engine(N, lookahead_ns=LAT, flags=flags)
    eng.configure_batch(np.arange(N), nw.configs_array(np.full(N, LAT)))
    return eng


def device_loop(windows=WINDOWS):
    eng, t = engine(abi.OPT_DISCARD_DELIVERIES), []
    eng.flow_init(flow_table(), **FLOW)
    for w in range(windows):
        eng.sync()
        t0 = time.perf_counter()
        eng.gen_flow(WIN)
        eng.step(WIN)
        eng.sync()
        t.append(time.perf_counter() - t0)
    return eng.flow_report(), t


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
    if mode == "run":
        print(json.dumps({k: int(v) for k, v in device_loop()[0].items() if k != "hist"}))
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
            name = r["Kernel_Name"].split("(")[0].split("::")[-1]
            if name.startswith(("k_flow_", "k_ping_")) or name in ("k_sim_sparse", "k_sim", "k_sim_list", "k_sim_multi"):
                per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        flows, w = N * PER_SOURCE, FLOW["window"]
        seg = flows * w  # the windows alternate: a busy window carries 6.4 M segments or their 6.4 M ACKs
        state = flows * (16 + 32 + 8 + w * 5)  # spec, row, bitmap, timers
        floors = {"k_flow_recv_data": seg * 24 + seg * 16,          # a window of segments read, an entry each written
                  "k_flow_recv_ack": seg * 24 + flows * (16 + 2 * 32 + 2 * 8) + seg * 5,  # ACKs once, state in and out, timers
                  "k_flow_count": state, "k_flow_write": state + seg * 16 + seg * 5 + flows * 32,
                  "k_ping_count_cal": seg * 16, "k_ping_write_cal": seg * 16 + seg * 16, "k_ping_order": seg * 16 * 2}
        out = {}
        for name, us in sorted(per.items()):
            out[name] = {"calls": len(us), "median_us": round(statistics.median(us), 1), "max_us": round(max(us), 1)}
            if name in floors:
                out[name]["floor_us_busy"] = round(floors[name] / HBM_BPS * 1e6, 1)
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
