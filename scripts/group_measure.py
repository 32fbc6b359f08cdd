"""The per-group traffic matrix at size (profiles/LOG.md).

  run WORKLOAD   armed windows of `storm` (C3: 10,000 instances, lambda 0.5, 2,000 ticks) or `gossip`
                 (1M peers, 64 floods, 5,000 ticks) for each layout (3 groups interleaved, 16 and 64
                 contiguous), the matrix read after every window; prints the packets offered and the
                 records delivered per window.  For a kernel trace of its own (no counters):
                   rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \
                       python scripts/group_measure.py run storm run_storm.json
  trace CSV JSON per-window device time of k_group_src and k_group_dst in such a trace (the k_group_read
                 of every window's read delimits the windows) beside their HBM floors: 17 B per offered
                 packet + a 2-B gather, and 24 B + a 2-B gather per delivered record
  wall           wall time per C3 window of three ways to the matrix, all fed the same host-made packets:
                 armed (the device folds), the host route the engine had before (keep deliveries,
                 drain + verdicts, GroupMatrix.fold), and TGSIM_OPT_METRICS alone (row and column
                 sums only); and of device-generated C3 windows armed against unarmed"""
import csv
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from testground_amd import abi, workloads as wl  # noqa: E402
from testground_amd.engine import Engine  # noqa: E402

HBM_BPS = 6.3e12  # the measured rate DESIGN.md §5.5 uses
STORM = dict(n=10_000, lam=0.5, window=2_000, windows=8)
GOSSIP = dict(n=1_000_000, floods=64, gap=1_000, window=5_000, windows=40)
LAYOUTS = {"3_interleaved": lambda n: (np.arange(n) % 3, 3),
           "16_contiguous": lambda n: (np.arange(n) * 16 // n, 16),
           "64_contiguous": lambda n: (np.arange(n) * 64 // n, 64)}


def run(workload, out_path=None):
    out = {}
    for name, layout in LAYOUTS.items():
        p = STORM if workload == "storm" else GOSSIP
        n = p["n"]
        eng = Engine(n, flags=abi.OPT_DISCARD_DELIVERIES, **({} if workload == "storm" else {"lookahead_ns": wl.GOSSIP_MIN_LAT}))
        if workload == "storm":
            wl.configure_storm(eng, n)
        else:
            wl.configure_gossip(eng, n)
            eng.gossip_init(n_floods=p["floods"], degree=8, msg_len=1024, start_gap_ticks=p["gap"], start_tick=0)
        eng.groups_init(*layout(n))
        rows, prev = [], np.zeros(2, dtype=np.int64)
        for _ in range(p["windows"]):
            eng.gen_storm(p["lam"], p["window"]) if workload == "storm" else eng.gen_gossip(p["window"])
            eng.step(p["window"])
            m = eng.group_matrix()
            tot = np.array([m[:, :, 0].sum(), m[:, :, 10].sum()], dtype=np.int64)
            rows.append((tot - prev).tolist())
            prev = tot
        out[name] = rows
        eng.close()
    text = json.dumps({"workload": workload, "windows": out})
    if out_path:
        Path(out_path).write_text(text + "\n")
    print(text)


def trace(csv_path, json_path):
    meta = json.load(open(json_path))
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    wins, cur = [], {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        if name in ("k_group_src", "k_group_dst"):
            cur[name] = cur.get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        elif name == "k_group_read":
            wins.append(cur)
            cur = {}
    out, at = {"workload": meta["workload"]}, 0
    for layout, counts in meta["windows"].items():
        mine = wins[at:at + len(counts)]
        at += len(counts)
        peak = max(c[0] for c in counts)
        steady = [i for i, c in enumerate(counts) if c[0] >= 0.5 * peak]  # the windows that carry traffic
        res = {"windows": len(counts), "steady_windows": len(steady)}
        for k, kern, per in ((0, "k_group_src", 19), (1, "k_group_dst", 26)):
            us = [mine[i].get(kern, 0.0) for i in steady]
            floor = [counts[i][k] * per / HBM_BPS * 1e6 for i in steady]
            res[kern] = {"median_us": round(statistics.median(us), 1), "max_us": round(max(us), 1),
                         "items_median": int(statistics.median(counts[i][k] for i in steady)),
                         "floor_us_median": round(statistics.median(floor), 1),
                         "ratio_median": round(statistics.median(u / f for u, f in zip(us, floor) if f), 2)}
        out[layout] = res
    assert at == len(wins), (at, len(wins))
    print(json.dumps(out, indent=1))


def wall():
    n, lam, window, k = STORM["n"], STORM["lam"], STORM["window"], 4
    rng, seqs, pks = np.random.default_rng(1), np.zeros(n, dtype=np.int64), []
    for _ in range(k):  # C3's traffic made on the host: uniform all-to-all, U[64, 1500] B, running seqs
        m = int(n * lam * window)
        pk = np.zeros(m, dtype=abi.PKT_DTYPE)
        src = np.sort(rng.integers(0, n, m))
        pk["src"], pk["dst"] = src, (src + 1 + rng.integers(0, n - 1, m)) % n
        pk["len"], pk["tick"] = rng.integers(64, 1501, m), rng.integers(0, window, m)
        counts = np.bincount(src, minlength=n)
        pk["seq"] = seqs[src] + np.arange(m) - np.repeat(np.cumsum(counts) - counts, counts)
        seqs += counts
        pks.append(pk)
    group_of, g = LAYOUTS["3_interleaved"](n)

    def timed(flags, armed, host):
        eng = Engine(n, flags=flags)
        wl.configure_storm(eng, n)
        if armed:
            eng.groups_init(group_of, g)
        gm, t = wl.GroupMatrix(group_of, g), []
        for pk in pks:
            eng.sync()
            t0 = time.perf_counter()
            eng.submit(pk)
            eng.step(window)
            if host:
                gm.fold(pk, eng.verdicts(), eng.drain())
            eng.sync()
            t.append(time.perf_counter() - t0)
        m = eng.group_matrix() if armed else gm.m if host else eng.metrics()
        return m, [round(1e3 * x, 2) for x in t]

    ma, ta = timed(abi.OPT_DISCARD_DELIVERIES, True, False)
    mh, th = timed(0, False, True)
    mm, tm = timed(abi.OPT_DISCARD_DELIVERIES | abi.OPT_METRICS, False, False)

    def generated(armed):
        eng = Engine(n, flags=abi.OPT_DISCARD_DELIVERIES)
        wl.configure_storm(eng, n)
        if armed:
            eng.groups_init(group_of, g)
        t = []
        for _ in range(12):
            eng.gen_storm(lam, window)
            eng.sync()
            t0 = time.perf_counter()
            eng.step(window)
            eng.sync()
            t.append(time.perf_counter() - t0)
        return [round(1e3 * x, 3) for x in t]

    rows = np.zeros((g, 10), dtype=np.uint64)
    np.add.at(rows, group_of, mm["src"][:, :10])
    print(json.dumps({"peers": n, "lambda": lam, "window": window, "packets_per_window": [len(p) for p in pks],
                      "matrices_agree": bool((ma == mh).all()),
                      "metrics_row_sums_agree": bool((ma[:, :, :10].sum(axis=1, dtype=np.uint64) == rows).all()),
                      "armed_ms": ta, "host_route_ms": th, "metrics_only_ms": tm,
                      "generated_armed_ms": generated(True), "generated_unarmed_ms": generated(False)}))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    elif sys.argv[1] == "trace":
        trace(sys.argv[2], sys.argv[3])
    else:
        wall()
