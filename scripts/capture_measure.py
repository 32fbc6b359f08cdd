"""What the packet capture costs at size (profiles/LOG.md).  GPU only.

The C3 storm (10,000 instances, lambda 0.5, 2,000 ticks: 10 M offered packets per window) with
TGSIM_OPT_DISCARD_DELIVERIES, windows generated and stepped one by one with tgsim_step (unfused in every
configuration, so the three differ only in the capture), 200 timed windows after a warm-up.  Three
configurations alternate in one process, three rounds each:

  unarmed   no capture
  w16       16 watched peers, one read at the end
  w1024     1,024 watched peers, a read every 10 windows

One JSON line per run, appended to profiles/capture/measure.jsonl (or the path given): wall time per
window, the engine's own simulate-kernel and delivery spans per window (tgsim_sim_kernel_ms brackets
k_sim alone, so the TX capture behind it shows in the wall time only; tgsim_delivery_kernel_ms brackets
the whole delivery, the RX capture included), the time spent inside the reads (their synchronization
and the copy into pageable host memory), and the records and bytes captured per window."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from testground_amd import abi, workloads as wl  # noqa: E402
from testground_amd.engine import Engine  # noqa: E402

STORM = dict(n=10_000, lam=0.5, window=2_000, warmup=20, windows=200)
CONFIGS = {"unarmed": (0, 0), "w16": (16, 0), "w1024": (1024, 10)}  # name -> (watched peers, windows per read)
ROOM = 1 << 24  # records per direction: ten windows of 1,024 storm sources (~1 M records a window) fit
REC = abi.CAPTURE_DTYPE.itemsize


def one(name, rnd):
    n, lam, window = STORM["n"], STORM["lam"], STORM["window"]
    watched, every = CONFIGS[name]
    eng = Engine(n, flags=abi.OPT_DISCARD_DELIVERIES)
    wl.configure_storm(eng, n)
    if watched:
        eng.capture_init(np.linspace(0, n - 1, watched).astype(np.int64), tx_cap=ROOM, rx_cap=ROOM)

    def windows(k):
        got = [0, 0, 0.0]  # TX records, RX records, seconds inside the reads (their synchronization included)
        for w in range(k):
            eng.gen_storm(lam, window)
            eng.step(window)
            if every and (w + 1) % every == 0:
                t = time.perf_counter()
                r = eng.capture_read()
                got[2] += time.perf_counter() - t
                got[0], got[1] = got[0] + len(r["tx"]), got[1] + len(r["rx"])
        return got

    windows(STORM["warmup"])
    if watched:
        eng.capture_read()
    eng.sync()
    eng.sim_kernel_ms(reset=True)
    eng.delivery_kernel_ms(reset=True)
    offered0 = eng.stats()["offered"]
    t0 = time.perf_counter()
    got = windows(STORM["windows"])
    eng.sync()
    wall = time.perf_counter() - t0
    sim_ms, sim_n = eng.sim_kernel_ms()  # (both are averages per window already)
    dv_ms, dv_n = eng.delivery_kernel_ms()
    out = {"config": name, "round": rnd, "peers": n, "watched": watched, "windows": STORM["windows"],
           "read_every": every, "wall_us_per_window": round(1e6 * wall / STORM["windows"], 2),
           "sim_kernel_us_per_window": round(1e3 * sim_ms, 2), "sim_windows_timed": sim_n,
           "delivery_us_per_window": round(1e3 * dv_ms, 2), "delivery_windows_timed": dv_n,
           "offered_per_window": (eng.stats()["offered"] - offered0) // STORM["windows"]}
    if watched:
        info = eng.capture_info()
        r = eng.capture_read()
        got = [got[0] + len(r["tx"]), got[1] + len(r["rx"]), got[2]]
        out.update(tx_records_per_window=got[0] // STORM["windows"], rx_records_per_window=got[1] // STORM["windows"],
                   capture_bytes_per_window=(got[0] + got[1]) * REC // STORM["windows"],
                   read_us_per_window=round(1e6 * got[2] / STORM["windows"], 2),
                   dropped=info["dropped"]["tx"] + info["dropped"]["rx"])
    eng.close()
    return out


def main(path):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("capture_measure: needs a GPU")
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a") as f:
        for rnd in range(3):
            for name in CONFIGS:
                line = json.dumps(one(name, rnd))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "capture" / "measure.jsonl")
