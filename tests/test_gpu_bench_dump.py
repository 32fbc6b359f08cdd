"""bench.py --dump-outputs: the files hold what the timed path computed in its last timed step, the
same from run to run, and --steps is the number of windows the timed path really ran.  A small storm
through bench.run_workload in this process (the bench's own settle, warm-up and timed stretches, the
latter cut into stretches of RESIDENT_WINDOWS), checked against the CPU oracle stepping the same
windows one by one."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from testground_amd import abi  # noqa: E402
from testground_amd import workloads as wl  # noqa: E402

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None

N, WINDOW, STEPS, WARMUP = 300, 200, 5, 1
ARGS = ["--peers", str(N), "--window", str(WINDOW), "--steps", str(STEPS), "--warmup", str(WARMUP), "--settle-ms", "1"]


def _run(tmp):
    a = bench.parse(ARGS + ["--dump-outputs", str(tmp)])
    res = bench.run_workload(a, "storm", a.peers, a.steps, a.warmup, a.window, a.lam, 1, 0, 0, None,
                             want_cpu=False, split=True, dump=a.dump_outputs)
    return res, {f.stem: np.load(f) for f in sorted(Path(tmp).glob("*.npy"))}


def test_dump_is_the_last_timed_window(make_oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "RESIDENT_WINDOWS", 3)  # the 5 timed steps run as 3 + 2
    res, got = _run(tmp_path / "a")
    assert sorted(got) == ["stats", "verdicts"]
    assert got["verdicts"].dtype == np.float32 and got["stats"].dtype == np.float64
    assert res["steps"] == STEPS and res["ms_per_step"] > 0
    settle = res["config"]["settle_sim_ms"] * 1000 / WINDOW
    assert settle == 5
    c = make_oracle(N)
    wl.configure_storm(c, N)
    for _ in range(int(settle) + WARMUP + STEPS):
        c.gen_storm(0.5, WINDOW)
        c.step(WINDOW)
        c.drain()
    s = c.stats()
    want = [s[k] for k in bench.STAT_NAMES] + [s["by_verdict"][k] for k in abi.VERDICT_NAMES]
    assert got["stats"].tolist() == [float(x) for x in want]
    assert s["now_tick"] == (settle + WARMUP + STEPS) * WINDOW
    assert np.array_equal(got["verdicts"], c.verdicts().astype(np.float32))
    # the same arguments give the same files
    _, again = _run(tmp_path / "b")
    assert all(np.array_equal(got[k], again[k]) for k in got)
