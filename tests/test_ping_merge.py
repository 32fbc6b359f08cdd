"""workloads.merge_ping_reports, the merge rule of include/tgsim.h for the sharded ping mesh (every
field by sum, min_ns by min, max_ns by max, hist by sum), against the host model over the CPU oracle:
the lossy mesh's run is split at [0, 50, 130] the way the shards of tgsim_ping_init_sharded see it --
a shard holds the pair rows of its own peers, folds the records addressed to them (so dup_ignored,
corrupt_ignored and the histogram count at the destination's shard) and keeps the calendar entries of
its own responders -- and the merged per-shard reports must be the model's report."""
import numpy as np
import pytest

import ping_cases as pc
from testground_amd import abi, metrics
from testground_amd import workloads as wl
from testground_amd.engine import CABIEngine

BOUNDS = [0, 50, 130]
U64_MAX = int(np.iinfo(np.uint64).max)


class _NoEngine:
    """What PingModel reads of an engine when it only folds records (receive)."""

    def __init__(self, tick_ns, now_tick):
        self.tick_ns, self._now = tick_ns, now_tick

    def stats(self):
        return {"now_tick": self._now}


@pytest.fixture(scope="module")
def mesh(oracle_lib):
    eng = CABIEngine(oracle_lib, "tgo_", pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"])
    return pc.run_mesh(eng, device=False)


def _shard_report(model, windows, ping, lo, hi):
    """The report of the shard that owns [lo, hi): its own fold of the records addressed to its peers."""
    own = wl.PingModel(_NoEngine(model.tick_ns, ping["start_tick"]), ping, model.targets)
    for _, d in windows:
        own.receive(d[(d["dst"] >= lo) & (d["dst"] < hi)])
    full, mine = model.pairs(), own.pairs()
    for key in ("received", "sum_ns", "min_ns", "max_ns"):  # the split is a partition of the pair table
        assert (mine[key][lo:hi] == full[key][lo:hi]).all(), key
    assert mine["received"][:lo].sum() == 0 and mine["received"][hi:].sum() == 0
    pr = full[lo:hi][model.targets[lo:hi] != abi.PING_NONE]
    got, sent = pr["received"] > 0, pr["sent"] > 0
    return {"pairs": len(pr), "sent": int(pr["sent"].sum(dtype=np.uint64)),
            "received": int(pr["received"].sum(dtype=np.uint64)), "sum_ns": int(pr["sum_ns"].sum(dtype=np.uint64)),
            "min_ns": int(pr["min_ns"][got].min()) if got.any() else U64_MAX,
            "max_ns": int(pr["max_ns"].max()) if len(pr) else 0,
            "pairs_all": int((sent & (pr["received"] == pr["sent"])).sum()), "pairs_none": int((sent & ~got).sum()),
            "dup_ignored": own.dup_ignored, "corrupt_ignored": own.corrupt_ignored,
            "pending_replies": int(((model.cal[:, 1] >= lo) & (model.cal[:, 1] < hi)).sum()), "hist": own.hist.copy()}


def _same(a, b):
    for key in abi.PING_SUMMARY_FIELDS:
        assert a[key] == b[key], (key, a[key], b[key])
    assert (np.asarray(a["hist"]) == np.asarray(b["hist"])).all()


@pytest.mark.parametrize("n_windows", [5, None])  # mid-run (replies waiting in the calendar) and the whole run
def test_merge_equals_model(oracle_lib, mesh, n_windows):
    if n_windows is None:
        model, windows = mesh["model"], mesh["windows"]
    else:
        eng = CABIEngine(oracle_lib, "tgo_", pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"])
        run = pc.run_mesh(eng, device=False, ticks=n_windows * pc.MESH["window"], probe_at=())
        model, windows = run["model"], run["windows"]
        assert len(model.cal) > 0
    shards = [_shard_report(model, windows, model.ping, BOUNDS[r], BOUNDS[r + 1]) for r in range(len(BOUNDS) - 1)]
    want = model.report()
    assert all(s["received"] > 0 and s["dup_ignored"] > 0 for s in shards) and want["corrupt_ignored"] > 0
    _same(wl.merge_ping_reports(shards), want)
    _same(wl.merge_ping_reports(reversed(shards)), want)


def test_shard_without_replies_is_neutral(mesh):
    want = mesh["model"].report()
    empty = dict({k: 0 for k in abi.PING_SUMMARY_FIELDS}, min_ns=U64_MAX, max_ns=0,
                 hist=np.zeros(len(want["hist"]), dtype=np.uint64))
    _same(wl.merge_ping_reports([empty, want]), want)
    _same(wl.merge_ping_reports([want, empty, empty]), want)
    both = wl.merge_ping_reports([empty, empty])
    assert both["min_ns"] == U64_MAX and both["max_ns"] == 0 and both["received"] == 0


def test_single_report_and_metrics(mesh):
    want = mesh["model"].report()
    one = wl.merge_ping_reports([want])
    _same(one, want)
    assert one["hist"] is not want["hist"] and one["hist"].dtype == np.uint64
    lines = metrics.ping_lines(one, pc.MESH_PING["bin_ns"], "mesh", "run0", 1)
    assert lines == metrics.ping_lines(want, pc.MESH_PING["bin_ns"], "mesh", "run0", 1) and len(lines) > 11
    with pytest.raises(ValueError):
        wl.merge_ping_reports([])
