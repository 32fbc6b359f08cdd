"""The CPU oracle's TGSIM_OPT_METRICS tables against metrics_cases.ArtifactModel, an independent numpy
model fed only with what a host sees per window (offered packets, verdict bytes, drained records),
after every window of every scenario of tests/metrics_cases.py; against the oracle's own statistics;
and against the closed forms of the parked-queue scenario.  tests/test_gpu_metrics_paths.py holds the
HIP engine to this oracle; this file is what holds the oracle.  The path conditions the GPU cases name
are asserted here too, where a CPU-only run can already tell that a generator misses its path."""
import numpy as np
import pytest

import metrics_cases as mc
from testground_amd import abi
from testground_amd import workloads as wl


def _series(cpu, scenario, n, what):
    """Runs a scenario on the oracle: after every window the tables equal the artifact model and sum to
    the statistics.  Returns the tables after every window and the windows' artifacts."""
    model, series, art = mc.ArtifactModel(n), [], []
    for w, pk in enumerate(scenario(cpu)):
        assert pk is not None, "the oracle reports its generated windows"
        v = cpu.verdicts() if len(pk) else np.zeros(0, dtype=np.uint8)
        d = cpu.drain()
        model.fold(pk, v, d)
        t = cpu.metrics()
        model.check(t, f"{what}, after window {w}")
        mc.assert_stats_sums(t, cpu.stats(), f"{what}, after window {w}")
        series.append(t)
        art.append((pk, v, d))
    return series, art


@pytest.mark.parametrize("name", sorted(mc.SCENARIOS))
def test_oracle_equals_artifact_model(make_oracle, name):
    n, kw, scenario = mc.SCENARIOS[name]
    cpu = make_oracle(n, flags=abi.OPT_METRICS, **kw)
    series, _ = _series(cpu, scenario, n, name)
    assert len(series) > 0 and series[-1]["src"][:, 10].sum() > 0


# -- the path conditions, from the oracle alone ----------------------------------------------------------------
def test_a_produces_every_verdict_it_can(make_oracle):
    cpu = make_oracle(mc.A["n"], flags=abi.OPT_METRICS, **mc.A["kw"])
    series, art = _series(cpu, mc.scenario_a, mc.A["n"], "A")
    sums = series[-1]["src"].sum(axis=0)
    assert all(sums[2 + v] > 0 for v in mc.A_VERDICTS), sums
    assert all(sums[2 + v] == 0 for v in range(8) if v not in mc.A_VERDICTS), sums
    st = cpu.stats()
    assert st["cloned"] > 0 and st["corrupted"] > 0
    # mixed senders: some sources offer more than 64 packets in a window, most fewer than 16
    per = np.bincount(art[0][0]["src"], minlength=mc.A["n"])
    assert per.max() > 64 and np.median(per) < 64


@pytest.mark.parametrize("reserve", [1, 8])
def test_b_reaches_the_pool(make_oracle, reserve):
    cpu = make_oracle(mc.B["n"], flags=abi.OPT_METRICS, **mc.B["kw"])
    series, _ = _series(cpu, mc.scenario_b, mc.B["n"], "B")
    assert mc.pool_reached(series, reserve)


def test_d_windows_are_sparse_and_floods_spread(make_oracle):
    n = mc.D["n"]
    cpu = make_oracle(n, flags=abi.OPT_METRICS, **mc.D["kw"])
    series, art = _series(cpu, mc.scenario_d, n, "D")
    largest = max(len(pk) for pk, _, _ in art)
    assert 0 < largest < 64 * n, largest  # below the engine's dense threshold: every window sparse
    assert cpu.gossip_reached().min() >= n - 3, cpu.gossip_reached()
    assert series[-1]["src"][:, 2 + abi.V_LOSS].sum() > 0


def test_g_flushes_and_loses_in_flight(make_oracle):
    n = mc.G["n"]
    cpu = make_oracle(n, flags=abi.OPT_METRICS)
    series, art = _series(cpu, mc.scenario_g, n, "G")
    st, last = cpu.stats(), series[-1]
    assert st["flushed"] > 0 and st["lost_in_flight"] > 0
    assert all(last["src"][:, c].sum() > 0 for c in range(2, 10)), last["src"].sum(axis=0)
    # the disconnected peer: fewer records reached it than were scheduled towards it, and what was lost
    # in flight is in nobody's served column
    gone = mc.G["gone"]
    scheduled_to = sum(int((((v & 15) == abi.V_SCHEDULED) & (pk["dst"] == gone)).sum()) for pk, v, _ in art)
    assert 0 < int(last["dst"][gone, 0]) < scheduled_to
    served = int(last["src"][:, 10].sum())
    assert served == st["scheduled"] == sum(len(d) for _, _, d in art)
    assert served + st["lost_in_flight"] <= int(last["src"][:, 2 + abi.V_SCHEDULED].sum())  # (originals and clones)
    assert st["flushed"] > 64  # the disconnected peer's own queue was deep


# -- C: closed forms -------------------------------------------------------------------------------------------
def test_c_ramp_bins_are_the_issue_numbers():
    n, k, queued, bins = mc.c_expected("ramp")
    assert n == 300 and (queued == k).all()
    assert bins[:10].tolist() == [1, 1, 2, 4, 8, 16, 32, 64, 128, 44] and bins[10:].sum() == 0
    assert (bins == np.bincount([int(i).bit_length() for i in range(300)], minlength=64)).all()


@pytest.mark.parametrize("variant", sorted(mc.C_VARIANTS))
def test_c_closed_form(make_oracle, variant):
    n, k, queued, bins = mc.c_expected(variant)
    cpu = make_oracle(n, flags=abi.OPT_METRICS, **mc.C["kw"])
    run = mc.scenario_c(variant)(cpu)
    pk = next(run)
    assert len(pk) == k.sum()
    t, drained = cpu.metrics(), [cpu.drain()]
    assert len(drained[0]) == 0  # 50 ms of latency against a 1 ms window: everything is parked
    assert (t["hist"][0] == bins).all(), t["hist"][0][:12]
    assert t["hist"][1][0] == n and t["hist"][1].sum() == n  # nothing served
    assert (t["src"][:, 0] == k).all() and (t["src"][:, 1] == k * mc.C["length"]).all()
    assert (t["src"][:, 2 + abi.V_SCHEDULED] == queued).all() and (t["src"][:, 2 + abi.V_QUEUE_FULL] == k - queued).all()
    assert t["src"][:, 10].sum() == 0
    full = cpu.stats()["by_verdict"]["queue_full"]
    if variant == "deep":
        assert full == int((k - queued).sum()) > 0 and bins[10] > 0 and bins[11] > 0
    else:
        assert full == 0
    for _ in run:
        drained.append(cpu.drain())
    t = cpu.metrics()
    assert (t["src"][:, 10] == queued).all() and (t["src"][:, 11] == queued * mc.C["length"]).all()
    assert sum(len(d) for d in drained) == queued.sum()
    assert t["hist"][0].sum() == (1 + mc.C["idle"]) * n
    assert (t["dst"][:, 0] == np.roll(queued, 1)).all()  # source i sends to peer i + 1
    if variant == "ramp":
        assert queued.sum() == 44_850 and t["hist"][0].sum() == 61 * 300


# -- E, F: the closed loops, host-driven over the oracle -------------------------------------------------------
def _check_recording(rec, n, what):
    model = mc.ArtifactModel(n)
    for w, ((pk, v, d), t) in enumerate(zip(rec.windows, rec.tables)):
        model.fold(pk, v, d)
        model.check(t, f"{what}, after window {w}")


def test_e_ping_over_the_oracle(make_oracle):
    n = mc.E["n"]
    rec = mc.Recording(make_oracle(n, flags=abi.OPT_METRICS, **mc.LOOP["kw"]))
    ping, targets = mc.e_setup(rec)
    ref = wl.ping_reference(rec, ping, targets, mc.E["windows"], mc.LOOP["window"])
    assert len(rec.windows) == mc.E["windows"]
    _check_recording(rec, n, "E")
    mc.assert_stats_sums(rec.tables[-1], rec.stats(), "E")
    s = ref["summary"]
    assert s["sent"] == n * mc.E["fanout"] * mc.E["ping"]["count"] and 0 < s["received"] < s["sent"]
    assert s["dup_ignored"] > 0 and s["corrupt_ignored"] > 0


def test_f_flows_over_the_oracle(make_oracle):
    n = mc.F["n"]
    rec = mc.Recording(make_oracle(n, flags=abi.OPT_METRICS, **mc.LOOP["kw"]))
    flows = mc.f_setup(rec)
    ref = wl.flow_reference(rec, mc.F["flow"], flows, mc.F["windows"], mc.LOOP["window"], fb=mc.F["fb"])
    _check_recording(rec, n, "F")
    mc.assert_stats_sums(rec.tables[-1], rec.stats(), "F")
    s, fb = ref["summary"], ref["fb_summary"]
    assert s["active"] == 0 and s["done"] + s["failed"] == s["flows"] == n * mc.F["per_source"]  # every flow is over
    assert fb["failed_blackhole"] == 1 == s["failed"] and s["retransmits"] > 0
    assert rec.tables[-1]["src"][mc.F["cut"][0], 2 + abi.V_BLACKHOLE] >= 1


# -- the C ABI's edges -----------------------------------------------------------------------------------------
def test_abi_edges(make_oracle):
    e = make_oracle(20, flags=abi.OPT_METRICS)
    wl.configure_storm(e, 20)
    e.gen_storm(0.5, 500)
    e.step(500)
    mc.check_abi_edges(e, make_oracle(4))


def test_assert_tables_same_names_the_first_difference():
    a = {"src": np.zeros((3, 12), dtype=np.uint64), "dst": np.zeros((3, 2), dtype=np.uint64),
         "hist": np.zeros((2, 64), dtype=np.uint64)}
    b = {k: v.copy() for k, v in a.items()}
    mc.assert_tables_same(a, b, "equal")
    b["src"][1, 10], b["src"][2, 11] = 7, 9
    with pytest.raises(AssertionError, match=r"table src: 2 words differ, first at instance 1, column 10 \(served\): 0 vs 7"):
        mc.assert_tables_same(a, b, "x")
    b = {k: v.copy() for k, v in a.items()}
    b["hist"][0, 5] = 1
    with pytest.raises(AssertionError, match=r"table hist.*row 0 \(backlog\), bin 5: 0 vs 1"):
        mc.assert_tables_same(a, b, "x")
