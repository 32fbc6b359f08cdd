"""The device-side TGSIM_OPT_METRICS tables (k_metrics_src, k_metrics_dst) against the CPU oracle's, bit
for bit after EVERY window, on every path that feeds them: the dense and the sparse simulate kernels,
the compact emit layout and its pool, parked and full queues (against closed forms too), gossip, ping
and flow windows, reconfiguration, shards over the engine's own exchange, tgsim_step_n and
tgsim_comm_run.  The cases are in tests/metrics_cases.py; tests/test_metrics_model.py holds the oracle
to an independent model of the tables on the same cases.

Every case first compares the window's verdict bytes and drained records, then the tables: a failure
that names a table, an instance and a column after the window's records matched is the metrics reader's.
Every case asserts, from the oracle's numbers, that it reached the path it is named for."""
import numpy as np
import pytest

import metrics_cases as mc
import ping_cases as pc
import flow_fb_cases as fb
from test_gpu_multirank import _ranks, lib  # noqa: F401  (lib: the mock-transport build, a fixture)
from testground_amd import abi
from testground_amd import workloads as wl
from testground_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None

ON = abi.OPT_METRICS


def both(make_oracle, n, **kw):
    return Engine(n, flags=ON, **kw), make_oracle(n, flags=ON, **kw)


def lockstep(g, c, scenario, what, stats=True):
    """The scenario on the engine and on the oracle, window by window: verdicts and deliveries, then the
    tables, after every window.  Returns the oracle's tables after every window and its windows'
    artifacts (packets, verdict bytes, drained records)."""
    series, art = [], []
    for w, (_, pk) in enumerate(zip(scenario(g), scenario(c))):
        v, d = mc.assert_window_same(g, c, f"{what}, window {w}")
        mc.assert_tables_same(g, c, f"{what}, after window {w}")
        if stats:
            assert g.stats() == c.stats(), f"{what}, window {w}: statistics"
        series.append(c.metrics())
        art.append((pk, v, d))
    assert len(series) > 0
    return series, art


def sparse_windows(e):
    return int(e._fn("debug_sparse_windows")(e._h))


# -- A. dense and sparse kernels, mixed senders ----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["0", "1"])
def test_a_dense_and_sparse_kernels(make_oracle, monkeypatch, mode):
    monkeypatch.setenv("TGSIM_SPARSE", mode)
    g, c = both(make_oracle, mc.A["n"], **mc.A["kw"])
    series, _ = lockstep(g, c, mc.scenario_a, f"A, TGSIM_SPARSE={mode}")
    sums = series[-1]["src"].sum(axis=0)
    assert all(sums[2 + v] > 0 for v in mc.A_VERDICTS), sums
    assert c.stats()["cloned"] > 0 and c.stats()["corrupted"] > 0
    assert sparse_windows(g) == (mc.A["steps"] if mode == "1" else 0)


# -- B. compact emit layout and its pool: k_metrics_src's pidx branch ------------------------------------------
@pytest.mark.parametrize("reserve", [1, 8])
def test_b_compact_layout_and_pool(make_oracle, monkeypatch, reserve):
    monkeypatch.setenv("TGSIM_SPARSE", "1")
    monkeypatch.setenv("TGSIM_EMIT_COMPACT", "2")
    monkeypatch.setenv("TGSIM_EMIT_R", str(reserve))
    g, c = both(make_oracle, mc.B["n"], **mc.B["kw"])
    series, _ = lockstep(g, c, mc.scenario_b, f"B, reserve {reserve}")
    assert mc.pool_reached(series, reserve)
    assert sparse_windows(g) == mc.B["steps"]


# -- C. parked queues, closed form -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant,sparse", [("ramp", None), ("ramp64", "1"), ("deep", None), ("deep", "1")])
def test_c_parked_queues(make_oracle, monkeypatch, variant, sparse):
    if sparse is None:
        monkeypatch.delenv("TGSIM_SPARSE", raising=False)
    else:
        monkeypatch.setenv("TGSIM_SPARSE", sparse)
    n, k, queued, bins = mc.c_expected(variant)
    g, c = both(make_oracle, n, **mc.C["kw"])
    first = []

    def scenario(e):
        for w, pk in enumerate(mc.scenario_c(variant)(e)):
            if w == 0 and e is g:
                first.append(e.metrics())
            yield pk

    series, _ = lockstep(g, c, scenario, f"C-{variant}, TGSIM_SPARSE={sparse}")
    # the closed forms, on the device's own tables: everything parked after the first window ...
    t = first[0]
    assert (t["hist"][0] == bins).all(), t["hist"][0][:12]
    assert t["hist"][1][0] == n and t["src"][:, 10].sum() == 0
    # ... and served by the end, every source exactly what its queue took
    t = g.metrics()
    assert (t["src"][:, 10] == queued).all() and (t["src"][:, 11] == queued * mc.C["length"]).all()
    assert (t["dst"][:, 0] == np.roll(queued, 1)).all()
    assert t["hist"][0].sum() == (1 + mc.C["idle"]) * n
    # the path, from the oracle: parked items in the first window's backlog bins, a full queue in `deep`
    assert (series[0]["hist"][0] == bins).all() and series[0]["src"][:, 10].sum() == 0
    full = c.stats()["by_verdict"]["queue_full"]
    if variant == "deep":
        assert full > 0 and bins[10] > 0 and bins[11] > 0
    else:
        assert full == 0
    if variant == "ramp":
        assert bins[:10].tolist() == [1, 1, 2, 4, 8, 16, 32, 64, 128, 44] and int(t["src"][:, 10].sum()) == 44_850
    if variant == "ramp64":  # sparse by the engine's own rule as well: fewer than 64 packets per source
        assert k.max() < 64 and sparse_windows(g) == 1 + mc.C["idle"]


# -- D. gossip: sparse generated windows, the records kept out of the buckets ----------------------------------
@pytest.mark.parametrize("dst_slot", [None, "0"])
def test_d_gossip_sparse_windows(make_oracle, monkeypatch, dst_slot):
    if dst_slot is None:
        monkeypatch.delenv("TGSIM_DST_SLOT", raising=False)
    else:
        monkeypatch.setenv("TGSIM_DST_SLOT", dst_slot)
    n = mc.D["n"]
    g, c = both(make_oracle, n, **mc.D["kw"])
    series, art = lockstep(g, c, mc.scenario_d, f"D, TGSIM_DST_SLOT={dst_slot}", stats=False)
    assert 0 < max(len(pk) for pk, _, _ in art) < 64 * n  # every window below the engine's dense threshold
    assert sparse_windows(g) == mc.D["windows"]
    assert g.bucket_records() == 0  # metrics keep the records out of the buckets
    assert (g.gossip_reached() == c.gossip_reached()).all() and c.gossip_reached().min() >= n - 3
    assert series[-1]["src"][:, 10].sum() > mc.D["floods"] * n


# -- E, F. the device loops armed ------------------------------------------------------------------------------
def _loop_tables(rec, dev_windows, snaps, what):
    """Window by window: verdicts and deliveries, then the tables, of a device loop against the
    host-driven loop recorded over the oracle."""
    assert len(dev_windows) == len(rec.windows) == len(snaps) == len(rec.tables)
    for w, ((dv, dd), (_, rv, rd)) in enumerate(zip(dev_windows, rec.windows)):
        assert dv.tobytes() == rv.tobytes(), f"{what}, window {w}: verdicts differ"
        assert dd.tobytes() == rd.tobytes(), f"{what}, window {w}: deliveries differ"
        mc.assert_tables_same(snaps[w], rec.tables[w], f"{what}, after window {w}")


def test_e_ping_mesh_armed(make_oracle):
    n, windows, window = mc.E["n"], mc.E["windows"], mc.LOOP["window"]
    probe_at = (0, windows // 2)
    rec = mc.Recording(make_oracle(n, flags=ON, **mc.LOOP["kw"]))
    ping, targets = mc.e_setup(rec)
    ref = wl.ping_reference(rec, ping, targets, windows, window, probe_at=probe_at)
    eng = Engine(n, flags=ON, **mc.LOOP["kw"])
    mc.e_setup(eng)
    eng.ping_init(targets, **ping)
    snaps = []
    dev = wl.ping_run(eng, windows, window, collect=True, probe_at=probe_at,
                      before=lambda w: snaps.append(eng.metrics()) if w else None)
    snaps.append(eng.metrics())
    dev["pairs"], dev["summary"] = eng.ping_pairs(), eng.ping_report()
    _loop_tables(rec, dev["windows"], snaps, "E")
    pc.assert_same_run(dev, ref)  # the ping report and pairs are still the model's
    s = ref["summary"]
    assert 0 < s["received"] < s["sent"] and s["dup_ignored"] > 0 and s["corrupt_ignored"] > 0


def test_f_flows_armed_with_feedback(make_oracle):
    """k_flow_fb and k_metrics_src both follow the simulate kernel on its stream."""
    n, windows, window = mc.F["n"], mc.F["windows"], mc.LOOP["window"]
    probe_at = (0, windows // 2)
    rec = mc.Recording(make_oracle(n, flags=ON, **mc.LOOP["kw"]))
    flows = mc.f_setup(rec)
    ref = wl.flow_reference(rec, mc.F["flow"], flows, windows, window, probe_at=probe_at, fb=mc.F["fb"])
    ref["flows"] = flows
    eng = Engine(n, flags=ON, **mc.LOOP["kw"])
    assert mc.f_setup(eng).tobytes() == flows.tobytes()
    eng.flow_init(flows, fb=mc.F["fb"], **mc.F["flow"])
    snaps = []
    dev = wl.flow_run(eng, windows, window, collect=True, probe_at=probe_at,
                      before=lambda w: snaps.append(eng.metrics()) if w else None)
    snaps.append(eng.metrics())
    dev["rows"], dev["summary"] = eng.flow_rows(), eng.flow_report()
    dev["fb_rows"], dev["fb_summary"] = eng.flow_fb_rows(), eng.flow_fb_report()
    dev["flows"] = flows
    _loop_tables(rec, dev["windows"], snaps, "F")
    fb.assert_same_run(dev, ref)
    s = ref["summary"]
    assert s["active"] == 0 and s["done"] + s["failed"] == s["flows"] == n * mc.F["per_source"]  # every flow is over
    assert ref["fb_summary"]["failed_blackhole"] == 1 and s["retransmits"] > 0
    assert rec.tables[-1]["src"][mc.F["cut"][0], 2 + abi.V_BLACKHOLE] >= 1


# -- G. reconfiguration ----------------------------------------------------------------------------------------
def test_g_reconfiguration(make_oracle):
    n, gone = mc.G["n"], mc.G["gone"]
    g, c = both(make_oracle, n)
    series, art = lockstep(g, c, mc.scenario_g, "G")
    st, last = c.stats(), series[-1]
    assert st["flushed"] > 0 and st["lost_in_flight"] > 0
    assert all(last["src"][:, col].sum() > 0 for col in range(2, 10)), last["src"].sum(axis=0)
    # the disconnected peer: fewer records reached it than were scheduled towards it, and what was lost
    # in flight is in no source's served column
    scheduled_to = sum(int((((v & 15) == abi.V_SCHEDULED) & (pk["dst"] == gone)).sum()) for pk, v, _ in art)
    assert 0 < int(last["dst"][gone, 0]) < scheduled_to
    served = int(last["src"][:, 10].sum())
    assert served == st["scheduled"] == sum(len(d) for _, _, d in art) == int(last["dst"][:, 0].sum())
    assert served + st["lost_in_flight"] <= int(last["src"][:, 2 + abi.V_SCHEDULED].sum())  # (originals and clones)


# -- H. shards over the engine's own exchange ------------------------------------------------------------------
def _ranks_against_oracle(lib, make_oracle, n, bounds, scenario, what, **kw):  # noqa: F811
    """scenario(step) -> generator function; the ranks run it through comm_step, one whole-peer oracle
    through step.  After every window: the ranks' verdicts and drains concatenated in rank order, then
    their src and dst tables concatenated and both histogram rows summed, equal the oracle's."""
    def rank(r, e):
        return [(e.verdicts(), e.drain(), e.metrics()) for _ in scenario(lambda eng, t: eng.comm_step(t))(e)]

    per_rank, info = _ranks(lib, n, bounds, rank, flags=ON, **kw)
    assert all(i["nranks"] == len(bounds) - 1 and i["bounds"] == bounds for i in info)
    c = make_oracle(n, flags=ON, **kw)
    series = []
    for w, _ in enumerate(scenario(lambda eng, t: eng.step(t))(c)):
        got = [p[w] for p in per_rank]
        assert np.concatenate([x[0] for x in got]).tobytes() == c.verdicts().tobytes(), f"{what}, window {w}: verdicts differ"
        assert np.concatenate([x[1] for x in got]).tobytes() == c.drain().tobytes(), f"{what}, window {w}: deliveries differ"
        mc.assert_tables_same(mc.merged([x[2] for x in got]), c, f"{what}, after window {w}")
        series.append(c.metrics())
    assert len(series) == len(per_rank[0]) > 0
    assert sum(i["exchanged_records"] for i in info) > 0
    return series, c


@pytest.mark.parametrize("bounds", [[0, 100, 240], [0, 70, 155, 240]])
def test_h_shards_storm(lib, make_oracle, bounds):  # noqa: F811
    h = mc.H
    series, c = _ranks_against_oracle(lib, make_oracle, h["n"], bounds,
                                      lambda step: mc.scenario_storm(h["n"], h["lam"], h["ticks"], h["windows"], step=step),
                                      f"H, {len(bounds) - 1} ranks")
    # every rank both sends to and receives from another rank
    last = series[-1]
    assert all(last["src"][lo:hi, 10].sum() > 0 and last["dst"][lo:hi, 0].sum() > 0 for lo, hi in zip(bounds, bounds[1:]))
    assert last["src"][:, 2 + abi.V_QUEUE_FULL].sum() > 0 and last["src"][:, 2 + abi.V_LOSS].sum() > 0


def test_h_shards_gossip(lib, make_oracle):  # noqa: F811
    n, bounds = mc.H["n"], [0, 100, 240]
    series, c = _ranks_against_oracle(lib, make_oracle, n, bounds,
                                      lambda step: (lambda e: mc.scenario_d(e, n=n, step=lambda t: step(e, t))),
                                      "H, gossip at 2 ranks", **mc.D["kw"])
    assert c.gossip_reached().min() >= n - 3 and series[-1]["dst"][:, 0].sum() > mc.D["floods"] * n // 2


# -- I. flags and step forms -----------------------------------------------------------------------------------
def test_i_step_n_with_discard(make_oracle):
    i = mc.I
    flags = ON | abi.OPT_DISCARD_DELIVERIES
    a, b, c = Engine(i["n"], flags=flags), Engine(i["n"], flags=flags), make_oracle(i["n"], flags=ON)
    # b one step at a time against the oracle, after every window
    for w, _ in enumerate(zip(mc.SCENARIOS["I"][2](b), mc.SCENARIOS["I"][2](c))):
        assert b.verdicts().tobytes() == c.verdicts().tobytes(), f"I, window {w}: verdicts differ"
        mc.assert_tables_same(b, c, f"I, after window {w}")
        assert b.pending() == 0
        assert len(c.drain()) > 0
    # a: the same windows through one tgsim_step_n call
    wl.configure_storm(a, i["n"])
    for _ in range(i["windows"]):
        a.gen_storm(i["lam"], i["ticks"])
    a.step_n(i["ticks"], i["windows"])
    mc.assert_tables_same(a, c, "I, one step_n call")
    assert a.pending() == 0
    assert int(a._fn("debug_fused_launches")(a._h)) == 0 and int(a._fn("debug_fused_windows")(a._h)) == 0
    sa, sc = a.stats(), c.stats()
    assert sa == sc
    # dense windows: an engine without the tables would have fused them
    assert sc["offered"] >= 64 * i["n"] * i["windows"] and sparse_windows(a) == 0


# -- tgsim_comm_run on engines with the tables -----------------------------------------------------------------
def test_comm_run_refuses_fused_groups_with_metrics(lib, make_oracle):  # noqa: F811
    """fuse >= 2 at two ranks: refused on every rank, with the reason, before anything is simulated; the
    same windows then run with fuse = 1, and the tables satisfy scenario H's equality."""
    import errno

    h = mc.H
    n, ticks, k, bounds = h["n"], h["ticks"], h["windows"], [0, 100, 240]

    def rank(r, e):
        wl.configure_storm(e, n)
        for _ in range(k):
            e.gen_storm(h["lam"], ticks)
        before = e.stats()
        try:
            e.comm_run(ticks, k, 4, 0)
            err = None
        except EngineError as ex:
            err = (ex.code, ex.msg)
        after = e.stats()
        e.comm_run(ticks, k, 1, 0)  # nothing generated again: the k windows were still queued
        e.sync()
        return err, before, after, e.stats(), e.drain(), e.metrics()

    per_rank, _ = _ranks(lib, n, bounds, rank, flags=ON)
    c = make_oracle(n, flags=ON)
    want = [c.drain() for _ in mc.scenario_storm(n, h["lam"], ticks, k)(c)]
    assert len(want) == k
    for r, (err, before, after, end, d, _) in enumerate(per_rank):
        assert err is not None, f"rank {r}: comm_run(fuse=4) succeeded"
        assert err[0] == -errno.EINVAL and "engine has TGSIM_OPT_METRICS" in err[1] and "fuse = 1" in err[1], err
        assert "dense" not in err[1], err
        assert after == before and before["now_tick"] == 0 and before["offered"] == 0, f"rank {r}: the refused run simulated"
        assert end["now_tick"] == k * ticks
        lo, hi = bounds[r], bounds[r + 1]
        mine = np.concatenate([x[(x["dst"] >= lo) & (x["dst"] < hi)] for x in want])
        assert len(d) == len(mine) > 0 and d.tobytes() == mine.tobytes(), f"rank {r}: deliveries differ"
    assert sum(p[3]["offered"] for p in per_rank) == c.stats()["offered"]
    mc.assert_tables_same(mc.merged([p[5] for p in per_rank]), c, f"after comm_run(fuse=1) of {k} windows")


# -- the C ABI's edges -----------------------------------------------------------------------------------------
def test_abi_edges():
    e = Engine(20, flags=ON)
    wl.configure_storm(e, 20)
    e.gen_storm(0.5, 500)
    e.step(500)
    mc.check_abi_edges(e, Engine(4))
