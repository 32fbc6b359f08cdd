"""The sharded ping mesh (tgsim_ping_init_sharded, tgsim_comm_ping_report) at 1, 2 and 3 ranks over
the engine's own exchange, against ONE engine over all peers armed with the unchanged tgsim_ping_init
and stepped with tgsim_step -- which tests/test_gpu_ping.py shows equal to the host model over the
oracle.  The ranks are threads over the test transport, as in tests/test_gpu_multirank.py.  Window by
window the ranks' verdict bytes and drains, concatenated in rank order, are the single engine's; at
every probe point and at the end so are the concatenated pair tables, workloads.merge_ping_reports of
the ranks' reports, and comm_ping_report on every rank."""
import ctypes
import errno
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ping_cases as pc
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl
from testground_amd.build import MOCK_COMM_LIB
from testground_amd.engine import CABIEngine, Engine, EngineError

pytestmark = pytest.mark.gpu
MS = nw.Millisecond


@pytest.fixture(scope="module")
def lib():
    if not MOCK_COMM_LIB.exists():
        pytest.fail(f"{MOCK_COMM_LIB} not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(MOCK_COMM_LIB))
    abi.declare(lib, "tgsim_")
    return lib


def _comm_id(lib) -> bytes:
    buf = ctypes.create_string_buffer(abi.COMM_ID_BYTES)
    assert lib.tgsim_comm_id(buf) == 0
    return buf.raw


def _ranks(lib, n, bounds, fn, **kw):
    """Runs fn(rank, engine) on one thread per rank (every collective call is made by all ranks at
    once, as processes would); returns the per-rank results in rank order."""
    world = len(bounds) - 1
    engs = [CABIEngine(lib, "tgsim_", n, shard=(bounds[r], bounds[r + 1]), device=0, **kw) for r in range(world)]
    cid = _comm_id(lib)

    def one(r):
        engs[r].comm_init(cid, r, world)
        return fn(r, engs[r])

    with ThreadPoolExecutor(world) as ex:
        futs = [ex.submit(one, r) for r in range(world)]
        out = [f.result(timeout=300) for f in futs]
    info = [e.comm_info() for e in engs]
    for e in engs:
        e.close()
    return out, info


class _Shard:
    """One rank's engine as the ping_cases runners drive it: ping_init arms the sharded form, step is
    the exchange's closed step, and ping_report carries the collective report beside the local one
    (every rank reaches every probe point, so the collective is made by all of them)."""

    def __init__(self, eng, comm=True):
        self._e, self._comm = eng, comm

    def __getattr__(self, name):
        return getattr(self._e, name)

    def ping_init(self, targets=None, **kw):
        self._e.ping_init(targets, sharded=True, **kw)

    def step(self, n_ticks):
        if self._comm:
            self._e.comm_step(n_ticks)
        else:
            self._e.step(n_ticks)

    def ping_report(self):
        rep = self._e.ping_report()
        if self._comm:
            rep["comm"] = self._e.comm_ping_report()
        return rep


def _assert_report(pairs, reports, ref, what):
    """Rank-ordered pair tables and reports against the single engine's (pairs, summary)."""
    pc.assert_same_report((np.concatenate(pairs), wl.merge_ping_reports(reports)), ref, f"{what}: merged")
    for r, rep in enumerate(reports):
        if "comm" in rep:
            pc.assert_same_report((ref[0], rep["comm"]), ref, f"{what}: comm_ping_report on rank {r}")


def _assert_equals_single(per_rank, ref, windows=True):
    if windows:
        assert all(len(p["windows"]) == len(ref["windows"]) for p in per_rank)
        for w, (rv, rd) in enumerate(ref["windows"]):
            v = np.concatenate([p["windows"][w][0] for p in per_rank])
            d = np.concatenate([p["windows"][w][1] for p in per_rank])
            assert v.tobytes() == rv.tobytes(), f"verdicts of window {w}"
            assert d.tobytes() == rd.tobytes(), f"deliveries of window {w}"
    assert all(sorted(p["probes"]) == sorted(ref["probes"]) for p in per_rank)
    for w in ref["probes"]:
        _assert_report([p["probes"][w][0] for p in per_rank], [p["probes"][w][1] for p in per_rank], ref["probes"][w],
                       f"probe after window {w}")
    _assert_report([p["pairs"] for p in per_rank], [p["summary"] for p in per_rank], (ref["pairs"], ref["summary"]),
                   "end of run")


def _sharded(lib, n, bounds, run, **kw):
    return _ranks(lib, n, bounds, lambda r, e: run(_Shard(e)), **kw)


@pytest.fixture(scope="module")
def mesh_single():
    """The lossy mesh on one engine over all peers (plain ping_init + step), once for the module."""
    return pc.run_mesh(Engine(pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"]), device=True)


# -- 1. verify ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("allow_all", [False, True])
def test_verify(lib, allow_all):
    n, kw = pc.VERIFY["n"], dict(lookahead_ns=pc.VERIFY["lookahead_ns"])
    per_rank, _ = _sharded(lib, n, [0, 1, 4], lambda e: pc.run_verify(e, device=True, allow_all=allow_all), **kw)
    _assert_equals_single(per_rank, pc.run_verify(Engine(n, **kw), device=True, allow_all=allow_all))
    assert [p["summary"]["pairs_none"] for p in per_rank] == [1, 3]  # the external slot, on every shard
    assert all(p["summary"]["comm"]["pairs_none"] == 4 for p in per_rank)


# -- 2. splitbrain -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [[0, 4, 9], [0, 3, 6, 9]])
@pytest.mark.parametrize("case", ["drop", "reject", "accept"])
def test_splitbrain(lib, bounds, case):
    n, kw = pc.SPLIT["n"], dict(lookahead_ns=pc.SPLIT["lookahead_ns"])
    per_rank, _ = _sharded(lib, n, bounds, lambda e: pc.run_splitbrain(e, device=True, case=case), **kw)
    _assert_equals_single(per_rank, pc.run_splitbrain(Engine(n, **kw), device=True, case=case))
    pairs = np.concatenate([p["pairs"] for p in per_rank])
    assert (pc.splitbrain_reached(pairs, n) == wl.splitbrain_expected(n, case)).all()


# -- 3. lossy mesh with the hot responder ------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [[0, 50, 130], [0, 1, 60, 130]])
def test_mesh_parity(lib, mesh_single, bounds):
    """[0, 1, 60, 130]: rank 0 owns only peer 0, whose rows exceed 64 entries (the long-row branch of
    k_cal_order on a one-source shard)."""
    n, kw = pc.MESH["n"], dict(lookahead_ns=pc.MESH["lookahead_ns"])
    per_rank, info = _sharded(lib, n, bounds, lambda e: pc.run_mesh(e, device=True), **kw)
    _assert_equals_single(per_rank, mesh_single)
    assert sum(i["exchanged_records"] for i in info) > 1000
    assert all(p["summary"]["received"] > 0 for p in per_rank)
    assert all(i["bounds"] == bounds for i in info)


# -- 4. the result does not depend on the step length -----------------------------------------------------
def test_mesh_window_length(lib, mesh_single):
    n, kw = pc.MESH["n"], dict(lookahead_ns=pc.MESH["lookahead_ns"])
    per_rank, _ = _sharded(lib, n, [0, 50, 130], lambda e: pc.run_mesh(e, device=True, window=2_000, probe_at=()), **kw)
    pairs = np.concatenate([p["pairs"] for p in per_rank])
    for key in abi.PING_PAIR_DTYPE.names:
        assert (pairs[key] == mesh_single["pairs"][key]).all(), key
    assert (wl.merge_ping_reports([p["summary"] for p in per_rank])["hist"] == mesh_single["summary"]["hist"]).all()
    for p in per_rank:
        assert (p["summary"]["comm"]["hist"] == mesh_single["summary"]["hist"]).all()
        assert p["summary"]["pending_replies"] == 0


# -- 5. nothing reaches the host ---------------------------------------------------------------------------
def test_mesh_discard_deliveries(lib, mesh_single):
    n, kw = pc.MESH["n"], dict(lookahead_ns=pc.MESH["lookahead_ns"], flags=abi.OPT_DISCARD_DELIVERIES)
    per_rank, _ = _sharded(lib, n, [0, 50, 130], lambda e: pc.run_mesh(e, device=True), **kw)
    _assert_equals_single(per_rank, mesh_single, windows=False)
    assert all(len(d) == 0 for p in per_rank for _, d in p["windows"])
    for w, (rv, _) in enumerate(mesh_single["windows"]):
        assert np.concatenate([p["windows"][w][0] for p in per_rank]).tobytes() == rv.tobytes(), f"verdicts of window {w}"


# -- 6. one rank: the local step, and the routed path delivered in place ----------------------------------
@pytest.mark.parametrize("route1", [False, True])
def test_one_rank(lib, mesh_single, monkeypatch, route1):
    if route1:
        monkeypatch.setenv("TGSIM_COMM_ROUTE1", "1")  # read by tgsim_comm_init: the engine comes after it
    else:
        monkeypatch.delenv("TGSIM_COMM_ROUTE1", raising=False)
    n, kw = pc.MESH["n"], dict(lookahead_ns=pc.MESH["lookahead_ns"])
    per_rank, info = _sharded(lib, n, [0, n], lambda e: pc.run_mesh(e, device=True), **kw)
    _assert_equals_single(per_rank, mesh_single)
    pc.assert_same_report((per_rank[0]["pairs"], per_rank[0]["summary"]["comm"]),
                          (per_rank[0]["pairs"], per_rank[0]["summary"]), "comm_ping_report at one rank")
    assert (info[0]["exchanged_records"] > 0) == route1


# -- 7. a whole-peer engine without a communicator --------------------------------------------------------
def test_whole_engine_step(mesh_single):
    eng = Engine(pc.MESH["n"], lookahead_ns=pc.MESH["lookahead_ns"])
    _assert_equals_single([pc.run_mesh(_Shard(eng, comm=False), device=True)], mesh_single)


# -- 8. a responder disconnected between two windows ------------------------------------------------------
def test_responder_disconnected(lib):
    def run(eng):
        def before(w):
            if w == 2:  # on every rank: every shard receives every configure call
                eng.configure(0, nw.Config(Network="default", Enable=False))
        return pc.run_mesh(eng, True, ticks=60_000, probe_at=(1, 3), before=before)

    n, kw = pc.MESH["n"], dict(lookahead_ns=pc.MESH["lookahead_ns"])
    ref = run(Engine(n, **kw))
    per_rank, _ = _sharded(lib, n, [0, 50, 130], run, **kw)
    _assert_equals_single(per_rank, ref)
    assert ref["probes"][1][1]["pending_replies"] > 0
    assert ((ref["windows"][2][0] & 15)[:4] == abi.V_DISCONNECTED).all()


# -- 9. the late rule across ranks -------------------------------------------------------------------------
def test_late_agreement(lib, monkeypatch):
    monkeypatch.setenv("TGSIM_COMM_TIMEOUT_MS", "20000")  # a rank left waiting fails instead of hanging
    n, win, bounds = pc.LATE["n"], pc.LATE["window"], [0, 2, 4]
    kw = dict(lookahead_ns=pc.LATE["lookahead_ns"])
    ping = dict(count=8, interval_ticks=500, length=64, start_tick=0, bin_ns=MS, n_bins=8)
    # the single engine: the window whose generation goes late
    ref = Engine(n, **kw)
    pc.configure_late(ref, reorder=50.0)
    ref.ping_init(wl.ping_targets_all(n), **ping)
    late_at = None
    for w in range(6):
        try:
            ref.gen_ping(win)
        except EngineError as ex:
            assert ex.code == -errno.EINVAL
            late_at = w
            break
        ref.step(win)
    assert late_at is not None and late_at >= 1

    def attempt(fn, *a):
        try:
            fn(*a)
        except EngineError as ex:
            return ex.code, ex.msg
        return 0, ""

    def rank(r, e):
        pc.configure_late(e, reorder=50.0)
        e.ping_init(wl.ping_targets_all(n), sharded=True, **ping)
        log = []
        for w in range(late_at + 1):  # every rank calls comm_step for every window, whatever gen_ping said
            log.append((attempt(e.gen_ping, win), attempt(e.comm_step, win)))
        again = attempt(e.comm_step, win)
        rep, pairs = e.ping_report(), e.ping_pairs()
        e.ping_init(None, sharded=True)  # drops the window this rank may have generated for the refused step
        pc.configure_late(e, reorder=0.0)
        e.ping_init(wl.ping_targets_all(n), count=2, interval_ticks=500, length=64, bin_ns=MS, n_bins=8, sharded=True)
        wl.ping_run(e, 4, win, step=e.comm_step)
        return log, again, rep, pairs, e.ping_report(), e.comm_ping_report()

    per_rank, _ = _ranks(lib, n, bounds, rank, **kw)
    for log, again, *_ in per_rank:
        for w in range(late_at):  # not earlier than the single engine
            assert log[w] == ((0, ""), (0, "")), (w, log[w])
        for code, msg in (log[late_at][1], again):
            assert code == -errno.EINVAL, (code, msg)
            assert re.search(r"tick \d+", msg) and re.search(r"rank \d", msg), msg
    assert any(p[0][late_at][0][0] == -errno.EINVAL for p in per_rank), "no rank's gen_ping saw the late receipt"
    pairs = n * (n - 1)
    assert sum(len(p[3]) for p in per_rank) == n and all(p[3].shape[1] == n - 1 for p in per_rank)
    assert wl.merge_ping_reports([p[2] for p in per_rank])["sent"] == pairs * 8
    merged = wl.merge_ping_reports([p[4] for p in per_rank])
    assert merged["received"] == merged["sent"] == pairs * 2 and merged["pairs_all"] == merged["pairs"] == pairs
    for p in per_rank:
        pc.assert_same_report((p[3], p[5]), (p[3], merged), "comm_ping_report after the re-arm")


# -- 10. arming rules --------------------------------------------------------------------------------------
def _raises(code, match, fn, *a, **kw):
    with pytest.raises(EngineError, match=match) as ei:
        fn(*a, **kw)
    assert ei.value.code == -code, ei.value


def test_arming_rules(lib):
    import torch

    n, bounds, slot_cap = 8, [0, 4, 8], 64
    t = wl.ping_targets_mesh(n, 2, seed=1)
    ok = dict(count=2, interval_ticks=100, length=64, start_tick=0)
    pkt = np.array([(0, 1, 0, 64, 0)], dtype=abi.PKT_DTYPE)
    # (a real buffer for the slotted launches: they must refuse before touching it)
    d_out = torch.zeros(2 * 2 * (slot_cap + 1) * abi.DELIVERY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")

    def rank(r, e):
        lo, hi = bounds[r], bounds[r + 1]
        _raises(errno.EINVAL, "comm_ping_report: the sharded ping driver is not armed", e.comm_ping_report)
        _raises(errno.EINVAL, "one engine for every peer", e.ping_init, t, **ok)
        for bad, match in ((dict(count=0), "ping: count 0 outside 1..65535"),):
            _raises(errno.EINVAL, match, e.ping_init, t, sharded=True, **dict(ok, **bad))
        self_t, far_t = t.copy(), t.copy()
        self_t[6, 1], far_t[3, 0] = 6, n  # (rows of either shard: every shard validates the whole table)
        _raises(errno.EINVAL, r"ping: targets\[6\]\[1\] = 6 is the peer itself", e.ping_init, self_t, sharded=True, **ok)
        _raises(errno.EINVAL, r"ping: targets\[3\]\[0\] = 8 is out of range", e.ping_init, far_t, sharded=True, **ok)
        e.ping_init(t, sharded=True, **ok)
        _raises(errno.EBUSY, "ping driver is armed", e.comm_run, 100, 2, 1, 0)
        _raises(errno.EBUSY, "ping driver is armed", e.step_sim_launch_slotted, 100, bounds, d_out.data_ptr(), slot_cap)
        _raises(errno.EBUSY, "ping driver is armed", e.step_sim_launch_slotted_n, 100, 2, bounds, d_out.data_ptr(), slot_cap)
        _raises(errno.EBUSY, "ping driver is armed", e.submit, pkt)
        _raises(errno.EBUSY, "ping driver is armed", e.gen_storm, 0.01, 10)
        _raises(errno.EBUSY, "ping driver is armed", e.gossip_init, n_floods=1, degree=2)
        assert e.ping_pairs().shape == (hi - lo, 2) and e.ping_pairs(lo + 1, 2).shape == (2, 2)
        other = bounds[1 - r]
        _raises(errno.EINVAL, rf"ping_pairs: peers \[{other}, {other + 4}\) outside this shard's \[{lo}, {hi}\)",
                e.ping_pairs, other, 4)
        _raises(errno.EINVAL, r"outside this shard's", e.ping_pairs, 3, 2)  # (across the boundary)
        e.gen_ping(100)
        _raises(errno.EBUSY, "one window at a time", e.gen_ping, 100)
        e.comm_launch(100)
        _raises(errno.EBUSY, "launched step is not finished", e.gen_ping, 100)
        e.comm_finish()
        e.ping_init(None)  # the plain disarm disarms either form
        _raises(errno.EINVAL, "not armed", e.ping_report)
        return True

    per_rank, _ = _ranks(lib, n, bounds, rank)
    assert per_rank == [True, True]
    # a whole-peer engine: no communicator; armed with the plain form, the collective report refuses
    eng = Engine(n)
    _raises(errno.EINVAL, "comm_ping_report: no communicator", eng.comm_ping_report)
    eng.ping_init(t, sharded=True, **ok)
    _raises(errno.EBUSY, "flow: the ping driver is armed", eng.flow_init, wl.flow_table_mesh(n, 1, 4))
    _raises(errno.EINVAL, "comm_ping_report: no communicator", eng.comm_ping_report)

    def plain(r, e):
        e.ping_init(t, **ok)
        _raises(errno.EINVAL, "comm_ping_report: the sharded ping driver is not armed", e.comm_ping_report)
        _raises(errno.EBUSY, "ping driver is armed", e.comm_step, 100)
        return True

    assert _ranks(lib, n, [0, n], plain)[0] == [True]
