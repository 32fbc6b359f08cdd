"""The device-side packet capture (tgsim_capture_*, k_capture_plan_* / k_capture_copy_*) against the host
model workloads.capture_reference fed from the CPU oracle's packets, verdict bytes and drained records,
compared as bytes after EVERY window, with every traffic source and on both delivery routines.  The
cases' traffic is tests/metrics_cases.py's; tests/test_capture_model.py holds the model to a hand case.

Engines are created without TGSIM_OPT_METRICS (the sparse windows' direct destination buckets stay on).
Every watch list holds peer 0, the last peer, the scenario's lightest sender (a peer that offers nothing
where the scenario has one) and its heaviest, chosen from a pass over the oracle alone.  Scenario A offers
from every peer in every window, so case 1 closes with a quiet window of its own: every row empty."""
import errno
import io
import tarfile

import numpy as np
import pytest

import metrics_cases as mc
from test_gpu_multirank import _ranks, lib  # noqa: F401  (lib: the mock-transport build, a fixture)
from testground_amd import abi
from testground_amd import network as nw
from testground_amd import pcap
from testground_amd import runner as rn
from testground_amd import workloads as wl
from testground_amd.engine import Engine, EngineError
from testground_amd.sidecar import Context

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None

DISCARD = abi.OPT_DISCARD_DELIVERIES
TX, RX = abi.CAPTURE_TX, abi.CAPTURE_RX
DIRS = ("tx", "rx")


# -- helpers ---------------------------------------------------------------------------------------------------
def survey(c, scenario):
    """The scenario on an oracle alone: per window (start tick, packets, verdict bytes, drained records)."""
    out, gen = [], scenario(c)
    while True:
        start = c.stats()["now_tick"]
        try:
            pk = next(gen)
        except StopIteration:
            return out
        pk = mc.NO_PACKETS if pk is None else pk
        out.append((start, pk, c.verdicts() if len(pk) else np.zeros(0, dtype=np.uint8), c.drain()))


def offered_per_window(windows, n):
    return np.stack([np.bincount(pk["src"].astype(np.int64), minlength=n)[:n] for _, pk, _, _ in windows])


def watch_list(windows, n, extra=()):
    """Peer 0, the last peer, the lightest and the heaviest sender of the run, and `extra`."""
    total = offered_per_window(windows, n).sum(axis=0)
    return sorted({0, n - 1, int(np.argmin(total)), int(np.argmax(total)), *map(int, extra)})


def first_difference(a, b):
    m = min(len(a), len(b))
    bad = np.nonzero(a[:m] != b[:m])[0]
    i = int(bad[0]) if len(bad) else m
    return i, (a[i] if i < len(a) else None), (b[i] if i < len(b) else None)


def assert_capture_same(got, want, what):
    """got: Engine.capture_read(); want: (tx, rx) of workloads.capture_reference.  As bytes."""
    for k, ref in zip(DIRS, want):
        a = got[k]
        assert a.dtype == ref.dtype == abi.CAPTURE_DTYPE
        if a.tobytes() != ref.tobytes():
            i, x, y = first_difference(a, ref)
            raise AssertionError(f"{what}: {k} capture differs ({len(a)} records against {len(ref)}), first at record {i}: "
                                 f"{x} against {y}")


class Account:
    """The counters' invariants over a run: seen == read so far + pending + dropped, per direction."""

    def __init__(self, watched, owned=None):
        self.read = {k: 0 for k in DIRS}
        self.watched = list(watched)
        self.n_owned = len(watched) if owned is None else sum(owned[0] <= p < owned[1] for p in watched)

    def check(self, e, got, what, dropped=(0, 0)):
        for k in DIRS:
            self.read[k] += len(got[k])
        info = e.capture_info()
        assert info["n_watched"] == len(self.watched) and info["n_owned"] == self.n_owned, (what, info)
        for k, dr in zip(DIRS, dropped):
            assert info["pending"][k] == 0 and info["dropped"][k] == dr, (what, k, info)
            assert info["seen"][k] == self.read[k] + info["pending"][k] + info["dropped"][k], (what, k, info, self.read)
        return info


def window_same(g, c, what, drained=True):
    """mc.assert_window_same; for an engine that discards its deliveries only the verdict bytes."""
    if drained:
        return mc.assert_window_same(g, c, what)
    vg, vc = g.verdicts(), c.verdicts()
    assert len(vg) == len(vc) and vg.tobytes() == vc.tobytes(), f"{what}: verdicts differ"
    assert g.pending() == 0
    return vc, c.drain()


def lockstep(g, c, scenario, watched, what, generated=False, drained=True, stats=True):
    """The scenario on the armed engine and on the oracle, window by window: verdicts and deliveries, then
    the window's capture against the model of the oracle's artifacts, then the counters.  Returns the
    captured windows [(tx, rx)] and the oracle's artifacts."""
    acct, caps, art = Account(watched), [], []
    gg, gc_ = scenario(g), scenario(c)
    w = 0
    while True:
        start = c.stats()["now_tick"]
        try:
            next(gg)
            pk = next(gc_)
        except StopIteration:
            break
        pk = mc.NO_PACKETS if pk is None else pk
        v, d = window_same(g, c, f"{what}, window {w}", drained)
        got = g.capture_read()
        want = wl.capture_reference(watched, pk, v, d, start, c.tick_ns, generated=generated)
        assert_capture_same(got, want, f"{what}, window {w}")
        acct.check(g, got, f"{what}, after window {w}")
        if stats:
            assert g.stats() == c.stats(), f"{what}, window {w}: statistics"
        caps.append(want)
        art.append((start, pk, v, d))
        w += 1
    assert w > 0
    return caps, art


def sparse_windows(e):
    return int(e._fn("debug_sparse_windows")(e._h))


def armed(n, watched, flags=0, tx_cap=1 << 18, rx_cap=1 << 18, **kw):
    e = Engine(n, flags=flags, **kw)
    e.capture_init(watched, tx_cap=tx_cap, rx_cap=rx_cap)
    return e


# -- 1. dense and sparse kernels, rows far longer than a wavefront ---------------------------------------------
def scenario_a_then_quiet(eng):
    yield from mc.scenario_a(eng)
    yield mc._submit_step(eng, mc.NO_PACKETS, mc.A["ticks"])


@pytest.mark.parametrize("mode", ["0", "1"])
def test_a_dense_and_sparse_kernels(make_oracle, monkeypatch, mode):
    monkeypatch.setenv("TGSIM_SPARSE", mode)
    n = mc.A["n"]
    seen = survey(make_oracle(n, **mc.A["kw"]), scenario_a_then_quiet)
    watched = watch_list(seen, n)
    rows = offered_per_window(seen, n)[:, watched]
    assert rows.max() > 64 and (rows == 0).any() and (rows[:-1] > 0).any(axis=1).all(), rows
    g, c = armed(n, watched, **mc.A["kw"]), make_oracle(n, **mc.A["kw"])
    caps, _ = lockstep(g, c, scenario_a_then_quiet, watched, f"A, TGSIM_SPARSE={mode}")
    assert sum(len(rx) for _, rx in caps) > 0 and any((rx["flags"] & abi.FLAG_DUP).any() for _, rx in caps)
    assert sparse_windows(g) == (len(seen) if mode == "1" else 0)


# -- 2. compact emit layout and its pool -----------------------------------------------------------------------
def test_b_compact_layout_and_pool(make_oracle, monkeypatch):
    monkeypatch.setenv("TGSIM_SPARSE", "1")
    monkeypatch.setenv("TGSIM_EMIT_COMPACT", "2")
    monkeypatch.setenv("TGSIM_EMIT_R", "1")
    n = mc.B["n"]
    seen = survey(make_oracle(n, **mc.B["kw"]), mc.scenario_b)
    watched = watch_list(seen, n, extra=(8, 13))  # (a k_sim_multi source and a duplicating one)
    rows = offered_per_window(seen, n)[:, watched]
    assert rows.max() > 64 and ((rows == 0).any(axis=1) & (rows > 0).any(axis=1)).any()  # empty rows between full ones
    g, c = armed(n, watched, **mc.B["kw"]), make_oracle(n, **mc.B["kw"])
    lockstep(g, c, mc.scenario_b, watched, "B")
    assert sparse_windows(g) == mc.B["steps"]


# -- 3. gossip: generated sparse windows, deliveries kept or discarded -----------------------------------------
@pytest.mark.parametrize("discard", [False, True])
def test_d_gossip(make_oracle, discard):
    n = mc.D["n"]
    seen = survey(make_oracle(n, **mc.D["kw"]), mc.scenario_d)
    watched = watch_list(seen, n)
    g, c = armed(n, watched, flags=DISCARD if discard else 0, **mc.D["kw"]), make_oracle(n, **mc.D["kw"])
    caps, art = lockstep(g, c, mc.scenario_d, watched, f"D, discard={discard}", generated=True, drained=not discard, stats=False)
    assert 0 < max(len(pk) for _, pk, _, _ in art) < 64 * n and sparse_windows(g) == mc.D["windows"]
    assert sum(len(tx) for tx, _ in caps) > 0 and sum(len(rx) for _, rx in caps) > 0
    assert (g.gossip_reached() == c.gossip_reached()).all()


# -- 4. the device loops: generated rows and the calendar's replies --------------------------------------------
def _loop_capture(rec, reads, watched, window, what):
    assert len(reads) == len(rec.windows) > 0
    n_tx = n_rx = 0
    for w, (got, (pk, v, d)) in enumerate(zip(reads, rec.windows)):
        want = wl.capture_reference(watched, pk, v, d, w * window, rec.tick_ns)
        assert_capture_same(got, want, f"{what}, window {w}")
        n_tx, n_rx = n_tx + len(want[0]), n_rx + len(want[1])
    assert n_tx > 0 and n_rx > 0
    return n_tx, n_rx


def _loop_watch(rec, n, extra=()):
    return watch_list([(0, pk, v, d) for pk, v, d in rec.windows], n, extra)


def test_e_ping_mesh_armed(make_oracle):
    n, windows, window = mc.E["n"], mc.E["windows"], mc.LOOP["window"]
    rec = mc.Recording(make_oracle(n, flags=abi.OPT_METRICS, **mc.LOOP["kw"]))  # (Recording reads the oracle's tables)
    ping, targets = mc.e_setup(rec)
    ref = wl.ping_reference(rec, ping, targets, windows, window)
    watched = _loop_watch(rec, n)
    eng = Engine(n, **mc.LOOP["kw"])
    mc.e_setup(eng)
    eng.ping_init(targets, **ping)
    eng.capture_init(watched)
    reads = []
    dev = wl.ping_run(eng, windows, window, collect=True, before=lambda w: reads.append(eng.capture_read()) if w else None)
    reads.append(eng.capture_read())
    for w, ((dv, dd), (_, rv, rd)) in enumerate(zip(dev["windows"], rec.windows)):
        assert dv.tobytes() == rv.tobytes() and dd.tobytes() == rd.tobytes(), f"E, window {w}: the windows differ"
    _loop_capture(rec, reads, watched, window, "E")
    assert eng.ping_report()["received"] == ref["summary"]["received"] > 0
    info = eng.capture_info()
    assert all(info["seen"][k] == sum(len(r[k]) for r in reads) and info["dropped"][k] == 0 for k in DIRS)


def test_f_flows_armed_with_feedback(make_oracle):
    n, windows, window = mc.F["n"], mc.F["windows"], mc.LOOP["window"]
    rec = mc.Recording(make_oracle(n, flags=abi.OPT_METRICS, **mc.LOOP["kw"]))
    flows = mc.f_setup(rec)
    ref = wl.flow_reference(rec, mc.F["flow"], flows, windows, window, fb=mc.F["fb"])
    watched = _loop_watch(rec, n, extra=(mc.F["cut"][0],))
    eng = Engine(n, **mc.LOOP["kw"])
    assert mc.f_setup(eng).tobytes() == flows.tobytes()
    eng.flow_init(flows, fb=mc.F["fb"], **mc.F["flow"])
    eng.capture_init(watched)
    reads = []
    dev = wl.flow_run(eng, windows, window, collect=True, before=lambda w: reads.append(eng.capture_read()) if w else None)
    reads.append(eng.capture_read())
    for w, ((dv, dd), (_, rv, rd)) in enumerate(zip(dev["windows"], rec.windows)):
        assert dv.tobytes() == rv.tobytes() and dd.tobytes() == rd.tobytes(), f"F, window {w}: the windows differ"
    _loop_capture(rec, reads, watched, window, "F")
    tx = np.concatenate([r["tx"] for r in reads])
    cut = tx[tx["src"] == mc.F["cut"][0]]
    assert ((cut["verdict"] & 15) == abi.V_BLACKHOLE).any()  # the refused offers of the cut flow
    assert eng.flow_report()["done"] == ref["summary"]["done"] > 0


# -- 5. reconfiguration: a disconnect and a reshape in mid-run -------------------------------------------------
def test_g_reconfiguration(make_oracle):
    n, gone = mc.G["n"], mc.G["gone"]
    seen = survey(make_oracle(n), mc.scenario_g)
    # a record lost in flight: scheduled towards `gone` before it left, in no window's drain
    delivered = {(int(r["src"]), int(r["seq"])) for _, _, _, d in seen for r in d[d["dst"] == gone]}
    lost = [(int(p["src"]), int(p["seq"])) for _, pk, v, _ in seen[:mc.G["at"]]
            for p in pk[(pk["dst"] == gone) & ((v & 15) == abi.V_SCHEDULED)] if (int(p["src"]), int(p["seq"])) not in delivered]
    assert lost
    watched = watch_list(seen, n, extra=(gone, lost[0][0], mc.g_reshaped(n)))
    g, c = armed(n, watched), make_oracle(n)
    caps, _ = lockstep(g, c, mc.scenario_g, watched, "G")
    assert c.stats()["flushed"] > 0 and c.stats()["lost_in_flight"] > 0
    tx, rx = np.concatenate([t for t, _ in caps]), np.concatenate([r for _, r in caps])
    assert ((tx["verdict"] & 15) == abi.V_DISCONNECTED).any()
    mine = tx[(tx["src"] == lost[0][0]) & (tx["seq"] == lost[0][1]) & (tx["dst"] == gone)]
    assert len(mine) == 1 and mine["verdict"][0] & 15 == abi.V_SCHEDULED
    assert not ((rx["dst"] == gone) & (rx["src"] == lost[0][0]) & (rx["seq"] == lost[0][1])).any()


# -- 6. tgsim_step_n on an armed engine: window by window, one read --------------------------------------------
def test_h_step_n_with_discard(make_oracle):
    h = mc.H
    n, ticks, k = h["n"], h["ticks"], h["windows"]
    seen = survey(make_oracle(n), mc.SCENARIOS["H"][2])
    watched = watch_list(seen, n)
    a = armed(n, watched, flags=DISCARD)
    wl.configure_storm(a, n)
    for _ in range(k):
        a.gen_storm(h["lam"], ticks)
    a.step_n(ticks, k)
    got = a.capture_read()
    assert int(a._fn("debug_fused_launches")(a._h)) == 0 and int(a._fn("debug_fused_windows")(a._h)) == 0
    assert min(len(pk) for _, pk, _, _ in seen) >= 64 * n and sparse_windows(a) == 0  # dense: unarmed they would fuse
    refs = [wl.capture_reference(watched, pk, v, d, start, a.tick_ns, generated=True) for start, pk, v, d in seen]
    want = tuple(np.concatenate([r[i] for r in refs]) for i in (0, 1))
    assert_capture_same(got, want, f"H, one read after step_n of {k} windows")
    Account(watched).check(a, got, "H, step_n")
    assert len(want[0]) > 0 and len(want[1]) > 0 and a.pending() == 0


# -- 7. room ---------------------------------------------------------------------------------------------------
def test_room(make_oracle):
    h = mc.H
    n, ticks = h["n"], h["ticks"]
    seen = survey(make_oracle(n), mc.SCENARIOS["H"][2])
    watched = watch_list(seen, n)
    refs = [wl.capture_reference(watched, pk, v, d, start, 1000, generated=True) for start, pk, v, d in seen]
    n0, n1, n2 = (len(refs[w][0]) for w in range(3))
    rows1 = np.bincount(refs[1][0]["src"], minlength=n)[watched]
    assert rows1[0] > 0 and rows1[1] > 2
    cap = n0 + int(rows1[0]) + int(rows1[1]) // 2  # ends inside the second watched row of the second window
    assert n0 < cap < n0 + n1 and n2 <= cap
    g = armed(n, watched, tx_cap=cap, rx_cap=0)
    gen = mc.SCENARIOS["H"][2](g)
    next(gen), next(gen)
    info = g.capture_info()
    assert info["pending"] == {"tx": cap, "rx": 0} and info["seen"] == {"tx": n0 + n1, "rx": 0}, info
    assert info["dropped"] == {"tx": n0 + n1 - cap, "rx": 0}, info
    fn = g._fn("capture_read")
    assert fn(g._h, TX, None, 0) == cap
    short = np.zeros(cap, dtype=abi.CAPTURE_DTYPE)
    assert fn(g._h, TX, short.ctypes.data, cap - 1) == -errno.ENOSPC and not short.view(np.uint8).any()
    assert g.capture_info() == info  # nothing was removed
    got = g.capture_read()
    kept = np.concatenate([refs[0][0], refs[1][0]])[:cap]
    assert_capture_same(got, (kept, refs[0][1][:0]), "room: the kept prefix")
    info = g.capture_info()
    assert info["pending"]["tx"] == 0 and info["seen"]["tx"] == cap + info["dropped"]["tx"]
    next(gen)  # the read made room: the next window is captured whole
    got = g.capture_read()
    assert_capture_same(got, (refs[2][0], refs[2][1][:0]), "room: the window after the read")
    info = g.capture_info()
    assert info["seen"] == {"tx": n0 + n1 + n2, "rx": 0} and info["dropped"] == {"tx": n0 + n1 - cap, "rx": 0}
    assert info["seen"]["tx"] == cap + n2 + info["pending"]["tx"] + info["dropped"]["tx"]


# -- 8. the shortest and the longest watch list ----------------------------------------------------------------
@pytest.mark.parametrize("entries", [1, 1024])
def test_watch_list_sizes(make_oracle, entries):
    n, lam, ticks, windows = 1100, 0.1, 1000, 2
    seen = survey(make_oracle(n), mc.scenario_storm(n, lam, ticks, windows))
    busiest = int(np.argmax(np.bincount(np.concatenate([d["dst"] for _, _, _, d in seen]).astype(np.int64), minlength=n)))
    watched = [busiest] if entries == 1 else [int(p) for p in np.r_[0:500, 576:n]]  # (the one that receives the most)
    assert len(watched) == entries == (1 if entries == 1 else abi.CAPTURE_MAX_PEERS)
    g, c = armed(n, watched, tx_cap=1 << 19, rx_cap=1 << 19), make_oracle(n)
    caps, _ = lockstep(g, c, mc.scenario_storm(n, lam, ticks, windows), watched, f"{entries} watched", generated=True)
    assert all(len(tx) > 0 for tx, _ in caps) and sum(len(rx) for _, rx in caps) > 0


# -- 9. shards over the engine's own exchange ------------------------------------------------------------------
SHARD_WATCH = [0, 69, 70, 99, 100, 101, 154, 155, 239]


@pytest.mark.parametrize("bounds", [[0, 100, 240], [0, 70, 155, 240]])
def test_shards(lib, make_oracle, bounds):  # noqa: F811
    h = mc.H
    n = h["n"]
    assert all(b - 1 in SHARD_WATCH and b in SHARD_WATCH for b in bounds[1:-1])  # both sides of each bound

    def rank(r, e):
        e.capture_init(SHARD_WATCH)
        out = []
        for _ in mc.scenario_storm(n, h["lam"], h["ticks"], h["windows"], step=lambda eng, t: eng.comm_step(t))(e):
            out.append((e.verdicts(), e.drain(), e.capture_read(), e.capture_info()))
        return out

    per_rank, info = _ranks(lib, n, bounds, rank)
    assert all(i["nranks"] == len(bounds) - 1 for i in info)
    c = make_oracle(n)
    seen = survey(c, mc.SCENARIOS["H"][2])
    assert len(seen) == len(per_rank[0]) == h["windows"]
    for w, (start, pk, v, d) in enumerate(seen):
        got = [p[w] for p in per_rank]
        assert np.concatenate([x[0] for x in got]).tobytes() == v.tobytes(), f"window {w}: verdicts differ"
        assert np.concatenate([x[1] for x in got]).tobytes() == d.tobytes(), f"window {w}: deliveries differ"
        want = wl.capture_reference(SHARD_WATCH, pk, v, d, start, c.tick_ns, generated=True)
        assert_capture_same(wl.merge_captures([x[2] for x in got]), want, f"{len(bounds) - 1} ranks, window {w}")
        for r, x in enumerate(got):  # each rank holds its own peers' part
            mine = wl.capture_reference(SHARD_WATCH, pk, v, d, start, c.tick_ns, owned=(bounds[r], bounds[r + 1]), generated=True)
            assert_capture_same(x[2], mine, f"rank {r}, window {w}")
        assert sum(x[3]["n_owned"] for x in got) == got[0][3]["n_watched"] == len(SHARD_WATCH)
        assert all(x[3]["n_owned"] > 0 and x[3]["dropped"] == {"tx": 0, "rx": 0} for x in got)
    assert sum(i["exchanged_records"] for i in info) > 0


def test_comm_run_refuses_fused_groups_with_capture(lib):  # noqa: F811
    h = mc.H
    n, ticks, k, bounds = h["n"], h["ticks"], h["windows"], [0, 100, 240]

    def rank(r, e):
        wl.configure_storm(e, n)
        e.capture_init(SHARD_WATCH)
        for _ in range(k):
            e.gen_storm(h["lam"], ticks)
        before = e.stats()
        try:
            e.comm_run(ticks, k, 2, 0)
            err = None
        except EngineError as ex:
            err = (ex.code, ex.msg)
        return err, before, e.stats(), e.capture_info()

    per_rank, _ = _ranks(lib, n, bounds, rank)
    for r, (err, before, after, info) in enumerate(per_rank):
        assert err is not None, f"rank {r}: comm_run(fuse=2) succeeded"
        assert err[0] == -errno.EINVAL and "capture" in err[1] and "fuse = 1" in err[1], err
        assert after == before and before["now_tick"] == 0 and before["offered"] == 0, f"rank {r}: the refused run simulated"
        assert info["seen"] == {"tx": 0, "rx": 0}


# -- 10. the C ABI's edges -------------------------------------------------------------------------------------
def _refused(e, code, *needles, **kw):
    with pytest.raises(EngineError) as ei:
        e.capture_init(**kw)
    assert ei.value.code == code and all(s in ei.value.msg for s in needles), (ei.value.code, ei.value.msg)


def test_abi_edges():
    n = 1100
    e = Engine(n)
    _refused(e, -errno.EINVAL, "peers[1] = 2", "peers[0] = 3", peers=[3, 2])        # unsorted
    _refused(e, -errno.EINVAL, "peers[2] = 5", "peers[1] = 5", peers=[1, 5, 5, 9])  # repeated
    _refused(e, -errno.EINVAL, f"peers[1] = {n}", f"n_peers {n}", peers=[0, n])     # out of range
    _refused(e, -errno.EINVAL, "n 0", peers=[])
    _refused(e, -errno.EINVAL, "n 1025", peers=list(range(1025)))
    _refused(e, -errno.EINVAL, "tx_cap and rx_cap are both 0", peers=[0], tx_cap=0, rx_cap=0)
    _refused(e, -errno.EINVAL, "tx_cap", peers=[0], tx_cap=(1 << 31) + 1)
    for name, args in (("capture_info", (abi.CaptureInfo(),)), ("capture_read", (TX, None, 0))):  # unarmed
        with pytest.raises(EngineError) as ei:
            e._check(e._fn(name)(e._h, *args), name)
        assert ei.value.code == -errno.EINVAL and "capture is not armed" in ei.value.msg
    e.capture_init(None)  # disarming an unarmed engine: a no-op
    wl.configure_storm(e, n)
    e.gen_storm(0.01, 1000)
    _refused(e, -errno.EBUSY, "generated windows are pending", peers=[0])
    e.step(1000)
    e.drain()
    e.capture_init([0, n - 1], tx_cap=1 << 16, rx_cap=1 << 16)
    with pytest.raises(EngineError) as ei:
        e._check(e._fn("capture_read")(e._h, 2, None, 0), "capture_read")
    assert ei.value.code == -errno.EINVAL and "dir 2" in ei.value.msg
    e.gen_storm(0.01, 1000)
    e.step(1000)
    info = e.capture_info()
    assert info["seen"]["tx"] == info["pending"]["tx"] > 0 and info["n_watched"] == info["n_owned"] == 2
    e.capture_init(None)  # disarm ...
    with pytest.raises(EngineError):
        e.capture_info()
    e.capture_init([5])   # ... and re-arm: everything zero
    info = e.capture_info()
    assert info == {"pending": {"tx": 0, "rx": 0}, "seen": {"tx": 0, "rx": 0}, "dropped": {"tx": 0, "rx": 0},
                    "n_watched": 1, "n_owned": 1}
    got = e.capture_read()
    assert len(got["tx"]) == 0 and len(got["rx"]) == 0
    e.capture_init([0, n - 1])  # re-arming an armed engine replaces the list and zeroes
    assert e.capture_info()["n_watched"] == 2 and e.capture_info()["seen"] == {"tx": 0, "rx": 0}


def test_capture_observes_and_never_alters():
    h = mc.H
    n = h["n"]
    plain, watching = Engine(n), armed(n, [0, 7, 100, n - 1])
    for _, _ in zip(mc.SCENARIOS["H"][2](plain), mc.SCENARIOS["H"][2](watching)):
        assert plain.verdicts().tobytes() == watching.verdicts().tobytes()
        assert plain.drain().tobytes() == watching.drain().tobytes()
    assert plain.stats() == watching.stats() and plain.stats()["scheduled"] > 0
    assert watching.capture_info()["seen"]["tx"] > 0


# -- 11. the runner: capture.pcap per watched instance ---------------------------------------------------------
def test_runner_writes_pcaps(tmp_path):
    times = {"sent": [], "received": []}

    def plan(env: rn.PlanEnv) -> None:
        env.net.WaitNetworkInitialized(env.ctx)
        env.net.ConfigureNetwork(env.ctx, wl.pingpong_config(10 * nw.Millisecond))
        env.sync.SignalAndWait(env.ctx, "ready", 2)
        if env.seq == 0:
            for k in range(3):
                times["sent"].append(env.data.now_ns())
                env.data.send(1, bytes([k]))
            while len(times["received"]) < 3:
                times["received"] += [t for t, _, _, _ in env.data.recv(timeout_ns=10**9)]
        else:
            got = 0
            while got < 3:
                for t_ns, src, data, _ in env.data.recv(timeout_ns=10**9):
                    env.data.send(src, data, at_ns=t_ns)  # echo at the arrival time
                    got += 1
        env.sync.SignalAndWait(env.ctx, "done", 2)

    cfg = rn.LocalSimRunnerCfg(outputs_dir=str(tmp_path), run_timeout_s=60, capture=[0, 1], capture_cap=1 << 12)
    job = rn.RunInput(RunID="cap", TestPlan="network", TestCase="echo", TotalInstances=2,
                      Groups=[rn.RunGroup("single", 2, plan)], RunnerConfig=cfg)
    r = rn.LocalSimRunner()
    out = r.Run(Context(), job)
    assert out.Result.Outcome == rn.OUTCOME_SUCCESS, out.Result.Errors
    run_dir = tmp_path / "network" / "cap"
    files = [run_dir / "single" / str(i) / "capture.pcap" for i in (0, 1)]
    pk = [pcap.read_pcap(io.BytesIO(f.read_bytes())) for f in files]
    ip0, ip1 = wl.peer_ip(0), wl.peer_ip(1)
    tx0 = [p for p in pk[0] if p["src_ip"] == ip0]
    rx0 = [p for p in pk[0] if p["dst_ip"] == ip0]
    assert len(pk[0]) == 6 and len(tx0) == 3 and len(rx0) == 3 and len(pk[1]) == 6
    assert all(p["dst_ip"] == ip1 for p in tx0) and all(p["src_ip"] == ip1 for p in rx0)
    assert [p["t_ns"] for p in tx0] == times["sent"] and [p["t_ns"] for p in rx0] == sorted(times["received"])
    assert all(p["checksum_ok"] and p["total_len"] == 1 + 28 for p in pk[0] + pk[1])
    assert min(p["t_ns"] for p in rx0) >= times["sent"][0] + 20 * nw.Millisecond
    import json
    doc = json.loads((run_dir / "run.json").read_text())
    assert doc["capture"]["seen"] == {"tx": 6, "rx": 6} and doc["capture"]["n_watched"] == 2
    buf = io.BytesIO()
    r.CollectOutputs(Context(), rn.CollectionInput("cap", "network"), buf, cfg)
    names = tarfile.open(fileobj=io.BytesIO(buf.getvalue()), mode="r:gz").getnames()
    assert "cap/single/0/capture.pcap" in names and "cap/single/1/capture.pcap" in names
