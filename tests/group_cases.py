"""The per-group traffic matrix cases shared by tests/test_group_model.py (the host model,
workloads.GroupMatrix, over the CPU oracle, cross-checked against the oracle's TGSIM_OPT_METRICS
tables) and tests/test_gpu_groups.py (the HIP engine's tgsim_group_matrix against that model, word
for word after every window).

The checker is always the model fed from the oracle: the packets offered to it (tgo_offered for
generated windows, the submitted array for host traffic), tgo_verdicts and tgo_drain; never the HIP
engine's own outputs."""
import ipaddress

import numpy as np

from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

N = 96            # peers of the base case
WINDOW = 2_000    # ticks per traffic window
PER_WINDOW = 40_000
IDLE = 200_000    # the last, idle window: everything in flight is delivered
SEED = 11


def base_groups(n=N):
    """splitbrain's regions: 3 groups, interleaved (seq % 3)."""
    return wl.splitbrain_regions(n).astype(np.uint16), 3


def configure_base(eng, n=N):
    """Storm shapes; splitbrain's drop rules (region A filters region B, on unshaped links); one
    Reject /32 rule, peer 2 towards peer 5; peer 7 disconnected; peers 8..15 AllowAll (the only ones
    whose TGSIM_EXTERNAL packets leave the data network)."""
    wl.configure_storm(eng, n)
    region = wl.configure_splitbrain(eng, n, "drop")
    shapes = wl.storm_shapes(n)

    def rules(i, extra=()):
        out = [nw.LinkRule(Subnet=(str(ipaddress.IPv4Address(wl.peer_ip(int(p)))), 32),
                           LinkShape=nw.LinkShape(Filter=nw.FilterAction.Drop))
               for p in np.nonzero(region == wl.REGION_B)[0]] if region[i] == wl.REGION_A else []
        return out + [nw.LinkRule(Subnet=(str(ipaddress.IPv4Address(wl.peer_ip(p))), 32),
                                  LinkShape=nw.LinkShape(Filter=nw.FilterAction.Reject)) for p in extra]

    assert region[2] == wl.REGION_A and region[5] == wl.REGION_A
    eng.configure(2, nw.Config(Network="default", Enable=True, Rules=rules(2, extra=(5,))))
    eng.configure(7, nw.Config(Network="default", Enable=False))
    for i in range(8, 16):
        eng.configure(i, nw.Config(Network="default", Enable=True, Rules=rules(i),
                                   Default=nw.LinkShape() if region[i] == wl.REGION_A else shapes[i],
                                   RoutingPolicy=nw.RoutingPolicyType.AllowAll))


def configure_plain(eng, n):
    """The layout and shard cases: storm shapes, peer 7 disconnected, peers 8..15 AllowAll."""
    wl.configure_storm(eng, n)
    shapes = wl.storm_shapes(n)
    eng.configure(7, nw.Config(Network="default", Enable=False))
    for i in range(8, 16):
        eng.configure(i, nw.Config(Network="default", Enable=True, Default=shapes[i],
                                   RoutingPolicy=nw.RoutingPolicyType.AllowAll))


def traffic(n, w, seqs, per_window=PER_WINDOW, window=WINDOW, seed=SEED, hot=0.0, external=0.05):
    """Window w's random packets: uniform sources, destinations other than the source (a fraction
    `external` of them TGSIM_EXTERNAL, a fraction `hot` peer 0), U[64, 1500] bytes, per-source running
    sequence numbers carried in `seqs` (updated)."""
    rng = np.random.default_rng(seed * 1000 + w)
    pk = np.zeros(per_window, dtype=abi.PKT_DTYPE)
    src = rng.integers(0, n, per_window)
    dst = (src + 1 + rng.integers(0, n - 1, per_window)) % n
    dst = np.where((rng.random(per_window) < hot) & (src != 0), 0, dst)
    dst = np.where(rng.random(per_window) < external, abi.EXTERNAL, dst)
    pk["src"], pk["dst"] = src, dst
    pk["len"] = rng.integers(64, 1501, per_window)
    pk["tick"] = rng.integers(0, window, per_window)
    order = np.argsort(src, kind="stable")
    counts = np.bincount(src, minlength=n)
    rank = np.arange(per_window) - np.repeat(np.cumsum(counts) - counts, counts)
    pk["seq"][order] = seqs[src[order]] + rank
    seqs += counts
    return pk


def base_windows(n=N, n_windows=3, idle=IDLE, **kw):
    """[(packets or None, ticks)]: the traffic windows, then the idle one."""
    seqs = np.zeros(n, dtype=np.int64)
    return [(traffic(n, w, seqs, **kw), kw.get("window", WINDOW)) for w in range(n_windows)] + [(None, idle)]


def model_series(cpu, group_of, n_groups, windows, before=None, artifacts=None):
    """The model folded over the oracle `cpu`, window by window: the matrix after every window.
    before(eng, w) runs ahead of window w (a reconfiguration); artifacts (a list) receives every
    window's (packets, verdict bytes, drained records)."""
    gm = wl.GroupMatrix(group_of, n_groups)
    out = []
    for w, (pk, ticks) in enumerate(windows):
        if before is not None:
            before(cpu, w)
        have = pk is not None and len(pk)
        if have:
            cpu.submit(pk)
        cpu.step(ticks)
        pk = pk if have else np.zeros(0, dtype=abi.PKT_DTYPE)
        v, d = cpu.verdicts() if have else np.zeros(0, dtype=np.uint8), cpu.drain()
        gm.fold(pk, v, d)
        if artifacts is not None:
            artifacts.append((pk, v, d))
        out.append(gm.m.copy())
    return out


def device_series(eng, windows, reset=False, before=None):
    """An armed engine driven through the same windows: its matrix after every window."""
    out = []
    for w, (pk, ticks) in enumerate(windows):
        if before is not None:
            before(eng, w)
        if pk is not None and len(pk):
            eng.submit(pk)
        eng.step(ticks)
        eng.drain()
        out.append(eng.group_matrix(reset=reset))
    return out


def offered(cpu, cap=1 << 21):
    """The packets the oracle will simulate in its next step (a generated window), in verdict order."""
    pk = np.zeros(cap, dtype=abi.PKT_DTYPE)
    m = cpu._lib.tgo_offered(cpu._h, pk.ctypes.data, len(pk))
    assert 0 <= m <= cap
    return pk[:m].copy()


def fold_step(gm, cpu, ticks):
    """One step of the oracle (its pending generated window or host packets already submitted are the
    input; `offered` is read first) folded into the model."""
    pk = offered(cpu)
    cpu.step(ticks)
    gm.fold(pk, cpu.verdicts(), cpu.drain())


def class_totals(m):
    """The classes the base case must exercise, from a matrix."""
    t = m.sum(axis=(0, 1))
    out = {name: int(t[2 + i]) for i, name in enumerate(abi.VERDICT_NAMES)}
    out.update(clones_delivered=int(t[12]), corrupt_delivered=int(t[13]), offered=int(t[0]), delivered=int(t[10]))
    return out


def assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first (src group, dst group, word) "
                           f"{bad[0].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")
