"""The batch loop of sim_source (k_sim, k_sim_recv, k_sim_fused): records of the next batches loaded
while a batch is resolved, each batch's verdict bytes stored during the next one (the last after the
loop), and the original's delay drawn once per packet however many sub-windows decide it again.
Bit-exact against the CPU oracle: batch counts of either parity with every tail length, a source
with nothing offered, the heavy regime whose batches take many sub-windows, and the same through
fused launches."""
import numpy as np
import pytest

from testground_amd import abi
from testground_amd import network as nw
from testground_amd import workloads as wl

from test_gpu_parity import assert_same, both, random_packets  # noqa: F401  (random_packets: the packet layout)

pytestmark = pytest.mark.gpu

try:  # torch ships its own HIP runtime: let it initialise first when both share a process
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()
except ImportError:  # pragma: no cover
    torch = None

# packets offered per source and window: no batch, one lane, a full batch and one lane either side
# of it, and the same around two, three and four batches (odd and even batch counts)
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)
N_PLAIN, N_HEAVY = 24, 64


def configure_plain(e):
    """24 sources with the storm's shapes: no rules, every peer connected (the kernel's plain filter)."""
    wl.configure_storm(e, N_PLAIN)


def configure_heavy(e):
    """64 sources at 1 Gbit/s, latency 1-7 ms and a jitter above it (delays clamped to 0: admissions
    eligible at their own offer time end the sub-window), 50 % reorder on every fourth source and
    20 % duplicates on every third."""
    for i in range(N_HEAVY):
        lat = (1 + i % 7) * nw.Millisecond
        s = nw.LinkShape(Latency=lat, Jitter=lat + (1 + i % 3) * nw.Millisecond, Bandwidth=10**9,
                         Reorder=50.0 if i % 4 == 0 else 0.0, Duplicate=20.0 if i % 3 == 0 else 0.0)
        e.configure(i, nw.Config(Network="default", Enable=True, Default=s))


def exact_counts(rng, n, counts, n_ticks, seq_base):
    """counts[i] packets of source i at random ticks of one window, to random other peers."""
    src = np.repeat(np.arange(n), counts)
    m = len(src)
    pk = np.zeros(m, dtype=abi.PKT_DTYPE)
    pk["src"] = src
    pk["dst"] = (src + 1 + rng.integers(0, n - 1, m)) % n
    pk["len"] = rng.integers(40, 1500, m)
    pk["tick"] = rng.integers(0, n_ticks, m)
    order = np.lexsort((pk["tick"], src))  # per-source sequence numbers in tick order
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    seq = np.empty(m, dtype=np.uint32)
    seq[order] = np.arange(m) - starts[src[order]] + seq_base[src[order]]
    pk["seq"] = seq
    seq_base += np.asarray(counts, dtype=np.uint32)
    return pk


def test_batch_count_parity_and_tails(make_oracle):
    """Source i is offered exactly COUNTS[i mod 12] packets in each of three windows: the last verdict
    byte of an odd and of an even number of batches, every tail length, and nothing at all."""
    g, c = both(make_oracle, N_PLAIN, queue_limit=32)
    configure_plain(g)
    configure_plain(c)
    rng = np.random.default_rng(71)
    counts = np.array([COUNTS[i % len(COUNTS)] for i in range(N_PLAIN)])
    seq = np.zeros(N_PLAIN, dtype=np.uint32)
    for step in range(3):
        pk = exact_counts(rng, N_PLAIN, counts, 2000, seq)
        assert np.array_equal(np.bincount(pk["src"], minlength=N_PLAIN), counts)
        g.submit(pk)
        c.submit(pk)
        g.step(2000)
        c.step(2000)
        v, _ = assert_same(g, c, f"exact counts, window {step}")
        assert len(v) == counts.sum()
    assert g.stats()["by_verdict"]["queue_full"] > 0  # the windowed path, not only the open queue


@pytest.mark.parametrize("queue_limit", [1000, 32])
def test_heavy_regime(make_oracle, queue_limit):
    """300 packets per source and window on the heavy shapes, four windows: batches of many
    sub-windows, in which a packet's drawn delay is used again."""
    g, c = both(make_oracle, N_HEAVY, queue_limit=queue_limit)
    configure_heavy(g)
    configure_heavy(c)
    rng = np.random.default_rng(73 + queue_limit)
    counts = np.full(N_HEAVY, 300)
    seq = np.zeros(N_HEAVY, dtype=np.uint32)
    for step in range(4):
        pk = exact_counts(rng, N_HEAVY, counts, 2000, seq)
        g.submit(pk)
        c.submit(pk)
        g.step(2000)
        c.step(2000)
        assert_same(g, c, f"heavy, limit {queue_limit}, window {step}")
    s = g.stats()
    assert s["scheduled"] > 0 and s["cloned"] > 0
    if queue_limit == 32:
        assert s["by_verdict"]["queue_full"] > 0


@pytest.mark.parametrize("ticks", [100, 130, 250, 260])
@pytest.mark.parametrize("shapes,queue_limit", [("plain", 32), ("heavy", 1000), ("heavy", 32)])
def test_fused(make_oracle, monkeypatch, shapes, queue_limit, ticks):
    """The same shapes through generated storm windows and step_n (fused groups of four, 4 + 2, where
    the engine fuses), one to five batches per source and window, against the oracle stepping one by
    one."""
    monkeypatch.setenv("TGSIM_FUSE", "4")  # read at engine creation
    n = N_PLAIN if shapes == "plain" else N_HEAVY
    g, c = both(make_oracle, n, queue_limit=queue_limit)
    for e in (g, c):
        (configure_plain if shapes == "plain" else configure_heavy)(e)
        for _ in range(6):
            e.gen_storm(0.5, ticks)
        e.step_n(ticks, 6)
    # the engine fuses windows of at least 64 packets per source on average: always at 250 and 260
    # ticks (125 and 130), never at 100 (50; those run k_sim or the sparse kernels), either way at 130
    if ticks >= 250:
        assert int(g._fn("debug_fused_windows")(g._h)) == 6
    v, _ = assert_same(g, c, f"fused {shapes}, limit {queue_limit}, {ticks} ticks")
    assert len(v) > 0
