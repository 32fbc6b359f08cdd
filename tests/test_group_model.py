"""The host model of the per-group traffic matrix (workloads.GroupMatrix) over the CPU oracle, checked
against an independent path: the oracle's own TGSIM_OPT_METRICS tables reduced by group.  Also the
helpers around it: merge_group_matrices, group_reachability (against splitbrain's expectErrors) and
metrics.group_lines."""
import numpy as np
import pytest

import group_cases as gc
from testground_amd import abi
from testground_amd import metrics
from testground_amd import workloads as wl


@pytest.fixture(scope="module")
def base(oracle_lib):
    from testground_amd.engine import CABIEngine

    cpu = CABIEngine(oracle_lib, "tgo_", gc.N, flags=abi.OPT_METRICS)
    gc.configure_base(cpu)
    group_of, g = gc.base_groups()
    windows = gc.base_windows()
    series = gc.model_series(cpu, group_of, g, windows)
    return dict(cpu=cpu, group_of=group_of.astype(np.int64), g=g, windows=windows, series=series)


def test_base_case_exercises_every_class(base):
    """A later edit cannot hollow the case out: every verdict, clones and corrupted copies occur."""
    t = gc.class_totals(base["series"][-1])
    for key in abi.VERDICT_NAMES + ["clones_delivered", "corrupt_delivered"]:
        assert t[key] > 0, (key, t)
    assert t["offered"] == 3 * gc.PER_WINDOW
    m = base["series"][-1]
    assert (m[:, :, :].sum(axis=(0, 1)) > 0).all()  # all 14 words
    # nothing is purged or flushed in this case: after the idle window every scheduled record was delivered
    assert base["cpu"].stats()["lost_in_flight"] == 0
    assert (m[:, :, 2] == m[:, :, 10]).all()
    assert (m[:, base["g"], 10:] == 0).all()  # nothing is delivered to TGSIM_EXTERNAL
    assert (np.diff(np.array([s[:, :, 10].sum() for s in base["series"]]).astype(np.int64)) >= 0).all()


def test_model_equals_the_oracle_metrics_reduced_by_group(base):
    m, g, group_of = base["series"][-1], base["g"], base["group_of"]
    tab = base["cpu"].metrics()
    rows = np.zeros((g, 10), dtype=np.uint64)
    np.add.at(rows, group_of, tab["src"][:, :10])
    assert (m[:, :, :10].sum(axis=1, dtype=np.uint64) == rows).all()
    cols = np.zeros((g, 2), dtype=np.uint64)
    np.add.at(cols, group_of, tab["dst"])
    assert (m[:, :g, 10:12].sum(axis=0, dtype=np.uint64) == cols).all()
    s = base["cpu"].stats()
    assert int(m[:, :, 0].sum()) == s["offered"]
    assert [int(m[:, :, 2 + i].sum()) for i in range(8)] == [s["by_verdict"][k] for k in abi.VERDICT_NAMES]


def test_fold_words():
    """The word definitions on a hand-made window."""
    gm = wl.GroupMatrix([0, 1, 1], 2)
    pk = np.array([(0, 1, 0, 100, 0), (1, 2, 0, 50, 1), (2, abi.EXTERNAL, 0, 7, 1), (0, 2, 1, 65535, 2)], dtype=abi.PKT_DTYPE)
    v = np.array([abi.V_SCHEDULED | abi.V_SCHEDULED << 4, abi.V_LOSS | abi.V_NONE << 4, abi.V_EXTERNAL | abi.V_NONE << 4,
                  abi.V_LOSS | abi.V_SCHEDULED << 4], dtype=np.uint8)
    d = np.array([(5, 0, 1, 0, 100, abi.FLAG_DUP), (6, 0, 1, 0, 100, abi.FLAG_CORRUPT), (7, 0, 2, 1, 65535, abi.FLAG_DUP | abi.FLAG_CORRUPT)],
                 dtype=abi.DELIVERY_DTYPE)
    m = gm.fold(pk, v, d).m
    assert m[0, 1].tolist() == [2, 65635, 3, 0, 0, 0, 0, 1, 0, 0, 3, 65735, 2, 2]
    assert m[1, 1].tolist() == [1, 50, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert m[1, 2].tolist() == [1, 7, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert m.sum() == m[0, 1].sum() + m[1, 1].sum() + m[1, 2].sum()
    with pytest.raises(ValueError):
        gm.fold(pk, v[:2], None)
    with pytest.raises(ValueError):
        wl.GroupMatrix([0, 2], 2)
    with pytest.raises(ValueError):
        wl.GroupMatrix([0], 65)


def test_merge_group_matrices(base):
    """Folding the sources of two disjoint peer ranges apart (words 0..9) and the destinations of the
    same ranges apart (words 10..13), as two shards do, sums to the whole."""
    a, b = base["series"][1], base["series"][-1]
    assert (wl.merge_group_matrices([a, b]) == a + b).all()
    assert wl.merge_group_matrices([a]).dtype == np.uint64
    with pytest.raises(ValueError):
        wl.merge_group_matrices([])
    with pytest.raises(ValueError):
        wl.merge_group_matrices([a, a[:2]])


@pytest.mark.parametrize("case", ["drop", "reject", "accept"])
def test_group_reachability_reproduces_expect_errors(make_oracle, case):
    """splitbrain's requests and replies folded by region: a round trip between two regions works
    exactly where expectErrors says it does (a reply needs both directions, so the one-way matrix is
    combined with its transpose)."""
    n = 12
    cpu = make_oracle(n)
    ok, art = wl.run_splitbrain(cpu, n, case)
    region = art["region"]
    gm = wl.GroupMatrix(region, 3).fold(drained=art["d_req"]).fold(drained=art["d_rep"])
    exp = wl.splitbrain_expected(n, case)
    assert (ok == exp).all()
    exp_regions = np.array([[exp[np.ix_(region == a, region == b)].any() for b in range(3)] for a in range(3)])
    one_way = wl.group_reachability(gm.m)
    assert one_way.shape == (3, 3) and one_way.dtype == bool
    assert (wl.group_reachability(gm.m, round_trip=True) == exp_regions).all()
    # one way, only region A's traffic towards region B is filtered
    want = np.ones((3, 3), dtype=bool)
    want[wl.REGION_A, wl.REGION_B] = case == "accept"
    assert (one_way == want).all()


def test_group_lines():
    m = np.zeros((2, 3, abi.GROUP_WORDS), dtype=np.uint64)
    m[0, 1, 0], m[0, 1, 1], m[0, 1, 2], m[0, 1, 10] = 3, 300, 3, 2
    m[1, 2, 0], m[1, 2, 9] = 1, 1
    got = metrics.group_lines(m, ["region a", "b"], "storm", "run 1", 42)
    assert got == [
        r"results.storm.group.offered,run=run\ 1,src_group=region\ a,dst_group=b value=3i 42",
        r"results.storm.group.offered,run=run\ 1,src_group=b,dst_group=external value=1i 42",
        r"results.storm.group.offered_bytes,run=run\ 1,src_group=region\ a,dst_group=b value=300i 42",
        r"results.storm.group.scheduled,run=run\ 1,src_group=region\ a,dst_group=b value=3i 42",
        r"results.storm.group.external,run=run\ 1,src_group=b,dst_group=external value=1i 42",
        r"results.storm.group.delivered,run=run\ 1,src_group=region\ a,dst_group=b value=2i 42",
    ]
    with pytest.raises(ValueError):
        metrics.group_lines(m, ["a"], "storm", "r", 0)
    assert len(abi.GROUP_NAMES) == abi.GROUP_WORDS == 14
