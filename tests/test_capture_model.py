"""The host model of the packet capture (workloads.capture_reference, merge_captures) and the pcap writer
(testground_amd/pcap.py), on the CPU: a hand case over the oracle with written-out records, the slicing by
owned range, and the pcap round trip.  tests/test_gpu_capture.py holds the device capture to this model."""
import io
import ipaddress

import numpy as np
import pytest

from testground_amd import abi
from testground_amd import network as nw
from testground_amd import pcap
from testground_amd import workloads as wl
from testground_amd.engine import EngineError, packets

MS = nw.Millisecond
NONE = abi.V_NONE << 4
FIELDS = ("t_ns", "src", "dst", "seq", "len", "flags", "verdict", "dir")


def tuples(recs):
    return [tuple(int(r[k]) for k in FIELDS) for r in recs]


def hand_windows(c):
    """Three peers: 0 -> 1 scheduled, 0 -> 2 blackholed by a rule of peer 0, 1 -> 0 with 100 % duplicate; a
    quiet window that delivers them; then peer 2 disconnected, whose own packet is refused.  Yields per
    window (start tick, packets, verdict bytes, drained records)."""
    ip2 = str(ipaddress.IPv4Address(wl.peer_ip(2)))
    c.configure(0, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=1 * MS),
                             Rules=[nw.LinkRule(Subnet=(ip2, 32), LinkShape=nw.LinkShape(Filter=nw.FilterAction.Drop))]))
    c.configure(1, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=2 * MS, Duplicate=100.0)))
    c.configure(2, nw.Config(Network="default", Enable=True, Default=nw.LinkShape(Latency=1 * MS)))
    steps = [(packets([(1, 0, 0, 300, 5), (0, 2, 1, 200, 20), (0, 1, 0, 100, 10)]), 1000),  # (submit order is not row order)
             (None, 4000),
             (packets([(2, 0, 0, 64, 7)]), 1000)]
    for w, (pk, ticks) in enumerate(steps):
        if w == 2:
            c.configure(2, nw.Config(Network="default", Enable=False))
        start = c.stats()["now_tick"]
        if pk is not None:
            c.submit(pk)
        c.step(ticks)
        yield start, pk, c.verdicts(), c.drain()


TX, RX = abi.CAPTURE_TX, abi.CAPTURE_RX
HAND = [  # per window: (tx, rx) as FIELDS tuples, watching all three peers
    ([(10_000, 0, 1, 0, 100, 0, NONE | abi.V_SCHEDULED, TX),
      (20_000, 0, 2, 1, 200, 0, NONE | abi.V_BLACKHOLE, TX),
      (5_000, 1, 0, 0, 300, 0, abi.V_SCHEDULED << 4 | abi.V_SCHEDULED, TX)],  # the clone: the high nibble, no record of its own
     []),
    ([],
     [(2_005_000, 1, 0, 0, 300, abi.FLAG_DUP, 0, RX),  # destination 0: the clone first
      (2_005_069, 1, 0, 0, 300, 0, 0, RX),
      (1_010_000, 0, 1, 0, 100, 0, 0, RX)]),          # then destination 1
    ([(5_007_000, 2, 0, 0, 64, 0, NONE | abi.V_DISCONNECTED, TX)],
     []),
]


def test_hand_case(make_oracle):
    c = make_oracle(3)
    n = 0
    for w, (start, pk, v, d) in enumerate(hand_windows(c)):
        tx, rx = wl.capture_reference([0, 1, 2], pk, v, d, start, c.tick_ns)
        assert tuples(tx) == HAND[w][0], (w, tuples(tx))
        assert tuples(rx) == HAND[w][1], (w, tuples(rx))
        assert tx.dtype == rx.dtype == abi.CAPTURE_DTYPE
        # a watch list of one peer is that peer's part
        tx1, rx1 = wl.capture_reference([1], pk, v, d, start, c.tick_ns)
        assert tuples(tx1) == [t for t in HAND[w][0] if t[1] == 1] and tuples(rx1) == [t for t in HAND[w][1] if t[2] == 1]
        n += 1
    assert n == len(HAND)
    st = c.stats()
    assert st["cloned"] == 1 and st["by_verdict"]["blackhole"] == 1 and st["by_verdict"]["disconnected"] == 1


def test_oracle_has_no_capture(make_oracle):
    with pytest.raises(EngineError) as ei:
        make_oracle(3).capture_init([0])
    assert ei.value.code == -38  # ENOSYS: the oracle's packets, verdicts and drain are the reference


def test_runner_refuses_capture_over_the_oracle(tmp_path, make_oracle):
    from testground_amd import runner as rn
    from testground_amd.sidecar import Context

    cfg = rn.LocalSimRunnerCfg(outputs_dir=str(tmp_path), engine_factory=make_oracle, capture=[0])
    job = rn.RunInput(RunID="nocap", TestPlan="network", TestCase="echo", TotalInstances=1,
                      Groups=[rn.RunGroup("single", 1, lambda env: None)], RunnerConfig=cfg)
    with pytest.raises(ValueError, match="no packet capture"):
        rn.LocalSimRunner().Run(Context(), job)
    assert rn.LocalSimRunnerCfg().capture == () and rn.LocalSimRunnerCfg().capture_cap == 1 << 20


def _storm_window(make_oracle, n=60):
    c = make_oracle(n)
    wl.configure_storm(c, n)
    out = []
    for _ in range(3):
        c.gen_storm(0.05, 1000)
        pk = np.zeros(1 << 16, dtype=abi.PKT_DTYPE)
        pk = pk[:c._lib.tgo_offered(c._h, pk.ctypes.data, len(pk))].copy()
        start = c.stats()["now_tick"]
        c.step(1000)
        out.append((start, pk, c.verdicts(), c.drain()))
    return c, out


def test_owned_slices_merge_to_the_whole(make_oracle):
    n, watched = 60, [0, 7, 19, 20, 21, 40, 59]
    c, windows = _storm_window(make_oracle, n)
    some_tx = some_rx = 0
    for start, pk, v, d in windows:
        whole = wl.capture_reference(watched, pk, v, d, start, c.tick_ns, generated=True)
        assert len(whole[0]) == int(np.isin(pk["src"], watched).sum()) and len(whole[1]) == int(np.isin(d["dst"], watched).sum())
        for bounds in ([0, 20, 60], [0, 8, 21, 60]):
            parts = [wl.capture_reference(watched, pk, v, d, start, c.tick_ns, owned=(lo, hi), generated=True)
                     for lo, hi in zip(bounds, bounds[1:])]
            m = wl.merge_captures([{"tx": t, "rx": r} for t, r in parts])
            assert m["tx"].tobytes() == whole[0].tobytes() and m["rx"].tobytes() == whole[1].tobytes(), bounds
        # the order contract: sources ascending, each row in the offered order; destinations ascending, drain order
        assert (np.diff(whole[0]["src"].astype(np.int64)) >= 0).all() and (np.diff(whole[1]["dst"].astype(np.int64)) >= 0).all()
        some_tx += len(whole[0])
        some_rx += len(whole[1])
    assert some_tx > 0 and some_rx > 0


def test_pcap_round_trip(make_oracle):
    c = make_oracle(3)
    recs = []
    for start, pk, v, d in hand_windows(c):
        recs.extend(wl.capture_reference([0, 1, 2], pk, v, d, start, c.tick_ns))
    recs = np.concatenate(recs)
    assert len(recs) == 7
    for refused, want in ((False, 5), (True, 7)):  # the blackholed and the disconnected TX never left their senders
        buf = io.BytesIO()
        assert pcap.write_pcap(buf, recs, refused=refused) == want
        raw = buf.getvalue()
        assert raw[:4] == (0xA1B23C4D).to_bytes(4, "little") and int.from_bytes(raw[20:24], "little") == 101
        assert int.from_bytes(raw[16:20], "little") == 28
        got = pcap.read_pcap(io.BytesIO(raw))
        assert len(got) == want
        keep = recs if refused else recs[(recs["dir"] == RX) | ((recs["verdict"] & 15) == abi.V_SCHEDULED)]
        keep = keep[np.lexsort((keep["seq"], keep["src"], keep["dir"], keep["t_ns"]))]
        assert [p["t_ns"] for p in got] == [int(t) for t in keep["t_ns"]] == sorted(int(t) for t in keep["t_ns"])
        assert 2_005_069 in [p["t_ns"] for p in got]  # nanoseconds survive
        for p, r in zip(got, keep):
            assert p["src_ip"] == wl.peer_ip(int(r["src"])) and p["dst_ip"] == wl.peer_ip(int(r["dst"]))
            assert p["total_len"] == p["orig_len"] == int(r["len"]) and p["incl_len"] == 28
            assert p["checksum_ok"] and p["proto"] == 17 and p["udp_len"] == int(r["len"]) - 20
    # a datagram shorter than the headers: what there is of them
    short = np.zeros(1, dtype=abi.CAPTURE_DTYPE)
    short["len"], short["dir"], short["src"], short["dst"] = 20, RX, 1, 2
    buf = io.BytesIO()
    pcap.write_pcap(buf, short)
    (p,) = pcap.read_pcap(io.BytesIO(buf.getvalue()))
    assert p["incl_len"] == 20 and p["orig_len"] == 20 and p["checksum_ok"] and "udp_len" not in p
