"""Synthetic equivalents of the reference's network workloads (SURVEY §8(d) C1–C3).

Each driver talks to an engine-shaped object (``Engine`` or any ``CABIEngine``), so the same
driver runs the HIP engine on the GPU and, in the tests, the CPU oracle with identical inputs.

  C1 pingpong    plans/network/pingpong.go:16-201 (RTT windows :185, :195)
  C2 splitbrain  plans/splitbrain/main.go:60-186 (expectErrors :50-58)
  C3 storm       plans/benchmarks/storm.go:31-197, random all-to-all with heterogeneous shapes
  C4 gossip      SURVEY §8(d): 1M-peer flood, degree 8, 1 KiB messages, L~U[5,50] ms, loss 1 %
  C5 epochs      SURVEY §8(d): C3 traffic, mid-run reshaping of 10 % of peers per epoch, barriers

A reaction to a delivery at time d (reply, echo, forward) is offered at tick floor(d/tick) + 1.
"""
from __future__ import annotations

import errno
import ipaddress
from typing import Dict, List, Tuple

import numpy as np

from . import abi
from .engine import EngineError
from .network import Config, FilterAction, LinkRule, LinkShape, Millisecond, RoutingPolicyType, configs_array

SEED = 0x7E576A0D00000001


# ---------------------------------------------------------------------------------------------
# C3: storm — heterogeneous LinkShape per instance.
def storm_shape_arrays(n_peers: int, seed: int = SEED) -> Dict[str, np.ndarray]:
    """L~U[1,100] ms, J~U[0,10] ms, Loss~U[0,5] %, Dup/Corrupt/Reorder~U[0,1] %,
    Bw in {1,10,100,1000} Mbit/s, correlations 0."""
    rng = np.random.default_rng(seed & 0xFFFFFFFF)
    lat = rng.integers(1 * Millisecond, 100 * Millisecond + 1, n_peers)
    jit = rng.integers(0, 10 * Millisecond + 1, n_peers)
    loss = rng.uniform(0, 5, n_peers).astype(np.float32)
    dup = rng.uniform(0, 1, n_peers).astype(np.float32)
    cor = rng.uniform(0, 1, n_peers).astype(np.float32)
    reo = rng.uniform(0, 1, n_peers).astype(np.float32)
    bw = rng.choice(np.array([1, 10, 100, 1000], dtype=np.int64) * 1_000_000, n_peers)
    return dict(latency_ns=lat, jitter_ns=jit, bandwidth_bps=bw, loss=loss, duplicate=dup, corrupt=cor,
                reorder=reo)


def storm_shapes(n_peers: int, seed: int = SEED) -> List[LinkShape]:
    a = storm_shape_arrays(n_peers, seed)
    return [LinkShape(Latency=int(a["latency_ns"][i]), Jitter=int(a["jitter_ns"][i]),
                      Bandwidth=int(a["bandwidth_bps"][i]), Loss=float(a["loss"][i]),
                      Duplicate=float(a["duplicate"][i]), Corrupt=float(a["corrupt"][i]),
                      Reorder=float(a["reorder"][i]))
            for i in range(n_peers)]


def storm_configs(n_peers: int, seed: int = SEED, open_links: bool = False) -> np.ndarray:
    """The storm shapes as tgsim_config records (RoutingPolicy DenyAll), for configure_batch.
    open_links: the sub-capacity variant, every link at 1 Gbit/s (latency, jitter, loss, dup,
    corrupt, reorder unchanged), driven at STORM_OPEN_LAMBDA so no netem queue reaches its limit."""
    a = storm_shape_arrays(n_peers, seed)
    if open_links:
        a["bandwidth_bps"] = np.full(n_peers, 1_000_000_000, dtype=np.int64)
    return configs_array(routing_policy=2, **a)


# Sub-capacity C3: 0.008 packets per us per source of U[64,1500] B is ~50 Mbit/s offered against
# 1 Gbit/s, and the netem queue holds lambda * (L + J) <= 0.008 * 110,000 us = 880 items at the very
# worst shape (~440 on average) against the limit of 1,000: the delay, HTB and delivery path is
# exercised, not the full-queue ballot.
STORM_OPEN_LAMBDA = 0.008


def configure_storm(eng, n_peers: int, seed: int = SEED, open_links: bool = False) -> None:
    eng.configure_batch(np.arange(n_peers), storm_configs(n_peers, seed, open_links))


# ---------------------------------------------------------------------------------------------
# C2: splitbrain.
REGION_A, REGION_B, REGION_C = 0, 1, 2


def splitbrain_regions(n: int) -> np.ndarray:
    """seq = i + 1 (SignalEntry is 1-based), region = seq % 3 (splitbrain/main.go:84-87)."""
    return (np.arange(n) + 1) % 3


def expect_errors(case: str, ra: int, rb: int) -> bool:
    """splitbrain/main.go:50-58."""
    if case == "accept" or ra == REGION_C or rb == REGION_C:
        return False
    return (ra == REGION_A and rb == REGION_B) or (ra == REGION_B and rb == REGION_A)


def peer_ip(i: int, subnet_base: int = 16 << 24) -> int:
    return subnet_base + 2 + i


def configure_splitbrain(eng, n: int, case: str) -> np.ndarray:
    action = {"drop": FilterAction.Drop, "reject": FilterAction.Reject, "accept": FilterAction.Accept}[case]
    region = splitbrain_regions(n)
    b_peers = np.nonzero(region == REGION_B)[0]
    for i in np.nonzero(region == REGION_A)[0]:
        rules = [LinkRule(Subnet=(str(ipaddress.IPv4Address(peer_ip(int(p)))), 32),
                          LinkShape=LinkShape(Filter=action)) for p in b_peers]
        eng.configure(int(i), Config(Network="default", Enable=True, Rules=rules,
                                     CallbackState=f"reconfigured{i}", CallbackTarget=1))
    return region


def run_splitbrain(eng, n: int, case: str, pkt_len: int = 66, gap: int = 8) -> Tuple[np.ndarray, Dict]:
    """Every instance contacts every other instance once, sequentially (one request every `gap`
    ticks, as the plan's `for _, p := range nodes { httpclient.Get(...) }`, main.go:159-175), and
    every delivered request is answered.  Replies run in a second window on the same relative time
    axis (reply tick = floor(d / tick) + 1).  Returns ok[i, j] = request i->j and its reply j->i
    both delivered, plus the step artifacts."""
    region = configure_splitbrain(eng, n, case)
    src, dst = np.nonzero(~np.eye(n, dtype=bool))
    k = dst - (dst > src)  # per-source request index 0..n-2
    req = np.zeros(len(src), dtype=abi.PKT_DTYPE)
    req["src"], req["dst"], req["len"] = src, dst, pkt_len
    req["seq"], req["tick"] = k, k * gap
    span = (n - 1) * gap
    t0 = eng.stats()["now_tick"]
    eng.submit(req)
    eng.step(span)
    v_req = eng.verdicts()
    d_req = eng.drain()
    tick = eng.tick_ns
    rep = np.zeros(len(d_req), dtype=abi.PKT_DTYPE)
    rep["src"], rep["dst"], rep["len"] = d_req["dst"], d_req["src"], pkt_len
    rep["seq"] = (n - 1) + d_req["src"]  # fresh per-source sequence numbers
    rep["tick"] = (d_req["t_ns"] // tick + 1) - t0
    eng.submit(rep)
    eng.step(span + 2)
    v_rep = eng.verdicts()
    d_rep = eng.drain()
    ok = np.zeros((n, n), dtype=bool)
    ok[d_rep["dst"], d_rep["src"]] = True  # reply j->i delivered to i => i->j round trip ok
    return ok, {"region": region, "v_req": v_req, "d_req": d_req, "v_rep": v_rep, "d_rep": d_rep}


def splitbrain_expected(n: int, case: str) -> np.ndarray:
    region = splitbrain_regions(n)
    exp = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for j in range(n):
            if i != j:
                exp[i, j] = not expect_errors(case, int(region[i]), int(region[j]))
    return exp


# ---------------------------------------------------------------------------------------------
# C1: ping-pong (2 instances).
def pingpong_config(latency_ns: int, callback: str = "network-configured", ipv4=None) -> Config:
    """pingpong.go:29-42 (and :61-65 for the re-addressing)."""
    return Config(Network="default", Enable=True, IPv4=ipv4,
                  Default=LinkShape(Latency=latency_ns, Bandwidth=1 << 20),
                  CallbackState=callback, RoutingPolicy=RoutingPolicyType.DenyAll)


def pingpong_round(eng, start_tick: int, seq0: int, pkt_len: int = 66, chunk: int = 1000,
                   max_ticks: int = 2_000_000) -> Tuple[List[int], int]:
    """One pingPong() exchange (pingpong.go:116-183): both sides write their id at start_tick,
    echo the other's id on receipt, and stop when their own id comes back.  The engine must have
    lookahead >= chunk ticks.  Returns (rtt_ns per instance, next free tick)."""
    tick = eng.tick_ns
    now = eng.stats()["now_tick"]
    assert now <= start_tick
    if start_tick > now:
        eng.step(start_tick - now)
        eng.drain()
        now = start_tick
    pending: List[tuple] = [(0, 1, seq0, pkt_len, 0), (1, 0, seq0, pkt_len, 0)]  # (src,dst,seq,len,abs tick)
    pending = [(s, d, q, l, start_tick) for (s, d, q, l, _) in pending]
    rtt = [None, None]
    while None in rtt and now - start_tick < max_ticks:
        window = [p for p in pending if now <= p[4] < now + chunk]
        pending = [p for p in pending if p[4] >= now + chunk]
        if window:
            arr = np.array([(s, d, q, l, t - now) for (s, d, q, l, t) in window], dtype=abi.PKT_DTYPE)
            eng.submit(arr)
        eng.step(chunk)
        now += chunk
        for r in eng.drain():
            dst, src, t = int(r["dst"]), int(r["src"]), int(r["t_ns"])
            react = t // tick + 1
            if int(r["seq"]) == seq0:  # the other's id arrived: echo it back
                pending.append((dst, src, seq0 + 1 + dst, pkt_len, react))
            elif rtt[dst] is None:  # own id came back
                rtt[dst] = t - start_tick * tick
    return rtt, now


# ---------------------------------------------------------------------------------------------
# Ping mesh: C1, C2 and plans/verify as one closed loop.  The HIP engine runs it on the device
# (tgsim_ping_init / tgsim_gen_ping, include/tgsim.h); PingModel is the same loop driven from the
# host over any engine-shaped object, the model the device loop is compared with.
def ping_targets_all(n: int) -> np.ndarray:
    """[n, n - 1]: every peer probes every other peer, slot k of peer s -> k + (k >= s)."""
    k = np.arange(n - 1, dtype=np.uint32)[None, :]
    s = np.arange(n, dtype=np.uint32)[:, None]
    return (k + (k >= s)).astype(np.uint32)


def ping_targets_mesh(n: int, fanout: int, seed: int = SEED) -> np.ndarray:
    """[n, fanout]: `fanout` distinct random peers other than the peer itself, per peer."""
    if not 1 <= fanout <= n - 1:
        raise ValueError("ping_targets_mesh: fanout must be in 1..n-1")
    rng = np.random.default_rng(seed & 0xFFFFFFFF)
    off = rng.integers(1, n, (n, fanout))  # target = (s + off) mod n, off in 1..n-1
    while True:
        srt = np.sort(off, axis=1)
        rows = np.nonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[0]
        if not len(rows):
            break
        off[rows] = rng.integers(1, n, (len(rows), fanout))
    return ((np.arange(n)[:, None] + off) % n).astype(np.uint32)


def ping_probes_before(ping: Dict, tick: int) -> int:
    """Probes per slot whose tick start + j * interval precedes `tick`."""
    if tick <= ping["start_tick"]:
        return 0
    return min(ping["count"], (tick - ping["start_tick"] - 1) // ping["interval_ticks"] + 1)


class PingLate(ValueError):
    """A reply's tick precedes the window being generated (the engine's -EINVAL)."""


class PingModel:
    """The ping loop of include/tgsim.h driven from the host: submit / step / verdicts / drain per
    window.  `ping` holds Engine.ping_init's keywords (count, interval_ticks, length, start_tick and,
    optionally, bin_ns, n_bins)."""

    def __init__(self, eng, ping: Dict, targets: np.ndarray):
        self.eng = eng
        self.ping = dict(bin_ns=0, n_bins=0, **{k: v for k, v in ping.items() if k not in ("bin_ns", "n_bins")})
        self.ping.update({k: ping[k] for k in ("bin_ns", "n_bins") if k in ping})
        self.targets = np.ascontiguousarray(targets, dtype=np.uint32)
        self.n, self.fanout = self.targets.shape
        self.now = eng.stats()["now_tick"]
        self.tick_ns = eng.tick_ns
        self.src, self.slot = np.nonzero(self.targets != abi.PING_NONE)  # row-major: (s, k) ascending
        self.dst = self.targets[self.src, self.slot]
        self.cal = np.zeros((0, 4), dtype=np.int64)  # tick, responder, requester, seq
        self.received = np.zeros(self.n * self.fanout, dtype=np.uint32)
        self.sum_ns = np.zeros(self.n * self.fanout, dtype=np.uint64)
        self.min_ns = np.full(self.n * self.fanout, np.iinfo(np.uint64).max, dtype=np.uint64)
        self.max_ns = np.zeros(self.n * self.fanout, dtype=np.uint64)
        self.hist = np.zeros(self.ping["n_bins"], dtype=np.uint64)
        self.dup_ignored = self.corrupt_ignored = 0
        # what the run exercised (the tests' conditions): the most windows ahead a calendar entry has been
        # due, the longest row, rows with equal (tick, seq), clones ignored per leg
        self.carried_max = self.max_row = self.ties = self.dup_requests = self.dup_replies = 0
        self.tie_sources: set = set()  # sources that offered two packets with equal (tick, seq)
        self.windows = 0

    def window_packets(self, window: int) -> np.ndarray:
        """The window's offered packets in (src, tick, seq, dst) order; the due entries leave the calendar."""
        p, win0, win1 = self.ping, self.now, self.now + window
        if win1 >= 1 << 31:  # the engine's -EOVERFLOW: ticks of the schedule and the calendar stay below 2^31
            raise EngineError(-errno.EOVERFLOW, "ping: the window ends beyond tick 2^31")
        j = np.arange(ping_probes_before(p, win0), ping_probes_before(p, win1), dtype=np.int64)
        src = np.tile(self.src, len(j))
        dst = np.tile(self.dst, len(j))
        seq = (j[:, None] * self.fanout + self.slot[None, :]).ravel()
        tick = np.repeat(p["start_tick"] + j * p["interval_ticks"], len(self.src))
        if len(self.cal) and self.cal[:, 0].min() < win0:
            raise PingLate(f"ping: a reply due at tick {int(self.cal[:, 0].min())} precedes the window at tick {win0}")
        due = self.cal[:, 0] < win1
        rep, self.cal = self.cal[due], self.cal[~due]
        src = np.concatenate([src, rep[:, 1]])
        dst = np.concatenate([dst.astype(np.int64), rep[:, 2]])
        seq = np.concatenate([seq, rep[:, 3] | 0x80000000])
        tick = np.concatenate([tick, rep[:, 0]])
        order = np.lexsort((dst, seq, tick, src))
        if len(order):
            s_, t_, q_ = src[order], tick[order], seq[order]
            self.max_row = max(self.max_row, int(np.bincount(s_).max()))
            tie = (s_[1:] == s_[:-1]) & (t_[1:] == t_[:-1]) & (q_[1:] == q_[:-1])
            self.ties += int(tie.sum())
            self.tie_sources.update(np.unique(s_[1:][tie]).tolist())
        pk = np.zeros(len(order), dtype=abi.PKT_DTYPE)
        pk["src"], pk["dst"], pk["seq"] = src[order], dst[order], seq[order]
        pk["len"], pk["tick"] = p["length"], tick[order] - win0
        return pk

    def receive(self, d: np.ndarray) -> None:
        """Folds one window's drained records: requests into the calendar, replies into the pairs."""
        p = self.ping
        flags = d["flags"]
        dup = (flags & abi.FLAG_DUP) != 0
        cor = ~dup & ((flags & abi.FLAG_CORRUPT) != 0)
        self.dup_ignored += int(dup.sum())
        self.dup_replies += int((dup & ((d["seq"] >> 31) != 0)).sum())
        self.dup_requests += int((dup & ((d["seq"] >> 31) == 0)).sum())
        self.corrupt_ignored += int(cor.sum())
        d = d[~dup & ~cor]
        seq = d["seq"].astype(np.int64)
        q = seq & 0x7FFFFFFF
        k, j = q % self.fanout, q // self.fanout
        src, dst = d["src"].astype(np.int64), d["dst"].astype(np.int64)
        is_rep = (seq >> 31) != 0
        tgt = self.targets.astype(np.int64)
        req = ~is_rep & (q < p["count"] * self.fanout) & (src < self.n)
        req[req] = tgt[src[req], k[req]] == dst[req]
        new = np.stack([d["t_ns"][req].astype(np.int64) // self.tick_ns + 1, dst[req], src[req], seq[req]], axis=1)
        self.cal = np.concatenate([self.cal, new.reshape(-1, 4)])
        t0 = (p["start_tick"] + j * p["interval_ticks"]) * self.tick_ns
        t = d["t_ns"].astype(np.int64)
        rep = is_rep & (j < p["count"]) & (dst < self.n)
        rep[rep] = (tgt[dst[rep], k[rep]] == src[rep]) & (t[rep] >= t0[rep])
        idx = dst[rep] * self.fanout + k[rep]
        rtt = (t[rep] - t0[rep]).astype(np.uint64)
        np.add.at(self.received, idx, 1)
        np.add.at(self.sum_ns, idx, rtt)
        np.minimum.at(self.min_ns, idx, rtt)
        np.maximum.at(self.max_ns, idx, rtt)
        if p["n_bins"]:
            np.add.at(self.hist, np.minimum(rtt // np.uint64(p["bin_ns"]), np.uint64(p["n_bins"] - 1)).astype(np.int64), 1)

    def step(self, window: int) -> Tuple[np.ndarray, np.ndarray]:
        pk = self.window_packets(window)
        if len(pk):
            self.eng.submit(pk)
        self.eng.step(window)
        self.now += window
        v, d = self.eng.verdicts(), self.eng.drain()
        self.receive(d)
        self.windows += 1
        if len(self.cal):  # 1: due in the next window; 2 and more: moved to the other calendar buffer first
            self.carried_max = max(self.carried_max, int((self.cal[:, 0].max() - self.now) // window) + 1)
        return v, d

    def pairs(self) -> np.ndarray:
        out = np.zeros((self.n, self.fanout), dtype=abi.PING_PAIR_DTYPE)
        out["sent"] = np.where(self.targets != abi.PING_NONE, ping_probes_before(self.ping, self.now), 0)
        for key in ("received", "sum_ns", "min_ns", "max_ns"):
            out[key] = getattr(self, key).reshape(self.n, self.fanout)
        return out

    def report(self) -> Dict:
        pr = self.pairs()[self.targets != abi.PING_NONE]
        got = pr["received"] > 0
        sent = pr["sent"] > 0
        return {"pairs": len(pr), "sent": int(pr["sent"].sum(dtype=np.uint64)),
                "received": int(pr["received"].sum(dtype=np.uint64)), "sum_ns": int(pr["sum_ns"].sum(dtype=np.uint64)),
                "min_ns": int(pr["min_ns"][got].min()) if got.any() else int(np.iinfo(np.uint64).max),
                "max_ns": int(pr["max_ns"].max()) if len(pr) else 0,
                "pairs_all": int((sent & (pr["received"] == pr["sent"])).sum()),
                "pairs_none": int((sent & ~got).sum()),
                "dup_ignored": self.dup_ignored, "corrupt_ignored": self.corrupt_ignored,
                "pending_replies": len(self.cal), "hist": self.hist.copy()}


def ping_reference(eng, ping: Dict, targets: np.ndarray, n_windows: int, window: int, probe_at=(), before=None) -> Dict:
    """The ping loop driven from the host over `eng` (submit / step / verdicts / drain): per-window
    (verdicts, deliveries) under "windows", the final "pairs", "summary" (report fields and hist),
    and under "probes" the (pairs, summary) after each window index in probe_at.  before(w) runs
    ahead of window w (a reshape, a disconnect).  The model itself is under "model"."""
    m = PingModel(eng, ping, targets)
    out = {"windows": [], "probes": {}, "model": m}
    for w in range(n_windows):
        if before is not None:
            before(w)
        out["windows"].append(m.step(window))
        if w in probe_at:
            out["probes"][w] = (m.pairs(), m.report())
    out["pairs"], out["summary"] = m.pairs(), m.report()
    out["hist"] = out["summary"]["hist"]
    return out


def ping_run(eng, n_windows: int, window: int, collect: bool = False, probe_at=(), before=None, step=None) -> Dict:
    """The device loop on an armed engine (Engine.ping_init): n_windows of gen_ping + step.  Nothing
    reaches the host unless asked for: collect keeps each window's (verdicts, deliveries), probe_at
    the (pairs, report) after those windows.  step(window) replaces eng.step (a shard of a run armed
    with sharded=True: eng.comm_step)."""
    step = eng.step if step is None else step
    out = {"windows": [], "probes": {}}
    for w in range(n_windows):
        if before is not None:
            before(w)
        eng.gen_ping(window)
        step(window)
        if collect:
            out["windows"].append((eng.verdicts(), eng.drain()))
        if w in probe_at:
            out["probes"][w] = (eng.ping_pairs(), eng.ping_report())
    return out


def merge_ping_reports(reports) -> Dict:
    """The shards' ping reports (Engine.ping_report of every rank) as the whole run's, by the merge
    rule of include/tgsim.h: every field by sum, except min_ns by min and max_ns by max; hist by sum.
    For hosts with their own exchange; Engine.comm_ping_report does the same on the device."""
    reports = list(reports)
    if not reports:
        raise ValueError("merge_ping_reports: no report")
    out = {}
    for key in abi.PING_SUMMARY_FIELDS:
        vals = [int(r[key]) for r in reports]
        out[key] = min(vals) if key == "min_ns" else max(vals) if key == "max_ns" else sum(vals)
    hists = [np.asarray(r["hist"], dtype=np.uint64) for r in reports]
    if len({len(h) for h in hists}) != 1:
        raise ValueError("merge_ping_reports: the reports' histograms differ in length")
    out["hist"] = np.sum(hists, axis=0, dtype=np.uint64)
    return out


# ---------------------------------------------------------------------------------------------
# Reliable transfers: windowed flows with a selective ACK and a retransmission timer per segment
# (tgsim_flow_init / tgsim_gen_flow, include/tgsim.h; not TCP).  The HIP engine runs the loop on the
# device; FlowModel is the same loop driven from the host over any engine-shaped object, in plain
# Python and numpy: the rules of the header and nothing cleverer.
def flow_table_mesh(n: int, per_source: int, n_seg, seed: int = SEED, start_tick: int = 0) -> np.ndarray:
    """The sorted flow table of a mesh: every peer sends `per_source` flows to distinct random peers
    other than itself; n_seg is one number or an array [n * per_source]."""
    t = np.zeros(n * per_source, dtype=abi.FLOW_SPEC_DTYPE)
    t["src"] = np.repeat(np.arange(n, dtype=np.uint32), per_source)
    t["dst"] = ping_targets_mesh(n, per_source, seed).ravel()
    t["n_seg"] = n_seg
    t["start_tick"] = start_tick
    return t


class FlowLate(ValueError):
    """An ACK's or a released segment's tick precedes the window being generated (the engine's -EINVAL)."""


class FlowModel:
    """The flow loop of include/tgsim.h driven from the host: submit / step / verdicts / drain per
    window.  `flow` holds Engine.flow_init's keywords (seg_len, ack_len, window, rto_ticks,
    max_attempts and, optionally, bin_ns, n_bins)."""

    def __init__(self, eng, flow: Dict, flows: np.ndarray):
        self.eng = eng
        self.flow = dict(dict(bin_ns=0, n_bins=0), **flow)
        p = self.flow
        if not (1 <= p["window"] <= 64 and 1 <= p["max_attempts"] <= 16 and p["rto_ticks"] >= 1):
            raise ValueError("flow: window 1..64, max_attempts 1..16, rto_ticks >= 1")
        self.spec = np.ascontiguousarray(flows, dtype=abi.FLOW_SPEC_DTYPE)
        src = self.spec["src"].astype(np.int64)
        if (np.diff(src) < 0).any():
            raise ValueError("flow: the table is not sorted by src")
        self.n = eng.n_peers
        self.cnt = np.bincount(src, minlength=self.n)
        if (self.cnt > abi.FLOW_SLOTS).any():
            raise ValueError(f"flow: more than {abi.FLOW_SLOTS} flows of source {int(np.argmax(self.cnt))}")
        self.first = np.concatenate([[0], np.cumsum(self.cnt)[:-1]])
        self.slot = np.arange(len(src)) - self.first[src]
        self.now = eng.stats()["now_tick"]
        self.tick_ns = eng.tick_ns
        nf, w = len(src), p["window"]
        self.state = np.zeros(nf, dtype=np.int64)
        self.base = np.zeros(nf, dtype=np.int64)
        self.acked_segs = [set() for _ in range(nf)]  # acknowledged segments at or above base
        self.due = np.repeat(self.spec["start_tick"].astype(np.int64)[:, None], w, axis=1)  # ring: seg % window
        self.att = np.zeros((nf, w), dtype=np.int64)
        self.acked = np.zeros(nf, dtype=np.int64)
        self.offered = np.zeros(nf, dtype=np.int64)
        self.retransmits = np.zeros(nf, dtype=np.int64)
        self.stale = np.zeros(nf, dtype=np.int64)
        self.done_ns = np.zeros(nf, dtype=np.int64)
        self.cal = np.zeros((0, 4), dtype=np.int64)  # tick, responder, requester, data seq
        self.hist = np.zeros(p["n_bins"], dtype=np.uint64)
        self.dup_ignored = self.corrupt_ignored = 0
        # what the run exercised (the tests' conditions): the largest attempt offered, the longest row,
        # the most windows ahead a calendar entry has been due, segments released onto a wrapped ring,
        # sources that offered two packets with equal (tick, seq)
        # (max_ack_row: the most ACKs one receiver offered in a window)
        self.max_attempt = self.max_row = self.max_ack_row = self.carried_max = self.ring_wraps = self.ties = 0
        self.tie_sources: set = set()
        self.windows = 0

    def _next(self, f: int) -> int:
        return min(self.base[f] + self.flow["window"], int(self.spec["n_seg"][f]))

    def _unacked(self, f: int):
        return [i for i in range(int(self.base[f]), self._next(f)) if i not in self.acked_segs[f]]

    # The three places the RTT estimator (FlowRtoMixin) changes: the longest window, a segment's timer
    # when it is offered at tick t with attempt count k, and a non-stale ACK ahead of anything else.
    def _window_limit(self) -> Tuple[str, int]:
        return "rto_ticks", self.flow["rto_ticks"]

    def _timer(self, f: int, i: int, k: int, t: int) -> int:
        return self.flow["rto_ticks"]

    def _non_stale_ack(self, f: int, seg: int, seq: int, tick: int) -> None:
        pass

    # The verdict feedback (FlowFbMixin): a simulated window's packets and verdict bytes, ahead of its records.
    def _verdicts(self, pk: np.ndarray, v: np.ndarray, win0: int) -> None:
        pass

    def window_packets(self, window: int) -> np.ndarray:
        """The window's offered packets in (src, tick, seq, dst) order: the segments due in it, and the
        calendar's ACKs due in it, which leave the calendar."""
        p, win0, win1 = self.flow, self.now, self.now + window
        if win1 >= 1 << 31:  # the engine's -EOVERFLOW: ticks of the timers and the calendar stay below 2^31
            raise EngineError(-errno.EOVERFLOW, "flow: the window ends beyond tick 2^31")
        name, longest = self._window_limit()
        if window > longest:
            raise ValueError(f"flow: a window of {window} ticks is longer than {name} {longest}")
        w = p["window"]
        live = np.nonzero(self.state == abi.FLOW_ACTIVE)[0]
        late = [int(self.cal[:, 0].min())] if len(self.cal) else []
        late += [int(self.due[f, i % w]) for f in live for i in self._unacked(f)]
        if late and min(late) < win0:  # nothing is generated, no state changes
            raise FlowLate(f"flow: a receipt due at tick {min(late)} precedes the window at tick {win0}")
        rows = []  # src, dst, seq, tick, len
        for f in live:
            segs = self._unacked(f)
            fail = [int(self.due[f, i % w]) for i in segs if self.due[f, i % w] < win1 and self.att[f, i % w] >= p["max_attempts"]]
            fail_tick = min(fail) if fail else None
            for i in segs:
                t, k = int(self.due[f, i % w]), int(self.att[f, i % w])
                if t >= win1 or (fail_tick is not None and t >= fail_tick):
                    continue
                rows.append((int(self.spec["src"][f]), int(self.spec["dst"][f]),
                             k << abi.FLOW_ATTEMPT_SHIFT | int(self.slot[f]) << abi.FLOW_SLOT_SHIFT | i, t, p["seg_len"]))
                self.due[f, i % w] = t + self._timer(f, i, k, t)
                self.att[f, i % w] = k + 1
                self.offered[f] += 1
                self.retransmits[f] += k > 0
                self.max_attempt = max(self.max_attempt, k)
            if fail_tick is not None:
                self.state[f] = abi.FLOW_FAILED
                self.done_ns[f] = fail_tick * self.tick_ns
        due = self.cal[:, 0] < win1
        ack, self.cal = self.cal[due], self.cal[~due]
        rows += [(int(r), int(q), int(s) | abi.FLOW_ACK, int(t), p["ack_len"]) for t, r, q, s in ack]
        a = np.array(rows, dtype=np.int64).reshape(-1, 5)
        a = a[np.lexsort((a[:, 1], a[:, 2], a[:, 3], a[:, 0]))]
        if len(a):
            self.max_row = max(self.max_row, int(np.bincount(a[:, 0]).max()))
            if len(ack):
                self.max_ack_row = max(self.max_ack_row, int(np.bincount(ack[:, 1]).max()))
            tie = (a[1:, 0] == a[:-1, 0]) & (a[1:, 3] == a[:-1, 3]) & (a[1:, 2] == a[:-1, 2])
            self.ties += int(tie.sum())
            self.tie_sources.update(np.unique(a[1:, 0][tie]).tolist())
        pk = np.zeros(len(a), dtype=abi.PKT_DTYPE)
        pk["src"], pk["dst"], pk["seq"], pk["tick"], pk["len"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3] - win0, a[:, 4]
        return pk

    def _flow_of(self, sender: int, seq: int, peer: int):
        """The flow of `sender` that seq names, when its dst is `peer` and the segment exists; else None."""
        slot, seg = seq >> abi.FLOW_SLOT_SHIFT & 15, seq & abi.FLOW_SEG_MASK
        if sender >= self.n or slot >= self.cnt[sender]:
            return None
        f = int(self.first[sender] + slot)
        if int(self.spec["dst"][f]) != peer or seg >= int(self.spec["n_seg"][f]):
            return None
        return f

    def receive(self, d: np.ndarray) -> None:
        """Folds one window's drained records, in drain order (dst, t_ns, src, seq): data segments into
        the ACK calendar, ACKs into their flows."""
        p, w = self.flow, self.flow["window"]
        new = []
        for flags, seq, t_ns, src, dst in zip(*(d[k].tolist() for k in ("flags", "seq", "t_ns", "src", "dst"))):
            if flags & abi.FLAG_DUP:
                self.dup_ignored += 1
                continue
            if flags & abi.FLAG_CORRUPT:
                self.corrupt_ignored += 1
                continue
            tick = t_ns // self.tick_ns + 1
            if not seq & abi.FLOW_ACK:
                if self._flow_of(src, seq, dst) is not None:
                    new.append((tick, dst, src, seq))
                continue
            f = self._flow_of(dst, seq, src)
            if f is None:
                continue
            seg, n_seg = seq & abi.FLOW_SEG_MASK, int(self.spec["n_seg"][f])
            nxt = self._next(f)
            if self.state[f] != abi.FLOW_ACTIVE or seg < self.base[f] or seg >= nxt or seg in self.acked_segs[f]:
                self.stale[f] += 1
                continue
            self._non_stale_ack(f, seg, seq, tick)
            self.acked_segs[f].add(seg)
            self.acked[f] += 1
            while int(self.base[f]) in self.acked_segs[f]:
                self.acked_segs[f].discard(int(self.base[f]))
                self.base[f] += 1
            for i in range(nxt, self._next(f)):  # the segments that entered the window
                self.due[f, i % w], self.att[f, i % w] = tick, 0
                self.ring_wraps += i >= w
            if self.base[f] == n_seg:
                self.state[f] = abi.FLOW_DONE
                self.done_ns[f] = t_ns
                if p["n_bins"]:
                    fct = t_ns - int(self.spec["start_tick"][f]) * self.tick_ns
                    self.hist[min(fct // p["bin_ns"], p["n_bins"] - 1)] += 1
        self.cal = np.concatenate([self.cal, np.array(new, dtype=np.int64).reshape(-1, 4)])

    def step(self, window: int) -> Tuple[np.ndarray, np.ndarray]:
        pk = self.window_packets(window)
        if len(pk):
            self.eng.submit(pk)
        self.eng.step(window)
        self.now += window
        v, d = self.eng.verdicts(), self.eng.drain()
        self._verdicts(pk, v, self.now - window)
        self.receive(d)
        self.windows += 1
        if len(self.cal):  # 1: due in the next window; 2 and more: moved to the other calendar buffer first
            self.carried_max = max(self.carried_max, int((self.cal[:, 0].max() - self.now) // window) + 1)
        return v, d

    def rows(self) -> np.ndarray:
        out = np.zeros(len(self.spec), dtype=abi.FLOW_ROW_DTYPE)
        for key, v in (("state", self.state), ("acked", self.acked), ("offered", self.offered),
                       ("retransmits", self.retransmits), ("stale_acks", self.stale), ("base", self.base),
                       ("done_ns", self.done_ns)):
            out[key] = v
        return out

    def fct(self) -> np.ndarray:
        """Flow completion times of the DONE flows, ns."""
        done = self.state == abi.FLOW_DONE
        return self.done_ns[done] - self.spec["start_tick"][done].astype(np.int64) * self.tick_ns

    def report(self) -> Dict:
        fct = self.fct()
        return {"flows": len(self.spec), "done": int((self.state == abi.FLOW_DONE).sum()),
                "failed": int((self.state == abi.FLOW_FAILED).sum()), "active": int((self.state == abi.FLOW_ACTIVE).sum()),
                "segs_acked": int(self.acked.sum()), "bytes_acked": int(self.acked.sum()) * self.flow["seg_len"],
                "data_offered": int(self.offered.sum()), "retransmits": int(self.retransmits.sum()),
                "stale_acks": int(self.stale.sum()), "dup_ignored": self.dup_ignored,
                "corrupt_ignored": self.corrupt_ignored, "pending_acks": len(self.cal),
                "fct_sum_ns": int(fct.sum()), "fct_min_ns": int(fct.min()) if len(fct) else int(np.iinfo(np.uint64).max),
                "fct_max_ns": int(fct.max()) if len(fct) else 0, "hist": self.hist.copy()}


FLOW_CC_DEFAULT = dict(init_cwnd=1, init_ssthresh=0, dupthresh=3)


class FlowCCModel(FlowModel):
    """FlowModel with the congestion window of tgsim_flow_init_cc (include/tgsim.h, "Congestion
    control"): `cc` holds init_cwnd, init_ssthresh and dupthresh.  `window` is the cap of cwnd; what is
    in flight is [base, next) with `next` stored; an ACK grows cwnd, marks segments below `dupthresh`
    acknowledged ones for a fast retransmission and releases what the window admits; a timer that runs
    out shrinks cwnd to 1."""

    def __init__(self, eng, flow: Dict, flows: np.ndarray, cc: Dict):
        super().__init__(eng, flow, flows)
        self.cc = dict(FLOW_CC_DEFAULT, **cc)
        c, w = self.cc, self.flow["window"]
        if not 1 <= c["init_cwnd"] <= w:
            raise ValueError(f"flow: init_cwnd {c['init_cwnd']} outside 1..window {w}")
        if c["init_ssthresh"] and not 2 <= c["init_ssthresh"] <= w:
            raise ValueError(f"flow: init_ssthresh {c['init_ssthresh']} neither 0 nor in 2..window {w}")
        if not 0 <= c["dupthresh"] <= 63:
            raise ValueError(f"flow: dupthresh {c['dupthresh']} outside 0..63")
        nf = len(self.spec)
        self.cwnd = np.full(nf, c["init_cwnd"], dtype=np.int64)
        self.ssthresh = np.full(nf, c["init_ssthresh"] or w, dtype=np.int64)
        self.next = np.minimum(c["init_cwnd"], self.spec["n_seg"].astype(np.int64))
        self.recover = np.zeros(nf, dtype=np.int64)
        self.cwnd_cnt = np.zeros(nf, dtype=np.int64)
        self.loss_events = np.zeros(nf, dtype=np.int64)
        self.fast_retransmits = np.zeros(nf, dtype=np.int64)
        self.timeouts = np.zeros(nf, dtype=np.int64)
        self.fast = np.zeros((nf, w), dtype=bool)  # ring, beside att
        # what the run exercised: loss events by cause, loss signals `recover` suppressed, growth by
        # regime, cwnd grown to the cap, a reduced window draining (next - base > cwnd), fast-marked
        # segments acknowledged before their re-offer, fast retransmissions recovered by their timer
        self.loss_fast = self.loss_timeout = self.suppressed = self.grow_ss = self.grow_ca = 0
        self.cwnd_at_cap = self.draining = self.fast_acked_early = self.fast_lost = 0
        self._was_fast = [set() for _ in range(nf)]

    def _next(self, f: int) -> int:
        return int(self.next[f])

    def window_packets(self, window: int) -> np.ndarray:
        p, win0, win1 = self.flow, self.now, self.now + window
        if win1 >= 1 << 31:  # the engine's -EOVERFLOW: ticks of the timers and the calendar stay below 2^31
            raise EngineError(-errno.EOVERFLOW, "flow: the window ends beyond tick 2^31")
        name, longest = self._window_limit()
        if window > longest:
            raise ValueError(f"flow: a window of {window} ticks is longer than {name} {longest}")
        w = p["window"]
        live = np.nonzero(self.state == abi.FLOW_ACTIVE)[0]
        late = [int(self.cal[:, 0].min())] if len(self.cal) else []
        late += [int(self.due[f, i % w]) for f in live for i in self._unacked(f)]
        if late and min(late) < win0:  # nothing is generated, no state changes, the cc rows included
            raise FlowLate(f"flow: a receipt due at tick {min(late)} precedes the window at tick {win0}")
        rows = []  # src, dst, seq, tick, len
        for f in live:
            segs = self._unacked(f)
            fail = [int(self.due[f, i % w]) for i in segs if self.due[f, i % w] < win1 and self.att[f, i % w] >= p["max_attempts"]]
            fail_tick = min(fail) if fail else None
            recover, timed_out, loss = int(self.recover[f]), False, False  # (recover: read once, before the pass)
            self.draining += self.next[f] - self.base[f] > self.cwnd[f]
            for i in segs:
                t, k = int(self.due[f, i % w]), int(self.att[f, i % w])
                if t >= win1 or (fail_tick is not None and t >= fail_tick):
                    continue
                rows.append((int(self.spec["src"][f]), int(self.spec["dst"][f]),
                             k << abi.FLOW_ATTEMPT_SHIFT | int(self.slot[f]) << abi.FLOW_SLOT_SHIFT | i, t, p["seg_len"]))
                self.due[f, i % w] = t + self._timer(f, i, k, t)
                self.att[f, i % w] = k + 1
                self.offered[f] += 1
                self.retransmits[f] += k > 0
                self.max_attempt = max(self.max_attempt, k)
                if self.fast[f, i % w]:  # the fast retransmission: attempt 1 in its seq
                    self.fast[f, i % w] = False
                    self._was_fast[f].add(i)
                elif k > 0:
                    self.timeouts[f] += 1
                    timed_out = True
                    loss |= i >= recover
                    self.fast_lost += k >= 2 and i in self._was_fast[f]
            if loss:  # one loss event per flow per generation
                self.ssthresh[f] = max(self.cwnd[f] // 2, 2)
                self.cwnd[f], self.cwnd_cnt[f], self.recover[f] = 1, 0, self.next[f]
                self.loss_events[f] += 1
                self.loss_timeout += 1
            elif timed_out:
                self.suppressed += 1
            if fail_tick is not None:
                self.state[f] = abi.FLOW_FAILED
                self.done_ns[f] = fail_tick * self.tick_ns
        due = self.cal[:, 0] < win1
        ack, self.cal = self.cal[due], self.cal[~due]
        rows += [(int(r), int(q), int(s) | abi.FLOW_ACK, int(t), p["ack_len"]) for t, r, q, s in ack]
        a = np.array(rows, dtype=np.int64).reshape(-1, 5)
        a = a[np.lexsort((a[:, 1], a[:, 2], a[:, 3], a[:, 0]))]
        if len(a):
            self.max_row = max(self.max_row, int(np.bincount(a[:, 0]).max()))
            if len(ack):
                self.max_ack_row = max(self.max_ack_row, int(np.bincount(ack[:, 1]).max()))
            tie = (a[1:, 0] == a[:-1, 0]) & (a[1:, 3] == a[:-1, 3]) & (a[1:, 2] == a[:-1, 2])
            self.ties += int(tie.sum())
            self.tie_sources.update(np.unique(a[1:, 0][tie]).tolist())
        pk = np.zeros(len(a), dtype=abi.PKT_DTYPE)
        pk["src"], pk["dst"], pk["seq"], pk["tick"], pk["len"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3] - win0, a[:, 4]
        return pk

    def receive(self, d: np.ndarray) -> None:
        p, w, dup = self.flow, self.flow["window"], self.cc["dupthresh"]
        new = []
        for flags, seq, t_ns, src, dst in zip(*(d[k].tolist() for k in ("flags", "seq", "t_ns", "src", "dst"))):
            if flags & abi.FLAG_DUP:
                self.dup_ignored += 1
                continue
            if flags & abi.FLAG_CORRUPT:
                self.corrupt_ignored += 1
                continue
            tick = t_ns // self.tick_ns + 1
            if not seq & abi.FLOW_ACK:
                if self._flow_of(src, seq, dst) is not None:
                    new.append((tick, dst, src, seq))
                continue
            f = self._flow_of(dst, seq, src)
            if f is None:
                continue
            seg, n_seg = seq & abi.FLOW_SEG_MASK, int(self.spec["n_seg"][f])
            if self.state[f] != abi.FLOW_ACTIVE or seg < self.base[f] or seg >= self.next[f] or seg in self.acked_segs[f]:
                self.stale[f] += 1
                continue
            self._non_stale_ack(f, seg, seq, tick)
            # 1, 2: mark, advance base
            self.acked_segs[f].add(seg)
            self.acked[f] += 1
            self.fast_acked_early += bool(self.fast[f, seg % w])
            while int(self.base[f]) in self.acked_segs[f]:
                self.acked_segs[f].discard(int(self.base[f]))
                self.base[f] += 1
            # 3: growth
            if self.base[f] >= self.recover[f]:
                before = int(self.cwnd[f])
                if self.cwnd[f] < self.ssthresh[f]:
                    self.cwnd[f] += 1
                    self.grow_ss += self.cwnd[f] <= w
                else:
                    self.cwnd_cnt[f] += 1
                    if self.cwnd_cnt[f] >= self.cwnd[f]:
                        self.cwnd[f] += 1
                        self.cwnd_cnt[f] = 0
                        self.grow_ca += self.cwnd[f] <= w
                self.cwnd[f] = min(self.cwnd[f], w)
                self.cwnd_at_cap += before < w == self.cwnd[f]
            # 4: fast retransmit
            if dup:
                for i in range(int(self.base[f]), int(self.next[f])):
                    if i in self.acked_segs[f] or sum(1 for s in self.acked_segs[f] if s > i) < dup:
                        continue
                    if self.att[f, i % w] != 1 or self.fast[f, i % w] or self.due[f, i % w] <= tick:
                        continue
                    self.due[f, i % w], self.fast[f, i % w] = tick, True
                    self.fast_retransmits[f] += 1
                    if i >= self.recover[f]:
                        self.ssthresh[f] = max(self.cwnd[f] // 2, 2)
                        self.cwnd[f], self.cwnd_cnt[f], self.recover[f] = self.ssthresh[f], 0, self.next[f]
                        self.loss_events[f] += 1
                        self.loss_fast += 1
                    else:
                        self.suppressed += 1
            # 5: release
            next2 = max(int(self.next[f]), min(int(self.base[f] + self.cwnd[f]), n_seg))
            for i in range(int(self.next[f]), next2):
                self.due[f, i % w], self.att[f, i % w], self.fast[f, i % w] = tick, 0, False
                self.ring_wraps += i >= w
            self.next[f] = next2
            # 6: done
            if self.base[f] == n_seg:
                self.state[f] = abi.FLOW_DONE
                self.done_ns[f] = t_ns
                if p["n_bins"]:
                    fct = t_ns - int(self.spec["start_tick"][f]) * self.tick_ns
                    self.hist[min(fct // p["bin_ns"], p["n_bins"] - 1)] += 1
        self.cal = np.concatenate([self.cal, np.array(new, dtype=np.int64).reshape(-1, 4)])

    def cc_rows(self) -> np.ndarray:
        out = np.zeros(len(self.spec), dtype=abi.FLOW_CC_ROW_DTYPE)
        for key, v in (("cwnd", self.cwnd), ("ssthresh", self.ssthresh), ("next", self.next), ("recover", self.recover),
                       ("cwnd_cnt", self.cwnd_cnt), ("loss_events", self.loss_events),
                       ("fast_retransmits", self.fast_retransmits), ("timeouts", self.timeouts)):
            out[key] = v
        return out

    def cc_report(self) -> Dict:
        cw = self.cwnd[self.state == abi.FLOW_ACTIVE]
        return {"loss_events": int(self.loss_events.sum()), "fast_retransmits": int(self.fast_retransmits.sum()),
                "timeouts": int(self.timeouts.sum()), "active": len(cw), "cwnd_sum": int(cw.sum()),
                "cwnd_min": int(cw.min()) if len(cw) else int(np.iinfo(np.uint64).max),
                "cwnd_max": int(cw.max()) if len(cw) else 0}


FLOW_RTO_DEFAULT = dict(min_rto_ticks=1, max_rto_ticks=abi.FLOW_MAX_RTO, backoff=1)


class FlowRtoMixin:
    """The RTT estimator and timer backoff of tgsim_flow_init_rto (include/tgsim.h) over FlowModel or
    FlowCCModel: `rto` holds min_rto_ticks, max_rto_ticks and backoff; flow["rto_ticks"] is every
    flow's initial timer.  An ACK of attempt 0 is a sample (RFC 6298 in integer ticks), a segment's
    timer is the flow's rto, doubled per earlier offer with backoff and capped at max_rto_ticks."""

    def __init__(self, eng, flow: Dict, flows: np.ndarray, *cc, rto: Dict):
        super().__init__(eng, flow, flows, *cc)
        self.rto_p = dict(FLOW_RTO_DEFAULT, **rto)
        r, t0 = self.rto_p, self.flow["rto_ticks"]
        if r["min_rto_ticks"] < 1:
            raise ValueError(f"flow: min_rto_ticks {r['min_rto_ticks']} below 1")
        if not r["min_rto_ticks"] <= r["max_rto_ticks"] <= abi.FLOW_MAX_RTO:
            raise ValueError(f"flow: max_rto_ticks {r['max_rto_ticks']} outside min_rto_ticks ({r['min_rto_ticks']})..2^27")
        if r["backoff"] not in (0, 1):
            raise ValueError(f"flow: backoff {r['backoff']} outside 0..1")
        if not r["min_rto_ticks"] <= t0 <= r["max_rto_ticks"]:
            raise ValueError(f"flow: rto_ticks {t0} outside min_rto_ticks..max_rto_ticks")
        nf, w = len(self.spec), self.flow["window"]
        self.srtt8 = np.zeros(nf, dtype=np.int64)
        self.rttvar4 = np.zeros(nf, dtype=np.int64)
        self.rto = np.full(nf, t0, dtype=np.int64)
        self.samples = np.zeros(nf, dtype=np.int64)
        self.rtt_min = np.full(nf, 0xFFFFFFFF, dtype=np.int64)
        self.rtt_max = np.zeros(nf, dtype=np.int64)
        self.rtt_last = np.zeros(nf, dtype=np.int64)
        self.sent = np.zeros((nf, w), dtype=np.int64)  # ring, beside due and att
        self.sample_log = [[] for _ in range(nf)]  # per flow, the samples in the order taken
        # what the run exercised: samples from a segment retransmitted since, rto clamped at either end,
        # timers shifted by two or more, shifted timers capped, ACKs of a later attempt (no sample)
        self.sampled_after_retransmit = self.clamped_min = self.clamped_max = 0
        self.shifted_twice = self.shift_capped = self.unsampled_attempts = 0

    def _window_limit(self) -> Tuple[str, int]:
        return "min_rto_ticks", self.rto_p["min_rto_ticks"]

    def _timer(self, f: int, i: int, k: int, t: int) -> int:
        r, rto = self.rto_p, int(self.rto[f])
        if k == 0:
            self.sent[f, i % self.flow["window"]] = t
        if not r["backoff"]:
            return rto
        self.shifted_twice += k >= 2
        self.shift_capped += k >= 1 and rto << k > r["max_rto_ticks"]
        return min(rto << k, r["max_rto_ticks"])

    def _non_stale_ack(self, f: int, seg: int, seq: int, tick: int) -> None:
        r, at = self.rto_p, seg % self.flow["window"]
        if seq >> abi.FLOW_ATTEMPT_SHIFT & 15:
            self.unsampled_attempts += 1
            return
        if self.att[f, at] < 1:
            return
        m = min(tick - int(self.sent[f, at]), r["max_rto_ticks"])
        if self.samples[f] == 0:
            self.srtt8[f], self.rttvar4[f] = 8 * m, 2 * m
        else:
            err = m - (int(self.srtt8[f]) >> 3)
            self.rttvar4[f] = self.rttvar4[f] - (int(self.rttvar4[f]) >> 2) + abs(err)
            self.srtt8[f] += err
        v = (int(self.srtt8[f]) >> 3) + max(int(self.rttvar4[f]), 1)
        self.rto[f] = min(max(v, r["min_rto_ticks"]), r["max_rto_ticks"])
        self.clamped_min += v < r["min_rto_ticks"]
        self.clamped_max += v > r["max_rto_ticks"]
        self.sampled_after_retransmit += self.att[f, at] >= 2
        self.samples[f] += 1
        self.rtt_min[f], self.rtt_max[f], self.rtt_last[f] = min(self.rtt_min[f], m), max(self.rtt_max[f], m), m
        self.sample_log[f].append(m)

    def rto_rows(self) -> np.ndarray:
        out = np.zeros(len(self.spec), dtype=abi.FLOW_RTO_ROW_DTYPE)
        for key, v in (("srtt8", self.srtt8), ("rttvar4", self.rttvar4), ("rto", self.rto), ("samples", self.samples),
                       ("rtt_min", self.rtt_min), ("rtt_max", self.rtt_max), ("rtt_last", self.rtt_last)):
            out[key] = v
        return out

    def rto_report(self) -> Dict:
        on = self.samples > 0
        srtt, rto, none = self.srtt8[on] >> 3, self.rto[on], int(np.iinfo(np.uint64).max)
        return {"samples": int(self.samples.sum()), "sampled_flows": int(on.sum()),
                "srtt_sum": int(srtt.sum()), "srtt_min": int(srtt.min()) if on.any() else none,
                "srtt_max": int(srtt.max()) if on.any() else 0,
                "rto_sum": int(rto.sum()), "rto_min": int(rto.min()) if on.any() else none,
                "rto_max": int(rto.max()) if on.any() else 0}


FLOW_FB_DEFAULT = dict(fail_mask=0)


class FlowFbMixin:
    """The verdict feedback of tgsim_flow_init_fb (include/tgsim.h) over any of the models: `fb` holds
    fail_mask.  After a window's simulation its data packets are counted per flow by verdict, and a
    flow with a refused offer whose verdict is in fail_mask fails at the earliest such offer's tick,
    ahead of the records the same step emitted."""

    def __init__(self, eng, flow: Dict, flows: np.ndarray, *cc, fb: Dict, **kw):
        super().__init__(eng, flow, flows, *cc, **kw)
        self.fb_p = dict(FLOW_FB_DEFAULT, **fb)
        if self.fb_p["fail_mask"] & ~abi.FLOW_FB_REFUSALS:
            raise ValueError(f"flow: fail_mask {self.fb_p['fail_mask']:#x} has bits outside the refusal verdicts")
        self.fb = np.zeros(len(self.spec), dtype=abi.FLOW_FB_ROW_DTYPE)
        # what the run exercised: timer failures of a window replaced by a refusal of the same window,
        # stale ACKs, in the step that failed them, of flows a verdict failed, refusals outside the mask
        self.fail_replaced = self.stale_after_fail = self.refused_unmasked = 0
        self._failed_now: list = []

    def _verdicts(self, pk: np.ndarray, v: np.ndarray, win0: int) -> None:
        mask, first = self.fb_p["fail_mask"], {}  # flow -> (tick, seq, verdict) of the refusal that fails it
        self._failed_now = []
        for src, seq, tick, vb in zip(pk["src"].tolist(), pk["seq"].tolist(), pk["tick"].tolist(), np.asarray(v).tolist()):
            if seq & abi.FLOW_ACK:
                continue
            f, low = int(self.first[src]) + (seq >> abi.FLOW_SLOT_SHIFT & 15), vb & 15
            row = self.fb[f]
            if low == abi.V_SCHEDULED:
                row["scheduled"] += 1
            elif low == abi.V_LOSS:
                row["lost"] += 1
            elif low == abi.V_QUEUE_FULL:
                row["queue_full"] += 1
            elif abi.V_DISCONNECTED <= low <= abi.V_PROHIBIT:
                row["refused"] += 1
                if not mask >> low & 1:
                    self.refused_unmasked += 1
                elif f not in first or (tick, seq) < first[f][:2]:
                    first[f] = (tick, seq, low)
            row["cloned"] += vb >> 4 != abi.V_NONE
        for f, (tick, seq, low) in first.items():
            timer = (self.state[f] == abi.FLOW_FAILED and not self.fb[f]["fail_verdict"]
                     and self.done_ns[f] >= win0 * self.tick_ns)
            if self.state[f] != abi.FLOW_ACTIVE and not timer:
                continue
            self.fail_replaced += bool(timer)
            self.state[f], self.done_ns[f] = abi.FLOW_FAILED, (win0 + tick) * self.tick_ns
            self.fb[f]["fail_verdict"], self.fb[f]["fail_seg"] = low, seq & abi.FLOW_SEG_MASK
            self.fb[f]["fail_attempt"] = seq >> abi.FLOW_ATTEMPT_SHIFT & 15
            self._failed_now.append(f)

    def receive(self, d: np.ndarray) -> None:
        before = int(self.stale[self._failed_now].sum())
        super().receive(d)
        self.stale_after_fail += int(self.stale[self._failed_now].sum()) - before
        self._failed_now = []

    def fb_rows(self) -> np.ndarray:
        return self.fb.copy()

    def fb_report(self) -> Dict:
        failed, fv = self.state == abi.FLOW_FAILED, self.fb["fail_verdict"]
        out = {k: int(self.fb[k].sum()) for k in ("scheduled", "lost", "queue_full", "refused", "cloned")}
        out["refused_flows"] = int((self.fb["refused"] > 0).sum())
        out["failed_timer"] = int((failed & (fv == 0)).sum())
        for k, name in enumerate(abi.FLOW_FB_SUMMARY_FIELDS[-4:]):
            out[name] = int((failed & (fv == 1 + k)).sum())
        return out


def flow_model(eng, flow: Dict, flows: np.ndarray, cc=None, rto=None, fb=None):
    """The host model for an arming: FlowModel, with the congestion window when `cc` is given, the RTT
    estimator when `rto` is, the verdict feedback when `fb` is (the dicts of Engine.flow_init)."""
    bases = ((FlowFbMixin,) if fb is not None else ()) + ((FlowRtoMixin,) if rto is not None else ())
    bases += (FlowModel if cc is None else FlowCCModel,)
    cls = bases[0] if len(bases) == 1 else type("Flow" + "".join(b.__name__[4:-5] for b in bases[:-1]) + bases[-1].__name__[4:], bases, {})
    kw = dict(**({} if rto is None else {"rto": rto}), **({} if fb is None else {"fb": fb}))
    return cls(eng, flow, flows, *(() if cc is None else (cc,)), **kw)


class FlowRtoModel(FlowRtoMixin, FlowModel):
    """FlowModel armed with `rto`: FlowRtoModel(eng, flow, flows, rto=dict(...))."""


class FlowCCRtoModel(FlowRtoMixin, FlowCCModel):
    """FlowCCModel armed with `rto`: FlowCCRtoModel(eng, flow, flows, cc, rto=dict(...))."""


def flow_reference(eng, flow: Dict, flows: np.ndarray, n_windows: int, window: int, probe_at=(), before=None,
                   cc=None, rto=None, fb=None) -> Dict:
    """The flow loop driven from the host over `eng` (submit / step / verdicts / drain): per-window
    (verdicts, deliveries) under "windows", the final "rows" and "summary" (report fields and hist),
    and under "probes" the (rows, summary) after each window index in probe_at.  before(w) runs ahead
    of window w (a reshape, a partition).  The model itself is under "model".  With `cc` (the dict of
    Engine.flow_init) the model is FlowCCModel, the result has "cc_rows" and "cc_summary" too, and a
    probe is (rows, summary, cc_rows, cc_summary).  With `rto` (the dict of Engine.flow_init) the model
    is FlowRtoModel or FlowCCRtoModel, the result has "rto_rows" and "rto_summary" too, and a probe ends
    with (rto_rows, rto_summary).  With `fb` (the dict of Engine.flow_init) the model has the verdict
    feedback (FlowFbMixin), the result has "fb_rows" and "fb_summary" too, and a probe ends with (fb_rows,
    fb_summary)."""
    if fb is not None:
        m = flow_model(eng, flow, flows, cc, rto, fb)
    elif rto is None:
        m = FlowModel(eng, flow, flows) if cc is None else FlowCCModel(eng, flow, flows, cc)
    else:
        m = FlowRtoModel(eng, flow, flows, rto=rto) if cc is None else FlowCCRtoModel(eng, flow, flows, cc, rto=rto)
    out = {"windows": [], "probes": {}, "model": m}
    for w in range(n_windows):
        if before is not None:
            before(w)
        out["windows"].append(m.step(window))
        if w in probe_at:
            out["probes"][w] = ((m.rows(), m.report()) + (() if cc is None else (m.cc_rows(), m.cc_report()))
                                + (() if rto is None else (m.rto_rows(), m.rto_report()))
                                + (() if fb is None else (m.fb_rows(), m.fb_report())))
    out["rows"], out["summary"] = m.rows(), m.report()
    if cc is not None:
        out["cc_rows"], out["cc_summary"] = m.cc_rows(), m.cc_report()
    if rto is not None:
        out["rto_rows"], out["rto_summary"] = m.rto_rows(), m.rto_report()
    if fb is not None:
        out["fb_rows"], out["fb_summary"] = m.fb_rows(), m.fb_report()
    return out


def flow_run(eng, n_windows: int, window: int, collect: bool = False, probe_at=(), before=None, step=None) -> Dict:
    """The device loop on an armed engine (Engine.flow_init): n_windows of gen_flow + step.  Nothing
    reaches the host unless asked for: collect keeps each window's (verdicts, deliveries), probe_at
    the (rows, report) after those windows, and the (cc rows, cc report) beside them when the engine
    is armed with congestion control, the (rto rows, rto report) when it is armed with the RTT
    estimator, and the (fb rows, fb report) last when it is armed with the verdict feedback.
    step(window) replaces eng.step (a shard of a run armed with sharded=True: eng.comm_step; the rows
    and reports are then the shard's)."""
    step = eng.step if step is None else step
    out = {"windows": [], "probes": {}}
    cc, rto = getattr(eng, "flow_cc_armed", False), getattr(eng, "flow_rto_armed", False)
    fb = getattr(eng, "flow_fb_armed", False)
    for w in range(n_windows):
        if before is not None:
            before(w)
        eng.gen_flow(window)
        step(window)
        if collect:
            out["windows"].append((eng.verdicts(), eng.drain()))
        if w in probe_at:
            out["probes"][w] = ((eng.flow_rows(), eng.flow_report()) + ((eng.flow_cc_rows(), eng.flow_cc_report()) if cc else ())
                                + ((eng.flow_rto_rows(), eng.flow_rto_report()) if rto else ())
                                + ((eng.flow_fb_rows(), eng.flow_fb_report()) if fb else ()))
    return out


# The merge rules of include/tgsim.h for the shards' flow reports: every field by sum, except these.
_FLOW_MERGE_MIN = {"fct_min_ns", "cwnd_min", "srtt_min", "rto_min"}
_FLOW_MERGE_MAX = {"fct_max_ns", "cwnd_max", "srtt_max", "rto_max"}


def _merge_flow_fields(who: str, reports, fields) -> Dict:
    reports = list(reports)
    if not reports:
        raise ValueError(f"{who}: no report")
    out = {}
    for key in fields:
        vals = [int(r[key]) for r in reports]
        out[key] = min(vals) if key in _FLOW_MERGE_MIN else max(vals) if key in _FLOW_MERGE_MAX else sum(vals)
    return out


def merge_flow_reports(reports) -> Dict:
    """The shards' flow reports (Engine.flow_report of every rank) as the whole run's, by the merge
    rule of include/tgsim.h: every field by sum, except fct_min_ns by min and fct_max_ns by max; hist
    by sum (a shard without a DONE flow reports the neutral UINT64_MAX and 0).  For hosts with their own
    exchange; Engine.comm_flow_report does the same on the device."""
    reports = list(reports)
    out = _merge_flow_fields("merge_flow_reports", reports, abi.FLOW_SUMMARY_FIELDS)
    hists = [np.asarray(r["hist"], dtype=np.uint64) for r in reports]
    if len({len(h) for h in hists}) != 1:
        raise ValueError("merge_flow_reports: the reports' histograms differ in length")
    out["hist"] = np.sum(hists, axis=0, dtype=np.uint64)
    return out


def merge_flow_cc_reports(reports) -> Dict:
    """The shards' Engine.flow_cc_report as the whole run's: sums, cwnd_min by min, cwnd_max by max."""
    return _merge_flow_fields("merge_flow_cc_reports", reports, abi.FLOW_CC_SUMMARY_FIELDS)


def merge_flow_rto_reports(reports) -> Dict:
    """The shards' Engine.flow_rto_report as the whole run's: sums, srtt_min and rto_min by min, srtt_max
    and rto_max by max."""
    return _merge_flow_fields("merge_flow_rto_reports", reports, abi.FLOW_RTO_SUMMARY_FIELDS)


def merge_flow_fb_reports(reports) -> Dict:
    """The shards' Engine.flow_fb_report as the whole run's: every field by sum."""
    return _merge_flow_fields("merge_flow_fb_reports", reports, abi.FLOW_FB_SUMMARY_FIELDS)


# ---------------------------------------------------------------------------------------------
# Per-group traffic matrix (tgsim_groups_init / tgsim_group_matrix, include/tgsim.h): the host model
# the device's folds are compared with, in numpy: the word definitions and nothing cleverer.
class GroupMatrix:
    """m[gs, gd, w]: cell (group of src, group of dst), column n_groups for abi.EXTERNAL, words
    abi.GROUP_NAMES.  fold() adds one window: its offered packets (abi.PKT_DTYPE), their verdict bytes
    (in the packets' order) and the records the step delivered (abi.DELIVERY_DTYPE)."""

    def __init__(self, group_of, n_groups: int):
        self.group_of = np.asarray(group_of, dtype=np.int64)
        self.n_groups = int(n_groups)
        if not 1 <= self.n_groups <= abi.GROUP_MAX:
            raise ValueError(f"GroupMatrix: n_groups {n_groups} outside 1..{abi.GROUP_MAX}")
        if len(self.group_of) and (self.group_of.min() < 0 or self.group_of.max() >= self.n_groups):
            raise ValueError("GroupMatrix: a group id outside 0..n_groups-1")
        self.m = np.zeros((self.n_groups, self.n_groups + 1, abi.GROUP_WORDS), dtype=np.uint64)

    def _col(self, dst: np.ndarray) -> np.ndarray:
        dst = dst.astype(np.int64)
        ext = dst == abi.EXTERNAL
        return np.where(ext, self.n_groups, self.group_of[np.where(ext, 0, dst)])

    def fold(self, pkts=None, verdicts=None, drained=None) -> "GroupMatrix":
        if pkts is not None and len(pkts):
            v = np.asarray(verdicts, dtype=np.uint8)
            if len(v) != len(pkts):
                raise ValueError("GroupMatrix.fold: one verdict byte per offered packet")
            gs, gd = self.group_of[pkts["src"].astype(np.int64)], self._col(pkts["dst"])
            np.add.at(self.m[:, :, 0], (gs, gd), np.uint64(1))
            np.add.at(self.m[:, :, 1], (gs, gd), pkts["len"].astype(np.uint64))
            lo, hi = (v & 15).astype(np.int64), (v >> 4).astype(np.int64)
            np.add.at(self.m, (gs, gd, 2 + lo), np.uint64(1))
            clone = hi != abi.V_NONE
            np.add.at(self.m, (gs[clone], gd[clone], 2 + hi[clone]), np.uint64(1))
        if drained is not None and len(drained):
            gs, gd = self.group_of[drained["src"].astype(np.int64)], self._col(drained["dst"])
            np.add.at(self.m[:, :, 10], (gs, gd), np.uint64(1))
            np.add.at(self.m[:, :, 11], (gs, gd), drained["len"].astype(np.uint64))
            np.add.at(self.m[:, :, 12], (gs, gd), ((drained["flags"] & abi.FLAG_DUP) != 0).astype(np.uint64))
            np.add.at(self.m[:, :, 13], (gs, gd), ((drained["flags"] & abi.FLAG_CORRUPT) != 0).astype(np.uint64))
        return self


def merge_group_matrices(ms) -> np.ndarray:
    """The matrix of a whole run from its shards' Engine.group_matrix() results: the plain sum."""
    ms = [np.asarray(m, dtype=np.uint64) for m in ms]
    if not ms:
        raise ValueError("merge_group_matrices: no matrices")
    if any(m.shape != ms[0].shape for m in ms):
        raise ValueError("merge_group_matrices: the shards' matrices differ in shape")
    return np.sum(ms, axis=0, dtype=np.uint64)


def group_reachability(m, round_trip: bool = False) -> np.ndarray:
    """ok[gs, gd] = some record from group gs was delivered to group gd (word 10 > 0); [G, G], without
    the external column, where nothing is ever delivered.  round_trip: both directions deliver, which
    is what a request and its reply need (splitbrain's expectErrors, negated)."""
    m = np.asarray(m)
    ok = m[:, :m.shape[0], 10] > 0
    return ok & ok.T if round_trip else ok


# ---------------------------------------------------------------------------------------------
# Packet capture of watched peers (tgsim_capture_*): the host model of one window.
def capture_reference(watched, pkts, verdicts, drained, start_tick: int, tick_ns: int, owned=None,
                      generated: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """What an engine owning the peers owned = (lo, hi) (default: every watched peer) captures in one
    window, from what a host sees of it: the packets offered (abi.PKT_DTYPE), their verdict bytes (one
    per packet, in the packets' order) and the records drained after the step.  Returns (tx, rx) of
    abi.CAPTURE_DTYPE in the capture's order (include/tgsim.h):
      tx  the packets of watched, owned sources in (src, tick, seq, dst) order -- a row of the
          engine's input is in (tick, seq) order, and host packets arrive in submit order; with
          generated=True the packets are a generated window's, already in row order (the oracle's
          `offered`), and are only stable-sorted by src;
      rx  the drained records of watched, owned destinations, by destination, each in drain order.
    start_tick: the window's first tick (stats()["now_tick"] before the step)."""
    w = np.asarray(watched, dtype=np.int64)
    lo, hi = (0, 1 << 32) if owned is None else owned
    w = w[(w >= lo) & (w < hi)]
    tx = np.zeros(0, dtype=abi.CAPTURE_DTYPE)
    if pkts is not None and len(pkts):
        v = np.asarray(verdicts, dtype=np.uint8)
        if len(v) != len(pkts):
            raise ValueError("capture_reference: one verdict byte per offered packet")
        keep = np.nonzero(np.isin(pkts["src"], w))[0]
        p, v = pkts[keep], v[keep]
        order = np.argsort(p["src"], kind="stable") if generated else np.lexsort((p["dst"], p["seq"], p["tick"], p["src"]))
        p, v = p[order], v[order]
        tx = np.zeros(len(p), dtype=abi.CAPTURE_DTYPE)
        tx["t_ns"] = (np.uint64(start_tick) + p["tick"].astype(np.uint64)) * np.uint64(tick_ns)
        tx["src"], tx["dst"], tx["seq"], tx["len"] = p["src"], p["dst"], p["seq"], p["len"]
        tx["verdict"], tx["dir"] = v, abi.CAPTURE_TX
    rx = np.zeros(0, dtype=abi.CAPTURE_DTYPE)
    if drained is not None and len(drained):
        d = drained[np.isin(drained["dst"], w)]
        d = d[np.argsort(d["dst"], kind="stable")]
        rx = np.zeros(len(d), dtype=abi.CAPTURE_DTYPE)
        for k in ("t_ns", "src", "dst", "seq", "len", "flags"):
            rx[k] = d[k]
        rx["dir"] = abi.CAPTURE_RX
    return tx, rx


def merge_captures(per_rank_reads) -> Dict[str, np.ndarray]:
    """One window's Engine.capture_read() results of a run's shards, in rank order, as the single engine's:
    shards own ascending contiguous ranges and every direction is in ascending peer order, so the merge
    is concatenation.  (Reads that span several windows do not merge this way.)"""
    reads = list(per_rank_reads)
    if not reads:
        raise ValueError("merge_captures: no reads")
    return {k: np.concatenate([np.asarray(r[k], dtype=abi.CAPTURE_DTYPE) for r in reads]) for k in ("tx", "rx")}


# ---------------------------------------------------------------------------------------------
# C4: gossip flood.  The engine generates and consumes the traffic on the device
# (tgsim_gossip_init / tgsim_gen_gossip); this module only shapes the peers and runs windows.
GOSSIP_MIN_LAT = 5 * Millisecond


def gossip_shapes(n_peers: int, seed: int = SEED) -> Tuple[np.ndarray, float]:
    """Per-peer latency L~U[5,50] ms in whole microseconds (what toMicroseconds keeps), loss 1 %."""
    rng = np.random.default_rng((seed >> 32) & 0xFFFFFFFF)
    lat_us = rng.integers(5_000, 50_001, n_peers)
    return lat_us * 1000, 1.0


def configure_gossip(eng, n_peers: int, seed: int = SEED) -> None:
    lat, loss = gossip_shapes(n_peers, seed)
    eng.configure_batch(np.arange(n_peers), configs_array(lat, loss=loss))


def gossip_window_ticks(eng) -> int:
    """The largest window whose receipts are all known before the next window: the engine serves
    items eligible before T_end + lookahead, so lookahead = window = the minimum latency."""
    return GOSSIP_MIN_LAT // eng.tick_ns


def gossip_run(eng, n_windows: int, window: int, collect: bool = True):
    """Runs n_windows gossip windows; returns per-window (verdicts, deliveries) when collect."""
    out = []
    for _ in range(n_windows):
        eng.gen_gossip(window)
        eng.step(window)
        if collect:
            out.append((eng.verdicts(), eng.drain()))
    return out


SPREAD_KEYS = ("reached", "sum_ticks", "min_ticks", "max_ticks", "hist")


def merge_spread(spreads) -> Dict[str, np.ndarray]:
    """The report of a whole run from its shards' Engine.gossip_spread() results (same floods, same
    bins): reached, sum_ticks and hist add, min_ticks and max_ticks are the extremes.  A shard no
    flood has reached carries the neutral values (0, 0, 0xFFFFFFFF, 0), so it merges like any other."""
    spreads = list(spreads)
    if not spreads:
        raise ValueError("merge_spread: no spreads")
    if any(s["hist"].shape != spreads[0]["hist"].shape for s in spreads):
        raise ValueError("merge_spread: the shards' histograms differ in shape")
    return {
        "reached": np.sum([s["reached"] for s in spreads], axis=0, dtype=np.uint64),
        "sum_ticks": np.sum([s["sum_ticks"] for s in spreads], axis=0, dtype=np.uint64),
        "min_ticks": np.min([s["min_ticks"] for s in spreads], axis=0).astype(np.uint32),
        "max_ticks": np.max([s["max_ticks"] for s in spreads], axis=0).astype(np.uint32),
        "hist": np.sum([s["hist"] for s in spreads], axis=0, dtype=np.uint64),
    }


def spread_coverage(spread: Dict[str, np.ndarray], bin_ticks: int, n_peers: int, fractions) -> np.ndarray:
    """The propagation curve read off a spread's histogram: out[f, i] = the upper edge, in ticks after
    flood f's start, of the first bin at which the cumulative count reaches ceil(fractions[i] * n_peers)
    peers; -1 where the flood has not reached that many, or reaches them only in the last bin (which
    collects every hold beyond the histogram, so it has no upper edge)."""
    hist = np.asarray(spread["hist"], dtype=np.uint64)
    n_floods, n_bins = hist.shape
    out = np.full((n_floods, len(fractions)), -1, dtype=np.int64)
    if n_bins == 0:
        return out
    cum = np.cumsum(hist, axis=1)
    for i, frac in enumerate(fractions):
        need = int(np.ceil(frac * n_peers - 1e-9))  # (0.9 * 1000 is 900.0000000000001 in binary)
        hit = cum >= need
        b = np.argmax(hit, axis=1)
        ok = hit.any(axis=1) & (b < n_bins - 1)
        out[ok, i] = (b[ok] + 1) * bin_ticks
    return out


# ---------------------------------------------------------------------------------------------
# C5: epochs of C3 traffic with mid-run reshaping and a barrier per epoch.
EPOCH_TICKS = 1000
EPOCH_LAMBDA = 0.2
EPOCH_RESHAPE_FRAC = 0.1


def _splitmix64(x: np.ndarray) -> np.ndarray:
    x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def epoch_selection(n_peers: int, epoch: int, frac: float = EPOCH_RESHAPE_FRAC, seed: int = SEED) -> np.ndarray:
    """Peers reshaped at the start of `epoch` (hash-selected, ~frac of all peers)."""
    with np.errstate(over="ignore"):
        x = _splitmix64(np.arange(n_peers, dtype=np.uint64) ^ np.uint64((seed ^ (epoch << 40)) & (2**64 - 1)))
    return np.nonzero((x >> np.uint64(32)) < np.uint64(int(frac * 2**32)))[0].astype(np.uint32)


def epoch_plan(n_peers: int, epoch: int, seed: int = SEED) -> Tuple[np.ndarray, np.ndarray]:
    """What epoch `epoch`'s plan asks for: the reshaped peers and their fresh C3-style configs."""
    sel = epoch_selection(n_peers, epoch, seed=seed)
    return sel, storm_configs(len(sel), (seed + 0x1000 * (epoch + 1)) & 0xFFFFFFFF)


def epoch_reshape(eng, n_peers: int, epoch: int, seed: int = SEED, plan=None) -> int:
    """Fresh C3-style shapes for the epoch's selected peers; every shard receives every call.
    plan: epoch_plan's output computed ahead (the bench keeps the plan's own work out of the timed
    loop, as it does the traffic; the ConfigureNetwork calls stay in it)."""
    sel, cfg = plan if plan is not None else epoch_plan(n_peers, epoch, seed)
    eng.configure_batch(sel, cfg)
    return len(sel)


def epoch_state(epoch: int) -> Tuple[int, int]:
    """Sync state id of barrier `epoch-k` and the round of that id (epochs cycle over 1024 of the
    engine's sync counters, so a long run keeps reusing the same few)."""
    return epoch % 1024, epoch // 1024 + 1


def run_epoch(eng, n_peers: int, epoch: int, n_local: int, step=None, barrier=None,
              lam: float = EPOCH_LAMBDA, ticks: int = EPOCH_TICKS, seed: int = SEED) -> None:
    """One C5 epoch: reshape (from epoch 1), traffic window, then every local peer signals
    `epoch-k` and the barrier must release with all n_peers signals (summed over shards)."""
    if epoch:
        epoch_reshape(eng, n_peers, epoch, seed)
    eng.gen_storm(lam, ticks)
    (step or eng.step)(ticks)
    state, rnd = epoch_state(epoch)
    eng.signal_async(state, n_local)
    ok = barrier(state, rnd * n_peers) if barrier else eng.barrier_poll(state, rnd * n_peers)
    if not ok:
        raise RuntimeError(f"barrier epoch-{epoch} did not release")


# ---------------------------------------------------------------------------------------------
# C6: bridge — real payloads through the native packet bridge: every
# instance sends BRIDGE_PER_WINDOW datagrams per window to random peers.
BRIDGE_PER_WINDOW = 16


def bridge_shape_arrays(n_peers: int, seed: int = SEED) -> Dict[str, np.ndarray]:
    """L~U[1,10] ms, J~U[0,1] ms, loss/dup/corrupt 1 %, 1 Gbit/s."""
    rng = np.random.default_rng((seed >> 16) & 0xFFFFFFFF)
    return dict(latency_ns=rng.integers(1 * Millisecond, 10 * Millisecond + 1, n_peers),
                jitter_ns=rng.integers(0, 1 * Millisecond + 1, n_peers),
                bandwidth_bps=np.full(n_peers, 1_000_000_000, dtype=np.int64),
                loss=np.full(n_peers, 1.0, np.float32), duplicate=np.full(n_peers, 1.0, np.float32),
                corrupt=np.full(n_peers, 1.0, np.float32))


def configure_bridge(eng, n_peers: int, seed: int = SEED) -> None:
    eng.configure_batch(np.arange(n_peers), configs_array(**bridge_shape_arrays(n_peers, seed)))


def bridge_traffic(n_peers: int, per_instance: int = BRIDGE_PER_WINDOW, seed: int = SEED):
    """One window of sends: (src, dst, payload bytes, offsets); payloads of U[64,512] bytes."""
    rng = np.random.default_rng(seed & 0xFFFF)
    src = np.repeat(np.arange(n_peers, dtype=np.uint32), per_instance)
    dst = ((src + 1 + rng.integers(0, n_peers - 1, len(src))) % n_peers).astype(np.uint32)
    lens = rng.integers(64, 513, len(src))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return src, dst, rng.bytes(int(off[-1])), off
