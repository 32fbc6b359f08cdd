"""K8 metrics export: the engine's device-side counters and histograms as InfluxDB line protocol.

The reference's plans record metrics through sdk-go `runenv.D()` / `runenv.R()` (counters and
histograms, e.g. plans/benchmarks/storm.go:72-208), which land in InfluxDB and are read back by
pkg/metrics: `SHOW MEASUREMENTS ... =~ /results.<name>.*/` and `SELECT last("value"), "run" ...
GROUP BY "run"` (pkg/metrics/viewer.go:46, :149).  `lines()` emits series in that shape: measurement
`results.<plan>.<metric>`, tag `run`, per-instance tag `instance` (or `bin` for histograms), field
`value`, timestamp in ns.
"""
from __future__ import annotations

from typing import Dict, Iterable, List

import numpy as np

from . import abi

SRC_METRICS = ["netem.offered", "netem.offered_bytes"] + [
    f"verdict.{abi.VERDICT_NAMES[i]}" for i in range(8)] + ["htb.served", "htb.served_bytes"]
DST_METRICS = ["delivery.records", "delivery.bytes"]
HIST_METRICS = ["hist.backlog", "hist.delivered"]


def _escape(v: str) -> str:
    return v.replace(" ", r"\ ").replace(",", r"\,").replace("=", r"\=")


def lines(m: Dict[str, np.ndarray], plan: str, run: str, ts_ns: int, shard_begin: int = 0,
          instances: Iterable[int] | None = None) -> List[str]:
    """One line per (metric, instance) of `m` (Engine.metrics()), plus one per histogram bin."""
    tags = f"run={_escape(run)}"
    out: List[str] = []
    src, dst = m["src"], m["dst"]
    sel = range(src.shape[0]) if instances is None else [i - shard_begin for i in instances]
    for col, name in enumerate(SRC_METRICS):
        meas = _escape(f"results.{plan}.{name}")
        out += [f"{meas},{tags},instance={shard_begin + i} value={int(src[i, col])}i {ts_ns}" for i in sel]
    for col, name in enumerate(DST_METRICS):
        meas = _escape(f"results.{plan}.{name}")
        out += [f"{meas},{tags},instance={shard_begin + i} value={int(dst[i, col])}i {ts_ns}" for i in sel]
    for h, name in enumerate(HIST_METRICS):
        meas = _escape(f"results.{plan}.{name}")
        out += [f"{meas},{tags},bin={b} value={int(c)}i {ts_ns}" for b, c in enumerate(m["hist"][h]) if c]
    return out


GOSSIP_METRICS = [("gossip.reached", "reached"), ("gossip.hold_min", "min_ticks"), ("gossip.hold_max", "max_ticks"),
                  ("gossip.hold_sum", "sum_ticks")]


def gossip_lines(spread: Dict[str, np.ndarray], bin_ticks: int, plan: str, run: str, ts_ns: int) -> List[str]:
    """The propagation report (Engine.gossip_spread(), or workloads.merge_spread of the shards') in
    the shape of lines(): one line per flood and measure (tag `flood`; hold times in ticks after the
    flood's start), and one per non-zero histogram bin (tags `flood` and `bin`, the bin's lower edge
    b * bin_ticks in ticks; the last bin holds everything from its edge on)."""
    tags = f"run={_escape(run)}"
    out: List[str] = []
    for name, key in GOSSIP_METRICS:
        meas = _escape(f"results.{plan}.{name}")
        out += [f"{meas},{tags},flood={f} value={int(v)}i {ts_ns}" for f, v in enumerate(spread[key])]
    meas = _escape(f"results.{plan}.gossip.hold_hist")
    for f, row in enumerate(spread["hist"]):
        out += [f"{meas},{tags},flood={f},bin={b * int(bin_ticks)} value={int(c)}i {ts_ns}"
                for b, c in enumerate(row) if c]
    return out


PING_METRICS = [("ping.pairs", "pairs"), ("ping.sent", "sent"), ("ping.received", "received"),
                ("ping.rtt_sum_ns", "sum_ns"), ("ping.rtt_min_ns", "min_ns"), ("ping.rtt_max_ns", "max_ns"),
                ("ping.pairs_all", "pairs_all"), ("ping.pairs_none", "pairs_none"),
                ("ping.dup_ignored", "dup_ignored"), ("ping.corrupt_ignored", "corrupt_ignored"),
                ("ping.pending_replies", "pending_replies")]


def ping_lines(report: Dict, bin_ns: int, plan: str, run: str, ts_ns: int) -> List[str]:
    """The ping mesh report (Engine.ping_report()) in the shape of lines(): one line per summary
    field (the RTT minimum and maximum only once a reply has been counted) and one per non-zero RTT
    histogram bin (tag `bin`: the bin's lower edge b * bin_ns in nanoseconds; the last bin holds
    everything from its edge on)."""
    tags = f"run={_escape(run)}"
    out: List[str] = []
    for name, key in PING_METRICS:
        if key in ("min_ns", "max_ns") and not report["received"]:
            continue
        out.append(f"{_escape(f'results.{plan}.{name}')},{tags} value={int(report[key])}i {ts_ns}")
    meas = _escape(f"results.{plan}.ping.rtt_hist")
    out += [f"{meas},{tags},bin={b * int(bin_ns)} value={int(c)}i {ts_ns}" for b, c in enumerate(report["hist"]) if c]
    return out


FLOW_METRICS = [(f"flow.{k}", k) for k in abi.FLOW_SUMMARY_FIELDS]


def flow_lines(report: Dict, bin_ns: int, plan: str, run: str, ts_ns: int) -> List[str]:
    """The flow report (Engine.flow_report()) in the shape of lines(): one line per summary field (the
    FCT minimum and maximum only once a flow is DONE) and one per non-zero FCT histogram bin (tag `bin`:
    the bin's lower edge b * bin_ns in nanoseconds; the last bin holds everything from its edge on).

    `flow.goodput_bps` is bytes_acked * 8 / the mean FCT.  The summary's bytes_acked counts every
    acknowledged segment, of ACTIVE and FAILED flows too, while the FCT exists for DONE flows only, so
    the line is written only when every flow is DONE: then it is one flow's own goodput, or the rate
    the run's flows reached together.  With unfinished or failed flows, take the bytes of the DONE
    rows from Engine.flow_rows() instead.

    A report that carries the congestion summary under "cc" (dict(eng.flow_report(),
    cc=eng.flow_cc_report()), flows armed with cc) adds one `flow.cc.<field>` line per field of it,
    the cwnd minimum and maximum only while a flow is ACTIVE.  One that carries the estimator's summary
    under "rto" (eng.flow_rto_report(), flows armed with rto) adds one `flow.rto.<field>` line per
    field of it, the minima and maxima only once a flow has a sample.  One that carries the verdict
    feedback's summary under "fb" (eng.flow_fb_report(), flows armed with fb) adds one
    `flow.fb.<field>` line per field of it."""
    tags = f"run={_escape(run)}"
    out: List[str] = []
    for name, key in FLOW_METRICS:
        if key in ("fct_min_ns", "fct_max_ns") and not report["done"]:
            continue
        out.append(f"{_escape(f'results.{plan}.{name}')},{tags} value={int(report[key])}i {ts_ns}")
    if report["done"] and report["done"] == report["flows"] and report["fct_sum_ns"]:
        goodput = report["bytes_acked"] * 8 * 10**9 * report["done"] // report["fct_sum_ns"]
        out.append(f"{_escape(f'results.{plan}.flow.goodput_bps')},{tags} value={int(goodput)}i {ts_ns}")
    cc = report.get("cc")
    for key in abi.FLOW_CC_SUMMARY_FIELDS if cc else ():
        if key in ("cwnd_min", "cwnd_max") and not cc["active"]:
            continue
        out.append(f"{_escape(f'results.{plan}.flow.cc.{key}')},{tags} value={int(cc[key])}i {ts_ns}")
    rto = report.get("rto")
    for key in abi.FLOW_RTO_SUMMARY_FIELDS if rto else ():
        if key.endswith(("_min", "_max")) and not rto["sampled_flows"]:
            continue
        out.append(f"{_escape(f'results.{plan}.flow.rto.{key}')},{tags} value={int(rto[key])}i {ts_ns}")
    fb = report.get("fb")
    for key in abi.FLOW_FB_SUMMARY_FIELDS if fb else ():
        out.append(f"{_escape(f'results.{plan}.flow.fb.{key}')},{tags} value={int(fb[key])}i {ts_ns}")
    meas = _escape(f"results.{plan}.flow.fct_hist")
    out += [f"{meas},{tags},bin={b * int(bin_ns)} value={int(c)}i {ts_ns}" for b, c in enumerate(report["hist"]) if c]
    return out


def group_lines(m: np.ndarray, names, plan: str, run: str, ts_ns: int) -> List[str]:
    """The per-group traffic matrix (Engine.group_matrix(), or workloads.merge_group_matrices of the
    shards') in the shape of lines(): one line per non-zero word of every cell, measurement
    `results.<plan>.group.<word name>` (abi.GROUP_NAMES), tags `run`, `src_group` and `dst_group`
    (names[g]; `external` for the last column)."""
    m = np.asarray(m)
    g = m.shape[0]
    if m.shape != (g, g + 1, abi.GROUP_WORDS) or len(names) != g:
        raise ValueError("group_lines: m must be [G, G + 1, 14] with one name per group")
    tags = f"run={_escape(run)}"
    col = [_escape(str(n)) for n in names] + ["external"]
    out: List[str] = []
    for w, name in enumerate(abi.GROUP_NAMES):
        meas = _escape(f"results.{plan}.group.{name}")
        out += [f"{meas},{tags},src_group={col[a]},dst_group={col[b]} value={int(m[a, b, w])}i {ts_ns}"
                for a in range(g) for b in range(g + 1) if m[a, b, w]]
    return out
