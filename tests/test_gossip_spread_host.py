"""Host side of the gossip propagation report: the shard merge, the coverage curve and the line
protocol on hand-made tables, the bin index's reciprocal division, and the oracle-backed engine,
whose library has no such report."""
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

from testground_amd import metrics
from testground_amd import workloads as wl
from testground_amd.engine import EngineError

NONE = 0xFFFFFFFF


def spread(reached, sum_ticks, min_ticks, max_ticks, hist):
    return {"reached": np.array(reached, dtype=np.uint64), "sum_ticks": np.array(sum_ticks, dtype=np.uint64),
            "min_ticks": np.array(min_ticks, dtype=np.uint32), "max_ticks": np.array(max_ticks, dtype=np.uint32),
            "hist": np.array(hist, dtype=np.uint64).reshape(len(reached), -1)}


# three floods over 4 bins of 10 ticks: flood 1 is empty on shard A, flood 2 on both
A = spread([5, 0, 0], [70, 0, 0], [0, NONE, 0xFFFFFFFF], [31, 0, 0], [[2, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]])
B = spread([3, 4, 0], [100, 200, 0], [12, 40, NONE], [55, 70, 0], [[0, 1, 0, 2], [0, 0, 0, 4], [0, 0, 0, 0]])
EMPTY = spread([0, 0, 0], [0, 0, 0], [NONE] * 3, [0, 0, 0], np.zeros((3, 4)))


def test_merge_spread():
    m = wl.merge_spread([A, B])
    assert m["reached"].tolist() == [8, 4, 0] and m["sum_ticks"].tolist() == [170, 200, 0]
    assert m["min_ticks"].tolist() == [0, 40, NONE] and m["max_ticks"].tolist() == [55, 70, 0]
    assert m["hist"].tolist() == [[2, 2, 1, 3], [0, 0, 0, 4], [0, 0, 0, 0]]
    for k in wl.SPREAD_KEYS:
        assert m[k].dtype == A[k].dtype and m[k].shape == A[k].shape
    # a shard nothing has reached changes nothing, wherever it stands; one shard merges to itself
    for parts in ([EMPTY, A, B], [A, B, EMPTY], [A, EMPTY, B]):
        mm = wl.merge_spread(parts)
        assert all((mm[k] == m[k]).all() for k in wl.SPREAD_KEYS)
    assert all((wl.merge_spread([B])[k] == B[k]).all() for k in wl.SPREAD_KEYS)
    assert all((wl.merge_spread([EMPTY, EMPTY])[k] == EMPTY[k]).all() for k in wl.SPREAD_KEYS)
    with pytest.raises(ValueError):
        wl.merge_spread([])
    with pytest.raises(ValueError):
        wl.merge_spread([A, spread([1, 1, 1], [0] * 3, [0] * 3, [0] * 3, np.zeros((3, 5)))])
    # sums beyond 32 bits stay exact
    big = spread([2 ** 31], [2 ** 40], [1], [2 ** 31], [[2 ** 31]])
    assert wl.merge_spread([big, big, big])["sum_ticks"][0] == 3 * 2 ** 40
    assert wl.merge_spread([big, big, big])["hist"][0, 0] == 3 * 2 ** 31


def test_spread_coverage():
    m = wl.merge_spread([A, B])  # flood 0: cumulative 2, 4, 5, 8 of 8 peers
    cov = wl.spread_coverage(m, 10, 8, [0.25, 0.5, 0.6, 0.625, 0.99, 1.0])
    assert cov.shape == (3, 6) and cov.dtype == np.int64
    # 2 peers by the end of bin 0, 4 by bin 1, ceil(4.8) = 5 by bin 2, 5 by bin 2; 8 only in the last
    # bin, which has no upper edge
    assert cov[0].tolist() == [10, 20, 30, 30, -1, -1]
    assert cov[1].tolist() == [-1, -1, -1, -1, -1, -1]  # flood 1: all 4 of its peers in the overflow bin
    assert cov[2].tolist() == [-1] * 6                  # the empty flood
    # a level never reached (10 peers, 8 have it) and exact products (0.9 * 1000 is above 900 in binary)
    assert wl.spread_coverage(m, 10, 10, [0.5, 0.9])[0].tolist() == [30, -1]
    s = spread([900], [0], [0], [5], [[899, 1, 0]])
    assert wl.spread_coverage(s, 7, 1000, [0.9, 0.899, 0.901])[0].tolist() == [14, 7, -1]
    # no histogram: nothing to read the curve from
    assert wl.spread_coverage(spread([3], [3], [1], [1], np.zeros((1, 0))), 10, 3, [0.5]).tolist() == [[-1]]


def test_gossip_lines():
    m = wl.merge_spread([A, B])
    out = metrics.gossip_lines(m, 10, "gossip plan", "r=1", 1234)
    tag = r"run=r\=1"
    for f, (r, lo, hi, su) in enumerate([(8, 0, 55, 170), (4, 40, 70, 200), (0, NONE, 0, 0)]):
        assert rf"results.gossip\ plan.gossip.reached,{tag},flood={f} value={r}i 1234" in out
        assert rf"results.gossip\ plan.gossip.hold_min,{tag},flood={f} value={lo}i 1234" in out
        assert rf"results.gossip\ plan.gossip.hold_max,{tag},flood={f} value={hi}i 1234" in out
        assert rf"results.gossip\ plan.gossip.hold_sum,{tag},flood={f} value={su}i 1234" in out
    hist = [ln for ln in out if ".gossip.hold_hist," in ln]
    # non-zero bins only, tagged with the flood and the bin's lower edge in ticks
    assert hist == [rf"results.gossip\ plan.gossip.hold_hist,{tag},flood=0,bin={b} value={c}i 1234"
                    for b, c in ((0, 2), (10, 2), (20, 1), (30, 3))] + [
                        rf"results.gossip\ plan.gossip.hold_hist,{tag},flood=1,bin=30 value=4i 1234"]
    assert len(out) == 4 * 3 + 5
    # the shape of lines(): measurement,tags field timestamp
    for ln in out:
        head, field, ts = ln.rsplit(" ", 2)
        assert head.startswith("results.") and field.startswith("value=") and field.endswith("i") and ts == "1234"


def test_oracle_engine_has_no_report(make_oracle):
    e = make_oracle(20, lookahead_ns=wl.GOSSIP_MIN_LAT)
    wl.configure_gossip(e, 20)
    e.gossip_init(n_floods=2, degree=2, msg_len=100, start_tick=0)
    for call in (lambda: e.gossip_spread(100, 8), lambda: e.gossip_spread(), lambda: e.gossip_times(0, 20)):
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == -errno.ENOSYS
    assert len(e.gossip_reached()) == 2  # what it does report


FASTDIV_CHECK = r"""
#include <stdint.h>
#include <stdio.h>
#include "tgsim_fastmod.h"
int main() {
  const uint32_t ms[] = {1u, 2u, 3u, 7u, 777u, 1000u, 5000u, 65535u, 65536u, 65537u, 0x7FFFFFFFu, 0x80000000u,
                         0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  uint64_t bad = 0, x = 88172645463325252ull;
  for (uint32_t m : ms) {
    const uint32_t rcp = tgsim::fastmod_rcp(m);
    for (uint32_t i = 0; i < 200000u; ++i) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      // random dividends, and the ones around multiples of m and the ends of the range
      uint32_t raw = (uint32_t)(x >> 32);
      if (i % 4 == 1) raw = (uint32_t)((uint64_t)(raw / m) * m) - (i >> 2 & 1u);
      if (i % 4 == 2) raw = 0xFFFFFFFFu - (i >> 2 & 1023u);
      if (i % 4 == 3) raw = i >> 2;
      if (tgsim::fastdiv_u32(raw, m, rcp) != raw / m) ++bad;
    }
  }
  printf("bad=%llu\n", (unsigned long long)bad);
  return bad != 0;
}
"""


def test_fastdiv_matches_division(tmp_path):
    """The histogram bin of k_gossip_spread: fastdiv_u32 (tgsim_fastmod.h) against / on the host."""
    from testground_amd.build import CSRC

    src = tmp_path / "fastdiv_check.cpp"
    src.write_text(FASTDIV_CHECK)
    exe = tmp_path / "fastdiv_check"
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler for the fastdiv check"
    subprocess.run([cxx, "-O2", "-std=c++17", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bad=0", r.stdout + r.stderr
