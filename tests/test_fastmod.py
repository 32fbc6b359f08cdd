"""The delay draw's modulus 2 sigma is divided once per source and every draw takes its remainder with
a multiply-high (tgsim_fastmod.h).  That is exact for every 32-bit draw or the results change, so the
host copy of the same function is compared with % here: scripts/fastmod_check.cpp, built as a
stand-alone program, over every sigma a storm shape can compile to (J ~ U[0, 10] ms in whole
microseconds: sigma = floor(15.625 us) << 6, tgsim_engine.cpp compile_shape) and the extreme ones."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def storm_sigmas():
    return sorted({int(us * 15.625) << 6 for us in range(0, 10_001)})


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler for scripts/fastmod_check.cpp"
    exe = tmp_path_factory.mktemp("fastmod") / "fastmod_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", str(exe), str(ROOT / "scripts" / "fastmod_check.cpp")], check=True)
    return exe


def run(exe, sigmas):
    r = subprocess.run([str(exe)], input="".join(f"{s}\n" for s in sigmas), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_storm_sigmas_exact(checker):
    sig = storm_sigmas()
    assert sig[0] == 0 and sig[-1] == 156_250 << 6
    out = run(checker, sig)
    assert out.startswith(f"ok: {len(sig) - 1} divisors")  # sigma 0 draws nothing


def test_extreme_sigmas_exact(checker):
    # the smallest moduli, a jitter without latency (microseconds taken as ticks), and the s32 ends
    # (2 sigma wraps modulo 2^32 as in delayed(): 0x7FFFFFFF -> 0xFFFFFFFE, 0xC0000000 -> 0x80000000)
    out = run(checker, [1, 2, 3, 64, 10_000 << 6, 0x3FFFFFFF, 0x40000000, 0x7FFFFFFF, 0xC0000000, 0xFFFFFFFF])
    assert out.startswith("ok: 10 divisors")
