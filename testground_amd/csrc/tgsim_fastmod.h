// tgsim_fastmod.h — remainder by a divisor that stays the same for many dividends (the tabledist
// modulus 2 sigma of a source): one division when the divisor is set, then a multiply-high, a
// multiply and one conditional subtraction per dividend.  Plain C++ (host and device).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TGSIM_HD __host__ __device__
#else
#define TGSIM_HD
#endif

namespace tgsim {

// rcp = floor((2^32 - 1) / m) for m >= 1 (0 for m = 0, which no caller divides by).
TGSIM_HD inline uint32_t fastmod_rcp(uint32_t m) { return m ? 0xFFFFFFFFu / m : 0u; }

// raw mod m for every 32-bit raw and every m >= 1, rcp = fastmod_rcp(m).
//   rcp < 2^32 / m, so q = floor(raw rcp / 2^32) <= floor(raw / m);
//   rcp >= (2^32 - 1 - (m - 1)) / m = 2^32 / m - 1, so raw rcp / 2^32 >= raw / m - raw / 2^32 > raw / m - 1,
//   hence q > raw / m - 2 and q >= floor(raw / m) - 1.
// The remainder raw - q m is raw mod m or m more, and at most raw: it neither wraps nor needs more
// than one subtraction.  scripts/fastmod_check.cpp compares it with % (tests/test_fastmod.py).
TGSIM_HD inline uint32_t fastmod_u32(uint32_t raw, uint32_t m, uint32_t rcp) {
  const uint32_t q = (uint32_t)(((uint64_t)raw * rcp) >> 32);
  const uint32_t r = raw - q * m;
  return r >= m ? r - m : r;
}

// floor(raw / m) from the same reciprocal: q above is the quotient or one less (same bounds), and the
// remainder tells which (the histogram bin of a hold time, k_gossip_spread).
TGSIM_HD inline uint32_t fastdiv_u32(uint32_t raw, uint32_t m, uint32_t rcp) {
  const uint32_t q = (uint32_t)(((uint64_t)raw * rcp) >> 32);
  return q + (raw - q * m >= m ? 1u : 0u);
}

}  // namespace tgsim
