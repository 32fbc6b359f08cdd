// Stand-alone check of tgsim_fastmod.h against the % operator (host code only).
//   fastmod_check [--full] SIGMA...      (or the sigmas, one per line, on standard input)
// For every sigma (the tabledist sigma of a source; the modulus is 2 sigma) it compares
// fastmod_u32(raw, m, rcp) with raw % m at the dividends where a quotient estimate can go wrong:
// every multiple of m with its two neighbours on each side (at most the first and the last 4096
// multiples below 2^32 without --full, all of them with it), the ends of the range, and 4096
// pseudo-random dividends.  --full also runs all 2^32 dividends for the smallest and the largest
// sigma given, and the boundary dividends for divisors spread over the whole 32-bit range (powers
// of two and their neighbours, divisors above 2^31).  Exit status 0 and "ok ..." when all agree.
// build: c++ -O2 -std=c++17 -fsanitize=undefined,address -o fastmod_check scripts/fastmod_check.cpp
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../testground_amd/csrc/tgsim_fastmod.h"

static uint64_t n_checked = 0;

static bool check(uint32_t raw, uint32_t m, uint32_t rcp) {
  ++n_checked;
  const uint32_t got = tgsim::fastmod_u32(raw, m, rcp), want = raw % m;
  if (got != want) {
    fprintf(stderr, "mismatch: raw %u mod %u: fastmod %u, %% %u\n", raw, m, got, want);
    return false;
  }
  return true;
}

static bool around(uint64_t c, uint32_t m, uint32_t rcp) {
  for (int64_t d = -2; d <= 2; ++d) {
    const int64_t v = (int64_t)c + d;
    if (v < 0 || v > 0xFFFFFFFFll) continue;
    if (!check((uint32_t)v, m, rcp)) return false;
  }
  return true;
}

static bool check_divisor(uint32_t m, bool full) {
  const uint32_t rcp = tgsim::fastmod_rcp(m);
  const uint64_t n_mult = (0xFFFFFFFFull / m) + 1;  // multiples k m <= 2^32 - 1, k = 0 ..
  const uint64_t head = full ? n_mult : (n_mult < 4096 ? n_mult : 4096);
  for (uint64_t k = 0; k < head; ++k)
    if (!around(k * m, m, rcp)) return false;
  for (uint64_t k = n_mult > 4096 && !full ? n_mult - 4096 : n_mult; k <= n_mult; ++k)
    if (!around(k * m, m, rcp)) return false;
  if (!around(0, m, rcp) || !around(0xFFFFFFFFull, m, rcp) || !around(0x80000000ull, m, rcp)) return false;
  uint64_t x = 0x9E3779B97F4A7C15ull ^ m;
  for (int i = 0; i < 4096; ++i) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    if (!check((uint32_t)(x >> 16), m, rcp)) return false;
  }
  return true;
}

static bool check_all_dividends(uint32_t m) {
  const uint32_t rcp = tgsim::fastmod_rcp(m);
  uint32_t want = 0;  // raw % m, kept incrementally
  for (uint64_t raw = 0; raw <= 0xFFFFFFFFull; ++raw) {
    if (tgsim::fastmod_u32((uint32_t)raw, m, rcp) != want) {
      fprintf(stderr, "mismatch: raw %llu mod %u\n", (unsigned long long)raw, m);
      return false;
    }
    if (++want == m) want = 0;
  }
  n_checked += 1ull << 32;
  return true;
}

int main(int argc, char** argv) {
  bool full = false;
  std::vector<uint32_t> sigmas;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--full")) full = true;
    else sigmas.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
  }
  if (sigmas.empty()) {
    char line[64];
    while (fgets(line, sizeof line, stdin))
      if (line[0] >= '0' && line[0] <= '9') sigmas.push_back((uint32_t)strtoul(line, nullptr, 10));
  }
  uint32_t lo = 0, hi = 0;
  size_t n_div = 0;
  for (uint32_t sg : sigmas) {
    const uint32_t m = 2u * sg;  // as delayed() forms it
    if (!m) continue;            // sigma 0: no draw
    if (!check_divisor(m, full)) return 1;
    lo = !lo || m < lo ? m : lo;
    hi = m > hi ? m : hi;
    ++n_div;
  }
  if (full) {
    if (lo && !check_all_dividends(lo)) return 1;
    if (hi && hi != lo && !check_all_dividends(hi)) return 1;
    for (uint32_t b = 0; b < 32; ++b)
      for (int64_t d = -3; d <= 3; ++d) {
        const int64_t m = (1ll << b) + d;
        if (m >= 1 && m <= 0xFFFFFFFFll && !check_divisor((uint32_t)m, m > 4096)) return 1;
      }
    for (uint32_t m : {0xFFFFFFFFu, 0xFFFFFFFEu, 0xC0000001u, 0xAAAAAAABu, 0x80000001u, 3u, 5u, 7u, 641u, 6700417u})
      if (!check_divisor(m, m > 4096)) return 1;
  }
  printf("ok: %zu divisors (2 sigma from %u to %u), %llu dividends compared\n", n_div, lo, hi,
         (unsigned long long)n_checked);
  return 0;
}
