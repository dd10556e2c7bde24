// tools/derep_resident_plain_check.cpp — check program for the integer rounding of a resident sample's quality bytes
// (dada2_amd/csrc/derep_resident_plain.h) against the rule on doubles that the host route applies: plain host C++ that includes
// the header alone and links nothing else, built with the sanitizers and run by tests/test_derep_resident.py:
//   hipcc -O1 -g -std=c++17 -Wall -Xarch_host -fsanitize=address,undefined -x c++ tools/derep_resident_plain_check.cpp -o derep_resident_plain_check
//   derep_resident_plain_check [random draws, default 10000000]
// The double rule is written out below as the host has it: the division of dd_quality_row (derep_dev_plain.h), the branch-free
// sweep of round_one and, for a value the sweep refuses, the exact scalar rule of marshal_rows (both hostsimd.cpp); the ceiling
// is ceil() of the same quotient (api.NativeDerep.qmax).  Compared value by value:
//   * every n in 1 .. 2 048 with every T in [-n, 95 n], and with every T in [254 n, 257 n] (the upper end of a byte);
//   * random (T, n), n up to 2^31 - 1 and T in [-n, 256 n], and for an even n also a tie T = k n + n / 2 with a random k;
//   * 4 096 random even n with the tie of every k in -1 .. 255.
// Output: the counts, and "ok"; the first disagreement is printed and the exit status is 1.
#include "../dada2_amd/csrc/derep_resident_plain.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

// marshal_rows on one value: the byte, or -1 for bad_qual
static int double_rule(int64_t T, int64_t n) {
  const double x = (double)T / (double)n;
  int ok = (int)(x >= 0.0) & (int)(x < 255.5);                     // round_one
  if (ok) {
    const int t = (int)x;
    return t + (int)((x - (double)t) >= 0.5);
  }
  double xr;                                                       // the row redone by the exact scalar rule
  if (x >= 0.0 && x < 256.0) { const int v = (int)x; xr = (double)(v + ((x - (double)v) >= 0.5 ? 1 : 0)); }
  else xr = std::round(x);
  if (!(xr >= 0.0 && xr <= 255.0)) return -1;
  return (int)xr;
}

static long long checked = 0;

static bool agree(int64_t T, int64_t n) {
  checked++;
  const int a = dr_round_byte(T, n), b = double_rule(T, n);
  const int64_t c = dr_ceil_mean(T, n);
  const double d = std::ceil((double)T / (double)n);
  if (a == b && (double)c == d) return true;
  printf("DISAGREE T = %lld n = %lld: byte %d (integers) %d (doubles), ceiling %lld (integers) %.17g (doubles)\n", (long long)T, (long long)n, a, b,
         (long long)c, d);
  return false;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                            // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char **argv) {
  const long long draws = argc > 1 ? atoll(argv[1]) : 10000000ll;
  for (int64_t n = 1; n <= 2048; n++) {
    for (int64_t T = -n; T <= 95 * n; T++) if (!agree(T, n)) return 1;
    for (int64_t T = 254 * n; T <= 257 * n; T++) if (!agree(T, n)) return 1;
  }
  const long long exhaustive = checked;
  long long ties = 0;
  for (long long i = 0; i < draws; i++) {
    // (a third of the draws from small n, where a count is likely to lie; the rest over the whole range)
    const int64_t n = 1 + (int64_t)(rnd() % (i % 3 == 0 ? 65536ull : 0x7FFFFFFFull));
    const int64_t T = (int64_t)(rnd() % (uint64_t)(257 * n + 1)) - n;
    if (!agree(T, n)) return 1;
    if ((n & 1) == 0) {
      const int64_t k = (int64_t)(rnd() % 257) - 1;
      ties++;
      if (!agree(k * n + n / 2, n)) return 1;
    }
  }
  for (int i = 0; i < 4096; i++) {
    const int64_t n = 2 * (1 + (int64_t)(rnd() % 0x3FFFFFFFull));
    for (int64_t k = -1; k <= 255; k++) {
      ties++;
      if (!agree(k * n + n / 2, n)) return 1;
    }
  }
  printf("exhaustive %lld random %lld ties %lld\nok\n", exhaustive, draws, ties);
  return 0;
}
