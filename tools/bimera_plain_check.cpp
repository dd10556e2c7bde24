// tools/bimera_plain_check.cpp — dada2_amd/csrc/bimera_plain.h on its own: plain host C++, no HIP, no library.  Reads cases from
// standard input - "n min_fold min_parent_abund skip_zero stride" and then n * stride abundances, of which every stride-th is the
// row - and prints per case the ranking, P, the sum of P and the window ends for per = 1, 3 and 64.  tests/test_bimera_denovo.py
// builds it with the address and undefined-behaviour sanitizers and compares what it prints with the restatement of
// R/chimeras.R:127-128 in tests/bimera_denovo_cases.py.
#include <cstdio>
#include <cstdlib>

#include "../dada2_amd/csrc/bimera_plain.h"

int main() {
  int n, skip_zero, stride;
  double min_fold, min_par;
  int ncase = 0;
  while (std::scanf("%d %lf %lf %d %d", &n, &min_fold, &min_par, &skip_zero, &stride) == 5) {
    if (n < 0 || stride < 1) return 2;
    std::vector<int32_t> ab((size_t)n * (size_t)stride);
    for (int32_t &a : ab) if (std::scanf("%d", &a) != 1) return 2;
    BimeraRanking R;
    bimera_rank(n, ab.data(), stride, min_fold, min_par, skip_zero != 0, R);
    std::printf("rank");
    for (int32_t r : R.rank) std::printf(" %d", r);
    std::printf("\nP");
    for (int32_t p : R.P) std::printf(" %d", p);
    std::printf("\nsum %lld nquery %d max %d\n", (long long)R.pairs_possible, R.nquery, R.max_P);
    for (int per : {1, 3, 64}) {
      std::printf("windows %d:", per);
      for (int32_t r0 = 0; r0 < R.max_P;) { r0 = bimera_window_end(r0, per, R.max_P); std::printf(" %d", r0); }
      std::printf("\n");
    }
    ncase++;
  }
  std::printf("bimera_plain_check: %d cases\n", ncase);
  return 0;
}
