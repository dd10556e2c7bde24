// bimera_plain.h — the plain-C++ core of dada2hip_bimera_denovo (bimera_denovo_host.h; isBimeraDenovo, R/chimeras.R:105-154): no HIP,
// no host pool, no driver.cpp types.  The ranking of one row of abundances and, per query, how long a prefix of that ranking its
// parents are.  tools/bimera_plain_check.cpp includes this header alone.
//
// The parents of query j are `unqs > minFold * abund_j & unqs > minParentAbundance` (:127): a condition on the parent's abundance
// alone that only a larger abundance can meet.  With the sequences ranked by abundance, descending, the parents of j are therefore
// the ranks [0, P_j): no list of parents exists anywhere, on the host or on the device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

struct BimeraRanking {
  std::vector<int32_t> rank;   // rank r -> index of the sequence: abundance descending, ties by index ascending
  std::vector<int32_t> P;      // index j -> its parents are rank[0 .. P[j]); 0 where the reference answers FALSE without an alignment
  int64_t pairs_possible = 0;  // the sum of P
  int32_t nquery = 0, max_P = 0;   // entries of P that are not 0; the largest
};

// R's comparison of :127: the integer abundance as a double against the double product, strictly greater, twice
inline bool bimera_is_parent(int32_t a_parent, int32_t a_query, double min_fold, double min_parent_abund) {
  return (double)a_parent > min_fold * (double)a_query && (double)a_parent > min_parent_abund;
}

// abund[i * stride], i < n: one row of a column-major table (stride = its rows) or a vector (stride = 1).  skip_zero: a query of
// abundance 0 gets P = 0 (removeBimeraDenovo's "per-sample" zeroes those cells whatever their flag).
inline void bimera_rank(int32_t n, const int32_t *abund, ptrdiff_t stride, double min_fold, double min_parent_abund, bool skip_zero,
                        BimeraRanking &R) {
  R = BimeraRanking();
  R.rank.resize((size_t)std::max(n, 0));
  R.P.assign((size_t)std::max(n, 0), 0);
  for (int32_t i = 0; i < n; i++) R.rank[i] = i;
  auto ab = [&](int32_t i) { return abund[(ptrdiff_t)i * stride]; };
  std::sort(R.rank.begin(), R.rank.end(), [&](int32_t a, int32_t b) { return ab(a) > ab(b) || (ab(a) == ab(b) && a < b); });
  for (int32_t j = 0; j < n; j++) {
    const int32_t aj = ab(j);
    if (skip_zero && aj == 0) continue;
    int32_t lo = 0, hi = n;      // the first rank that is NOT a parent: the predicate is true on a prefix of the ranking
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo) / 2;
      if (bimera_is_parent(ab(R.rank[mid]), aj, min_fold, min_parent_abund)) lo = mid + 1;
      else hi = mid;
    }
    if (lo < 2) continue;        // length(pars) < 2 -> FALSE (:128)
    R.P[j] = lo;
    R.pairs_possible += lo;
    R.nquery++;
    R.max_P = std::max(R.max_P, lo);
  }
}

// The windows of parent ranks: the first is one chunk of `per` ranks, each later one four times as wide as the one before, none
// past `upto`.  Returns the end of the window that starts at r0 (r0 = 0: the first).
inline int32_t bimera_window_end(int32_t r0, int32_t per, int32_t upto) {
  const int64_t w = r0 == 0 ? (int64_t)per : 3 * (int64_t)r0;   // per, 4 per, 16 per, ...: the ends; the widths are 3 r0 behind the first
  return (int32_t)std::min<int64_t>((int64_t)upto, (int64_t)r0 + w);
}

}  // namespace
