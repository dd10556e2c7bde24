// pool_plain.h — the plain-C++ core of dada2hip_derep_combine (derep.cpp; combineDereps2, R/multiSample.R:165-203): no HIP, no
// host pool, no driver.cpp types.  The union of the samples' uniques in order of first appearance, the contributors of every
// pooled unique in sample order, the stable order by decreasing abundance and the renumbering of the per-sample indices.
// derep.cpp adds the hashes, the quality rows and the threads; tools/pool_plain_check.cpp includes this header alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {

// One sample as the grouping sees it: its uniques, their lengths and hashes (any function of the bytes: equal sequences must
// hash alike, nothing else is asked of it) and their abundances.
struct PoolSample {
  int32_t n = 0;
  const char *const *seqs = nullptr;
  const uint32_t *len = nullptr;
  const uint64_t *hash = nullptr;
  const int32_t *abund = nullptr;
};

struct PoolPlan {
  int32_t npool = 0;
  std::vector<int32_t> src_sample, src_index;   // per pooled unique, in order of first appearance: where its sequence stands
  std::vector<int64_t> total;                   // ... its summed abundance
  std::vector<int64_t> contrib_off;             // ... its contributors contrib[contrib_off[p] .. contrib_off[p + 1]), in sample order
  std::vector<int32_t> contrib_sample, contrib_index;
  std::vector<int32_t> to_pool;                 // the samples' uniques one sample after the other -> pooled index (pool_order: -> output row)
  std::vector<int32_t> order;                   // output row -> pooled unique (pool_order)
};

enum { POOL_OK = 0, POOL_DUPLICATE = 1, POOL_OVERFLOW = 2 };

// The union.  POOL_DUPLICATE: sample *bad_sample holds the sequence of its unique *bad_index twice.  POOL_OVERFLOW: a summed
// abundance passes INT32_MAX (R's integer sum would be NA).
inline int pool_group(int32_t nsamples, const PoolSample *S, PoolPlan &P, int32_t *bad_sample, int32_t *bad_index) {
  size_t nall = 0;
  for (int32_t s = 0; s < nsamples; s++) nall += (size_t)S[s].n;
  P = PoolPlan();
  P.to_pool.resize(nall);
  size_t cap = 16;
  while (cap < 2 * nall + 2) cap <<= 1;
  std::vector<int32_t> slot(cap, -1);                           // open addressing: a pooled index, or -1
  std::vector<int32_t> last_sample;                             // per pooled unique: the last sample that contributed
  std::vector<int32_t> ncontrib;
  size_t at = 0;
  for (int32_t s = 0; s < nsamples; s++) {
    const PoolSample &A = S[s];
    for (int32_t j = 0; j < A.n; j++, at++) {
      size_t h = (size_t)A.hash[j] & (cap - 1);
      int32_t p = -1;
      for (;; h = (h + 1) & (cap - 1)) {
        p = slot[h];
        if (p < 0) break;
        const PoolSample &B = S[P.src_sample[p]];
        const int32_t k = P.src_index[p];
        if (B.hash[k] == A.hash[j] && B.len[k] == A.len[j] && memcmp(B.seqs[k], A.seqs[j], A.len[j]) == 0) break;
      }
      if (p < 0) {
        p = (int32_t)P.src_sample.size();
        slot[h] = p;
        P.src_sample.push_back(s); P.src_index.push_back(j); P.total.push_back(0); last_sample.push_back(-1); ncontrib.push_back(0);
      }
      if (last_sample[p] == s) { *bad_sample = s; *bad_index = j; return POOL_DUPLICATE; }
      last_sample[p] = s;
      P.total[p] += (int64_t)A.abund[j];
      if (P.total[p] > (int64_t)INT32_MAX) { *bad_sample = s; *bad_index = j; return POOL_OVERFLOW; }
      ncontrib[p]++;
      P.to_pool[at] = p;
    }
  }
  P.npool = (int32_t)P.src_sample.size();
  // the contributors, a counting sort of (sample, unique) by pooled index: inside a pooled unique they stay in sample order
  P.contrib_off.assign((size_t)P.npool + 1, 0);
  for (int32_t p = 0; p < P.npool; p++) P.contrib_off[p + 1] = P.contrib_off[p] + ncontrib[p];
  P.contrib_sample.resize(nall); P.contrib_index.resize(nall);
  std::vector<int64_t> fill(P.contrib_off.begin(), P.contrib_off.end() - 1);
  at = 0;
  for (int32_t s = 0; s < nsamples; s++)
    for (int32_t j = 0; j < S[s].n; j++, at++) {
      const int64_t k = fill[P.to_pool[at]]++;
      P.contrib_sample[k] = s; P.contrib_index[k] = j;
    }
  return POOL_OK;
}

// order(total, decreasing = TRUE), stable: (total descending, first appearance ascending) is a strict order, so `sort` may be any
// correct sort of distinct elements - sort(first, n, less).  Renumbers to_pool to the output rows.
template <typename Sort>
inline void pool_order(PoolPlan &P, Sort &&sort) {
  P.order.resize((size_t)P.npool);
  for (int32_t p = 0; p < P.npool; p++) P.order[p] = p;
  const int64_t *tot = P.total.data();
  sort(P.order.data(), (size_t)P.npool, [tot](int32_t a, int32_t b) { return tot[a] > tot[b] || (tot[a] == tot[b] && a < b); });
  std::vector<int32_t> rank((size_t)P.npool);
  for (int32_t k = 0; k < P.npool; k++) rank[P.order[k]] = k;
  for (int32_t &t : P.to_pool) t = rank[t];
}

// One read's entry of a sample's map through that sample's piece of to_pool: NA stays NA; false = the entry names no unique.
inline bool pool_map_entry(int32_t m, const int32_t *to_pool, int32_t nuniques, int32_t na, int32_t *out) {
  if (m == na) { *out = na; return true; }
  if (m < 0 || m >= nuniques) return false;
  *out = to_pool[m];
  return true;
}

}  // namespace
