// tools/pool_plain_check.cpp — check program for the plain-C++ core of dada2hip_derep_combine (dada2_amd/csrc/pool_plain.h): the
// union of the samples' uniques, the contributors of every pooled unique, the stable order by decreasing abundance and the
// renumbering.  No HIP, no library; meant to be built with the sanitizers:
//   hipcc -O1 -g -std=c++17 -Wall -Xarch_host -fsanitize=address,undefined -x c++ tools/pool_plain_check.cpp -o pool_plain_check
//   pool_plain_check [hand|drawn]      (neither: both)
// Exit status: 0 = every property holds ("pool_plain_check: ok"), 1 = one does not (the first is printed), 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "../dada2_amd/csrc/pool_plain.h"

namespace {

[[noreturn]] void fail(const char *what, long a = 0, long b = 0, long c = 0) {
  printf("pool_plain_check: FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
  exit(1);
}

struct Sample {
  std::vector<std::string> seqs;
  std::vector<int32_t> abund;
  std::vector<const char *> ptr;
  std::vector<uint32_t> len;
  std::vector<uint64_t> hash;
};

// weak: every sequence of one length hashes alike, so the table has to tell them apart by their bytes
PoolSample view(Sample &s, bool weak) {
  s.ptr.clear(); s.len.clear(); s.hash.clear();
  for (const std::string &x : s.seqs) {
    s.ptr.push_back(x.c_str());
    s.len.push_back((uint32_t)x.size());
    uint64_t h = 1469598103934665603ull;
    if (!weak) for (char c : x) h = (h ^ (unsigned char)c) * 1099511628211ull;
    s.hash.push_back(weak ? (uint64_t)x.size() : h);
  }
  PoolSample v;
  v.n = (int32_t)s.seqs.size(); v.seqs = s.ptr.data(); v.len = s.len.data(); v.hash = s.hash.data(); v.abund = s.abund.data();
  return v;
}

// the plan of `samples` against a restatement over std::map and std::stable_sort
void check_plan(std::vector<Sample> &samples, bool weak) {
  std::vector<PoolSample> V;
  for (Sample &s : samples) V.push_back(view(s, weak));
  PoolPlan P;
  int32_t bs = -1, bj = -1;
  if (pool_group((int32_t)V.size(), V.data(), P, &bs, &bj) != POOL_OK) fail("a valid input is refused", bs, bj);
  std::map<std::string, int> pos;
  std::vector<std::string> names;
  std::vector<int64_t> total;
  std::vector<int32_t> flat;
  for (const Sample &s : samples)
    for (size_t j = 0; j < s.seqs.size(); j++) {
      auto it = pos.emplace(s.seqs[j], (int)names.size());
      if (it.second) { names.push_back(s.seqs[j]); total.push_back(0); }
      total[it.first->second] += s.abund[j];
      flat.push_back(it.first->second);
    }
  if (P.npool != (int32_t)names.size()) fail("the number of pooled uniques", P.npool, (long)names.size());
  for (int32_t p = 0; p < P.npool; p++) {
    if (samples[P.src_sample[p]].seqs[P.src_index[p]] != names[p]) fail("first-appearance order", p);
    if (P.total[p] != total[p]) fail("a summed abundance", p, (long)P.total[p], (long)total[p]);
    int32_t last = -1;
    int64_t sum = 0;
    if (P.contrib_off[p + 1] <= P.contrib_off[p]) fail("a pooled unique without a contributor", p);
    for (int64_t c = P.contrib_off[p]; c < P.contrib_off[p + 1]; c++) {
      if (P.contrib_sample[c] <= last) fail("contributors out of sample order", p, (long)c);
      last = P.contrib_sample[c];
      if (samples[last].seqs[P.contrib_index[c]] != names[p]) fail("a contributor holds another sequence", p, (long)c);
      sum += samples[last].abund[P.contrib_index[c]];
    }
    if (sum != total[p]) fail("the contributors do not add up", p);
  }
  if (P.contrib_off[P.npool] != (int64_t)flat.size()) fail("the contributor list's length");
  for (size_t i = 0; i < flat.size(); i++) if (P.to_pool[i] != flat[i]) fail("to_pool before ordering", (long)i);
  pool_order(P, [](int32_t *f, size_t n, auto less) { std::sort(f, f + n, less); });
  std::vector<int32_t> ord(names.size());
  for (size_t p = 0; p < ord.size(); p++) ord[p] = (int32_t)p;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return total[a] > total[b]; });
  for (size_t k = 0; k < ord.size(); k++) if (P.order[k] != ord[k]) fail("the stable order by decreasing abundance", (long)k, P.order[k], ord[k]);
  for (size_t i = 0; i < flat.size(); i++) if (P.order[P.to_pool[i]] != flat[i]) fail("to_pool after ordering", (long)i);
  // a map through one sample's piece of to_pool
  const int32_t NA = INT32_MIN;
  size_t first = 0;
  for (const Sample &s : samples) {
    const int32_t n = (int32_t)s.seqs.size(), *tp = P.to_pool.data() + first;
    int32_t out = 7;
    if (!pool_map_entry(NA, tp, n, NA, &out) || out != NA) fail("NA does not stay NA");
    for (int32_t j = 0; j < n; j++) if (!pool_map_entry(j, tp, n, NA, &out) || out != tp[j]) fail("a map entry", j);
    if (pool_map_entry(n, tp, n, NA, &out) || pool_map_entry(-1, tp, n, NA, &out)) fail("a map entry that names no unique is taken");
    first += (size_t)n;
  }
}

long check_hand() {
  // three samples: AAAA in all, CCCC in the first and last only, the rest in one; ties: GGGG (3) is seen before TTTT (1 + 2 = 3)
  std::vector<Sample> S(3);
  S[0].seqs = {"AAAA", "CCCC", "GGGG", "TTTT"}; S[0].abund = {5, 2, 3, 1};
  S[1].seqs = {"ACGT", "AAAA", "TTTT", "AAAAA"}; S[1].abund = {9, 1, 2, 3};
  S[2].seqs = {"CCCC", "AAAA", "AAA"}; S[2].abund = {1, 3, 3};
  for (int weak = 0; weak < 2; weak++) {
    check_plan(S, weak != 0);
    std::vector<PoolSample> V;
    for (Sample &s : S) V.push_back(view(s, weak != 0));
    PoolPlan P;
    int32_t bs, bj;
    pool_group(3, V.data(), P, &bs, &bj);
    pool_order(P, [](int32_t *f, size_t n, auto less) { std::sort(f, f + n, less); });
    // totals: AAAA 9, CCCC 3, GGGG 3, TTTT 3, ACGT 9, AAAAA 3, AAA 3 -> AAAA, ACGT, CCCC, GGGG, TTTT, AAAAA, AAA
    static const int32_t want_order[7] = {0, 4, 1, 2, 3, 5, 6}, want_to[11] = {0, 2, 3, 4, 1, 0, 4, 5, 2, 0, 6};
    for (int k = 0; k < 7; k++) if (P.order[k] != want_order[k]) fail("hand-made order", k, P.order[k]);
    for (int i = 0; i < 11; i++) if (P.to_pool[i] != want_to[i]) fail("hand-made unique_to_pool", i, P.to_pool[i]);
  }
  // a sample that holds one sequence twice; an abundance sum past the integer range
  std::vector<Sample> D(2);
  D[0].seqs = {"AAAA", "CCCC"}; D[0].abund = {1, 1};
  D[1].seqs = {"CCCC", "GG", "CCCC"}; D[1].abund = {1, 1, 1};
  {
    std::vector<PoolSample> V{view(D[0], false), view(D[1], false)};
    PoolPlan P;
    int32_t bs = -1, bj = -1;
    if (pool_group(2, V.data(), P, &bs, &bj) != POOL_DUPLICATE || bs != 1 || bj != 2) fail("a duplicate inside a sample is not found", bs, bj);
  }
  D[1].seqs = {"CCCC", "GG"}; D[1].abund = {INT32_MAX, INT32_MAX};
  {
    std::vector<PoolSample> V{view(D[0], false), view(D[1], false)};
    PoolPlan P;
    int32_t bs = -1, bj = -1;
    if (pool_group(2, V.data(), P, &bs, &bj) != POOL_OVERFLOW || bs != 1 || bj != 0) fail("an abundance sum past INT32_MAX is not found", bs, bj);
    D[0].abund = {1, 0};                                          // exactly INT32_MAX is a valid sum
    V[0] = view(D[0], false);
    if (pool_group(2, V.data(), P, &bs, &bj) != POOL_OK || P.total[1] != INT32_MAX) fail("a sum of exactly INT32_MAX is refused");
  }
  // no samples, and samples without uniques
  {
    PoolPlan P;
    int32_t bs, bj;
    if (pool_group(0, nullptr, P, &bs, &bj) != POOL_OK || P.npool != 0) fail("no samples");
    std::vector<Sample> E(2);
    check_plan(E, false);
  }
  return 5;
}

long check_drawn() {
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  auto next = [&](uint32_t m) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 33) % m; };
  long cases = 0;
  for (int rep = 0; rep < 300; rep++) {
    const int ns = 1 + (int)next(5);
    std::vector<Sample> S((size_t)ns);
    for (Sample &s : S) {
      const int n = (int)next(40);
      std::map<std::string, int> seen;
      while ((int)s.seqs.size() < n) {                          // short sequences over two letters: many are shared between samples
        std::string x;
        const int l = 1 + (int)next(5);
        for (int i = 0; i < l; i++) x.push_back("AC"[next(2)]);
        if (seen.emplace(x, 0).second) { s.seqs.push_back(x); s.abund.push_back((int32_t)next(4)); }
      }
    }
    check_plan(S, (rep & 1) != 0);
    cases++;
  }
  return cases;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  if (argc > 2 || (which != "" && which != "hand" && which != "drawn")) { printf("usage: pool_plain_check [hand|drawn]\n"); return 2; }
  long cases = 0;
  if (which != "drawn") cases += check_hand();
  if (which != "hand") cases += check_drawn();
  printf("pool_plain_check: ok (%ld cases)\n", cases);
  return 0;
}
