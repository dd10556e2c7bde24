// tools/merge_plain_check.cpp — check program for the host's part of the run-level mergePairs (dada2_amd/csrc/merge_plain.h: the
// table's capacity, the checks of a sample's maps, the message for an index past a table, the reference's row order from the
// table's records, the chunk cutter, the scan of the accepted lengths, rc()) without a device: plain host C++ that includes the
// header alone and links nothing else, built with the sanitizers and run by tests/test_paired.py:
//   hipcc -O1 -g -std=c++17 -Wall -Xarch_host -fsanitize=address,undefined -x c++ tools/merge_plain_check.cpp -o merge_plain_check
//   merge_plain_check <sample file>
// The sample file: a line "<reads> <nuniqF> <nuniqR> <nclustF> <nclustR> <chunk>", the two derep maps (0-based, negative: NA) and
// the two dada maps (1-based, <= 0: NA) one per line, and a line of letters.  A stand-in for the device makes what the header is
// given: per read the gather and the range checks of k_mp_tally, the records of the distinct pairs in an order that has nothing
// to do with arrival (descending key), the largest entries of the derep maps.
// Output: "<capacity> <rows> <pairs NA>", per row "<forward> <reverse> <abundance> <first read>", the chunk ends on one line, the
// arena offsets on one line and the arena's size (a made-up verdict: a row is accepted when its abundance is odd, its merged
// sequence is forward + reverse letters long), the reverse complement of the letters.
// Exit status: 0; 2 = usage or a bad file; 3 = refused, with "error <code> <message>" printed.
#include "../dada2_amd/csrc/merge_plain.h"

#include <cstdio>
#include <cstdlib>
#include <map>

static int refuse(int code, const std::string &m) { printf("error %d %s\n", code, m.c_str()); return 3; }

static bool read_ints(FILE *f, long long n, std::vector<int32_t> &v) {
  v.resize((size_t)n);
  for (long long i = 0; i < n; i++)
    if (fscanf(f, "%d", &v[(size_t)i]) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: merge_plain_check <sample file>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  long long nreads = 0, chunk = 0;
  int nuniqF = 0, nuniqR = 0, nclustF = 0, nclustR = 0;
  std::vector<int32_t> derepF, derepR, dadaF, dadaR;
  char letters[4096] = "";
  const bool ok = fscanf(f, "%lld %d %d %d %d %lld", &nreads, &nuniqF, &nuniqR, &nclustF, &nclustR, &chunk) == 6 && nreads >= 0 && nreads < (1 << 24) &&
                  nuniqF >= 0 && nuniqR >= 0 && read_ints(f, nreads, derepF) && read_ints(f, nreads, derepR) && read_ints(f, nuniqF, dadaF) &&
                  read_ints(f, nuniqR, dadaR) && fscanf(f, "%4095s", letters) == 1;
  fclose(f);
  if (!ok) return 2;
  const std::string m = mp_check_sample(0, nreads, true, true, nuniqF, nuniqR, nclustF, nclustR);
  if (!m.empty()) return refuse(1, m);
  // ---- the stand-in for k_mp_tally and k_mp_compact ----
  std::map<unsigned long long, MpRec, std::greater<unsigned long long>> table;
  long long max_f = -1, max_r = -1, na = 0;
  for (long long i = 0; i < nreads; i++) {
    const int uf = derepF[(size_t)i], ur = derepR[(size_t)i];
    if (uf >= nuniqF) return refuse(1, mp_index_message(0, i, MP_BAD_DEREP_F, (long long)uf + 1, nuniqF));
    if (ur >= nuniqR) return refuse(1, mp_index_message(0, i, MP_BAD_DEREP_R, (long long)ur + 1, nuniqR));
    const int vf = uf >= 0 ? dadaF[(size_t)uf] : 0, vr = ur >= 0 ? dadaR[(size_t)ur] : 0;
    if (vf > nclustF) return refuse(1, mp_index_message(0, i, MP_BAD_DADA_F, vf, nclustF));
    if (vr > nclustR) return refuse(1, mp_index_message(0, i, MP_BAD_DADA_R, vr, nclustR));
    max_f = std::max<long long>(max_f, uf < 0 ? -1 : uf); max_r = std::max<long long>(max_r, ur < 0 ? -1 : ur);
    if (vf <= 0 || vr <= 0) { na++; continue; }
    const unsigned long long key = ((unsigned long long)(unsigned)vf << 32) | (unsigned long long)(unsigned)vr;
    auto it = table.find(key);
    if (it == table.end()) table.emplace(key, MpRec{key, 1, (int32_t)i});
    else it->second.count++;
  }
  const std::string mm = mp_check_maps(0, max_f, nuniqF, max_r, nuniqR);
  if (!mm.empty()) return refuse(1, mm);
  std::vector<MpRec> rec;
  for (const auto &kv : table) rec.push_back(kv.second);
  std::vector<int32_t> order;
  if (!mp_order(rec.data(), rec.size(), nreads, order)) return refuse(5, "the records are no table's output");
  printf("%lld %zu %lld\n", mp_capacity(nreads, nclustF, nclustR), rec.size(), na);
  std::vector<int32_t> accept, mlen;
  for (int32_t k : order) {
    const MpRec &r = rec[(size_t)k];
    const int fwd = (int)(r.key >> 32), rev = (int)(r.key & 0xFFFFFFFFull);
    printf("%d %d %d %d\n", fwd, rev, r.count, r.first);
    accept.push_back(r.count & 1); mlen.push_back(fwd + rev);
  }
  for (size_t p0 = 0; p0 < rec.size(); p0 = mp_next_chunk(p0, rec.size(), (size_t)chunk)) printf("%zu ", mp_next_chunk(p0, rec.size(), (size_t)chunk));
  printf("\n");
  std::vector<long long> off;
  const long long total = mp_scan_accepted(rec.size(), accept.data(), mlen.data(), off);
  for (long long o : off) printf("%lld ", o);
  printf("\n%lld\n", total);
  const std::string s(letters);
  printf("%s %d\n", mp_revcomp(s.data(), s.size()).c_str(), (int)mp_is_acgt(s.data(), s.size()));
  return 0;
}
