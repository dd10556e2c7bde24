// tools/derep_dev_plain_check.cpp — check program for the finalisation of the device dereplicator (dada2_amd/csrc/
// derep_dev_plain.h: derepFastq's order, the means, the map's renumbering) without a device: plain host C++ that includes the
// header alone and links nothing else, built with the sanitizers and run by tests/test_derep_dev.py:
//   hipcc -O1 -g -std=c++17 -Wall -Xarch_host -fsanitize=address,undefined -x c++ tools/derep_dev_plain_check.cpp -o derep_dev_plain_check
//   derep_dev_plain_check <reads file>
// The reads file: a line "<reads> <chunk_reads> <qual_offset>", then per read a line of letters and a line of quality characters
// (both empty for a zero-length read).  A stand-in for the device makes the rows: the uniques numbered in an order that has
// nothing to do with arrival or with their letters (descending hash), the arena laid out in that order, the raw quality
// characters summed in 64-bit words, the smallest read index kept, the smallest quality character of the first chunk noted.
// Output: "<uniques> <maxlen> <reads> <offset>", per unique "<abundance> <letters>" and a line of the row's doubles as 16 hex
// digits each, then the map.  Exit status: 0, 2 = usage or a bad file, 3 = "Only zero-length sequences ..." (printed).
#include "../dada2_amd/csrc/derep_dev_plain.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <unordered_map>

static bool read_line(FILE *f, std::string &s) {
  s.clear();
  int c;
  while ((c = fgetc(f)) != EOF && c != '\n') s.push_back((char)c);
  return c != EOF || !s.empty();
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: derep_dev_plain_check <reads file>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string line;
  long long n = 0, chunk = 0;
  int qual_offset = 0;
  if (!read_line(f, line) || sscanf(line.c_str(), "%lld %lld %d", &n, &chunk, &qual_offset) != 3 || n < 0 || chunk <= 0) { fclose(f); return 2; }
  std::vector<std::string> seqs((size_t)n), quals((size_t)n);
  for (long long i = 0; i < n; i++) {
    read_line(f, seqs[(size_t)i]);
    read_line(f, quals[(size_t)i]);
    if (seqs[(size_t)i].size() != quals[(size_t)i].size()) { fclose(f); fprintf(stderr, "read %lld: lengths differ\n", i + 1); return 2; }
  }
  fclose(f);
  // ---- the stand-in for the device ----
  std::unordered_map<std::string, int32_t> seen;
  std::vector<const std::string *> uniq;
  for (const std::string &s : seqs)
    if (!s.empty() && seen.emplace(s, 0).second) uniq.push_back(&s);
  std::sort(uniq.begin(), uniq.end(), [](const std::string *a, const std::string *b) {
    const size_t ha = std::hash<std::string>()(*a), hb = std::hash<std::string>()(*b);
    return ha != hb ? ha > hb : *a > *b;
  });
  const size_t U = uniq.size();
  std::vector<int64_t> off(U), count(U, 0), first(U, INT64_MAX);
  std::vector<int32_t> len(U);
  std::vector<uint8_t> bytes;
  for (size_t u = 0; u < U; u++) {
    seen[*uniq[u]] = (int32_t)u;
    off[u] = (int64_t)bytes.size(); len[u] = (int32_t)uniq[u]->size();
    bytes.insert(bytes.end(), uniq[u]->begin(), uniq[u]->end());
  }
  std::vector<uint64_t> sums(bytes.size(), 0);
  std::vector<int32_t> ruid((size_t)n, -1);
  int min_char = 255;
  for (long long i = 0; i < n; i++) {
    const std::string &s = seqs[(size_t)i], &q = quals[(size_t)i];
    if (s.empty()) continue;
    const int32_t u = seen[s];
    ruid[(size_t)i] = u;
    count[(size_t)u]++;
    first[(size_t)u] = std::min<int64_t>(first[(size_t)u], i);
    for (size_t p = 0; p < q.size(); p++) {
      sums[(size_t)off[(size_t)u] + p] += (unsigned char)q[p];
      if (i < chunk) min_char = std::min(min_char, (int)(unsigned char)q[p]);
    }
  }
  // ---- the header under test ----
  DdRows R;
  R.nuniq = (int64_t)U; R.off = off.data(); R.len = len.data(); R.count = count.data(); R.first = first.data(); R.bytes = bytes.data();
  R.sums = sums.data();
  DdPlan P;
  const int rc = dd_order(R, chunk, P, [](int32_t *b, size_t m, auto less) { std::sort(b, b + m, less); });
  if (rc == DDP_NONE) { printf("Only zero-length sequences detected during dereplication.\n"); return 3; }
  if (rc != DDP_OK) { printf("overflow\n"); return 2; }
  const int offset = dd_offset(qual_offset, min_char);
  union { double d; uint64_t u; } na;
  na.u = 0x7FF00000000007A2ull;
  printf("%zu %d %lld %d\n", U, (int)P.maxlen, n, offset);
  std::vector<double> row((size_t)P.maxlen);
  for (size_t k = 0; k < U; k++) {
    const int32_t u = P.order[k];
    printf("%lld %.*s\n", (long long)count[(size_t)u], (int)len[(size_t)u], (const char *)bytes.data() + off[(size_t)u]);
    dd_quality_row(R, u, offset, P.maxlen, na.d, row.data());
    for (int32_t p = 0; p < P.maxlen; p++) {
      uint64_t bits;
      memcpy(&bits, &row[(size_t)p], 8);
      printf("%016llx", (unsigned long long)bits);
    }
    printf("\n");
  }
  for (long long i = 0; i < n; i++) printf("%d%c", (int)dd_map_entry(ruid[(size_t)i], P, -1), i + 1 < n ? ' ' : '\n');
  if (n == 0) printf("\n");
  return 0;
}
