// tools/stage_plain_check.cpp — check program for the plain-C++ parts of the stages' shared host layer
// (dada2_amd/csrc/stage_plain.h): the piece cutter of the two-slot read pipeline and the prefix keys of collapseNoMismatch's join
// and assignSpecies' seed.  No HIP, no library:
//   hipcc -O2 -std=c++17 -Wall -x c++ tools/stage_plain_check.cpp -o stage_plain_check
//   stage_plain_check [pieces|keys]      (neither: both)
// Exit status: 0 = every property holds ("stage_plain_check: ok"), 1 = one does not (the first is printed), 2 = usage.
#include <cstdio>
#include <cstdlib>

#include "../dada2_amd/csrc/stage_plain.h"

namespace {

[[noreturn]] void fail(const char *what, long a = 0, long b = 0, long c = 0) {
  printf("stage_plain_check: FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
  exit(1);
}

// ---- next_piece: the pieces of every vector of 0..9 reads with lengths in {0, 1, 7, 8, 9}, under every pair of limits ----
void check_pieces(const std::vector<int64_t> &off, int64_t max_reads, int64_t max_bytes) {
  const int64_t n = (int64_t)off.size() - 1;
  int64_t r0 = 0;
  while (r0 < n) {
    const int64_t r1 = next_piece(off.data(), n, r0, max_reads, max_bytes);
    if (r1 <= r0) fail("an empty piece", n, r0, r1);
    if (r1 > n) fail("a piece runs past the last read", n, r0, r1);
    if (r1 - r0 > max_reads) fail("a piece exceeds the read limit", n, r0, r1);
    if (off[r1] - off[r0] > max_bytes && r1 - r0 != 1) fail("a piece of several reads exceeds the byte limit", n, r0, r1);
    // (and it ends for a reason: the reads are out, the read limit is reached, or the next read would not fit)
    if (r1 < n && r1 - r0 < max_reads && off[r1 + 1] - off[r0] <= max_bytes) fail("a piece ends early", n, r0, r1);
    r0 = r1;                                                    // in order, each piece starting where the one before ended
  }
  if (r0 != n) fail("the pieces do not tile [0, n)", n, r0);
}

long check_all_pieces() {
  static const int64_t LEN[5] = {0, 1, 7, 8, 9}, READS[3] = {1, 2, 3}, BYTES[4] = {1, 8, 9, 64};
  long cases = 0;
  uint64_t lcg = 0x2545F4914F6CDD1Dull;
  for (int n = 0; n <= 9; n++) {
    // every vector up to 7 reads (5^7 = 78 125); 20 000 drawn ones of 8 and of 9 reads
    long nvec = 1;
    for (int i = 0; i < n; i++) nvec *= 5;
    const bool all = n <= 7;
    if (!all) nvec = 20000;
    std::vector<int64_t> off(n + 1, 0);
    for (long v = 0; v < nvec; v++) {
      long code = v;
      for (int i = 0; i < n; i++) {
        int pick;
        if (all) { pick = (int)(code % 5); code /= 5; }
        else { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; pick = (int)((lcg >> 33) % 5); }
        off[i + 1] = off[i] + LEN[pick];
      }
      for (int64_t mr : READS) for (int64_t mb : BYTES) { check_pieces(off, mr, mb); cases++; }
    }
  }
  // offsets that do not start at 0 (a call on the middle of a blob)
  const std::vector<int64_t> shifted = {100, 107, 107, 116, 117, 125};
  for (int64_t mr : READS) for (int64_t mb : BYTES) { check_pieces(shifted, mr, mb); cases++; }
  return cases;
}

// ---- prefix keys ----
int base_of(int pattern, int i) {
  switch (pattern) {
    case 0: return i % 4;
    case 1: return (i * i + 1) % 4;
    case 2: return 3;                                           // all T: every bit of the key set, the mask's worst case
    case 3: return (i / 3) % 4;
    case 4: return i == 35 ? 2 : i % 4;                         // pattern 0 up to base 34: equal in the first 32 bases, different behind
    default: return i < 15 ? i % 4 : 3 - i % 4;                 // pattern 0 through base 14: equal through a row of 15 bases
  }
}

struct Row { int pattern, len; std::vector<int> bases; std::vector<uint32_t> words; };

// the lower bound of seqkeys.inc.hip's key_lower_bound, restated
int lower_bound_restated(const std::vector<unsigned long long> &keys, int first, int cnt, unsigned long long w) {
  int lo = first, hi = first + cnt;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < w) lo = mid + 1; else hi = mid; }
  return lo;
}

long check_keys(int cap) {                                      // cap: 32 (assignSpecies), less (collapseNoMismatch's minOverlap)
  static const int LENS[8] = {1, 15, 16, 17, 31, 32, 33, 40};
  std::vector<Row> rows;
  for (int pattern = 0; pattern < 6; pattern++)
    for (int len : LENS) {
      Row r{pattern, len, {}, std::vector<uint32_t>((size_t)(len + 15) / 16, 0u)};
      for (int i = 0; i < len; i++) { r.bases.push_back(base_of(pattern, i)); r.words[i >> 4] |= (uint32_t)r.bases[i] << (2 * (i & 15)); }
      rows.push_back(r);
    }
  std::vector<PrefixKey> kp;
  for (const Row &r : rows) kp.push_back(prefix_key(r.words.data(), std::min(r.len, cap)));
  PrefixKeyTable T;
  build_prefix_keys(kp, T);
  const int ng = (int)T.groups.size() / 3;
  if (T.groups.size() % 3 != 0 || T.key_of.size() != rows.size()) fail("the table's shape", (long)T.groups.size(), (long)T.key_of.size());
  int next = 0;
  for (int g = 0; g < ng; g++) {
    const int kl = T.groups[3 * g], first = T.groups[3 * g + 1], cnt = T.groups[3 * g + 2];
    if (g > 0 && kl <= T.groups[3 * (g - 1)]) fail("the groups do not ascend by length", g, kl);
    if (first != next || cnt < 1) fail("the groups do not tile the keys", g, first, cnt);
    for (int k = first + 1; k < first + cnt; k++)
      if (!(T.keys[k - 1] < T.keys[k])) fail("the keys of a group do not ascend strictly", g, k);
    next = first + cnt;
  }
  if (next != (int)T.keys.size()) fail("the groups do not tile the keys", next, (long)T.keys.size());
  for (size_t i = 0; i < rows.size(); i++) {
    const Row &r = rows[i];
    const int kl = std::min(r.len, cap);
    unsigned long long want = 0;                                // bit by bit: base k in bits 2k, 2k + 1
    for (int k = 0; k < kl; k++)
      for (int bit = 0; bit < 2; bit++)
        if ((r.bases[k] >> bit) & 1) want |= 1ull << (2 * k + bit);
    if (kp[i].kl != kl || kp[i].key != want) fail("a row's key", (long)i, r.pattern, r.len);
    int g = 0;
    while (g < ng && T.groups[3 * g] != kl) g++;
    if (g == ng) fail("a row's length has no group", (long)i, kl);
    const int first = T.groups[3 * g + 1], cnt = T.groups[3 * g + 2], lo = lower_bound_restated(T.keys, first, cnt, want);
    if (!(lo < first + cnt && T.keys[lo] == want)) fail("a row's key is not found in its group", (long)i, r.pattern, r.len);
    if (T.key_of[i] != lo) fail("key_of", (long)i, T.key_of[i], lo);
  }
  // rows that are equal in their first `cap` bases share a key; rows that are equal only through the shorter one's length do not
  auto row_of = [&](int pattern, int len) {
    for (size_t i = 0; i < rows.size(); i++) if (rows[i].pattern == pattern && rows[i].len == len) return (int)i;
    fail("no such row", pattern, len);
  };
  if (T.key_of[row_of(0, 40)] != T.key_of[row_of(4, 40)]) fail("rows equal in their first 32 bases have two keys");
  if (T.key_of[row_of(0, 15)] != T.key_of[row_of(5, 15)]) fail("equal rows have two keys");
  if (cap >= 17 && (T.key_of[row_of(0, 15)] == T.key_of[row_of(0, 17)] || T.key_of[row_of(0, 17)] == T.key_of[row_of(5, 17)]))
    fail("rows equal through the shorter one's length share a key");
  return (long)rows.size();
}

}  // namespace

int main(int argc, char **argv) {
  const std::string which = argc > 1 ? argv[1] : "all";
  if (which != "all" && which != "pieces" && which != "keys") { printf("usage: stage_plain_check [pieces|keys]\n"); return 2; }
  long pieces = 0, keys = 0;
  if (which != "keys") pieces = check_all_pieces();
  if (which != "pieces") keys = check_keys(32) + check_keys(20) + check_keys(16) + check_keys(1);
  printf("stage_plain_check: ok (%ld piece cases, %ld keyed rows)\n", pieces, keys);
  return 0;
}
