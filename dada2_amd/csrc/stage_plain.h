// stage_plain.h — the parts of the stages' shared host layer that are plain C++ (no HIP, no driver.cpp types): the A/C/G/T code,
// the prefix keys of collapseNoMismatch's join and assignSpecies' seed, and the piece cutter of the two-slot read pipeline.
// stage_common.h and read_pieces.h build on it; tools/stage_plain_check.cpp includes it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace {

inline int acgt_code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
inline std::string revcomp_acgt(const std::string &s) {         // of a sequence of A/C/G/T only
  std::string rc(s.rbegin(), s.rend());
  for (char &c : rc) c = "TGCA"[acgt_code(c)];
  return rc;
}
// The prefix key of a packed 2-bit row (base k of a word in bits 2k..2k+1): its first kl <= 32 bases as a 64-bit word, and kl;
// seqkeys.inc.hip's window_key is the same word of a window.  row[1] is read only where the key reaches into it.
struct PrefixKey { int32_t kl; unsigned long long key; };
inline PrefixKey prefix_key(const uint32_t *row, int kl) {
  unsigned long long key = row[0];
  if (kl > 16) key |= (unsigned long long)row[1] << 32;
  if (kl < 32) key &= (1ull << (2 * kl)) - 1ull;
  return PrefixKey{kl, key};
}
inline bool operator<(const PrefixKey &a, const PrefixKey &b) { return a.kl != b.kl ? a.kl < b.kl : a.key < b.key; }
inline bool operator==(const PrefixKey &a, const PrefixKey &b) { return a.kl == b.kl && a.key == b.key; }
// What the kernels search: the distinct keys of `rows`, ascending by length, then key; groups = {length, first key, number of
// keys} per length; key_of[i] = the index of rows[i]'s key.
struct PrefixKeyTable { std::vector<unsigned long long> keys; std::vector<int32_t> groups, key_of; };
inline void build_prefix_keys(const std::vector<PrefixKey> &rows, PrefixKeyTable &T) {
  std::vector<PrefixKey> ks(rows);
  std::sort(ks.begin(), ks.end());
  ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
  T.keys.resize(ks.size()); T.groups.clear(); T.key_of.resize(rows.size());
  for (size_t k = 0; k < ks.size(); k++) {
    T.keys[k] = ks[k].key;
    if (k == 0 || ks[k].kl != ks[k - 1].kl) { T.groups.push_back(ks[k].kl); T.groups.push_back((int32_t)k); T.groups.push_back(0); }
    T.groups.back()++;
  }
  for (size_t i = 0; i < rows.size(); i++) T.key_of[i] = (int32_t)(std::lower_bound(ks.begin(), ks.end(), rows[i]) - ks.begin());
}

// The end of the piece that starts at read r0 < n (read r is bytes offsets[r] .. offsets[r + 1]): at most max_reads reads and
// max_bytes bytes, but never less than one read - a read longer than max_bytes is a piece of its own.
inline int64_t next_piece(const int64_t *offsets, int64_t n, int64_t r0, int64_t max_reads, int64_t max_bytes) {
  int64_t r1 = r0 + 1;
  while (r1 < n && r1 - r0 < max_reads && offsets[r1 + 1] - offsets[r0] <= max_bytes) r1++;
  return r1;
}

}  // namespace
