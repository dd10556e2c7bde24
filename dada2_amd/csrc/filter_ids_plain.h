// filter_ids_plain.h — matchIDs / id.sep / id.field of fastqPairedFilter (R/filter.R:940-991) on plain C++: the split of an id
// line by strsplit's rules, the detection of the id field, the key a record is matched by and the membership join of a chunk.
// No HIP and nothing of the library's: derep.cpp includes it, and a stand-alone program can.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

namespace fid {

// id.sep: "\\s" (the regex class: space \t \n \v \f \r) or one literal character
struct Sep { bool space = true; char ch = ' '; };
inline bool is_sep(const Sep &s, char c) { return s.space ? (c == ' ' || (c >= '\t' && c <= '\r')) : c == s.ch; }

// strsplit(id, sep)[[1]][field], field 1-based; false: no such field (NA).  A separator ends a field, so consecutive separators
// give empty fields, a leading one a leading empty field, and a trailing one nothing
inline bool split_field(std::string_view id, const Sep &sep, int field, std::string_view &out) {
  size_t start = 0;
  for (int t = 1;; t++) {
    if (start >= id.size()) return false;
    size_t e = start;
    while (e < id.size() && !is_sep(sep, id[e])) e++;
    if (t == field) { out = id.substr(start, e - start); return true; }
    start = e + 1;
  }
}

// :945-957 on the first forward id: the 1-based field, 0 when it cannot be told; old_format: the 4-colon form (CASAVA <= 1.7)
inline int detect_field(std::string_view id, const Sep &sep, bool &old_format) {
  std::vector<int> ncolon;
  std::string_view f;
  for (int t = 1; split_field(id, sep, t, f); t++) {
    int c = 0;
    for (char ch : f) c += ch == ':';
    ncolon.push_back(c == 0 ? 1 : c);                            // gregexpr's -1 has length 1
  }
  int mx = 0, cnt = 0, at = 0;
  for (size_t i = 0; i < ncolon.size(); i++) {
    if (ncolon[i] > mx) { mx = ncolon[i]; cnt = 0; }
    if (ncolon[i] == mx) { cnt++; at = (int)i + 1; }
  }
  if (cnt != 1 || (mx != 6 && mx != 4)) return 0;
  old_format = mx == 4;
  return at;
}

// the key a record is matched by: the field's bytes inside the header blob, or NA; h: its hash
struct Key { const char *p; uint32_t len; uint32_t na; uint64_t h; };
inline bool key_eq(const Key &a, const Key &b) { return a.h == b.h && a.na == b.na && (a.na || (a.len == b.len && memcmp(a.p, b.p, a.len) == 0)); }

// the key of a header line ('@' in front).  strip_hash (the forward ids of the old format, :974-976):
// sapply(strsplit(ids, "#"), `[`, 1) - up to the first '#', and NA for an empty field
inline Key id_key(std::string_view hdr, const Sep &sep, int field, bool strip_hash) {
  const Key na{nullptr, 0, 1, 0x9e3779b97f4a7c15ull};
  std::string_view f;
  if (!split_field(hdr.substr(hdr.empty() ? 0 : 1), sep, field, f)) return na;
  if (strip_hash) {
    if (f.empty()) return na;
    f = f.substr(0, f.find('#'));
  }
  return Key{f.data(), (uint32_t)f.size(), 0, (uint64_t)std::hash<std::string_view>()(f)};
}

// the distinct keys of one side in an open-addressing table of indices into `keys` (linear probing, at most half full)
struct KeySet {
  const std::vector<Key> &keys;
  std::vector<uint32_t> slot;
  size_t mask;
  explicit KeySet(const std::vector<Key> &k) : keys(k) {
    size_t cap = 16;
    while (cap < 2 * k.size()) cap <<= 1;
    mask = cap - 1;
    slot.assign(cap, UINT32_MAX);
    for (size_t i = 0; i < k.size(); i++) {
      size_t at = (size_t)k[i].h & mask;
      while (slot[at] != UINT32_MAX && !key_eq(k[slot[at]], k[i])) at = (at + 1) & mask;
      if (slot[at] == UINT32_MAX) slot[at] = (uint32_t)i;
    }
  }
  bool has(const Key &x) const {
    for (size_t at = (size_t)x.h & mask; slot[at] != UINT32_MAX; at = (at + 1) & mask)
      if (key_eq(keys[slot[at]], x)) return true;
    return false;
  }
};

// in_a[i] = a[i] %in% b, in_b[j] = b[j] %in% a (NA matches NA).  pfor(n, grain, f(lo, hi)) runs the look-ups: a plain loop, or
// the host pool's parallel_for
template <typename PFor>
void join(const std::vector<Key> &a, const std::vector<Key> &b, std::vector<uint8_t> &in_a, std::vector<uint8_t> &in_b, PFor &&pfor) {
  const KeySet sa(a), sb(b);
  in_a.resize(a.size()); in_b.resize(b.size());
  pfor(a.size(), (size_t)4096, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) in_a[i] = sb.has(a[i]) ? 1 : 0; });
  pfor(b.size(), (size_t)4096, [&](size_t lo, size_t hi) { for (size_t j = lo; j < hi; j++) in_b[j] = sa.has(b[j]) ? 1 : 0; });
}

// one past the last set entry (0: none): what lies behind it is carried into the next chunk (:977-988)
inline size_t past_last(const std::vector<uint8_t> &in) {
  size_t n = in.size();
  while (n > 0 && !in[n - 1]) n--;
  return n;
}

}  // namespace fid
