// merge_plain.h — the host's part of the run-level mergePairs (merge_host.h, merge.inc.hip; R/paired.R:92-201) in plain C++: no HIP,
// no host pool, no driver.cpp types.  tools/merge_plain_check.cpp includes this header alone.
//   mp_capacity       the slots of a sample's pair table: known up front, never grown
//   mp_check_sample   the arguments of one sample
//   mp_check_maps     the reference's check of the two derep maps against the dada-class objects (:116-119)
//   mp_index_message  the refusal of an index past a table, with the sample and the first offending read
//   mp_order          unique(pairdf) - first appearance (:125) - then order(abundance, decreasing = TRUE), stable (:185)
//   mp_revcomp        rc() of the denoised reverse sequences (:139)
//   mp_next_chunk     the end of a chunk of the run's pair list
//   mp_scan_accepted  where the merged sequence of every accepted pair of a chunk starts in the chunk's arena
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace {

// what the tally kernel found wrong with a read, in the order it looks: the derep maps, then the dada maps
enum { MP_BAD_NONE = 0, MP_BAD_DEREP_F = 1, MP_BAD_DEREP_R = 2, MP_BAD_DADA_F = 3, MP_BAD_DADA_R = 4 };

// One record of a sample's pair table as the device hands it out, in no order: the pair (f << 32 | r, both 1-based), the number
// of read pairs that name it and the first of them.
struct MpRec { unsigned long long key; int32_t count, first; };

// The next power of two at or above 2 min(reads, nclustF nclustR), at least 64: the table is at most half full.
inline long long mp_capacity(long long nreads, long long nclustF, long long nclustR) {
  const long long distinct = std::max<long long>(1, std::min(nreads, nclustF * nclustR));
  long long cap = 64;
  while (cap < 2 * distinct) cap <<= 1;
  return cap;
}

// "" when the sample may run, else the message.  max_f / max_r: the largest 0-based entry of the derep maps (-1: none), which the
// reference holds against the length of the dada-class object's map: equality, not just "in range" (:117-118; an empty map or one
// of NAs alone has the maximum -Inf there and is refused too).
inline std::string mp_check_maps(int32_t sample, long long max_f, int32_t nuniqF, long long max_r, int32_t nuniqR) {
  if (max_f >= 0 && max_r >= 0 && max_f + 1 == nuniqF && max_r + 1 == nuniqR) return "";
  return "Non-corresponding derep-class and dada-class objects. (sample " + std::to_string(sample + 1) + ": the largest entries of the maps name unique " +
         std::to_string(max_f + 1) + " of " + std::to_string(nuniqF) + " forward and " + std::to_string(max_r + 1) + " of " + std::to_string(nuniqR) +
         " reverse)";
}

inline std::string mp_check_sample(int32_t sample, long long nreads, bool maps, bool dada_maps, int32_t nuniqF, int32_t nuniqR, int32_t nclustF,
                                   int32_t nclustR) {
  const std::string at = " (sample " + std::to_string(sample + 1) + ")";
  if (nreads < 0 || nuniqF < 0 || nuniqR < 0 || nclustF < 0 || nclustR < 0) return "dada2hip: bad arguments" + at;
  if (nreads > (long long)INT32_MAX) return "dada2hip: a derep-class map of more than 2^31 - 1 reads" + at;
  if ((nreads > 0 && !maps) || ((nuniqF > 0 || nuniqR > 0) && !dada_maps)) return "dada2hip: bad arguments" + at;
  return "";
}

inline std::string mp_index_message(int32_t sample, long long read, int what, long long value, long long size) {
  static const char *const names[] = {"", "the forward derep-class map names unique ", "the reverse derep-class map names unique ",
                                      "the forward dada-class map names sequence ", "the reverse dada-class map names sequence "};
  return "Non-corresponding derep-class and dada-class objects. (sample " + std::to_string(sample + 1) + ", read " + std::to_string(read) +
         " counted from 0: " + names[what] + std::to_string(value) + " of " + std::to_string(size) + ")";
}

// order[k] = the record of row k.  false: two records share a first read, or one lies outside the reads - not a table's output.
inline bool mp_order(const MpRec *rec, size_t n, long long nreads, std::vector<int32_t> &order) {
  order.resize(n);
  for (size_t i = 0; i < n; i++) order[i] = (int32_t)i;
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return rec[a].first < rec[b].first; });
  for (size_t i = 0; i < n; i++) {
    const MpRec &r = rec[order[i]];
    if (r.first < 0 || r.first >= nreads || r.count < 1 || (i && rec[order[i - 1]].first == r.first)) return false;
  }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return rec[a].count > rec[b].count; });
  return true;
}

inline std::string mp_revcomp(const char *s, size_t n) {          // R/misc.R rc(); a letter outside ACGT stays (merge.cpp's revcomp)
  std::string r(n, 'N');
  for (size_t i = 0; i < n; i++) {
    const char c = s[n - 1 - i];
    r[i] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
  }
  return r;
}

inline bool mp_is_acgt(const char *s, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (s[i] != 'A' && s[i] != 'C' && s[i] != 'G' && s[i] != 'T') return false;
  return true;
}

// The chunk that starts at pair p0 < n ends in front of the returned pair: at most `chunk` pairs, whatever sample they belong to.
inline size_t mp_next_chunk(size_t p0, size_t n, size_t chunk) { return p0 + std::min(std::max<size_t>(chunk, 1), n - p0); }

// off[i] = the first byte of pair i's merged sequence in the arena (accepted pairs one behind the other; a rejected pair has the
// offset of the next accepted one and writes nothing); returns the arena's size.  -1: a length that no alignment has.
inline long long mp_scan_accepted(size_t n, const int32_t *accept, const int32_t *mlen, std::vector<long long> &off) {
  off.resize(n);
  long long at = 0;
  for (size_t i = 0; i < n; i++) {
    off[i] = at;
    if (!accept[i]) continue;
    if (mlen[i] < 0) return -1;
    at += mlen[i];
  }
  return at;
}

}  // namespace
