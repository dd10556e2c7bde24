// derep_dev_plain.h — the finalisation of the device dereplicator (derep_dev_host.h, derep_dev.inc.hip) in plain C++: no HIP, no
// host pool, no driver.cpp types.  What comes back from the device is one row per unique in the order the device happened to
// number them (which is not defined): its bytes, its count, the smallest index of a read that had it, and per position the sum of
// the RAW quality characters of its reads.  Here are derepFastq's order (R/sequenceIO.R:85-88 the chunk a unique was first seen
// in, :161 C-locale lexical order inside it, :98 the stable order by decreasing abundance on top), the means (:95) with the
// encoding offset taken off once, and the map's renumbering (:101).  derep.cpp builds the dada2hip_derep from it;
// tools/derep_dev_plain_check.cpp includes this header alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dada2hip.h"

// Between the two homes of the device dereplicator - derep_dev_host.h (driver.cpp: the device) and derep.cpp (the file level and
// the dada2hip_derep struct); not part of the interface.  `dd` is a dereplicator in the making (d2_dd_open .. d2_dd_free).
// d2_dd_feed: reads in memory, read r cut to window[2 r], [2 r + 1] (null: whole) and taken if keep[r] (null: all).
// d2_dd_filter_chunk: dada2hip_filter_reads' verdicts of a chunk, every kept window dereplicated out of the filter's own slots.
// d2_dd_finish: the rows come back and d2_derep_from_rows (derep.cpp) makes the object; allow_none: no read at all is *out = null.
#define D2_HIDDEN extern "C" __attribute__((visibility("hidden")))
D2_HIDDEN int d2_dd_open(int32_t device, int64_t chunk_reads, int32_t qual_offset, void **dd, char *errbuf, size_t errlen);
D2_HIDDEN void d2_dd_free(void *dd);
D2_HIDDEN int32_t d2_filter_device(const dada2hip_filter *ctx);   // the device a filter context lives on
D2_HIDDEN int d2_dd_feed(void *dd, int64_t n, const char *seq, const char *qual, const int64_t *offsets, const int32_t *window,
                         const uint8_t *keep, char *errbuf, size_t errlen);
D2_HIDDEN int d2_dd_filter_chunk(dada2hip_filter *ctx, void *dd, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                                 const dada2hip_filter_params *params, int32_t *code, int32_t *window, int64_t *stats, char *errbuf,
                                 size_t errlen);
D2_HIDDEN int d2_dd_finish(void *dd, int32_t allow_none, dada2hip_derep **out, int64_t *stats, char *errbuf, size_t errlen);
D2_HIDDEN int d2_derep_from_rows(int64_t nuniq, const int64_t *off, const int32_t *len, const int64_t *count, const int64_t *first,
                                 const uint8_t *bytes, const uint64_t *sums, int64_t nreads, const int32_t *ruid, int64_t chunk_reads,
                                 int32_t qual_offset, int32_t min_char, dada2hip_derep **out, char *errbuf, size_t errlen);
// The resident form (derep_dev_host.h).  d2_dd_finish_resident: the small rows come back, never the sums; d2_derep_from_rows_resident
// (derep.cpp) makes the object without a quality matrix and says the order (output row -> device unique); the sample's rows are
// written on the device in that order and d2_derep_set_qmax stores the largest ceil(mean) the device found.  An input error of
// the sample (a letter outside ACGT, a read of five bases, a mean that is no byte) fails the call with neither object.
D2_HIDDEN int d2_dd_finish_resident(void *dd, int32_t allow_none, dada2hip_derep **out, dada2hip_sample **sample, int64_t *stats,
                                    int64_t *resident_stats, char *errbuf, size_t errlen);
D2_HIDDEN int d2_derep_from_rows_resident(int64_t nuniq, const int64_t *off, const int32_t *len, const int64_t *count, const int64_t *first,
                                          const uint8_t *bytes, int64_t nreads, const int32_t *ruid, int64_t chunk_reads, int32_t *order,
                                          dada2hip_derep **out, char *errbuf, size_t errlen);
D2_HIDDEN void d2_derep_set_qmax(dada2hip_derep *d, int32_t qmax);
#undef D2_HIDDEN

namespace {

// the rows as the device leaves them: unique u is bytes[off[u] .. off[u] + len[u]), sums[off[u] + p] is its position p
struct DdRows {
  int64_t nuniq = 0;
  const int64_t *off = nullptr;
  const int32_t *len = nullptr;
  const int64_t *count = nullptr;
  const int64_t *first = nullptr;           // the smallest 0-based index of a read with this sequence
  const uint8_t *bytes = nullptr;
  const uint64_t *sums = nullptr;
};

struct DdPlan {
  std::vector<int32_t> order;               // output row -> device unique
  std::vector<int32_t> rank;                // device unique -> output row
  int32_t maxlen = 0;
};

enum { DDP_OK = 0, DDP_NONE = 1, DDP_OVERFLOW = 2 };

// "Auto" (ShortRead's rule as dada2hip_derep_fastq has it): a character below ';' in the first chunk means Phred+33, else +64;
// min_char is 255 when the first chunk held no quality character at all
inline int dd_offset(int32_t qual_offset, int min_char) {
  if (qual_offset > 0) return qual_offset;
  if (min_char >= 255) return 33;
  return min_char < 59 ? 33 : 64;
}

// (abundance descending, first chunk ascending, bytes ascending with a prefix first) is a strict order of distinct sequences, so
// any sort gives the one result: the stable sort by decreasing abundance of the chunk-lexical order.  sort(first, n, less) is the
// caller's (std::sort here, the host pool's in derep.cpp).
template <typename Sort> int dd_order(const DdRows &R, int64_t chunk_reads, DdPlan &P, Sort &&sort) {
  if (R.nuniq <= 0) return DDP_NONE;
  if (R.nuniq > (int64_t)INT32_MAX) return DDP_OVERFLOW;
  const size_t U = (size_t)R.nuniq;
  P.maxlen = 0;
  for (size_t u = 0; u < U; u++) {
    if (R.count[u] > (int64_t)INT32_MAX) return DDP_OVERFLOW;
    P.maxlen = std::max(P.maxlen, R.len[u]);
  }
  P.order.resize(U);
  for (size_t u = 0; u < U; u++) P.order[u] = (int32_t)u;
  sort(P.order.data(), U, [&R, chunk_reads](int32_t a, int32_t b) {
    if (R.count[a] != R.count[b]) return R.count[a] > R.count[b];
    const int64_t ca = R.first[a] / chunk_reads, cb = R.first[b] / chunk_reads;
    if (ca != cb) return ca < cb;
    const size_t la = (size_t)R.len[a], lb = (size_t)R.len[b];
    const int c = memcmp(R.bytes + R.off[a], R.bytes + R.off[b], std::min(la, lb));
    return c < 0 || (c == 0 && la < lb);
  });
  P.rank.resize(U);
  for (size_t k = 0; k < U; k++) P.rank[P.order[k]] = (int32_t)k;
  return DDP_OK;
}

// derepQuals / derepCounts (:95) of device unique u into row[0 .. maxlen): the integer sum less count x offset, divided in double
inline void dd_quality_row(const DdRows &R, int32_t u, int offset, int32_t maxlen, double na, double *row) {
  const int64_t cnt = R.count[u];
  const uint64_t *s = R.sums + R.off[u];
  const int32_t len = R.len[u];
  for (int32_t p = 0; p < len; p++) row[p] = (double)((int64_t)s[p] - (int64_t)offset * cnt) / (double)cnt;
  for (int32_t p = len; p < maxlen; p++) row[p] = na;
}

// a read's device unique (negative: a zero-length read) -> its map entry
inline int32_t dd_map_entry(int32_t uid, const DdPlan &P, int32_t na) { return uid < 0 ? na : P.rank[(size_t)uid]; }

}  // namespace
