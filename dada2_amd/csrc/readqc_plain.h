// readqc_plain.h — what the two homes of the read diagnostics share: readqc_host.h (driver.cpp: the calls on reads in memory) and
// derep.cpp (the file level, where the FASTQ reader is).  Plain C++.
//
// seqComplexity's window loop (R/filter.R:1259-1265) asks for max(width(seqs)) of the whole call, which a piece of a call or a
// chunk of a file does not know.  So the device reports two numbers per read (engine.h: ComplexityOut) that do not depend on it,
// and cw_finish settles the read once the maximum is known.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

// the pairs of dada2hip_complexity_reads with window > 0, before cw_finish: pairs[2 r] the smallest H over the window starts
// i = 1, 1 + by, ... <= len - window, pairs[2 r + 1] H of the start len - window + 1 where it is on that grid; +infinity where
// there is none, NaN where one of them holds no countable k-mer.  Not part of the interface (include/dada2hip.h).
extern "C" __attribute__((visibility("hidden"))) int d2_complexity_pairs(int64_t n, const char *seq, const int64_t *offsets,
                                                                          int32_t kmer_size, int32_t window, int32_t by,
                                                                          int32_t device, double *pairs, int64_t *stats,
                                                                          char *errbuf, size_t errlen);

// R's seq(1, max(width) - window, by) stops when the longest sequence is not longer than the window (:1260)
constexpr const char *CW_ERR_NO_START =
    "dada2hip: the longest sequence must be longer than the window (seq(1, max(width) - window, by): wrong sign in 'by' argument).";

// A read of `len` letters in a call whose longest has `maxlen`: the start len - window + 1 is tested only when it is <= maxlen -
// window (:1260), that is for every read shorter than the longest; si starts at 4^k (:1259) and pmin keeps a NaN (:1264).
inline double cw_finish(int64_t len, int64_t maxlen, double lo, double last, int k) {
  const double cap = (double)(1 << (2 * k));
  double h = lo;
  if (len < maxlen && (last < h || last != last)) h = h != h ? h : last;
  if (h != h) return h;
  const double v = std::isinf(h) ? cap : exp(h);
  return v < cap ? v : cap;
}
