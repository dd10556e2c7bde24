// tests/golden/filter_ref_wrap.cpp — TEST INFRASTRUCTURE ONLY (tests/golden/make_filter_golden.py, tools/filter_bench.py).
//
// Compiles the reference's src/filter.cpp UNMODIFIED and in place (the compile line puts its src directory and oracle/shim on the
// include path) behind two C entries: C_matchRef and C_matrixEE.  The shim's four externals are defined here, as in
// taxonomy_ref_wrap.cpp, so the wrapper links against nothing of the oracle.  Nothing built from this file is committed.
#include <climits>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include <Rcpp.h>

extern "C" {
int dada2_shim_verbose = 0;
int dada2_shim_nthreads = 1;
double dada2_oracle_ppois(double, double, int) { return 0.0; }   // (not reached from filter.cpp)
void dada2_shim_parallel_for(std::size_t begin, std::size_t end, std::size_t, void (*fn)(void *, std::size_t, std::size_t), void *ctx) {
  fn(ctx, begin, end);                                           // (not reached from filter.cpp)
}
}

#include "filter.cpp"

// out[nseq] = C_matchRef(seqs, ref, word_size, non_overlapping).  Returns 0, or 1 with the message in err.
extern "C" int filter_ref_match(int nseq, const char *const *seqs, const char *ref, unsigned int word_size, int non_overlapping, int *out,
                                char *err, std::size_t errlen) {
  try {
    std::vector<std::string> s(seqs, seqs + nseq);
    Rcpp::IntegerVector r = C_matchRef(s, std::string(ref), word_size, non_overlapping != 0);
    for (int i = 0; i < nseq; i++) out[i] = r[i];
    return 0;
  } catch (const std::exception &e) {
    if (err && errlen) snprintf(err, errlen, "%s", e.what());
    return 1;
  }
}

// q: nrow x ncol quality scores, ROW-major, INT_MIN = NA (the end of a shorter read); out[nrow] = C_matrixEE(q)
extern "C" int filter_ref_ee(int nrow, int ncol, const int *q, double *out, char *err, std::size_t errlen) {
  try {
    Rcpp::IntegerMatrix m(nrow, ncol);
    for (int i = 0; i < nrow; i++) for (int j = 0; j < ncol; j++) m(i, j) = q[(std::size_t)i * ncol + j] == INT_MIN ? NA_INTEGER : q[(std::size_t)i * ncol + j];
    Rcpp::NumericVector r = C_matrixEE(m);
    for (int i = 0; i < nrow; i++) out[i] = r[i];
    return 0;
  } catch (const std::exception &e) {
    if (err && errlen) snprintf(err, errlen, "%s", e.what());
    return 1;
  }
}
