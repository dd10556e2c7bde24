// tools/readqc_file_check.cpp — check program for the FILE level of the read diagnostics (dada2_amd/csrc/derep.cpp:
// dada2hip_qprofile_fastq, dada2hip_complexity_fastq, fq_run_chunks without writers) with the device calls replaced by plain
// host stand-ins below, so that the host code around them - the reader, the chunks, the record limit, the table that grows under a
// later chunk, the pairs kept until the longest read is known, the messages - runs on the CPU, under the sanitizers:
//   hipcc -O1 -g -std=c++17 -w -I tests/emu -Xarch_host -fsanitize=address,undefined -x c++ tools/readqc_file_check.cpp -o readqc_file_check -lz -ldl -lpthread
//   readqc_file_check <an empty directory to write FASTQ files into>
// (tests/emu/hip/hip_runtime.h stands in for the HIP header that derep.cpp's includes ask for; no HIP call is made.)
// Exit status: 0 = every property holds ("readqc_file_check: ok"), 1 = one does not (the first is printed), 2 = usage.
#include "../dada2_amd/csrc/derep.cpp"

#include <cmath>
#include <random>

namespace {

[[noreturn]] void fail(const char *what, long a = 0, long b = 0, long c = 0) {
  printf("readqc_file_check: FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
  exit(1);
}

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// H = sum(-y log y) of the k-mers of s[at .. at + w) that are A/C/G/T only; NaN without one
double window_h(const char *s, int64_t at, int w, int k) {
  std::vector<int> h((size_t)1 << (2 * k), 0);
  int tot = 0;
  for (int p = 0; p + k <= w; p++) {
    int idx = 0, bad = 0;
    for (int t = 0; t < k; t++) { const int c = code_of(s[at + p + t]); if (c < 0) bad = 1; idx = idx * 4 + (c < 0 ? 0 : c); }
    if (!bad) { h[(size_t)idx]++; tot++; }
  }
  if (tot == 0) return NAN;
  double acc = 0.0;
  for (int c : h) if (c > 0) { const double y = (double)c / tot; acc += -y * log(y); }
  return acc;
}

int64_t stand_in_calls = 0;

}  // namespace

// ---- the stand-ins for what driver.cpp defines ------------------------------------------------------------------------------------
extern "C" {

int dada2hip_qprofile_reads(int64_t n, const char *qual, const int64_t *offsets, int32_t, int32_t ncycle, int64_t *counts, int64_t *stats,
                            char *errbuf, size_t errlen) {
  stand_in_calls++;
  if (n > 0 && (!qual || !offsets)) { set_err(errbuf, errlen, "dada2hip: bad arguments"); return DADA2HIP_ERR_INPUT; }
  if (ncycle > 0) memset(counts, 0, (size_t)ncycle * 94 * sizeof(int64_t));
  if (stats) { memset(stats, 0, DADA2HIP_READQC_NSTATS * sizeof(int64_t)); stats[RQ_PIECES] = 1; }
  for (int64_t r = 0; r < n; r++) {
    if (offsets[r + 1] - offsets[r] > ncycle) { set_err(errbuf, errlen, "dada2hip: the quality table has fewer cycles than the longest read."); return DADA2HIP_ERR_INPUT; }
    if (stats) stats[RQ_CYCLES] = std::max(stats[RQ_CYCLES], offsets[r + 1] - offsets[r]);
    for (int64_t p = offsets[r]; p < offsets[r + 1]; p++) {
      const int q = (unsigned char)qual[p] - 33;
      if (q < 0 || q >= 94) { set_err(errbuf, errlen, ("dada2hip: read " + std::to_string(r + 1) + " holds a quality letter outside '!'..'~'.").c_str()); return DADA2HIP_ERR_INPUT; }
      counts[(p - offsets[r]) * 94 + q]++;
    }
  }
  return DADA2HIP_OK;
}

int d2_complexity_pairs(int64_t n, const char *seq, const int64_t *offsets, int32_t kmer_size, int32_t window, int32_t by, int32_t,
                        double *pairs, int64_t *stats, char *errbuf, size_t errlen) {
  stand_in_calls++;
  const int k = kmer_size == 0 ? 2 : kmer_size;
  if (k >= window) { set_err(errbuf, errlen, "The window over which kmer frequency is calculated must be larger than the kmerSize."); return DADA2HIP_ERR_INPUT; }
  if (stats) { memset(stats, 0, DADA2HIP_READQC_NSTATS * sizeof(int64_t)); stats[RQ_PIECES] = 1; }
  for (int64_t r = 0; r < n; r++) {
    const int64_t len = offsets[r + 1] - offsets[r];
    double lo = INFINITY, last = INFINITY;
    for (int64_t s = 0; s + window <= len; s += by) {
      const double H = window_h(seq + offsets[r], s, window, k);
      if (s + window < len) { if (H < lo || H != H) lo = H; } else last = H;
    }
    pairs[2 * r] = lo; pairs[2 * r + 1] = last;
  }
  return DADA2HIP_OK;
}

int dada2hip_complexity_reads(int64_t n, const char *seq, const int64_t *offsets, int32_t kmer_size, int32_t window, int32_t, int32_t,
                              double *complexity, int64_t *stats, char *errbuf, size_t errlen) {
  stand_in_calls++;
  if (window != 0) { set_err(errbuf, errlen, "the file level asks for window 0 only"); return DADA2HIP_ERR_RUNTIME; }
  if (stats) memset(stats, 0, DADA2HIP_READQC_NSTATS * sizeof(int64_t));
  const int k = kmer_size == 0 ? 2 : kmer_size;
  for (int64_t r = 0; r < n; r++) complexity[r] = exp(window_h(seq + offsets[r], 0, (int)(offsets[r + 1] - offsets[r]), k));
  return DADA2HIP_OK;
}

int dada2hip_filter_reads(dada2hip_filter *, int64_t, const char *, const char *, const int64_t *, const dada2hip_filter_params *, int32_t *,
                          int32_t *, double *, int32_t *, int32_t *, double *, int64_t *, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
int dada2hip_filter_reads_oriented(dada2hip_filter *, int64_t, const char *, const char *, const int64_t *, const dada2hip_filter_params *,
                                   const char *, int32_t, int32_t *, int32_t *, double *, int32_t *, int32_t *, double *, int8_t *, int64_t *,
                                   char *, size_t) { return DADA2HIP_ERR_DEVICE; }
int dada2hip_primers_reads(int64_t, const char *, const int64_t *, const dada2hip_primer_params *, int32_t, int32_t *, int32_t *, int32_t *,
                           int32_t *, int32_t *, int32_t *, int64_t *, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
int dada2hip_sample_create(int32_t, const char *const *, const int32_t *, const uint8_t *, const double *, int32_t, int32_t,
                           dada2hip_sample **, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
// (the device dereplicator's ends, derep_dev_plain.h: the fused entries of derep.cpp are not run here)
int d2_dd_open(int32_t, int64_t, int32_t, void **, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
void d2_dd_free(void *) {}
int32_t d2_filter_device(const dada2hip_filter *) { return 0; }
int d2_dd_feed(void *, int64_t, const char *, const char *, const int64_t *, const int32_t *, const uint8_t *, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
int d2_dd_filter_chunk(dada2hip_filter *, void *, int64_t, const char *, const char *, const int64_t *, const dada2hip_filter_params *, int32_t *,
                       int32_t *, int64_t *, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
int d2_dd_finish(void *, int32_t, dada2hip_derep **, int64_t *, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
int d2_dd_finish_resident(void *, int32_t, dada2hip_derep **, dada2hip_sample **, int64_t *, int64_t *, char *, size_t) { return DADA2HIP_ERR_DEVICE; }
void dada2hip_sample_free(dada2hip_sample *) {}

}  // extern "C"

namespace {

struct Rec { std::string id, seq, qual; };

void write_file(const std::string &path, const std::vector<Rec> &recs, bool gz) {
  std::string text;
  for (const Rec &r : recs) text += r.id + "\n" + r.seq + "\n+\n" + r.qual + "\n";
  if (gz) {
    gzFile f = gzopen(path.c_str(), "wb");
    if (!f || (text.size() && gzwrite(f, text.data(), (unsigned)text.size()) <= 0)) fail("cannot write the gzip file");
    gzclose(f);
  } else {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(text.data(), 1, text.size(), f) != text.size()) fail("cannot write the plain file");
    fclose(f);
  }
}

void check_profile(const std::string &path, const std::vector<Rec> &recs, int64_t chunk, int64_t max_reads) {
  char eb[512] = "";
  dada2hip_qprofile *p = nullptr;
  int64_t st[DADA2HIP_READQC_NSTATS];
  const int rc = dada2hip_qprofile_fastq(path.c_str(), chunk, max_reads, 0, 0, &p, st, eb, sizeof eb);
  if (rc != DADA2HIP_OK || !p) { printf("%s\n", eb); fail("qprofile_fastq failed", rc, chunk, max_reads); }
  const int64_t take = max_reads > 0 ? std::min<int64_t>(max_reads, (int64_t)recs.size()) : (int64_t)recs.size();
  size_t mx = 0;
  for (int64_t i = 0; i < take; i++) mx = std::max(mx, recs[(size_t)i].qual.size());
  std::vector<int64_t> want(mx * 94, 0);
  for (int64_t i = 0; i < take; i++)
    for (size_t c = 0; c < recs[(size_t)i].qual.size(); c++) want[c * 94 + (size_t)(recs[(size_t)i].qual[c] - 33)]++;
  if (dada2hip_qprofile_ncycle(p) != (int32_t)mx) fail("ncycle", dada2hip_qprofile_ncycle(p), (long)mx, chunk);
  if (dada2hip_qprofile_reads_total(p) != (int64_t)recs.size() || dada2hip_qprofile_profiled(p) != take) fail("reads / profiled", chunk, max_reads);
  if (st[RQ_IN] != (int64_t)recs.size() || st[RQ_PROFILED] != take || st[RQ_CYCLES] != (int64_t)mx) fail("stats", st[RQ_IN], st[RQ_PROFILED], st[RQ_CYCLES]);
  const int64_t *got = dada2hip_qprofile_counts(p);
  for (size_t i = 0; i < want.size(); i++) if (got[i] != want[i]) fail("a cell of the table", (long)i, got[i], want[i]);
  if (dada2hip_qprofile_qual_offset(p) != 33) fail("offset");
  dada2hip_qprofile_free(p);
}

void check_complexity(const std::string &path, const std::vector<Rec> &recs, int64_t chunk, int64_t max_reads, int window, int by) {
  char eb[512] = "";
  double *vals = nullptr;
  int64_t nvals = -1;
  const int rc = dada2hip_complexity_fastq(path.c_str(), chunk, max_reads, 2, window, by, 0, &vals, &nvals, nullptr, eb, sizeof eb);
  if (rc != DADA2HIP_OK) { printf("%s\n", eb); fail("complexity_fastq failed", rc, chunk, max_reads); }
  const int64_t take = max_reads > 0 ? std::min<int64_t>(max_reads, (int64_t)recs.size()) : (int64_t)recs.size();
  if (nvals != take) fail("number of values", nvals, take);
  int64_t maxlen = 0;
  for (int64_t i = 0; i < take; i++) maxlen = std::max<int64_t>(maxlen, (int64_t)recs[(size_t)i].seq.size());
  for (int64_t i = 0; i < take; i++) {                          // the R loop, literally (R/filter.R:1259-1265)
    const std::string &s = recs[(size_t)i].seq;
    double si = 16.0;
    if (window == 0) si = exp(window_h(s.data(), 0, (int)s.size(), 2));
    else
      for (int64_t st = 1; st <= maxlen - window; st += by)
        if ((int64_t)s.size() >= st + window - 1) {
          const double v = exp(window_h(s.data(), st - 1, window, 2));
          si = (si != si || v != v) ? NAN : std::min(si, v);
        }
    const double g = vals[i];
    if ((g != g) != (si != si) || (g == g && fabs(g - si) > 1e-12 * fabs(si))) fail("a complexity", (long)i, (long)(g * 1e6), (long)(si * 1e6));
  }
  dada2hip_complexity_free(vals);
}

void expect_error(int rc, int want, const char *eb, const char *text, const char *what) {
  if (rc != want || !strstr(eb, text)) { printf("%d: %s\n", rc, eb); fail(what, rc, want); }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { printf("usage: readqc_file_check <directory>\n"); return 2; }
  const std::string dir = argv[1];
  std::mt19937 rng(20);
  std::vector<Rec> recs;
  for (int i = 0; i < 157; i++) {                                // lengths that grow, shrink and vanish: a later chunk holds a longer read
    const int len = i == 40 ? 0 : i < 50 ? 20 + i : i < 100 ? 300 - i : 64 + (i % 3) * 64 + (i == 150 ? 200 : 0);
    Rec r;
    r.id = "@r" + std::to_string(i) + " some text";
    for (int p = 0; p < len; p++) {
      r.seq += (i % 11 == 3 && p > 10 && p < 40) ? 'N' : "ACGT"[rng() % (i % 7 == 0 ? 2 : 4)];
      r.qual += (char)(33 + rng() % 94);
    }
    recs.push_back(r);
  }
  const std::string plain = dir + "/in.fastq", gz = dir + "/in.fastq.gz", empty = dir + "/empty.fastq", bad = dir + "/bad.fastq";
  write_file(plain, recs, false);
  write_file(gz, recs, true);
  write_file(empty, {}, false);
  for (const std::string &path : {plain, gz})
    for (int64_t chunk : {1, 7, 50, 1000, 0})
      for (int64_t max_reads : {0, 1, 45, 101, 157, 5000}) {
        if (chunk == 1 && max_reads != 0 && max_reads != 45) continue;
        check_profile(path, recs, chunk, max_reads);
        check_complexity(path, recs, chunk, max_reads, 0, 5);
        check_complexity(path, recs, chunk, max_reads, 12, 5);
        if (max_reads == 0) check_complexity(path, recs, chunk, 0, 30, 1);
      }
  check_profile(empty, {}, 10, 0);
  check_complexity(empty, {}, 10, 0, 0, 5);
  char eb[512] = "";
  dada2hip_qprofile *p = nullptr;
  double *vals = nullptr;
  int64_t nvals = 0;
  std::vector<Rec> broken(recs.begin(), recs.begin() + 30);
  broken[22].qual[5] = ' ';
  write_file(bad, broken, false);
  expect_error(dada2hip_qprofile_fastq(bad.c_str(), 4, 0, 0, 0, &p, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "read 23 (@r22 some text)", "the bad letter's record");
  if (p) fail("a profile came back with the error");
  if (dada2hip_qprofile_fastq(bad.c_str(), 4, 22, 0, 0, &p, nullptr, eb, sizeof eb) != DADA2HIP_OK || dada2hip_qprofile_profiled(p) != 22) fail("the record past the limit was looked at");
  dada2hip_qprofile_free(p); p = nullptr;
  expect_error(dada2hip_qprofile_fastq(dir.c_str(), 0, 0, 0, 0, &p, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "directory", "a directory");
  expect_error(dada2hip_qprofile_fastq((dir + "/none.fastq").c_str(), 0, 0, 0, 0, &p, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "do not exist", "a missing file");
  expect_error(dada2hip_qprofile_fastq(plain.c_str(), 0, 0, 50, 0, &p, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "offset", "an offset of 50");
  expect_error(dada2hip_qprofile_fastq(plain.c_str(), 0, -1, 0, 0, &p, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "negative", "a negative limit");
  expect_error(dada2hip_complexity_fastq(plain.c_str(), 0, 0, 2, 400, 5, 0, &vals, &nvals, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "longest sequence", "a window no read is longer than");
  expect_error(dada2hip_complexity_fastq(empty.c_str(), 0, 0, 2, 20, 5, 0, &vals, &nvals, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "longest sequence", "a window on no reads");
  expect_error(dada2hip_complexity_fastq(plain.c_str(), 0, 0, 3, 3, 5, 0, &vals, &nvals, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "larger than the kmerSize", "kmerSize = window");
  expect_error(dada2hip_complexity_fastq(dir.c_str(), 0, 0, 2, 20, 5, 0, &vals, &nvals, nullptr, eb, sizeof eb), DADA2HIP_ERR_INPUT, eb, "directory", "a directory's complexity");
  if (vals || nvals != 0) fail("values came back with an error");
  printf("readqc_file_check: ok (%ld calls of the stand-ins)\n", (long)stand_in_calls);
  return 0;
}
