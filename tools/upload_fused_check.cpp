// tools/upload_fused_check.cpp — check program for the row work of the boundary's fused upload pass (dada2_amd/csrc/hostsimd.cpp,
// marshal_rows: length, abundance, prior, 2-bit words and rounded quality bytes of a row in one visit).  Plain C++, no HIP;
// meant for the host sanitizers:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x c++ tools/upload_fused_check.cpp dada2_amd/csrc/hostsimd.cpp -o upload_fused_check
// Every buffer the pass reads or writes is a heap block of exactly the stated size (the sanitizer's red zone follows it), and the
// two row matrices it writes carry a canary row in front and behind as well, so that a write outside a row's W2 words / LQ bytes
// shows even where it stays inside the block.  Checked against the rules restated below:
//   ragged reads of 6..60 nt with the longest in the last row, the first row and a row of the middle; NaN behind each read's end;
//   strides from two below to two above the longest read (a row longer than the stride is only recorded: its len / reads / prior
//   are right and its packed row and quality row are untouched); a bad letter as the last base of the last row; qualities of -1,
//   300 and NaN inside a read; rows cut into pieces at every border a pool could cut them at.
// Exit status: 0 = all as the rules say, 1 = a difference.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../dada2_amd/csrc/marshal.h"

namespace {

const int LEN_CAP = 3000;   // (SEQLEN of the library; any value above the reads' lengths serves)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int fails = 0;
void fail(const char *what, int a, int b, int c) {
  if (fails++ < 20) fprintf(stderr, "FAIL %s (%d, %d, %d)\n", what, a, b, c);
}

// ---- the rules, restated ---------------------------------------------------------------------------
uint32_t rule_code(char c, bool *bad) {
  switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: *bad = true; return 0;
  }
}
// (uint8) round(x), half away from zero; outside 0..255 after rounding, or NaN: bad, stored as 0
int rule_quality(double x, bool *bad) {
  const double r = std::round(x);
  if (!(r >= 0.0 && r <= 255.0)) { *bad = true; return 0; }
  return (int)r;
}

template <typename T> struct Exact {   // a heap block of exactly n elements
  T *p;
  size_t n;
  explicit Exact(size_t count) : p((T *)malloc(std::max<size_t>(1, count * sizeof(T)))), n(count) {}
  ~Exact() { free(p); }
  Exact(const Exact &) = delete;
  Exact &operator=(const Exact &) = delete;
};

struct Sample {
  std::vector<std::string> seqs;
  std::vector<int32_t> abund;
  std::vector<uint8_t> priors;
};

Sample ragged(int n, int longest_row, int maxlen) {
  Sample s;
  for (int i = 0; i < n; i++) {
    const int l = i == longest_row ? maxlen : 6 + (int)(rng() % (uint64_t)(maxlen - 6));   // 6 .. maxlen - 1
    std::string q((size_t)l, 'A');
    for (int p = 0; p < l; p++) q[p] = "ACGT"[rng() & 3];
    s.seqs.push_back(q);
    s.abund.push_back(1 + (int32_t)(rng() % 1000));
    s.priors.push_back((uint8_t)((rng() % 5) == 0 ? 7 : 0));   // (any non-zero byte is a set flag)
  }
  return s;
}

// One pass over the sample at the given stride, cut into pieces of `piece` rows; everything it leaves is compared with the rules.
void check(const Sample &s, int stride, int piece, bool with_priors, int bad_qual_row, double bad_qual_value, const char *label) {
  const int n = (int)s.seqs.size();
  const int W2 = (((stride + 15) / 16) + 3) & ~3, LQ = (stride + 15) & ~15;
  // inputs: every string a block of exactly its length + 1, the quality matrix exactly n x stride, NaN behind each read's end
  std::vector<char *> ptr(n);
  for (int i = 0; i < n; i++) { ptr[i] = (char *)malloc(s.seqs[i].size() + 1); memcpy(ptr[i], s.seqs[i].c_str(), s.seqs[i].size() + 1); }
  Exact<const char *> seqs(n);
  for (int i = 0; i < n; i++) seqs.p[i] = ptr[i];
  Exact<int32_t> abund(n);
  Exact<uint8_t> priors(n);
  for (int i = 0; i < n; i++) { abund.p[i] = s.abund[i]; priors.p[i] = s.priors[i]; }
  Exact<double> quals((size_t)n * stride);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int i = 0; i < n; i++)
    for (int p = 0; p < stride; p++) {
      const double v = (double)(2 + rng() % 39) + (double)(rng() & 3) * 0.25;   // mean qualities: quarters, ties among them
      quals.p[(size_t)i * stride + p] = p < (int)s.seqs[i].size() ? v : nan;
    }
  if (bad_qual_row >= 0) quals.p[(size_t)bad_qual_row * stride + std::min<int>(stride, (int)s.seqs[bad_qual_row].size()) / 2] = bad_qual_value;
  // outputs, the two row matrices with a canary row in front and behind
  Exact<int32_t> len(n);
  Exact<uint32_t> reads(n);
  Exact<uint8_t> prior(n);
  Exact<uint32_t> packed((size_t)(n + 2) * W2);
  Exact<uint8_t> qbytes((size_t)(n + 2) * LQ);
  for (size_t k = 0; k < packed.n; k++) packed.p[k] = 0xC0FFEE11u;
  memset(qbytes.p, 0xEE, qbytes.n);
  const d2::MarshalRows m{seqs.p, abund.p, with_priors ? priors.p : nullptr, quals.p, stride, W2, LQ, LEN_CAP,
                          len.p, reads.p, prior.p, packed.p + W2, qbytes.p + LQ};
  d2::MarshalTally total;
  for (int lo = 0; lo < n; lo += piece) {
    d2::MarshalTally t;
    d2::marshal_rows(m, (size_t)lo, (size_t)std::min(n, lo + piece), &t);
    total.maxlen = std::max(total.maxlen, t.maxlen); total.minlen = std::min(total.minlen, t.minlen);
    total.reads += t.reads; total.bad_base |= t.bad_base; total.bad_qual |= t.bad_qual; total.qmax = std::max(total.qmax, t.qmax);
  }
  // the rules
  int want_max = 0, want_min = 0x7FFFFFFF, want_qmax = 0;
  uint64_t want_reads = 0;
  bool want_bad_base = false, want_bad_qual = false;
  for (int i = 0; i < n; i++) {
    const int l = (int)s.seqs[i].size();
    want_max = std::max(want_max, l); want_min = std::min(want_min, l);
    want_reads += (uint32_t)s.abund[i];
    if (len.p[i] != l) fail("length differs", stride, i, len.p[i]);
    if (reads.p[i] != (uint32_t)s.abund[i]) fail("reads differ", stride, i, 0);
    if (prior.p[i] != (with_priors && s.priors[i] ? 1 : 0)) fail("prior flag differs", stride, i, prior.p[i]);
    const uint32_t *row = packed.p + (size_t)(i + 1) * W2;
    const uint8_t *qrow = qbytes.p + (size_t)(i + 1) * LQ;
    if (l > stride) {   // only recorded: both rows as they were
      for (int w = 0; w < W2; w++) if (row[w] != 0xC0FFEE11u) fail("a row longer than its stride was packed", stride, i, w);
      for (int p = 0; p < LQ; p++) if (qrow[p] != 0xEE) fail("a row longer than its stride was converted", stride, i, p);
      continue;
    }
    for (int w = 0; w < W2; w++) {
      uint32_t word = 0;
      for (int k = 0; k < 16 && 16 * w + k < l; k++) word |= rule_code(s.seqs[i][16 * w + k], &want_bad_base) << (2 * k);
      if (row[w] != word) fail("packed word differs", stride, i, w);
    }
    for (int p = 0; p < LQ; p++) {
      int v = 0;
      if (p < l) { v = rule_quality(quals.p[(size_t)i * stride + p], &want_bad_qual); want_qmax = std::max(want_qmax, v); }
      if (qrow[p] != (uint8_t)v) fail("quality byte differs", stride, i, p);
    }
  }
  for (int w = 0; w < W2; w++) if (packed.p[w] != 0xC0FFEE11u || packed.p[(size_t)(n + 1) * W2 + w] != 0xC0FFEE11u) fail("canary row of the packed rows written", stride, w, 0);
  for (int p = 0; p < LQ; p++) if (qbytes.p[p] != 0xEE || qbytes.p[(size_t)(n + 1) * LQ + p] != 0xEE) fail("canary row of the quality rows written", stride, p, 0);
  if (total.maxlen != want_max || total.minlen != want_min) fail("longest / shortest read differ", stride, total.maxlen, total.minlen);
  if (total.reads != want_reads) fail("total reads differ", stride, 0, 0);
  if ((total.bad_base != 0) != want_bad_base) fail("bad-letter flag differs", stride, (int)total.bad_base, 0);
  if ((total.bad_qual != 0) != want_bad_qual) fail("bad-quality flag differs", stride, total.bad_qual, 0);
  // (the row maximum of a pass that found a bad quality is never used: the call fails)
  if (!want_bad_qual && total.qmax != want_qmax) fail("largest quality differs", stride, total.qmax, want_qmax);
  for (int i = 0; i < n; i++) free(ptr[i]);
  if (fails) fprintf(stderr, "  in: %s, stride %d, pieces of %d\n", label, stride, piece);
}

}  // namespace

int main() {
  const int n = 70, maxlen = 60;
  const int rows[3] = {n - 1, 0, 37};
  const char *labels[3] = {"longest read in the last row", "longest read in the first row", "longest read in a middle row"};
  for (int k = 0; k < 3; k++) {
    const Sample s = ragged(n, rows[k], maxlen);
    for (int stride = maxlen - 2; stride <= maxlen + 2; stride++)
      for (int piece : {1, 7, 32, n})
        check(s, stride, piece, (stride + piece) % 2 == 0, -1, 0.0, labels[k]);
    // a stride that is no multiple of 16 and one that is: the padding of both row kinds
    Sample t = ragged(n, rows[k], 48);
    check(t, 48, 16, true, -1, 0.0, "reads of up to 48 nt");
    // bad letters: the last base of the last row, a lower-case letter, a byte above 127
    Sample b = s;
    b.seqs[n - 1][b.seqs[n - 1].size() - 1] = 'N';
    check(b, maxlen, 32, false, -1, 0.0, "N as the last base of the last row");
    b = s; b.seqs[5][3] = 'a';
    check(b, maxlen, 32, false, -1, 0.0, "a lower-case letter");
    b = s; b.seqs[9][0] = (char)0x80;
    check(b, maxlen, 32, false, -1, 0.0, "a byte above 127");
    // bad qualities inside a read of the last piece; a legal one that takes the exact scalar rule (255.5 rounds to 256: bad; 255.4 not)
    check(s, maxlen, 32, false, n - 2, -1.0, "a quality of -1");
    check(s, maxlen, 32, false, n - 2, 300.0, "a quality of 300");
    check(s, maxlen, 32, false, n - 2, std::numeric_limits<double>::quiet_NaN(), "NaN inside a read");
    check(s, maxlen, 32, false, n - 2, 255.5, "a quality of 255.5");
    check(s, maxlen, 32, false, n - 2, -0.4, "a quality of -0.4 (rounds to 0: legal)");
  }
  // a read of 5 and one of 6 nt, an empty one: recorded like any other (the caller raises the k-mer-size rule)
  {
    Sample s = ragged(20, 19, 40);
    s.seqs[3] = s.seqs[3].substr(0, 5); s.seqs[4] = s.seqs[4].substr(0, 6); s.seqs[7] = "";
    check(s, 40, 8, true, -1, 0.0, "reads of 5, 6 and 0 nt");
  }
  if (fails) { fprintf(stderr, "%d difference(s)\n", fails); return 1; }
  printf("upload_fused_check: ok\n");
  return 0;
}
