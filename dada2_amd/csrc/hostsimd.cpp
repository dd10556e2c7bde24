// hostsimd.cpp — the two host loops of the boundary that are worth a vector unit: the R-side quality matrix (8 bytes per base,
// 2 GB at 10^6 uniques x 250 nt) turned into the byte matrix the device keeps, and the sequences' characters turned into 2-bit
// words.  A translation unit of its own because it is plain C++ (target attributes and x86 intrinsics do not exist in a HIP
// compilation).  Each loop has a scalar form that is the rule, and an explicit AVX2 form (the compiler vectorises neither: the
// double -> byte conversion with its range test comes out as one vcvttsd2si and one branch per element); which one serves is
// decided once, at load, from the CPU.  tools/host_marshal.cpp times and checks every form against the scalar rule.
// marshal_rows (marshal.h) is the row work of the boundary's fused upload pass built from the two: length, abundance, prior,
// packing and rounding of a row in one visit; tools/upload_fused_check.cpp runs it under the host sanitizers.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "marshal.h"

#if defined(__x86_64__)
#include <immintrin.h>
#define D2_HOSTSIMD_AVX2 1
#endif

namespace d2 {

// ---- quality rounding ----------------------------------------------------------------------------
// (uint8) round(x) of one quality row, round() = half away from zero (raw_new, src/containers.cpp:34 of the reference), for
// values in [0, 255.5): t = (int)x; t + ((x - t) >= 0.5).  Only the first L doubles of the row are read (NA behind a read's end
// is legal input).  Returns false - the caller (driver.cpp, sample_create) redoes the row by the exact scalar rule - when a
// value lies outside that range or is NaN (the compares are ordered: a NaN fails them); *mx_out is the row's maximum.
static inline int round_one(double x, int *ok) {
  *ok &= (int)(x >= 0.0) & (int)(x < 255.5);
  const double xc = x >= 0.0 ? (x < 255.5 ? x : 0.0) : 0.0;   // (keeps the conversion defined for the values the caller will redo)
  const int t = (int)xc;
  return t + (int)((xc - (double)t) >= 0.5);
}

bool round_quality_row_scalar(const double *__restrict__ src, uint8_t *__restrict__ dst, int L, int *mx_out) {
  int ok = 1, mx = 0;
  for (int p = 0; p < L; p++) {
    const int v = round_one(src[p], &ok);
    mx = v > mx ? v : mx;
    dst[p] = (uint8_t)v;
  }
  *mx_out = mx;
  return ok != 0;
}

#ifdef D2_HOSTSIMD_AVX2
// Four doubles -> four int32.  For x in [0, 255.5) the rule equals trunc(x + h) with h = the largest double below 0.5: the sum
// is exact or rounds to a neighbour on the same side of the next integer for every x but the ties x = n + 0.5, whose sum
// n + 1 - 2^-54 rounds up to n + 1 as the rule wants (n = 0: a tie that goes to the even 1.0); with h = 0.5 itself the
// largest double below 0.5 would come out as 1.  tools/host_marshal.cpp --check walks the neighbours of every n + 0.5.
// Out-of-range values and NaN are clamped (the row is redone) and set *badv.
__attribute__((target("avx2"))) static inline __m128i round4_avx2(const double *p, __m256d *badv) {
  const __m256d x = _mm256_loadu_pd(p);
  const __m256d xc = _mm256_min_pd(_mm256_max_pd(x, _mm256_setzero_pd()), _mm256_set1_pd(255.49999999999997));   // NaN -> 0 (max returns its second operand)
  *badv = _mm256_or_pd(*badv, _mm256_cmp_pd(xc, x, _CMP_NEQ_UQ));  // (-0.0 == 0.0: in range)
  return _mm256_cvttpd_epi32(_mm256_add_pd(xc, _mm256_set1_pd(0.49999999999999994)));
}

__attribute__((target("avx2")))
bool round_quality_row_avx2(const double *__restrict__ src, uint8_t *__restrict__ dst, int L, int *mx_out) {
  __m256d badv = _mm256_setzero_pd();
  __m128i mxv = _mm_setzero_si128();
  int p = 0;
  for (; p + 16 <= L; p += 16) {
    const __m128i a = round4_avx2(src + p, &badv), b = round4_avx2(src + p + 4, &badv);
    const __m128i c = round4_avx2(src + p + 8, &badv), d = round4_avx2(src + p + 12, &badv);
    const __m128i bytes = _mm_packus_epi16(_mm_packs_epi32(a, b), _mm_packs_epi32(c, d));   // values are 0..255: no saturation
    mxv = _mm_max_epu8(mxv, bytes);
    _mm_storeu_si128((__m128i *)(dst + p), bytes);
  }
  int ok = _mm256_movemask_pd(badv) == 0, mx = 0;
  for (; p < L; p++) {                                             // scalar tail: nothing behind src[L - 1] is read
    const int v = round_one(src[p], &ok);
    mx = v > mx ? v : mx;
    dst[p] = (uint8_t)v;
  }
  mxv = _mm_max_epu8(mxv, _mm_srli_si128(mxv, 8));
  mxv = _mm_max_epu8(mxv, _mm_srli_si128(mxv, 4));
  mxv = _mm_max_epu8(mxv, _mm_srli_si128(mxv, 2));
  mxv = _mm_max_epu8(mxv, _mm_srli_si128(mxv, 1));
  const int vm = _mm_cvtsi128_si32(mxv) & 255;
  *mx_out = vm > mx ? vm : mx;
  return ok != 0;
}
#endif

// ---- 2-bit packing -------------------------------------------------------------------------------
// The first len characters of q as W2 words of sixteen 2-bit codes (A C G T = 0 1 2 3, base k of a word in bits 2k..2k+1), the
// words behind the last base zero.  Returns non-zero if any of the len bytes is not one of A C G T (its code is 0): an
// OR-accumulator, no branch and no store per base.  Nothing behind q[len - 1] is read.
namespace {
struct PackTab {
  uint8_t t[256];
  constexpr PackTab() : t() {
    for (int c = 0; c < 256; c++) t[c] = 0x80;
    t['A'] = 0; t['C'] = 1; t['G'] = 2; t['T'] = 3;               // = ((c >> 1) ^ (c >> 2)) & 3 for these four
  }
};
constexpr PackTab pack_tab;

// words [w, W2) of the row from base p on, by the table
inline uint32_t pack_tail(const char *q, int len, int p, uint32_t *row, int w, int W2) {
  uint32_t bad = 0;
  for (; w < W2; w++) {
    uint32_t word = 0;
    const int e = len - p < 16 ? (len - p > 0 ? len - p : 0) : 16;
    for (int k = 0; k < e; k++, p++) {
      const uint32_t t = pack_tab.t[(uint8_t)q[p]];
      bad |= t;
      word |= (t & 3u) << (k << 1);
    }
    row[w] = word;
  }
  return bad & 0x80u;
}
}  // namespace

uint32_t pack_row_2bit_scalar(const char *q, int len, uint32_t *row, int W2) { return pack_tail(q, len, 0, row, 0, W2); }

#ifdef D2_HOSTSIMD_AVX2
__attribute__((target("avx2")))
uint32_t pack_row_2bit_avx2(const char *q, int len, uint32_t *row, int W2) {
  __m256i badv = _mm256_setzero_si256();
  int p = 0, w = 0;
  for (; p + 32 <= len && w + 2 <= W2; p += 32, w += 2) {
    const __m256i c = _mm256_loadu_si256((const __m256i *)(q + p));
    const __m256i valid = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(c, _mm256_set1_epi8('A')), _mm256_cmpeq_epi8(c, _mm256_set1_epi8('C'))),
                                          _mm256_or_si256(_mm256_cmpeq_epi8(c, _mm256_set1_epi8('G')), _mm256_cmpeq_epi8(c, _mm256_set1_epi8('T'))));
    badv = _mm256_or_si256(badv, _mm256_xor_si256(valid, _mm256_set1_epi8(-1)));
    // ((c >> 1) ^ (c >> 2)) & 3 per byte (16-bit shifts: the bits that cross a byte border are masked off), 0 for invalid bytes
    __m256i code = _mm256_and_si256(_mm256_xor_si256(_mm256_srli_epi16(c, 1), _mm256_srli_epi16(c, 2)), _mm256_set1_epi8(3));
    code = _mm256_and_si256(code, valid);
    const __m256i n4 = _mm256_maddubs_epi16(code, _mm256_set1_epi16(0x0401));      // two bases per 16 bits: b0 + 4 b1
    const __m256i n8 = _mm256_madd_epi16(n4, _mm256_set1_epi32(0x00100001));       // four bases per 32 bits: n0 + 16 n1
    const __m256i h = _mm256_packus_epi32(n8, n8);
    const __m256i b = _mm256_packus_epi16(h, h);                                   // per 128-bit half: its sixteen bases in 4 bytes
    row[w] = (uint32_t)_mm256_extract_epi32(b, 0);
    row[w + 1] = (uint32_t)_mm256_extract_epi32(b, 4);
  }
  const uint32_t bad = (uint32_t)(_mm256_testz_si256(badv, badv) == 0);
  return bad | pack_tail(q, len, p, row, w, W2);
}
#endif

// ---- the forms by name (tools/host_marshal.cpp, tests/test_host_marshal.py) and the load-time choice ----------------------
typedef bool (*round_fn)(const double *, uint8_t *, int, int *);
typedef uint32_t (*pack_fn)(const char *, int, uint32_t *, int);

static bool have_avx2() {
#ifdef D2_HOSTSIMD_AVX2
  __builtin_cpu_init();                                            // (called from a static initialiser)
  return __builtin_cpu_supports("avx2") != 0;
#else
  return false;
#endif
}

// 0 = the name is unknown, 1 = compiled and usable on this CPU, -1 = compiled in but this CPU lacks it
int hostsimd_variant(const char *name, round_fn *r, pack_fn *p) {
  if (!strcmp(name, "scalar")) { *r = round_quality_row_scalar; *p = pack_row_2bit_scalar; return 1; }
#ifdef D2_HOSTSIMD_AVX2
  if (!strcmp(name, "avx2")) { *r = round_quality_row_avx2; *p = pack_row_2bit_avx2; return have_avx2() ? 1 : -1; }
#endif
  return 0;
}

namespace {
struct Chosen {
  round_fn r = round_quality_row_scalar;
  pack_fn p = pack_row_2bit_scalar;
  Chosen() { if (have_avx2()) hostsimd_variant("avx2", &r, &p); }
};
const Chosen chosen;
}  // namespace

bool round_quality_row(const double *src, uint8_t *dst, int L, int *mx_out) { return chosen.r(src, dst, L, mx_out); }
uint32_t pack_row_2bit(const char *q, int len, uint32_t *row, int W2) { return chosen.p(q, len, row, W2); }

// ---- the fused upload pass: everything the boundary does to a row, in one visit (marshal.h) --------------------------------
void marshal_rows(const MarshalRows &m, size_t lo, size_t hi, MarshalTally *t) {
  for (size_t i = lo; i < hi; i++) {
    const int l = (int)strnlen(m.seqs[i], (size_t)m.len_cap + 1);
    m.len[i] = l;
    t->maxlen = l > t->maxlen ? l : t->maxlen;
    t->minlen = l < t->minlen ? l : t->minlen;
    m.reads[i] = (uint32_t)m.abund[i];
    t->reads += (uint32_t)m.abund[i];
    m.prior[i] = m.priors && m.priors[i] ? 1 : 0;
    if (l > m.stride || l >= m.len_cap) continue;                  // (an input error: the caller raises it, the row is only recorded)
    t->bad_base |= pack_row_2bit(m.seqs[i], l, m.packed + i * (size_t)m.W2, m.W2);
    const double *src = m.quals + i * (size_t)m.stride;
    uint8_t *dst = m.qbytes + i * (size_t)m.LQ;
    // the row by the branch-free sweep - valid for values in [0, 255.5); a row with anything else (negative, too large, NaN
    // inside the read) is redone by the exact scalar rule
    int row_mx = 0;
    if (!round_quality_row(src, dst, l, &row_mx)) {
      row_mx = 0;
      for (int p = 0; p < l; p++) {
        const double x = src[p];
        double xr;
        if (x >= 0.0 && x < 256.0) { const int v = (int)x; xr = (double)(v + ((x - (double)v) >= 0.5 ? 1 : 0)); }   // round(): half away from zero
        else xr = std::round(x);
        if (!(xr >= 0.0 && xr <= 255.0)) { t->bad_qual = 1; xr = 0.0; }
        const int v = (int)xr;
        row_mx = v > row_mx ? v : row_mx;
        dst[p] = (uint8_t)v;
      }
    }
    t->qmax = row_mx > t->qmax ? row_mx : t->qmax;
    memset(dst + l, 0, (size_t)(m.LQ - l));
  }
}

}  // namespace d2
