// tools/host_marshal.cpp — timing and check program for the host loops of the boundary's marshalling (dada2_amd/csrc/hostsimd.cpp).
// Plain C++, no HIP; linked with hostsimd.o:
//   hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -x c++ tools/host_marshal.cpp dada2_amd/csrc/hostsimd.cpp -lpthread -o host_marshal
//
//   host_marshal [--threads n] [--rows N] [--len L] [--reps r]
//       over a synthetic N x L matrix (default 10^6 x 250, 2 GB of doubles) on n threads, best of r:
//         sum          vectorised streaming sum of the doubles: the host's read ceiling for the matrix
//         round/...    the quality conversion, scalar rule and every other compiled form
//         pack/switch  the 2-bit packing as a switch per base (the form sample_create had), then hostsimd.cpp's forms
//   host_marshal --check [--variant scalar|avx2]
//       compares a form of hostsimd.cpp against the rules restated below, on inputs with no slack behind the last element.
//       Exit status: 0 = all equal, 1 = a difference, 77 = this CPU lacks the variant, 2 = no such variant.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include <sys/mman.h>
#include <unistd.h>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace d2 {   // (hostsimd.cpp; engine.h declares the two dispatchers for the library, but pulls in the HIP runtime)
typedef bool (*round_fn)(const double *, uint8_t *, int, int *);
typedef uint32_t (*pack_fn)(const char *, int, uint32_t *, int);
int hostsimd_variant(const char *name, round_fn *r, pack_fn *p);
bool round_quality_row(const double *src, uint8_t *dst, int L, int *mx_out);
uint32_t pack_row_2bit(const char *q, int len, uint32_t *row, int W2);
}  // namespace d2

namespace {

// ---- the rules, restated ---------------------------------------------------------------------------
bool rule_in_range(double x) { return x >= 0.0 && x < 255.5; }
int rule_round(double x) { const int t = (int)x; return t + ((x - (double)t) >= 0.5 ? 1 : 0); }
bool rule_acgt(unsigned char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
// the packing loop sample_create had: a switch per base, invalid bytes pack as 0
uint32_t rule_pack(const char *q, int l, uint32_t *row, int W2) {
  uint32_t bad = 0;
  int p = 0;
  for (int w = 0; w < W2; w++) {
    uint32_t word = 0;
    const int e = std::max(0, std::min(l - p, 16));
    for (int k = 0; k < e; k++, p++) {
      uint32_t c;
      switch (q[p]) {
        case 'A': c = 0; break;
        case 'C': c = 1; break;
        case 'G': c = 2; break;
        case 'T': c = 3; break;
        default: c = 0; bad = 1;
      }
      word |= c << (k << 1);
    }
    row[w] = word;
  }
  return bad;
}

// ---- an array of exactly n elements: an access behind the last one faults ------------------------------
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define TIGHT_BY_ASAN 1
#endif
#endif
template <typename T> struct Tight {
  T *p = nullptr;
  size_t n = 0;
#ifdef TIGHT_BY_ASAN
  explicit Tight(size_t count) : n(count) { p = (T *)malloc(std::max<size_t>(1, n * sizeof(T))); }   // (the sanitizer's red zone follows)
  ~Tight() { free(p); }
#else
  void *map = nullptr;
  size_t map_bytes = 0;
  explicit Tight(size_t count) : n(count) {   // the array ends where an inaccessible page begins
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), bytes = n * sizeof(T);
    map_bytes = (bytes + page - 1) / page * page + page;
    map = mmap(nullptr, map_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (map == MAP_FAILED) { perror("mmap"); exit(3); }
    mprotect((char *)map + map_bytes - page, page, PROT_NONE);
    p = (T *)((char *)map + map_bytes - page - bytes);
  }
  ~Tight() { munmap(map, map_bytes); }
#endif
  Tight(const Tight &) = delete;
  Tight &operator=(const Tight &) = delete;
  T &operator[](size_t i) { return p[i]; }
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int fails = 0;
void fail(const char *what, int a, int b, int c) {
  if (fails++ < 20) fprintf(stderr, "FAIL %s (%d, %d, %d)\n", what, a, b, c);
}

// ---- --check -------------------------------------------------------------------------------------------
void check_round(d2::round_fn f) {
  const double special[] = {0.0, 0.5, 1.5, 2.5, 29.4999, 30.5, 254.5, 255.49, std::nextafter(0.5, 0.0), -0.0};
  const int nspecial = (int)(sizeof special / sizeof special[0]);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double outside[] = {-0.2, 255.5, 256.0, 1e300, -1.0, nan, inf, -inf};
  std::vector<int> lengths;
  for (int L = 1; L <= 70; L++) lengths.push_back(L);
  lengths.push_back(250); lengths.push_back(251); lengths.push_back(1510);
  for (int L : lengths) {
    Tight<double> src(L);
    Tight<uint8_t> dst(L);
    // every special value at every position (the rotation moves them through the 16-wide body and the tail), random values between
    for (int rot = 0; rot < 2 * nspecial; rot++) {
      for (int p = 0; p < L; p++)
        src[p] = (p + rot) % 2 == 0 ? special[((p + rot) / 2) % nspecial] : (double)(rng() >> 11) * (1.0 / 9007199254740992.0) * 255.5;
      for (int p = 0; p < L; p++) if (!rule_in_range(src[p])) src[p] = 255.49;   // (255.5 itself cannot come out of the product; be sure)
      memset(dst.p, 0xAA, L);
      int mx = -1, want_mx = 0;
      if (!f(src.p, dst.p, L, &mx)) fail("round: valid row reported for redo", L, rot, 0);
      for (int p = 0; p < L; p++) {
        const int v = rule_round(src[p]);
        want_mx = std::max(want_mx, v);
        if (dst[p] != (uint8_t)v) fail("round: byte differs", L, rot, p);
      }
      if (mx != want_mx) fail("round: row maximum differs", L, rot, mx);
    }
    // the neighbours of every n + 0.5 and of every n (three doubles to either side), at every position
    if (L == 16 || L == 17 || L == 251) {
      for (int n = 0; n <= 255; n++)
        for (int half = 0; half < 2; half++) {
          double lo = n + 0.5 * half, v[7];
          if (n == 255 && half) break;                             // (255.5 is outside)
          v[3] = lo;
          for (int k = 1; k <= 3; k++) { v[3 + k] = std::nextafter(v[3 + k - 1], 1e9); v[3 - k] = n + half == 0 ? 0.0 : std::nextafter(v[3 - k + 1], -1.0); }
          for (int rot = 0; rot < 7; rot++) {
            for (int p = 0; p < L; p++) src[p] = v[(p + rot) % 7];
            int mx = 0;
            if (!f(src.p, dst.p, L, &mx)) fail("round: neighbour of a half reported for redo", L, n, half);
            for (int p = 0; p < L; p++) if (dst[p] != (uint8_t)rule_round(src[p])) fail("round: byte differs next to a half", L, n, p);
          }
        }
    }
    // a value outside [0, 255.5) at the first, a middle and the last position: the row is reported for redo
    for (double bad : outside) {
      const int pos[3] = {0, L / 2, L - 1};
      for (int k = 0; k < 3; k++) {
        for (int p = 0; p < L; p++) src[p] = (double)(p % 41);
        src[pos[k]] = bad;
        int mx = 0;
        if (f(src.p, dst.p, L, &mx)) fail("round: row with a value outside the range accepted", L, pos[k], (int)(&bad - outside));
      }
    }
    // NaN behind the read's end (the row of a shorter read in a wider matrix) is not looked at
    {
      Tight<double> wide(L + 3);
      for (int p = 0; p < L; p++) wide[p] = (double)(p % 41) + 0.5;
      wide[L] = nan; wide[L + 1] = nan; wide[L + 2] = -1.0;
      int mx = 0;
      if (!f(wide.p, dst.p, L, &mx)) fail("round: NaN behind L looked at", L, 0, 0);
      for (int p = 0; p < L; p++) if (dst[p] != (uint8_t)rule_round(wide[p])) fail("round: byte differs (NaN behind L)", L, 0, p);
    }
  }
}

void check_pack(d2::pack_fn f) {
  std::vector<int> lengths;
  for (int L = 6; L <= 70; L++) lengths.push_back(L);
  lengths.push_back(250); lengths.push_back(1510);
  for (int L : lengths) {
    const int W2 = (((L + 15) / 16) + 3) & ~3;
    Tight<char> q(L);
    Tight<uint32_t> got(W2);
    std::vector<uint32_t> want(W2);
    for (int p = 0; p < L; p++) q[p] = "ACGT"[rng() & 3];
    auto compare = [&](int a, int b) {
      for (int w = 0; w < W2; w++) got[w] = 0xDEADBEEFu;
      const uint32_t bad = f(q.p, L, got.p, W2), want_bad = rule_pack(q.p, L, want.data(), W2);
      if ((bad != 0) != (want_bad != 0)) fail("pack: invalid flag differs", L, a, b);
      for (int w = 0; w < W2; w++) if (got[w] != want[w]) fail("pack: word differs", L, a, w);
      for (int w = (L + 15) / 16; w < W2; w++) if (got[w] != 0) fail("pack: padding word not zero", L, a, w);
    };
    compare(-1, -1);
    // every byte value at every position (all positions mod 32 of the vector body where the row has one, and the tail)
    if (L <= 70 || L == 250) {
      for (int p = 0; p < L; p++) {
        if (L > 70 && p >= 64 && p < L - 32) continue;           // (250: the first two blocks and the last 32 positions)
        const char keep = q[p];
        for (int b = 0; b < 256; b++) {
          q[p] = (char)b;
          compare(p, b);
          const uint32_t bad = f(q.p, L, got.p, W2);
          if ((bad != 0) != !rule_acgt((unsigned char)b)) fail("pack: invalid flag not exactly for non-ACGT bytes", L, p, b);
        }
        q[p] = keep;
      }
    }
  }
}

// ---- timing ----------------------------------------------------------------------------------------------
#if defined(__x86_64__)
__attribute__((target("avx2"))) double sum_avx2(const double *p, size_t n) {
  __m256d a = _mm256_setzero_pd(), b = a, c = a, d = a;
  size_t i = 0;
  for (; i + 16 <= n; i += 16) {
    a = _mm256_add_pd(a, _mm256_loadu_pd(p + i)); b = _mm256_add_pd(b, _mm256_loadu_pd(p + i + 4));
    c = _mm256_add_pd(c, _mm256_loadu_pd(p + i + 8)); d = _mm256_add_pd(d, _mm256_loadu_pd(p + i + 12));
  }
  double t[4];
  _mm256_storeu_pd(t, _mm256_add_pd(_mm256_add_pd(a, b), _mm256_add_pd(c, d)));
  double s = t[0] + t[1] + t[2] + t[3];
  for (; i < n; i++) s += p[i];
  return s;
}
#endif
double sum_plain(const double *p, size_t n) { double s = 0; for (size_t i = 0; i < n; i++) s += p[i]; return s; }

template <typename F> void on_threads(int nt, size_t rows, F f) {
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++) th.emplace_back([=] { f(rows * t / nt, rows * (t + 1) / nt, t); });
  for (auto &x : th) x.join();
}
template <typename F> double best_ms(int reps, F f) {
  double best = 1e300;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    f();
    best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  return best;
}

int timing(int nt, size_t rows, int L, int reps) {
  const int LQ = (L + 15) & ~15, W2 = (((L + 15) / 16) + 3) & ~3;
  const size_t S = (size_t)L + 1;
  double *quals = (double *)malloc(rows * L * sizeof(double));
  char *seqs = (char *)malloc(rows * S);
  uint8_t *qb = (uint8_t *)malloc(rows * LQ);
  uint32_t *words = (uint32_t *)malloc(rows * W2 * 4);
  if (!quals || !seqs || !qb || !words) { fprintf(stderr, "out of memory\n"); return 3; }
  on_threads(nt, rows, [=](size_t lo, size_t hi, int t) {   // (first touch by the thread that will read it)
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(t + 1);
    for (size_t r = lo; r < hi; r++) {
      for (int p = 0; p < L; p++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        quals[r * L + p] = (double)(2 + (x >> 40) % 39) + ((x >> 20) & 3) * 0.25;   // mean qualities of a few reads: quarters
        seqs[r * S + p] = "ACGT"[(x >> 10) & 3];
      }
      seqs[r * S + L] = 0;
      memset(qb + r * LQ, 0, LQ);
      memset(words + r * W2, 0, (size_t)W2 * 4);
    }
  });
  const double gb_q = (double)rows * L * 8 / 1e9, gb_s = (double)rows * L / 1e9, n_el = (double)rows * L;
  printf("# %zu rows x %d, %d threads, best of %d\n", rows, L, nt, reps);
  printf("%-14s %10s %10s %12s %18s\n", "pass", "ms", "GB/s read", "ns/element", "checksum");
  std::vector<double> part(nt);
  std::vector<uint64_t> ck(nt);
  auto line = [&](const char *name, double ms, double gb, uint64_t sum) {
    printf("%-14s %10.2f %10.1f %12.3f %18llx\n", name, ms, gb / (ms * 1e-3), ms * 1e6 * nt / n_el, (unsigned long long)sum);
  };
  {
#if defined(__x86_64__)
    const bool v = __builtin_cpu_supports("avx2");
#else
    const bool v = false;
#endif
    const double ms = best_ms(reps, [&] {
      on_threads(nt, rows, [&, v](size_t lo, size_t hi, int t) {
#if defined(__x86_64__)
        part[t] = v ? sum_avx2(quals + lo * L, (hi - lo) * L) : sum_plain(quals + lo * L, (hi - lo) * L);
#else
        part[t] = sum_plain(quals + lo * L, (hi - lo) * L);
#endif
      });
    });
    double s = 0;
    for (double x : part) s += x;
    line("sum", ms, gb_q, (uint64_t)s);
  }
  const char *names[] = {"scalar", "avx2"};
  for (const char *nm : names) {
    d2::round_fn rf; d2::pack_fn pf;
    if (d2::hostsimd_variant(nm, &rf, &pf) != 1) continue;
    const double ms = best_ms(reps, [&] {
      on_threads(nt, rows, [&](size_t lo, size_t hi, int t) {
        uint64_t c = 0;
        for (size_t r = lo; r < hi; r++) { int mx; rf(quals + r * L, qb + r * LQ, L, &mx); c += (uint64_t)mx; }
        ck[t] = c;
      });
    });
    uint64_t c = 0;
    for (size_t i = 0; i < rows * (size_t)LQ; i++) c = c * 31 + qb[i];
    line((std::string("round/") + nm).c_str(), ms, gb_q, c);
  }
  for (int k = -1; k < 2; k++) {
    d2::round_fn rf; d2::pack_fn pf = rule_pack;
    if (k >= 0 && d2::hostsimd_variant(names[k], &rf, &pf) != 1) continue;
    const double ms = best_ms(reps, [&] {
      on_threads(nt, rows, [&](size_t lo, size_t hi, int t) {
        uint32_t bad = 0;
        for (size_t r = lo; r < hi; r++) bad |= pf(seqs + r * S, L, words + r * W2, W2);
        ck[t] = bad;
      });
    });
    uint64_t c = 0;
    for (size_t i = 0; i < rows * (size_t)W2; i++) c = c * 31 + words[i];
    line(k < 0 ? "pack/switch" : (std::string("pack/") + names[k]).c_str(), ms, gb_s, c);
  }
  free(quals); free(seqs); free(qb); free(words);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  bool check = false;
  const char *variant = nullptr;
  int nt = 1, L = 250, reps = 3;
  size_t rows = 1000000;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--check") check = true;
    else if (a == "--variant" && i + 1 < argc) variant = argv[++i];
    else if (a == "--threads" && i + 1 < argc) nt = std::max(1, atoi(argv[++i]));
    else if (a == "--rows" && i + 1 < argc) rows = (size_t)std::max(1ll, atoll(argv[++i]));
    else if (a == "--len" && i + 1 < argc) L = std::max(1, atoi(argv[++i]));
    else if (a == "--reps" && i + 1 < argc) reps = std::max(1, atoi(argv[++i]));
    else { fprintf(stderr, "usage: host_marshal [--threads n] [--rows N] [--len L] [--reps r] | --check [--variant scalar|avx2]\n"); return 2; }
  }
  if (!check) return timing(nt, rows, L, reps);
  d2::round_fn rf = d2::round_quality_row;      // no --variant: the form the library would use on this CPU
  d2::pack_fn pf = d2::pack_row_2bit;
  if (variant) {
    const int have = d2::hostsimd_variant(variant, &rf, &pf);
    if (have == 0) { fprintf(stderr, "no such variant: %s\n", variant); return 2; }
    if (have < 0) { fprintf(stderr, "this CPU lacks %s\n", variant); return 77; }
  }
  check_round(rf);
  check_pack(pf);
  if (fails) { fprintf(stderr, "%d difference(s)\n", fails); return 1; }
  printf("host_marshal --check %s: ok\n", variant ? variant : "(load-time choice)");
  return 0;
}
