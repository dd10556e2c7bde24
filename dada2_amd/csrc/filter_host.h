// filter_host.h — host side of filterAndTrim's per-read verdicts (R/filter.R:613-730; src/filter.cpp); included by driver.cpp inside
// its extern "C" block, behind species_host.h.  The file-level entries (dada2hip_filter_fastq, _paired) are derep.cpp's, where the
// FASTQ reader is; they call dada2hip_filter_reads per chunk.
//
// dada2hip_filter_open builds the word table of C_matchRef (src/filter.cpp:13-18: the reference extended by its own first
// word_size letters, its `len` windows) for the reference and for its reverse complement (R/filter.R:1183) as ONE sorted array of
// distinct keys with two flag bits, in the key form of filter.inc.hip, and the two tables pow(10.0, -q / 10.0) per quality
// CHARACTER (offset 33 and 64) with the host's pow, so that every term of the EE sum is the reference's bit for bit.
// dada2hip_filter_reads cuts the call into pieces of at most FT_PIECE_READS reads / FT_PIECE_BYTES bytes (DADA2HIP_FILTER_PIECE,
// DADA2HIP_FILTER_PIECE_BYTES: fewer, for the tests) and runs them through two slots, each with pinned staging, device buffers and
// a stream of its own: while the kernels of one piece run, the host copies the next piece into the other slot's pinned buffers and
// queues its upload, so the copy of piece k + 1 runs under the kernels of piece k.  The Shannon number of seqComplexity
// (:1271-1275) is computed here from the device's integer counts.
#pragma once

namespace {

constexpr int64_t FT_PIECE_READS = 1 << 16;
constexpr int64_t FT_PIECE_BYTES = 32 << 20;

struct FtSlot {
  PinBuf<uint8_t> h_seq, h_qual;
  PinBuf<long long> h_off;
  PinBuf<FilterOut> h_out;
  PinBuf<int32_t> h_km;
  DevBuf<uint8_t> d_seq, d_qual;
  DevBuf<long long> d_off;
  DevBuf<FilterOut> d_out;
  DevBuf<int32_t> d_km;
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t first = 0, count = 0;
  bool busy = false;
  ~FtSlot() {
    for (int i = 0; i < 4; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (st) (void)hipStreamDestroy(st);
  }
};

}  // namespace

struct dada2hip_filter {
  int device = 0;
  int word_size = 0, nkeys = 0;
  bool in_lds = false;
  DevBuf<unsigned long long> keys;
  DevBuf<uint8_t> flags;
  DevBuf<double> ee_tab;               // [2][256]: offset 33, offset 64
  FtSlot slot[2];
  std::mutex mu;                       // calls on one context take turns (its slots and streams)
};

namespace {

enum { FS_IN = 0, FS_KEPT, FS_STAGE1, FS_KEYS = 13, FS_LDS, FS_BYTES, FS_US_UP, FS_US_SCAN, FS_US_EE, FS_US_KMERS, FS_US_DOWN, FS_US_PARSE,
       FS_US_DEFLATE, FS_US_WRITE, FS_US_TOTAL };

inline int ft_base(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// the keys of the `len` circular windows of s (filter.inc.hip's form: the two bit planes of the window side by side)
void ft_strand_keys(const std::string &s, int W, std::vector<unsigned long long> &keys) {
  const size_t len = s.size();
  std::string e = s;
  e.append(s, 0, (size_t)W);                                   // src/filter.cpp:14
  keys.resize(len);
  parallel_for(len, 1024, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      unsigned long long k = 0;
      for (int t = 0; t < W; t++) {
        const unsigned long long b = (unsigned long long)ft_base(e[i + (size_t)t]);
        k |= (b & 1ull) << t | (b >> 1) << (32 + t);
      }
      keys[i] = k;
    }
  });
}

void filter_open_body(const char *ref, int32_t word_size, int32_t device, dada2hip_filter **out, int64_t *stats) {
  auto t_call = clk::now();
  if (!out) throw InputError{"dada2hip: bad arguments"};
  *out = nullptr;
  std::vector<unsigned long long> keys;
  std::vector<uint8_t> flags;
  if (ref) {
    if (word_size < 1 || word_size > 32) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: the screen's word size must be 1..32 (one 64-bit key)."};
    const std::string s(ref);
    for (char c : s)
      if (ft_base(c) < 0) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: the screen's reference sequence must be upper-case A/C/G/T only."};
    if (s.size() < (size_t)word_size) throw InputError{"dada2hip: the screen's reference sequence is shorter than the word size."};
    if (s.size() > (size_t)1 << 28) throw InputError{"dada2hip: the screen's reference sequence is too long."};
    std::string rc(s.rbegin(), s.rend());
    for (char &c : rc) c = "TGCA"[ft_base(c)];
    std::vector<unsigned long long> kf, kr;
    ft_strand_keys(s, word_size, kf);
    ft_strand_keys(rc, word_size, kr);
    std::vector<std::pair<unsigned long long, uint8_t>> all;
    all.reserve(kf.size() + kr.size());
    for (unsigned long long k : kf) all.emplace_back(k, (uint8_t)1);
    for (unsigned long long k : kr) all.emplace_back(k, (uint8_t)2);
    std::sort(all.begin(), all.end());
    for (const auto &kv : all) {
      if (!keys.empty() && keys.back() == kv.first) flags.back() |= kv.second;
      else { keys.push_back(kv.first); flags.push_back(kv.second); }
    }
  }
  std::vector<double> tab(512);
  for (int c = 0; c < 256; c++) {
    tab[c] = pow(10.0, -(c - 33) / 10.0);                      // src/filter.cpp:44
    tab[256 + c] = pow(10.0, -(c - 64) / 10.0);
  }
  select_device(device);
  std::unique_ptr<dada2hip_filter> m(new dada2hip_filter());
  m->device = device; m->word_size = ref ? word_size : 0; m->nkeys = (int)keys.size();
  m->in_lds = !keys.empty() && keys.size() * 9 + 8 <= (size_t)FT_LDS_MAX;
  for (FtSlot &S : m->slot) {
    D2_HIP(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
    for (int i = 0; i < 4; i++) D2_HIP(hipEventCreate(&S.ev[i]));
  }
  m->keys.alloc(keys.size()); m->flags.alloc(flags.size()); m->ee_tab.alloc(512);
  if (!keys.empty()) {
    D2_HIP(hipMemcpy(m->keys.p, keys.data(), keys.size() * 8, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(m->flags.p, flags.data(), flags.size(), hipMemcpyHostToDevice));
  }
  D2_HIP(hipMemcpy(m->ee_tab.p, tab.data(), 512 * 8, hipMemcpyHostToDevice));
  if (stats) {
    memset(stats, 0, DADA2HIP_FILTER_NSTATS * sizeof(int64_t));
    stats[FS_KEYS] = m->nkeys; stats[FS_LDS] = m->in_lds ? 1 : 0; stats[FS_BYTES] = (int64_t)(keys.size() * 9 + 512 * 8);
    stats[FS_US_TOTAL] = (int64_t)(ms_since(t_call) * 1e3);
  }
  *out = m.release();
}

void filter_reads_body(dada2hip_filter *m, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                       const dada2hip_filter_params *P, int32_t *code, int32_t *window, double *ee, int32_t *hits, int32_t *kmer_counts,
                       double *complexity, int64_t *stats) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_FILTER_NSTATS] = {0};
  if (!m) throw InputError{"dada2hip: no filter context."};
  if (!P || n < 0 || (n > 0 && (!seq || !qual || !offsets))) throw InputError{"dada2hip: bad arguments"};
  if (P->qual_offset != 0 && P->qual_offset != 33 && P->qual_offset != 64) throw InputError{"dada2hip: the quality offset must be 33, 64 or 0 (Auto)."};
  if (P->kmer_size < 0 || P->kmer_size > 4) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: seqComplexity's kmerSize must be 1..4."};
  if (P->rm_phix && m->nkeys == 0) throw InputError{"dada2hip: rm_phix needs a context opened with the screen's reference sequence."};
  if (P->rm_phix && P->min_matches < 1) throw InputError{"dada2hip: minMatches must be at least 1."};
  const int k = P->kmer_size == 0 ? 2 : P->kmer_size, nb = 1 << (2 * k);
  const bool want_km = kmer_counts || complexity || P->rm_lowcomplex > 0;
  for (int64_t r = 0; r < n; r++) {
    const int64_t l = offsets[r + 1] - offsets[r];
    if (l < 0 || l > (int64_t)INT32_MAX - 128) throw InputError{"dada2hip: bad read offsets."};
  }
  st[FS_IN] = n; st[FS_KEYS] = m->nkeys; st[FS_LDS] = m->in_lds ? 1 : 0;
  int offset = P->qual_offset;
  if (offset == 0) {                                           // Auto, as dada2hip_derep_fastq: below ';' only Phred+33 encodings
    const size_t b0 = n ? (size_t)offsets[0] : 0, b1 = n ? (size_t)offsets[n] : 0;
    std::atomic<int> mn{255};
    parallel_for(b1 - b0, (size_t)1 << 20, [&](size_t lo, size_t hi) {
      int v = 255;
      for (size_t i = lo; i < hi; i++) v = std::min(v, (int)(unsigned char)qual[b0 + i]);
      int cur = mn.load();
      while (v < cur && !mn.compare_exchange_weak(cur, v)) {}
    });
    offset = mn.load() < 59 ? 33 : 64;
  }
  FilterArgs A;
  const long long start = std::max<long long>(1, (long long)P->trim_left + 1);   // :622
  A.max_len = P->max_len; A.skip = (int)(start - 1); A.trim_right = P->trim_right; A.cut_char = P->trunc_q + offset;
  A.trunc_end = (long long)P->trunc_len >= start ? (int)(P->trunc_len - start + 1) : 0;   // :623-625
  A.min_len = P->min_len; A.max_n = P->max_n; A.minq_on = P->min_q > P->trunc_q ? 1 : 0; A.minq_char = P->min_q + offset;
  A.ee_on = std::isfinite(P->max_ee) ? 1 : 0; A.max_ee = A.ee_on ? P->max_ee : 0.0;
  A.rm_phix = P->rm_phix ? 1 : 0; A.min_matches = P->min_matches; A.non_overlapping = P->non_overlapping ? 1 : 0;
  FilterTable T;
  T.keys = m->keys.p; T.flags = m->flags.p; T.nkeys = m->nkeys; T.word_size = m->word_size;

  std::lock_guard<std::mutex> lock(m->mu);
  select_device(m->device);
  const double *d_tab = m->ee_tab.p + (offset == 64 ? 256 : 0);
  auto harvest = [&](FtSlot &S) {
    if (!S.busy) return;
    auto t0 = clk::now();
    D2_HIP(hipStreamSynchronize(S.st));
    D2_HIP(hipGetLastError());
    S.busy = false;
    float ms = 0.0f;
    D2_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[1])); st[FS_US_SCAN] += (int64_t)((double)ms * 1e3);
    D2_HIP(hipEventElapsedTime(&ms, S.ev[1], S.ev[2])); st[FS_US_EE] += (int64_t)((double)ms * 1e3);
    D2_HIP(hipEventElapsedTime(&ms, S.ev[2], S.ev[3])); st[FS_US_KMERS] += (int64_t)((double)ms * 1e3);
    const int64_t f = S.first, c = S.count;
    const FilterOut *o = S.h_out.p;
    const int32_t *km = S.h_km.p;
    int64_t dropped[12] = {0};
    std::mutex cmu;
    parallel_for((size_t)c, 4096, [&](size_t lo, size_t hi) {
      int64_t loc[12] = {0};
      for (size_t i = lo; i < hi; i++) {
        int cd = o[i].code;
        double cx = 0.0;
        if (want_km) {
          const int32_t *x = km + i * (size_t)nb;
          if (kmer_counts) memcpy(kmer_counts + ((size_t)f + i) * nb, x, (size_t)nb * 4);
          if (complexity || cd == 0) {                         // sindex, :1271-1275
            long long tot = 0;
            for (int b = 0; b < nb; b++) tot += x[b];
            long double acc = 0.0L;                            // (R's sum() accumulates in long double)
            for (int b = 0; b < nb; b++)
              if (x[b] > 0) { const double y = (double)x[b] / (double)tot; acc += (long double)(-y * log(y)); }
            cx = tot > 0 ? exp((double)acc) : std::numeric_limits<double>::quiet_NaN();
            if (complexity) complexity[f + (int64_t)i] = cx;
            if (cd == 0 && P->rm_lowcomplex > 0 && !(cx >= P->rm_lowcomplex)) cd = 11;   // :705
          }
        }
        if (code) code[f + (int64_t)i] = cd;
        if (window) { window[2 * (f + (int64_t)i)] = o[i].off; window[2 * (f + (int64_t)i) + 1] = o[i].len; }
        if (ee) ee[f + (int64_t)i] = o[i].ee;
        if (hits) { hits[2 * (f + (int64_t)i)] = o[i].hits_f; hits[2 * (f + (int64_t)i) + 1] = o[i].hits_r; }
        loc[cd]++;
      }
      std::lock_guard<std::mutex> g(cmu);
      for (int s = 0; s < 12; s++) dropped[s] += loc[s];
    });
    st[FS_KEPT] += dropped[0];
    for (int s = 1; s < 12; s++) st[FS_STAGE1 + s - 1] += dropped[s];
    st[FS_US_DOWN] += (int64_t)(ms_since(t0) * 1e3);
  };
  struct Drain { dada2hip_filter *m; ~Drain() { for (FtSlot &S : m->slot) if (S.busy) { (void)hipStreamSynchronize(S.st); S.busy = false; } } } drain{m};

  const int64_t piece_reads = knobs().filter_piece > 0 ? std::min<int64_t>(knobs().filter_piece, FT_PIECE_READS) : FT_PIECE_READS;
  const int64_t piece_bytes = knobs().filter_piece_bytes > 0 ? std::min<int64_t>(knobs().filter_piece_bytes, FT_PIECE_BYTES) : FT_PIECE_BYTES;
  int64_t r0 = 0;
  for (int piece = 0; r0 < n; piece++) {
    int64_t r1 = r0 + 1;
    while (r1 < n && r1 - r0 < piece_reads && offsets[r1 + 1] - offsets[r0] <= piece_bytes) r1++;
    FtSlot &S = m->slot[piece & 1];
    harvest(S);
    auto t_up = clk::now();
    const int64_t c = r1 - r0, base = offsets[r0], bytes = offsets[r1] - base;
    S.h_seq.alloc((size_t)bytes); S.h_qual.alloc((size_t)bytes); S.h_off.alloc((size_t)c + 1); S.h_out.alloc((size_t)c);
    S.d_seq.alloc((size_t)bytes); S.d_qual.alloc((size_t)bytes); S.d_off.alloc((size_t)c + 1); S.d_out.alloc((size_t)c);
    if (want_km) { S.h_km.alloc((size_t)c * nb); S.d_km.alloc((size_t)c * nb); }
    parallel_for((size_t)bytes, (size_t)1 << 20, [&](size_t lo, size_t hi) {
      memcpy(S.h_seq.p + lo, seq + base + lo, hi - lo);
      memcpy(S.h_qual.p + lo, qual + base + lo, hi - lo);
    });
    for (int64_t i = 0; i <= c; i++) S.h_off.p[i] = (long long)(offsets[r0 + i] - base);
    if (bytes > 0) {
      D2_HIP(hipMemcpyAsync(S.d_seq.p, S.h_seq.p, (size_t)bytes, hipMemcpyHostToDevice, S.st));
      D2_HIP(hipMemcpyAsync(S.d_qual.p, S.h_qual.p, (size_t)bytes, hipMemcpyHostToDevice, S.st));
    }
    D2_HIP(hipMemcpyAsync(S.d_off.p, S.h_off.p, (size_t)(c + 1) * 8, hipMemcpyHostToDevice, S.st));
    D2_HIP(hipEventRecord(S.ev[0], S.st));
    launch_filter_scan(T, A, (int)c, S.d_seq.p, S.d_qual.p, S.d_off.p, S.d_out.p, S.st);
    D2_HIP(hipEventRecord(S.ev[1], S.st));
    launch_filter_ee(A, (int)c, S.d_qual.p, S.d_off.p, d_tab, S.d_out.p, S.st);
    D2_HIP(hipEventRecord(S.ev[2], S.st));
    if (want_km) launch_filter_kmers((int)c, k, S.d_seq.p, S.d_off.p, S.d_out.p, S.d_km.p, S.st);
    D2_HIP(hipEventRecord(S.ev[3], S.st));
    D2_HIP(hipMemcpyAsync(S.h_out.p, S.d_out.p, (size_t)c * sizeof(FilterOut), hipMemcpyDeviceToHost, S.st));
    if (want_km) D2_HIP(hipMemcpyAsync(S.h_km.p, S.d_km.p, (size_t)c * nb * 4, hipMemcpyDeviceToHost, S.st));
    S.first = r0; S.count = c; S.busy = true;
    st[FS_BYTES] += 2 * bytes + (c + 1) * 8;
    st[FS_US_UP] += (int64_t)(ms_since(t_up) * 1e3);
    r0 = r1;
  }
  harvest(m->slot[0]); harvest(m->slot[1]);
  st[FS_US_TOTAL] = (int64_t)(ms_since(t_call) * 1e3);
  if (stats) memcpy(stats, st, sizeof st);
}

}  // namespace

int dada2hip_filter_open(const char *ref, int32_t word_size, int32_t device, dada2hip_filter **out, int64_t *stats, char *errbuf,
                         size_t errlen) {
  return guarded(errbuf, errlen, [&] { filter_open_body(ref, word_size, device, out, stats); });
}

void dada2hip_filter_free(dada2hip_filter *ctx) { delete ctx; }

int dada2hip_filter_reads(dada2hip_filter *ctx, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                          const dada2hip_filter_params *params, int32_t *code, int32_t *window, double *ee, int32_t *hits,
                          int32_t *kmer_counts, double *complexity, int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen,
                 [&] { filter_reads_body(ctx, n, seq, qual, offsets, params, code, window, ee, hits, kmer_counts, complexity, stats); });
}
