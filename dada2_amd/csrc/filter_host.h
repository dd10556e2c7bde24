// filter_host.h — host side of filterAndTrim's per-read verdicts (R/filter.R:613-730; src/filter.cpp); included by driver.cpp inside
// its extern "C" block, behind species_host.h.  The file-level entries (dada2hip_filter_fastq, _paired) are derep.cpp's, where the
// FASTQ reader is; they call dada2hip_filter_reads per chunk.
//
// dada2hip_filter_open builds the word table of C_matchRef (src/filter.cpp:13-18: the reference extended by its own first
// word_size letters, its `len` windows) for the reference and for its reverse complement (R/filter.R:1183) as ONE sorted array of
// distinct keys with two flag bits, in the key form of filter.inc.hip, and the two tables pow(10.0, -q / 10.0) per quality
// CHARACTER (offset 33 and 64) with the host's pow, so that every term of the EE sum is the reference's bit for bit.
// dada2hip_filter_reads takes sequences and qualities up through read_pieces.h's two-slot pipeline (DADA2HIP_FILTER_PIECE,
// DADA2HIP_FILTER_PIECE_BYTES: smaller pieces, for the tests), the slots kept in the context, and supplies the three kernels
// between four events and the scatter, where the Shannon number of seqComplexity (:1271-1275) is computed from the device's
// integer counts.  dada2hip_filter_reads_oriented (orient.fwd, R/filter.R:648-658) is the same body with k_filter_orient in front
// and the kernels' oriented instances behind it; its stats words follow the filter's (FO_*, stage_stats.h).  From stage_common.h: the A/C/G/T code, the reverse complement, the clocks, the end of a call.
#pragma once

struct dada2hip_filter {
  int device = 0;
  int word_size = 0, nkeys = 0;
  bool in_lds = false;
  DevBuf<unsigned long long> keys;
  DevBuf<uint8_t> flags;
  DevBuf<double> ee_tab;               // [2][256]: offset 33, offset 64
  PieceSlot<FilterOut, 4> slot[2];     // aux: the k-mer counts
  Events<1> ev_orient[2];              // per slot, behind k_filter_orient (dada2hip_filter_reads_oriented)
  std::mutex mu;                       // calls on one context take turns (its slots and streams)
};

namespace {

using FtSlot = PieceSlot<FilterOut, 4>;
// what a caller of filter_reads_body may hang behind a piece's scatter: the piece's verdicts stand in the caller's arrays, its
// stream is idle and its reads still lie in the slot (derep_dev_host.h dereplicates the kept windows out of it)
using FilterPieceHook = std::function<void(FtSlot &)>;

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
        const unsigned long long b = (unsigned long long)acgt_code(e[i + (size_t)t]);
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
      if (acgt_code(c) < 0) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: the screen's reference sequence must be upper-case A/C/G/T only."};
    if (s.size() < (size_t)word_size) throw InputError{"dada2hip: the screen's reference sequence is shorter than the word size."};
    if (s.size() > (size_t)1 << 28) throw InputError{"dada2hip: the screen's reference sequence is too long."};
    std::vector<unsigned long long> kf, kr;
    ft_strand_keys(s, word_size, kf);
    ft_strand_keys(revcomp_acgt(s), word_size, kr);
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
  for (FtSlot &S : m->slot) S.create();
  for (auto &e : m->ev_orient) e.create();
  m->keys.alloc(keys.size()); m->flags.alloc(flags.size()); m->ee_tab.alloc(512);
  if (!keys.empty()) {
    D2_HIP(hipMemcpy(m->keys.p, keys.data(), keys.size() * 8, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(m->flags.p, flags.data(), flags.size(), hipMemcpyHostToDevice));
  }
  D2_HIP(hipMemcpy(m->ee_tab.p, tab.data(), 512 * 8, hipMemcpyHostToDevice));
  int64_t st[DADA2HIP_FILTER_NSTATS] = {0};
  st[FS_KEYS] = m->nkeys; st[FS_LDS] = m->in_lds ? 1 : 0; st[FS_BYTES] = (int64_t)(keys.size() * 9 + 512 * 8);
  finish_stats(st, FS_US_TOTAL, t_call, stats);
  *out = m.release();
}

// the barcode of orient.fwd as the kernel takes it (R/filter.R:650 C_isACGT, :651 barlen)
FilterBarcode filter_barcode(const char *orient_fwd) {
  FilterBarcode B;
  memset(&B, 0, sizeof B);
  const size_t len = strlen(orient_fwd);
  if (len == 0) throw InputError{"dada2hip: orient_fwd is empty."};
  if (len > (size_t)FT_ORIENT_MAX) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: orient_fwd is longer than 256 letters."};
  for (size_t i = 0; i < len; i++) {
    const int c = acgt_code(orient_fwd[i]);
    if (c < 0) throw InputError{"Non-ACGT characters detected in orient.fwd"};
    B.fwd[i] = (uint8_t)orient_fwd[i];
    B.comp[i] = (uint8_t)"TGCA"[c];
  }
  B.len = (int)len;
  return B;
}

// orient_fwd == nullptr: dada2hip_filter_reads.  Otherwise dada2hip_filter_reads_oriented in orient_mode 0 (single-end: both tests,
// a flipped read judged as its reverse complement) or 1 (the paired form: the forward test alone and nothing else - the caller
// rebuilds its chunks from the verdicts of both files before anything is judged)
void filter_reads_body(dada2hip_filter *m, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                       const dada2hip_filter_params *P, int32_t *code, int32_t *window, double *ee, int32_t *hits, int32_t *kmer_counts,
                       double *complexity, int64_t *stats, const char *orient_fwd = nullptr, int32_t orient_mode = 0,
                       int8_t *orient = nullptr, const FilterPieceHook *after_piece = nullptr) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_FILTER_NSTATS] = {0};
  if (!m) throw InputError{"dada2hip: no filter context."};
  const bool ori = orient_fwd != nullptr, only = ori && orient_mode == 1;
  if (ori && orient_mode != 0 && orient_mode != 1) throw InputError{"dada2hip: bad arguments"};
  FilterBarcode B;
  if (ori) B = filter_barcode(orient_fwd);
  if (only) {
    if (n < 0 || (n > 0 && (!seq || !offsets))) throw InputError{"dada2hip: bad arguments"};
    static const dada2hip_filter_params none = {-1, 0, 0, 0, 0, 0, INT32_MAX, 0, HUGE_VAL, 0.0, 0, 2, 1, 0, 33, 0};
    P = &none; qual = nullptr; ee = nullptr; hits = nullptr; kmer_counts = nullptr; complexity = nullptr;
  }
  if (!P || n < 0 || (n > 0 && (!seq || (!qual && !only) || !offsets))) throw InputError{"dada2hip: bad arguments"};
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
  if (offset == 0 && !only) {                                  // Auto, as dada2hip_derep_fastq: below ';' only Phred+33 encodings
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
  // ---- the stage's part of the pipeline: three kernels between four events; the scatter ----
  auto launch = [&](FtSlot &S, int c) {
    if (ori) {
      hipEvent_t e_or = m->ev_orient[&S - m->slot][0];
      launch_filter_orient(B, only ? 1 : 0, c, S.d_seq.p, S.d_off.p, S.d_out.p, S.st);
      D2_HIP(hipEventRecord(e_or, S.st));
      if (only) return;
      launch_filter_scan_oriented(T, A, c, S.d_seq.p, S.d_qual.p, S.d_off.p, S.d_out.p, S.st);
      D2_HIP(hipEventRecord(S.ev[1], S.st));
      launch_filter_ee_oriented(A, c, S.d_qual.p, S.d_off.p, d_tab, S.d_out.p, S.st);
      D2_HIP(hipEventRecord(S.ev[2], S.st));
      if (want_km) launch_filter_kmers_oriented(c, k, S.d_seq.p, S.d_off.p, S.d_out.p, S.d_aux.p, S.st);
      return;
    }
    launch_filter_scan(T, A, c, S.d_seq.p, S.d_qual.p, S.d_off.p, S.d_out.p, S.st);
    D2_HIP(hipEventRecord(S.ev[1], S.st));
    launch_filter_ee(A, c, S.d_qual.p, S.d_off.p, d_tab, S.d_out.p, S.st);
    D2_HIP(hipEventRecord(S.ev[2], S.st));
    if (want_km) launch_filter_kmers(c, k, S.d_seq.p, S.d_off.p, S.d_out.p, S.d_aux.p, S.st);
  };
  auto scatter = [&](FtSlot &S) {
    const int64_t f = S.first, c = S.count;
    const FilterOut *o = S.h_out.p;
    if (ori) {
      hipEvent_t e_or = m->ev_orient[&S - m->slot][0];
      add_elapsed(st[FO_US_ORIENT], S.ev[0], e_or);
      int64_t nflip = 0, nshort = 0, first_short = -1;
      for (int64_t i = 0; i < c; i++) {
        const int v = o[i].pad;
        if (orient) orient[f + i] = (int8_t)v;
        nflip += v == 1;
        if (v == 3 && nshort++ == 0) first_short = f + i;
      }
      st[FO_FLIPPED] += nflip;
      if (nshort) throw InputError{"dada2hip: read " + std::to_string(first_short + 1) + " is shorter than orient_fwd."};
      if (only) {
        int64_t drop = 0;
        for (int64_t i = 0; i < c; i++) {
          const int cd = o[i].pad == 0 ? 0 : FT_CODE_ORIENT;
          if (code) code[f + i] = cd;
          if (window) { window[2 * (f + i)] = 0; window[2 * (f + i) + 1] = 0; }
          drop += cd != 0;
        }
        st[FO_DROPPED_ORIENT] += drop; st[FS_KEPT] += c - drop;
        return;
      }
      add_elapsed(st[FS_US_SCAN], e_or, S.ev[1]);
    } else
    add_elapsed(st[FS_US_SCAN], S.ev[0], S.ev[1]);
    add_elapsed(st[FS_US_EE], S.ev[1], S.ev[2]);
    add_elapsed(st[FS_US_KMERS], S.ev[2], S.ev[3]);
    const int32_t *km = S.h_aux.p;
    int64_t dropped[13] = {0};
    std::mutex cmu;
    parallel_for((size_t)c, 4096, [&](size_t lo, size_t hi) {
      int64_t loc[13] = {0};
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
      for (int s = 0; s < 13; s++) dropped[s] += loc[s];
    });
    st[FS_KEPT] += dropped[0];
    for (int s = 1; s < 12; s++) st[FS_STAGE1 + s - 1] += dropped[s];
    st[FO_DROPPED_ORIENT] += dropped[FT_CODE_ORIENT];
    if (after_piece) (*after_piece)(S);
  };
  run_pieces(m->slot, n, seq, only ? nullptr : qual, offsets, knobs().filter_piece, knobs().filter_piece_bytes, want_km ? (size_t)nb : 0, st, FS_BYTES,
             FS_US_UP, FS_US_DOWN, launch, scatter);
  finish_stats(st, FS_US_TOTAL, t_call, stats);
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

int dada2hip_filter_reads_oriented(dada2hip_filter *ctx, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                                   const dada2hip_filter_params *params, const char *orient_fwd, int32_t orient_mode, int32_t *code,
                                   int32_t *window, double *ee, int32_t *hits, int32_t *kmer_counts, double *complexity, int8_t *orient,
                                   int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (!orient_fwd) throw InputError{"dada2hip: bad arguments"};
    filter_reads_body(ctx, n, seq, qual, offsets, params, code, window, ee, hits, kmer_counts, complexity, stats, orient_fwd, orient_mode,
                      orient);
  });
}
