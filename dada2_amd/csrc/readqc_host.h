// readqc_host.h — host side of the read diagnostics on reads in memory: the per-cycle quality table behind plotQualityProfile
// (R/plot-methods.R:163-243, ShortRead qa()'s perCycle$quality) and seqComplexity with a window (R/filter.R:1248-1275); included
// by driver.cpp inside its extern "C" block, behind primers_host.h.  The file-level entries (dada2hip_qprofile_fastq,
// dada2hip_complexity_fastq) are derep.cpp's, where the FASTQ reader is; they call these per chunk.
//
// Both go up through read_pieces.h's two-slot pipeline (DADA2HIP_READQC_PIECE, DADA2HIP_READQC_PIECE_BYTES: smaller pieces, for
// the tests), the slots made per call.  The table's call sends the quality bytes alone; a piece's table - its longest read rounded
// up to a tile of 64 cycles - is zeroed, filled and copied back on the slot's stream between the slot's events, and the scatter
// adds it into the caller's, so a later piece with a longer read simply reaches further.  The per-read record of that call is one
// word, "a letter outside '!'..'~'".  The complexity's call sends the sequence bytes and gets readqc_plain.h's pair per read.
#pragma once

namespace {

constexpr int64_t QP_MAX_CYCLES = 1 << 18;    // a table of 262 144 cycles is 188 MiB on either side

struct QpTable {                              // beside a PieceSlot: the piece's table
  DevBuf<unsigned long long> d_tab;
  PinBuf<unsigned long long> h_tab;
  int ncyc_pad = 0;
};

void qprofile_reads_body(int64_t n, const char *qual, const int64_t *offsets, int32_t device, int32_t ncycle, int64_t *counts,
                         int64_t *stats) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_READQC_NSTATS] = {0};
  if (n < 0 || ncycle < 0 || (n > 0 && (!qual || !offsets)) || (ncycle > 0 && !counts)) throw InputError{"dada2hip: bad arguments"};
  int64_t maxlen = 0;
  for (int64_t r = 0; r < n; r++) {
    const int64_t l = offsets[r + 1] - offsets[r];
    if (l < 0) throw InputError{"dada2hip: bad read offsets."};
    if (l > QP_MAX_CYCLES)
      throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: read " + std::to_string(r + 1) + " has more than 262144 cycles: not supported by the quality profile."};
    maxlen = std::max(maxlen, l);
  }
  if (maxlen > ncycle) throw InputError{"dada2hip: the quality table has fewer cycles than the longest read."};
  if (ncycle > 0) memset(counts, 0, (size_t)ncycle * QP_NSCORE * sizeof(int64_t));
  st[RQ_IN] = n; st[RQ_PROFILED] = n; st[RQ_CYCLES] = maxlen;
  select_device(device);
  using Slot = PieceSlot<int32_t, 4>;         // ev[1]: behind the zeroing; ev[2]: behind the kernel, in front of the table's way back
  Slot slot[2];
  QpTable tab[2];
  for (Slot &S : slot) S.create();
  int64_t bad_read = -1;
  auto launch = [&](Slot &S, int c) {
    QpTable &T = tab[&S - slot];
    long long mx = 0;
    for (int i = 0; i < c; i++) mx = std::max(mx, S.h_off.p[i + 1] - S.h_off.p[i]);
    T.ncyc_pad = (int)((mx + QP_TILE - 1) / QP_TILE * QP_TILE);
    const size_t cells = (size_t)T.ncyc_pad * QP_NSCORE;
    T.d_tab.alloc(cells); T.h_tab.alloc(cells);
    if (cells) D2_HIP(hipMemsetAsync(T.d_tab.p, 0, cells * 8, S.st));
    D2_HIP(hipMemsetAsync(S.d_out.p, 0, (size_t)c * sizeof(int32_t), S.st));
    D2_HIP(hipEventRecord(S.ev[1], S.st));
    launch_qprofile(c, T.ncyc_pad, S.d_seq.p, S.d_off.p, T.d_tab.p, S.d_out.p, S.st);
    D2_HIP(hipEventRecord(S.ev[2], S.st));
    if (cells) D2_HIP(hipMemcpyAsync(T.h_tab.p, T.d_tab.p, cells * 8, hipMemcpyDeviceToHost, S.st));
    st[RQ_PIECES]++;
  };
  auto scatter = [&](Slot &S) {
    add_elapsed(st[RQ_US_KERNEL], S.ev[1], S.ev[2]);
    const QpTable &T = tab[&S - slot];
    const size_t cells = (size_t)std::min<int64_t>(T.ncyc_pad, ncycle) * QP_NSCORE;   // (behind the longest read the table is zero)
    for (size_t i = 0; i < cells; i++) counts[i] += (int64_t)T.h_tab.p[i];
    if (bad_read < 0)
      for (int64_t i = 0; i < S.count; i++)
        if (S.h_out.p[i] != 0) { bad_read = S.first + i; break; }
  };
  run_pieces(slot, n, qual, nullptr, offsets, knobs().readqc_piece, knobs().readqc_piece_bytes, 0, st, RQ_BYTES, RQ_US_UP, RQ_US_DOWN,
             launch, scatter);
  finish_stats(st, RQ_US_TOTAL, t_call, stats);
  if (bad_read >= 0)
    throw InputError{"dada2hip: read " + std::to_string(bad_read + 1) + " holds a quality letter outside '!'..'~'."};
}

// the refusals of seqComplexity's arguments (window 0: window = NULL); returns k
int cw_check(int32_t kmer_size, int32_t window, int32_t by) {
  if (kmer_size < 0 || kmer_size > 4) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: seqComplexity's kmerSize must be 1..4."};
  const int k = kmer_size == 0 ? 2 : kmer_size;
  if (window < 0) throw InputError{"dada2hip: seqComplexity's window must not be negative (0: the whole sequence)."};
  if (window == 0) return k;
  if (k >= window) throw InputError{"The window over which kmer frequency is calculated must be larger than the kmerSize."};   // :1249
  if (window > CW_WINDOW_MAX) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: seqComplexity's window above 1024 is not supported."};
  if (by < 1) throw InputError{"dada2hip: seqComplexity's by must be at least 1."};
  return k;
}

void complexity_pairs_body(int64_t n, const char *seq, const int64_t *offsets, int32_t kmer_size, int32_t window, int32_t by,
                           int32_t device, double *pairs, int64_t *stats) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_READQC_NSTATS] = {0};
  const int k = cw_check(kmer_size, window, by);
  if (window == 0) throw InputError{"dada2hip: bad arguments"};
  if (n < 0 || (n > 0 && (!seq || !offsets || !pairs))) throw InputError{"dada2hip: bad arguments"};
  int64_t maxlen = 0;
  for (int64_t r = 0; r < n; r++) {
    const int64_t l = offsets[r + 1] - offsets[r];
    if (l < 0 || l > (int64_t)INT32_MAX - 128) throw InputError{"dada2hip: bad read offsets."};
    maxlen = std::max(maxlen, l);
  }
  st[RQ_IN] = n; st[RQ_PROFILED] = n; st[RQ_CYCLES] = maxlen;
  const int full = window - k + 1;
  std::vector<double> ylogy((size_t)full + 1, 0.0);              // sindex's terms (:1272-1274) by the host's log, as the filter's
  for (int c = 1; c <= full; c++) { const double y = (double)c / (double)full; ylogy[c] = -y * log(y); }
  select_device(device);
  DevBuf<double> d_ylogy;
  d_ylogy.alloc(ylogy.size());
  D2_HIP(hipMemcpy(d_ylogy.p, ylogy.data(), ylogy.size() * sizeof(double), hipMemcpyHostToDevice));
  using Slot = PieceSlot<ComplexityOut, 2>;
  Slot slot[2];
  for (Slot &S : slot) S.create();
  auto launch = [&](Slot &S, int c) {
    launch_complexity_win(c, k, window, by, S.d_seq.p, S.d_off.p, d_ylogy.p, S.d_out.p, S.st);
    st[RQ_PIECES]++;
  };
  auto scatter = [&](Slot &S) {
    add_elapsed(st[RQ_US_KERNEL], S.ev[0], S.ev[1]);
    for (int64_t i = 0; i < S.count; i++) { pairs[2 * (S.first + i)] = S.h_out.p[i].lo; pairs[2 * (S.first + i) + 1] = S.h_out.p[i].last; }
  };
  run_pieces(slot, n, seq, nullptr, offsets, knobs().readqc_piece, knobs().readqc_piece_bytes, 0, st, RQ_BYTES, RQ_US_UP, RQ_US_DOWN,
             launch, scatter);
  finish_stats(st, RQ_US_TOTAL, t_call, stats);
}

void complexity_reads_body(int64_t n, const char *seq, const int64_t *offsets, int32_t kmer_size, int32_t window, int32_t by,
                           int32_t device, double *complexity, int64_t *stats) {
  auto t_call = clk::now();
  const int k = cw_check(kmer_size, window, by);
  if (n < 0 || (n > 0 && (!seq || !offsets || !complexity))) throw InputError{"dada2hip: bad arguments"};
  if (window == 0) {                                             // window = NULL (:1257): the filter stage's number, its bits
    int64_t st[DADA2HIP_READQC_NSTATS] = {0}, fst[DADA2HIP_FILTER_NSTATS];
    dada2hip_filter *ctx = nullptr;
    filter_open_body(nullptr, 16, device, &ctx, nullptr);
    std::unique_ptr<dada2hip_filter> hold(ctx);
    dada2hip_filter_params P;                                    // every non-empty read is kept whole
    memset(&P, 0, sizeof P);
    P.trunc_q = -1; P.max_n = INT32_MAX; P.max_ee = std::numeric_limits<double>::infinity(); P.min_matches = 2; P.non_overlapping = 1;
    P.kmer_size = k; P.qual_offset = 33;
    const std::string qual(n ? (size_t)offsets[n] : 0, 'I');
    filter_reads_body(ctx, n, seq, qual.data(), offsets, &P, nullptr, nullptr, nullptr, nullptr, nullptr, complexity, fst);
    st[RQ_IN] = n; st[RQ_PROFILED] = n; st[RQ_PIECES] = (n + PIECE_READS - 1) / PIECE_READS; st[RQ_BYTES] = fst[FS_BYTES];
    st[RQ_US_UP] = fst[FS_US_UP]; st[RQ_US_KERNEL] = fst[FS_US_SCAN] + fst[FS_US_EE] + fst[FS_US_KMERS]; st[RQ_US_DOWN] = fst[FS_US_DOWN];
    for (int64_t r = 0; r < n; r++) st[RQ_CYCLES] = std::max(st[RQ_CYCLES], offsets[r + 1] - offsets[r]);
    finish_stats(st, RQ_US_TOTAL, t_call, stats);
    return;
  }
  int64_t st[DADA2HIP_READQC_NSTATS] = {0};
  std::vector<double> pairs(2 * (size_t)n);
  int64_t maxlen = 0;
  for (int64_t r = 0; r < n; r++) maxlen = std::max(maxlen, offsets[r + 1] - offsets[r]);
  if (maxlen - window < 1)                                       // R's seq(1, max(width) - window, by) stops (:1260)
    throw InputError{CW_ERR_NO_START};
  complexity_pairs_body(n, seq, offsets, kmer_size, window, by, device, pairs.data(), st);
  for (int64_t r = 0; r < n; r++) complexity[r] = cw_finish(offsets[r + 1] - offsets[r], maxlen, pairs[2 * r], pairs[2 * r + 1], k);
  finish_stats(st, RQ_US_TOTAL, t_call, stats);
}

}  // namespace

int dada2hip_qprofile_reads(int64_t n, const char *qual, const int64_t *offsets, int32_t device, int32_t ncycle, int64_t *counts,
                            int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] { qprofile_reads_body(n, qual, offsets, device, ncycle, counts, stats); });
}

int d2_complexity_pairs(int64_t n, const char *seq, const int64_t *offsets, int32_t kmer_size, int32_t window, int32_t by, int32_t device,
                        double *pairs, int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] { complexity_pairs_body(n, seq, offsets, kmer_size, window, by, device, pairs, stats); });
}

int dada2hip_complexity_reads(int64_t n, const char *seq, const int64_t *offsets, int32_t kmer_size, int32_t window, int32_t by,
                              int32_t device, double *complexity, int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] { complexity_reads_body(n, seq, offsets, kmer_size, window, by, device, complexity, stats); });
}
