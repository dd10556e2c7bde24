// bimera_denovo_host.h — host side of dada2hip_bimera_denovo (isBimeraDenovo, R/chimeras.R:105-154; the rows of a table one after
// the other: removeBimeraDenovo(method = "per-sample"), :321-333); included by driver.cpp inside its extern "C" block, behind
// priors_host.h.
//
// The sequences become resident once, as a lite sample (what bimera_pairs() does).  Per row the host ranks the abundances and finds
// every query's P (bimera_plain.h) - the parents of query j are the ranks [0, P[j]) -, sends the ranking, P and the first live
// list (the queries with P >= 2) up, and then only steers: a window of ranks [r0, r1) is cut into launches of at most the slot
// budget of bimera_pairs() (DADA2HIP_BIMERA_SLOTS lowers it) - whole queries x the window's ranks, or, where one query's window
// is wider than the budget, pieces of its ranks -, each launch being k_bimera_worklist, the bimera-mode aligner and k_bimera_fold
// (bimera_denovo.inc.hip).  The fold of a window's last launch over a query decides whether it stays live.  One word per window
// comes back (the next live count), n flag bytes per row, and one counter per call.
// Windows: ranks [0, per), then [per, 4 per), [4 per, 16 per), ...: bimera_window_end.  A real bimera's parents are among the most
// abundant sequences, so it leaves the work after a window or two; a query that is no bimera is aligned with all its parents
// whatever the schedule, and the factor of four keeps the host's round trips at log4(n / per).
#pragma once

namespace {

struct BdDev {
  DevBuf<int32_t> rank, P, live[2], maxima, n_next, out;
  DevBuf<uint8_t> flags;
  DevBuf<unsigned long long> aligned;
};

void bimera_denovo_body(int32_t nrow, int32_t ncol, const int32_t *mat, const char *const *seqs, double min_fold, double min_parent_abund,
                        int32_t allow_one_off, int32_t min_one_off_par_dist, int32_t match, int32_t mismatch, int32_t gap_p,
                        int32_t max_shift, int32_t skip_zero, int32_t device, uint8_t *flags, int64_t *stats) {
  auto t_call = clk::now();
  if (nrow < 0 || ncol < 0 || (nrow > 0 && ncol > 0 && (!mat || !seqs || !flags))) throw InputError{"dada2hip: bad sequence table"};
  int64_t st[DADA2HIP_BIMERA_DENOVO_NSTATS] = {0};
  st[BD_SEQS] = ncol; st[BD_ROWS] = nrow;
  if (nrow == 0 || ncol == 0) { finish_stats(st, BD_US_TOTAL, t_call, stats); return; }
  const size_t ncell = (size_t)nrow * (size_t)ncol;
  for (size_t c = 0; c < ncell; c++)
    if (mat[c] < 0) throw InputError{"dada2hip: the abundances must not be negative."};
  memset(flags, 0, ncell);
  select_device(device);
  require_acgt(ncol, seqs, "bimera identification");
  if (max_shift == 0) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: maxShift 0 is outside the implemented path."};

  // the rankings (host only), and whether any row asks for an alignment at all
  std::vector<BimeraRanking> R((size_t)nrow);
  parallel_for((size_t)nrow, 1, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) bimera_rank(ncol, mat + i, (ptrdiff_t)nrow, min_fold, min_parent_abund, skip_zero != 0, R[i]);
  });
  int64_t max_row_pairs = 0;
  for (const BimeraRanking &r : R) {
    st[BD_QUERIES] += r.nquery; st[BD_PAIRS_POSSIBLE] += r.pairs_possible;
    max_row_pairs = std::max(max_row_pairs, r.pairs_possible);
  }
  add_lap(st[BD_US_PACK], t_call);
  if (st[BD_PAIRS_POSSIBLE] == 0) { finish_stats(st, BD_US_TOTAL, t_call, stats); return; }

  auto t_dev = clk::now();
  std::vector<int32_t> ab(ncol, 1);
  dada2hip_sample *s = new dada2hip_sample();
  std::unique_ptr<dada2hip_sample, void (*)(dada2hip_sample *)> guard(s, dada2hip_sample_free);
  sample_create(s, ncol, seqs, ab.data(), nullptr, nullptr, 0, device, /*lite=*/true);
  std::vector<double> errm(16, 1.0), rowm;
  upload_err(s, errm.data(), 1, rowm);
  dada2hip_opts o;
  memset(&o, 0, sizeof o);
  o.match = match; o.mismatch = mismatch; o.gap = gap_p; o.vectorized_alignment = 1;   // nwalign_vectorized2 (chimera.cpp:26)
  AlignParams ap{match, mismatch, gap_p, max_shift, nw_sentinel(o), 0, 1};
  ap.homo_gap = gap_p;
  const int stride = 2 * s->D.maxlen + 2;
  // the aligner: bimera_pairs()'s choice
  const bool coop = [&] {
    const int f = knobs().nw_kernel;
    if (f == NWK_LANE || f == NWK_WIDE) return false;
    const size_t b = nw_ad_lr_lds_bytes(s->D, ap);
    return b > 0 && b <= 150 * 1024;
  }();
  const int per = coop ? nw_ad_apw(s->D, ap) : 64;
  size_t budget = coop ? ((size_t)1 << 23) : std::max<size_t>(4096, ((size_t)256 << 20) / (size_t)stride);
  if (knobs().bimera_slots > 0) budget = std::min<size_t>(budget, (size_t)knobs().bimera_slots);
  budget = std::max<size_t>((size_t)per, budget / (size_t)per * (size_t)per);   // whole chunks, at least one
  st[BD_ROUTE] = coop ? 1 : 2; st[BD_PER] = per; st[BD_SLOTS] = (int64_t)budget;
  AdRingGuard ring{s};
  if (coop) ensure_ad_ring(s);
  else ensure_scratch(s, max_shift, (size_t)std::min<int64_t>((int64_t)budget, max_row_pairs));
  s->d_lambda.alloc(ncol); s->d_ham.alloc(ncol);

  hipStream_t q = s->stream;
  BdDev B;
  B.rank.alloc((size_t)ncol); B.P.alloc((size_t)ncol); B.live[0].alloc((size_t)ncol); B.live[1].alloc((size_t)ncol);
  B.maxima.alloc((size_t)ncol * 6); B.flags.alloc((size_t)ncol); B.n_next.alloc(1); B.aligned.alloc(1);
  B.aligned.zero(q);
  PinBuf<int32_t> h_word;
  PinBuf<uint8_t> h_flags;
  PinBuf<unsigned long long> h_aligned;
  h_word.alloc(1); h_flags.alloc((size_t)ncol); h_aligned.alloc(1);
  std::vector<int32_t> live0;
  Events<2> ev;
  const bool timed = knobs().profile;
  if (timed) ev.create();

  for (int32_t i = 0; i < nrow; i++) {
    const BimeraRanking &r = R[(size_t)i];
    if (r.nquery == 0) continue;
    live0.clear();
    for (int32_t k = 0; k < ncol; k++) if (r.P[r.rank[k]] > 0) live0.push_back(r.rank[k]);   // in rank order
    D2_HIP(hipMemcpyAsync(B.rank.p, r.rank.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, q));
    D2_HIP(hipMemcpyAsync(B.P.p, r.P.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, q));
    D2_HIP(hipMemcpyAsync(B.live[0].p, live0.data(), live0.size() * 4, hipMemcpyHostToDevice, q));
    B.maxima.zero(q); B.flags.zero(q);
    int cur = 0;
    int32_t nlive = (int32_t)live0.size(), r0 = 0;
    while (nlive > 0 && r0 < r.max_P) {
      const int32_t r1 = bimera_window_end(r0, per, r.max_P);
      const int32_t wpad = (r1 - r0 + per - 1) / per * per;            // whole chunks: the ranks past a query's P are empty slots
      st[BD_WINDOWS]++;
      B.n_next.zero(q);
      if (timed) D2_HIP(hipEventRecord(ev[0], q));
      const int32_t wr_tile = (int32_t)std::min<size_t>((size_t)wpad, budget);
      {   // the window's buffers, sized once for its largest launch: the stream is idle here, no launch holds the old ones
        const size_t most = std::min<size_t>(budget, (size_t)nlive * (size_t)wr_tile);
        s->d_work.alloc(most); s->d_chunk_centre.alloc(most / (size_t)per); B.out.alloc(most * 5);
        if (!coop) { s->d_moves.alloc(most * (size_t)stride); s->d_nmoves.alloc(most); }
      }
      for (int32_t rt = r0; rt < r0 + wpad; rt += wr_tile) {
        const int32_t wr = std::min(wr_tile, r0 + wpad - rt);
        const int32_t nq_tile = (int32_t)std::max<size_t>(1, budget / (size_t)wr);
        for (int32_t q0 = 0; q0 < nlive; q0 += nq_tile) {
          const int32_t nq = std::min(nq_tile, nlive - q0);
          const size_t nslots = (size_t)nq * (size_t)wr;
          const int nwork = (int)nslots;
          launch_bimera_worklist(B.live[cur].p + q0, nq, rt, wr, per, B.rank.p, B.P.p, B.flags.p, s->d_chunk_centre.p, s->d_work.p, q);
          if (coop)
            launch_nw_ad_lr(s->D, s->d_chunk_centre.p, s->d_work.p, nwork, ap, s->d_err.p, allow_one_off, max_shift, B.out.p, q);
          else {
            launch_nw(s->D, s->scr_class, 0, s->d_chunk_centre.p, s->d_work.p, nullptr, nwork, ap, s->d_err.p, s->scr, s->d_lambda.p,
                      s->d_ham.p, nullptr, 0, 0, s->d_moves.p, stride, s->d_nmoves.p, q);
            launch_bimera_lr(s->D, s->d_chunk_centre.p, s->d_work.p, nwork, s->d_moves.p, stride, s->d_nmoves.p, allow_one_off, max_shift,
                             B.out.p, q);
          }
          BimeraFold F;
          F.live = B.live[cur].p + q0; F.nq = nq; F.r0 = rt; F.wr = wr; F.work = s->d_work.p; F.rec = B.out.p;
          F.len = s->D.len; F.P = B.P.p; F.allow_one_off = allow_one_off; F.min_one_off_par_dist = min_one_off_par_dist;
          F.maxima = B.maxima.p; F.flags = B.flags.p; F.aligned = B.aligned.p; F.last = rt + wr >= r0 + wpad ? 1 : 0;
          F.next_live = B.live[cur ^ 1].p; F.n_next = B.n_next.p;
          launch_bimera_fold(F, q);
          D2_HIP(hipGetLastError());
          st[BD_LAUNCHES]++;
        }
      }
      if (timed) D2_HIP(hipEventRecord(ev[1], q));
      D2_HIP(hipMemcpyAsync(h_word.p, B.n_next.p, 4, hipMemcpyDeviceToHost, q));   // the one word of the window
      sync_checked(q);
      if (timed) add_elapsed(st[BD_US_KERNEL], ev[0], ev[1]);
      nlive = h_word.p[0];
      if (nlive < 0 || nlive > ncol) throw RuntimeErr{DADA2HIP_ERR_RUNTIME, "dada2hip: the live count of a bimera window is out of range."};
      cur ^= 1;
      r0 = r1;
    }
    D2_HIP(hipMemcpyAsync(h_flags.p, B.flags.p, (size_t)ncol, hipMemcpyDeviceToHost, q));
    sync_checked(q);
    check_nw_flag(s);
    for (int32_t j = 0; j < ncol; j++) {
      const uint8_t f = h_flags.p[j] ? 1 : 0;
      flags[(size_t)i + (size_t)j * (size_t)nrow] = f;
      st[BD_FLAGGED] += f;
    }
  }
  D2_HIP(hipMemcpyAsync(h_aligned.p, B.aligned.p, 8, hipMemcpyDeviceToHost, q));
  sync_checked(q);
  st[BD_PAIRS_ALIGNED] = (int64_t)h_aligned.p[0];
  add_lap(st[BD_US_DEVICE], t_dev);
  finish_stats(st, BD_US_TOTAL, t_call, stats);
}

}  // namespace

int dada2hip_bimera_denovo(int32_t nrow, int32_t ncol, const int32_t *mat, const char *const *seqs, double min_fold, double min_parent_abund,
                           int32_t allow_one_off, int32_t min_one_off_par_dist, int32_t match, int32_t mismatch, int32_t gap_p,
                           int32_t max_shift, int32_t skip_zero, int32_t device, uint8_t *flags, int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    bimera_denovo_body(nrow, ncol, mat, seqs, min_fold, min_parent_abund, allow_one_off, min_one_off_par_dist, match, mismatch, gap_p,
                       max_shift, skip_zero, device, flags, stats);
  });
}

// The two kernels on arrays the caller made up (tests: work lists and folds against restatements, records written by hand).
// n sequences; nq live queries, ranks [r0, r0 + wr).  worklist: chunk_centre[nq * wr / per], work[nq * wr] out.
int dada2hip_bimera_worklist_probe(int32_t n, const int32_t *rank, const int32_t *P, const uint8_t *flags, int32_t nq, const int32_t *live,
                                   int32_t r0, int32_t wr, int32_t per, int32_t device, int32_t *chunk_centre, int32_t *work, char *errbuf,
                                   size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (n <= 0 || nq <= 0 || wr <= 0 || per <= 0 || wr % per != 0 || r0 < 0 || (long long)nq * wr > (1ll << 23) || !rank || !P || !flags ||
        !live || !chunk_centre || !work)
      throw InputError{"dada2hip: bad arguments"};
    for (int32_t k = 0; k < nq; k++) if (live[k] < 0 || live[k] >= n) throw InputError{"dada2hip: bad arguments"};
    for (int32_t k = 0; k < n; k++) if (rank[k] < 0 || rank[k] >= n || P[k] < 0 || P[k] > n) throw InputError{"dada2hip: bad arguments"};
    select_device(device);
    const size_t ns = (size_t)nq * (size_t)wr;
    DevBuf<int32_t> d_rank, d_P, d_live, d_cc, d_work;
    DevBuf<uint8_t> d_flags;
    d_rank.alloc(n); d_P.alloc(n); d_flags.alloc(n); d_live.alloc(nq); d_cc.alloc(ns / per); d_work.alloc(ns);
    D2_HIP(hipMemcpy(d_rank.p, rank, (size_t)n * 4, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_P.p, P, (size_t)n * 4, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_flags.p, flags, (size_t)n, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_live.p, live, (size_t)nq * 4, hipMemcpyHostToDevice));
    launch_bimera_worklist(d_live.p, nq, r0, wr, per, d_rank.p, d_P.p, d_flags.p, d_cc.p, d_work.p, nullptr);
    D2_HIP(hipGetLastError());
    D2_HIP(hipDeviceSynchronize());
    D2_HIP(hipMemcpy(chunk_centre, d_cc.p, ns / per * 4, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(work, d_work.p, ns * 4, hipMemcpyDeviceToHost));
  });
}

// fold: work[nq * wr] and rec[5 nq * wr] in; maxima[6 n] and flags[n] in and out; next_live[nq], *n_next and *aligned out.
int dada2hip_bimera_fold_probe(int32_t n, const int32_t *len, const int32_t *P, int32_t nq, const int32_t *live, int32_t r0, int32_t wr,
                               const int32_t *work, const int32_t *rec, int32_t allow_one_off, int32_t min_one_off_par_dist, int32_t last,
                               int32_t device, int32_t *maxima, uint8_t *flags, int32_t *next_live, int32_t *n_next, int64_t *aligned,
                               char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (n <= 0 || nq <= 0 || wr <= 0 || r0 < 0 || (long long)nq * wr > (1ll << 23) || !len || !P || !live || !work || !rec || !maxima ||
        !flags || !next_live || !n_next || !aligned)
      throw InputError{"dada2hip: bad arguments"};
    for (int32_t k = 0; k < nq; k++) if (live[k] < 0 || live[k] >= n) throw InputError{"dada2hip: bad arguments"};
    select_device(device);
    const size_t ns = (size_t)nq * (size_t)wr;
    DevBuf<int32_t> d_len, d_P, d_live, d_work, d_rec, d_max, d_next, d_nn;
    DevBuf<uint8_t> d_flags;
    DevBuf<unsigned long long> d_al;
    d_len.alloc(n); d_P.alloc(n); d_live.alloc(nq); d_work.alloc(ns); d_rec.alloc(ns * 5); d_max.alloc((size_t)n * 6); d_next.alloc(nq);
    d_nn.alloc(1); d_flags.alloc(n); d_al.alloc(1);
    D2_HIP(hipMemcpy(d_len.p, len, (size_t)n * 4, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_P.p, P, (size_t)n * 4, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_live.p, live, (size_t)nq * 4, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_work.p, work, ns * 4, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_rec.p, rec, ns * 20, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_max.p, maxima, (size_t)n * 24, hipMemcpyHostToDevice));
    D2_HIP(hipMemcpy(d_flags.p, flags, (size_t)n, hipMemcpyHostToDevice));
    D2_HIP(hipMemset(d_next.p, 0xFF, (size_t)nq * 4));
    D2_HIP(hipMemset(d_nn.p, 0, 4));
    D2_HIP(hipMemset(d_al.p, 0, 8));
    BimeraFold F;
    F.live = d_live.p; F.nq = nq; F.r0 = r0; F.wr = wr; F.work = d_work.p; F.rec = d_rec.p; F.len = d_len.p; F.P = d_P.p;
    F.allow_one_off = allow_one_off; F.min_one_off_par_dist = min_one_off_par_dist; F.maxima = d_max.p; F.flags = d_flags.p;
    F.aligned = d_al.p; F.last = last; F.next_live = d_next.p; F.n_next = d_nn.p;
    launch_bimera_fold(F, nullptr);
    D2_HIP(hipGetLastError());
    D2_HIP(hipDeviceSynchronize());
    unsigned long long al = 0;
    D2_HIP(hipMemcpy(maxima, d_max.p, (size_t)n * 24, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(flags, d_flags.p, (size_t)n, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(next_live, d_next.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(n_next, d_nn.p, 4, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(&al, d_al.p, 8, hipMemcpyDeviceToHost));
    *aligned = (int64_t)al;
  });
}
