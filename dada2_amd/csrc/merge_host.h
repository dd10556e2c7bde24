// merge_host.h — host side of the run-level mergePairs (merge.inc.hip; R/paired.R:92-201); included by driver.cpp inside its
// extern "C" block, behind seqtab_host.h, on top of stage_common.h and merge_plain.h.  dada2hip_merge_pairs (merge.cpp) is the
// one-sample entry and stays as it is.
//
// Sample after sample, the four maps go up and k_mp_tally counts the sample's (forward, reverse) pairs in a table of its own -
// samples never see each other -, k_mp_compact hands the occupied slots back and merge_plain.h puts them in the reference's row
// order.  The unique pairs of ALL samples then form one work list, cut into chunks of DADA2HIP_MERGE_CHUNK pairs: a chunk is
// aligned exactly as nwvec_any aligns dada2hip_merge_pairs' (a throw-away resident sample, k_nw_gen<pair>, unbanded, ends-free),
// but its move strings stay on the device, where k_mp_eval judges them and k_mp_consensus writes the accepted pairs' merged
// sequences into an arena whose offsets the host scans from the verdicts.  Six integers per pair and the arena come back.
#pragma once

struct dada2hip_run_mergers {
  int32_t nsamples = 0;
  std::vector<int64_t> row0;                   // [nsamples + 1]: a sample's rows are row0[s] .. row0[s + 1] of every column
  std::vector<int32_t> col[8];                 // abundance, forward, reverse, nmatch, nmismatch, nindel, prefer, accept
  std::string seq_bytes;                       // the rows' sequences one behind the other ("" for a reject)
  std::vector<int64_t> seq_off;                // [rows + 1]
};

namespace {

enum { MC_ABUNDANCE = 0, MC_FORWARD, MC_REVERSE, MC_NMATCH, MC_NMISMATCH, MC_NINDEL, MC_PREFER, MC_ACCEPT };

// One chunk of the run's pair list through the aligner: the sibling of nwvec_any's first half.  The move strings are left in
// s->d_moves (stride bytes a pair) and s->d_nmoves; pair i of the chunk is (centre 2i, raw 2i + 1) of the throw-away sample.
int mp_align_chunk(dada2hip_sample *s, int n, const std::vector<const char *> &seqs, int maxlen, int32_t match, int32_t mismatch, int device) {
  std::vector<int32_t> ab(seqs.size(), 1);
  sample_create(s, (int32_t)seqs.size(), seqs.data(), ab.data(), nullptr, nullptr, 0, device, /*lite=*/true);
  ensure_scratch(s, /*band=*/-1, 0, /*force_generic=*/false);
  std::vector<double> errm(16, 1.0), rowm;
  upload_err(s, errm.data(), 1, rowm);
  dada2hip_opts o;
  memset(&o, 0, sizeof o);
  o.match = match; o.mismatch = mismatch; o.gap = mismatch; o.vectorized_alignment = 1;
  AlignParams ap{match, mismatch, mismatch, /*band=*/-1, nw_sentinel(o), 0, 1};
  ap.endsfree = 1;                                               // nwalign(x, y, band = -1): nwalign_endsfree, one gap penalty (evaluate.cpp:36-48)
  ap.homo_gap = mismatch;
  if (!ap.plain()) ap.sentinel = -9999;
  ap.hi_off = 0;
  std::vector<int32_t> work((size_t)n), cc((size_t)n);
  for (int i = 0; i < n; i++) { work[i] = 2 * i + 1; cc[i] = 2 * i; }
  const int stride = 2 * maxlen + 2;
  s->d_work.alloc((size_t)n); s->d_chunk_centre.alloc((size_t)n); s->d_moves.alloc((size_t)n * (size_t)stride);
  s->d_nmoves.alloc((size_t)n); s->d_lambda.alloc(2 * (size_t)n); s->d_ham.alloc(2 * (size_t)n);
  D2_HIP(hipMemcpyAsync(s->d_work.p, work.data(), (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
  D2_HIP(hipMemcpyAsync(s->d_chunk_centre.p, cc.data(), (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
  launch_nw(s->D, s->scr_class, 0, nullptr, s->d_work.p, nullptr, n, ap, s->d_err.p, s->scr, s->d_lambda.p, s->d_ham.p, nullptr, 0, 0,
            s->d_moves.p, stride, s->d_nmoves.p, s->stream, s->d_chunk_centre.p);
  sync_checked(s->stream);                                       // (work and cc are the host's until the copies have run)
  check_nw_flag(s);
  return stride;
}

void merge_run_body(int32_t S, const int64_t *nreads, const int32_t *const *derepF, const int32_t *const *derepR, const int32_t *nuniqF,
                    const int32_t *const *dadaF, const int32_t *nuniqR, const int32_t *const *dadaR, const int32_t *nclustF, const char *f_bytes,
                    const int64_t *f_off, const int32_t *n0F, const int32_t *nclustR, const char *r_bytes, const int64_t *r_off, const int32_t *n0R,
                    int32_t min_overlap, int32_t max_mismatch, int32_t trim_overhang, int32_t just_concatenate, int32_t device,
                    dada2hip_run_mergers **out, int64_t *stats) {
  const auto t_call = clk::now();
  int64_t st[DADA2HIP_MERGE_NSTATS] = {0};
  if (!out) throw InputError{"dada2hip: bad arguments"};
  *out = nullptr;
  if (S < 0 || (S > 0 && (!nreads || !derepF || !derepR || !nuniqF || !dadaF || !nuniqR || !dadaR || !nclustF || !nclustR || !f_off || !r_off ||
                          !n0F || !n0R)))
    throw InputError{"dada2hip: merge_run needs the read maps, the unique-to-cluster maps and both clustering tables of every sample."};
  // ---- the arguments (:100-120), the clustering tables as strings ----
  std::vector<int64_t> cF((size_t)S + 1, 0), cR((size_t)S + 1, 0);   // a sample's first sequence in the run's two lists
  int64_t most_reads = 0, most_uniq = 0;
  long long most_cap = 0, most_rec = 0;
  for (int32_t s = 0; s < S; s++) {
    const std::string m = mp_check_sample(s, nreads[s], derepF[s] && derepR[s], dadaF[s] && dadaR[s], nuniqF[s], nuniqR[s], nclustF[s], nclustR[s]);
    if (!m.empty()) throw InputError{m};
    cF[(size_t)s + 1] = cF[(size_t)s] + nclustF[s]; cR[(size_t)s + 1] = cR[(size_t)s] + nclustR[s];
    most_reads = std::max(most_reads, nreads[s]); most_uniq = std::max<int64_t>(most_uniq, std::max(nuniqF[s], nuniqR[s]));
    most_cap = std::max(most_cap, mp_capacity(nreads[s], nclustF[s], nclustR[s]));
    most_rec = std::max<long long>(most_rec, std::min<long long>(nreads[s], (long long)nclustF[s] * nclustR[s]));
  }
  const int64_t NF = cF[(size_t)S], NR = cR[(size_t)S];
  if (NF > (int64_t)INT32_MAX || NR > (int64_t)INT32_MAX) throw InputError{"dada2hip: more than 2^31 - 1 denoised sequences in one run."};
  if ((NF > 0 && !f_bytes) || (NR > 0 && !r_bytes)) throw InputError{"dada2hip: bad arguments"};
  auto strings = [&](int64_t n, const char *bytes, const int64_t *off, const std::vector<int64_t> &c0, bool rc, const char *side,
                     std::vector<std::string> &to) {
    to.resize((size_t)n);
    int32_t s = 0;
    for (int64_t i = 0; i < n; i++) {
      while (i >= c0[(size_t)s + 1]) s++;
      if (off[i + 1] < off[i] || off[0] != 0) throw InputError{"dada2hip: bad sequence offsets."};
      const size_t len = (size_t)(off[i + 1] - off[i]);
      if (!just_concatenate && (len == 0 || !mp_is_acgt(bytes + off[i], len)))
        throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, std::string("dada2hip: mergePairs on the device takes denoised sequences of A/C/G/T only: sample ") +
                                                       std::to_string(s + 1) + ", " + side + " sequence " + std::to_string(i - c0[(size_t)s] + 1) + "."};
      to[(size_t)i] = rc ? mp_revcomp(bytes + off[i], len) : std::string(bytes + off[i], len);
    }
  };
  std::vector<std::string> Fs, Rs;                               // Rs: reverse-complemented (:139)
  strings(NF, f_bytes, f_off, cF, false, "forward", Fs);
  strings(NR, r_bytes, r_off, cR, true, "reverse", Rs);
  select_device(device);
  StStream Q;
  Q.create();

  // ---- the tally: unique(pairdf) and table() per sample (:121-127, :175) ----
  std::unique_ptr<dada2hip_run_mergers> H(new dada2hip_run_mergers());
  H->nsamples = S;
  H->row0.assign((size_t)S + 1, 0);
  std::vector<int32_t> pair_f, pair_r;                           // the run's unique pairs in row order, as places in Fs / Rs
  {
    DevBuf<int32_t> d_derepF, d_derepR, d_dadaF, d_dadaR, d_count;
    DevBuf<uint32_t> d_first;
    DevBuf<unsigned long long> d_key;
    DevBuf<MpRec> d_rec;
    DevBuf<MpCounters> d_ctr;
    d_derepF.alloc((size_t)most_reads); d_derepR.alloc((size_t)most_reads); d_dadaF.alloc((size_t)most_uniq); d_dadaR.alloc((size_t)most_uniq);
    d_key.alloc((size_t)most_cap); d_count.alloc((size_t)most_cap); d_first.alloc((size_t)most_cap); d_rec.alloc((size_t)most_rec); d_ctr.alloc(1);
    const int bits = knobs().merge_hash_bits;
    std::vector<MpRec> rec;
    std::vector<int32_t> order;
    for (int32_t s = 0; s < S; s++) {
      const int64_t n = nreads[s];
      auto t0 = clk::now();
      MpTable T{d_key.p, d_count.p, d_first.p, mp_capacity(n, nclustF[s], nclustR[s]), bits >= 64 ? ~0ull : ((1ull << bits) - 1ull)};
      const long long max_rec = std::min<long long>(n, (long long)nclustF[s] * nclustR[s]);
      MpCounters h;
      memset(&h, 0, sizeof h);
      h.bad_first = ~0ull; h.max_f = h.max_r = -1;
      if (n) D2_HIP(hipMemcpyAsync(d_derepF.p, derepF[s], (size_t)n * 4, hipMemcpyHostToDevice, Q.s));
      if (n) D2_HIP(hipMemcpyAsync(d_derepR.p, derepR[s], (size_t)n * 4, hipMemcpyHostToDevice, Q.s));
      if (nuniqF[s]) D2_HIP(hipMemcpyAsync(d_dadaF.p, dadaF[s], (size_t)nuniqF[s] * 4, hipMemcpyHostToDevice, Q.s));
      if (nuniqR[s]) D2_HIP(hipMemcpyAsync(d_dadaR.p, dadaR[s], (size_t)nuniqR[s] * 4, hipMemcpyHostToDevice, Q.s));
      D2_HIP(hipMemcpyAsync(d_ctr.p, &h, sizeof h, hipMemcpyHostToDevice, Q.s));
      sync_checked(Q.s);
      st[MR_BYTES_UP] += (2 * n + nuniqF[s] + nuniqR[s]) * 4 + (int64_t)sizeof h;
      add_lap(st[MR_US_UP], t0);
      t0 = clk::now();
      D2_HIP(hipMemsetAsync(d_key.p, 0xFF, (size_t)T.cap * 8, Q.s));     // MP_EMPTY
      D2_HIP(hipMemsetAsync(d_count.p, 0, (size_t)T.cap * 4, Q.s));
      D2_HIP(hipMemsetAsync(d_first.p, 0xFF, (size_t)T.cap * 4, Q.s));   // above every read
      MpSample A{d_derepF.p, d_derepR.p, d_dadaF.p, d_dadaR.p, (int)n, nuniqF[s], nuniqR[s], nclustF[s], nclustR[s]};
      launch_mp_tally(A, T, d_ctr.p, Q.s);
      launch_mp_compact(T, d_rec.p, (int)max_rec, d_ctr.p, Q.s);
      D2_HIP(hipMemcpyAsync(&h, d_ctr.p, sizeof h, hipMemcpyDeviceToHost, Q.s));
      sync_checked(Q.s);
      st[MR_BYTES_DOWN] += (int64_t)sizeof h;
      if (h.bad_first != ~0ull) {                                // an index past a table: the first read that has one, and which of its four
        const long long i = (long long)(h.bad_first >> 3);
        const int what = (int)(h.bad_first & 7);
        if (i >= n || what < MP_BAD_DEREP_F || what > MP_BAD_DADA_R) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the tally refused no read."};
        const bool fwd = what == MP_BAD_DEREP_F || what == MP_BAD_DADA_F, derep = what <= MP_BAD_DEREP_R;
        const long long u = fwd ? derepF[s][i] : derepR[s][i];
        throw InputError{derep ? mp_index_message(s, i, what, u + 1, fwd ? nuniqF[s] : nuniqR[s])
                               : mp_index_message(s, i, what, fwd ? dadaF[s][u] : dadaR[s][u], fwd ? nclustF[s] : nclustR[s])};
      }
      const std::string m = mp_check_maps(s, h.max_f, nuniqF[s], h.max_r, nuniqR[s]);
      if (!m.empty()) throw InputError{m};
      if (h.err || h.nrec < 0 || h.nrec > max_rec) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the pair table overflowed its known size."};
      rec.resize((size_t)h.nrec);
      if (h.nrec) {
        D2_HIP(hipMemcpyAsync(rec.data(), d_rec.p, (size_t)h.nrec * sizeof(MpRec), hipMemcpyDeviceToHost, Q.s));
        sync_checked(Q.s);
        st[MR_BYTES_DOWN] += (int64_t)h.nrec * (int64_t)sizeof(MpRec);
      }
      if (!mp_order(rec.data(), rec.size(), n, order)) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the pair table lost a first appearance."};
      int64_t counted = 0;
      for (int32_t k : order) {
        const MpRec &r = rec[(size_t)k];
        const int32_t f = (int32_t)(r.key >> 32), b = (int32_t)(r.key & 0xFFFFFFFFull);
        if (f < 1 || f > nclustF[s] || b < 1 || b > nclustR[s]) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the pair table holds no pair of this sample."};
        H->col[MC_ABUNDANCE].push_back(r.count); H->col[MC_FORWARD].push_back(f); H->col[MC_REVERSE].push_back(b);
        pair_f.push_back((int32_t)(cF[(size_t)s] + f - 1)); pair_r.push_back((int32_t)(cR[(size_t)s] + b - 1));
        counted += r.count;
      }
      if (counted + (int64_t)h.na != n) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the pair table lost a read pair."};
      H->row0[(size_t)s + 1] = (int64_t)pair_f.size();
      st[MR_PAIRS_IN] += n; st[MR_NA] += (int64_t)h.na; st[MR_COLLISIONS] += (int64_t)h.collisions;
      st[MR_CAPACITY] = std::max<int64_t>(st[MR_CAPACITY], T.cap);
      add_lap(st[MR_US_TALLY], t0);
    }
  }
  const size_t P = pair_f.size();
  if (P > (size_t)INT32_MAX) throw InputError{"dada2hip: more than 2^31 - 1 unique pairs in one run."};
  st[MR_SAMPLES] = S; st[MR_UNIQUE] = (int64_t)P;
  for (int k = MC_NMATCH; k <= MC_NINDEL; k++) H->col[k].assign(P, 0);
  H->col[MC_PREFER].assign(P, DADA2HIP_NA_INTEGER); H->col[MC_ACCEPT].assign(P, 1);
  std::vector<std::string> seq(P);

  if (just_concatenate) {                                        // (:140-148) nothing is aligned or judged
    for (size_t p = 0; p < P; p++) seq[p] = Fs[(size_t)pair_f[p]] + "NNNNNNNNNN" + Rs[(size_t)pair_r[p]];
    st[MR_ACCEPTED] = (int64_t)P;
  } else if (P > 0) {
    // ---- the denoised sequences and the pair list, once for the run ----
    auto t0 = clk::now();
    std::string fb, rb;
    std::vector<long long> fo((size_t)NF + 1, 0), ro((size_t)NR + 1, 0);
    for (int64_t i = 0; i < NF; i++) { fb += Fs[(size_t)i]; fo[(size_t)i + 1] = (long long)fb.size(); }
    for (int64_t i = 0; i < NR; i++) { rb += Rs[(size_t)i]; ro[(size_t)i + 1] = (long long)rb.size(); }
    DevBuf<uint8_t> d_fb, d_rb, d_arena;
    DevBuf<long long> d_fo, d_ro, d_off;
    DevBuf<int32_t> d_n0F, d_n0R, d_pf, d_pr, d_v;
    DevBuf<MpCounters> d_ctr;
    d_fb.alloc(fb.size()); d_rb.alloc(rb.size()); d_fo.alloc(fo.size()); d_ro.alloc(ro.size()); d_n0F.alloc((size_t)NF); d_n0R.alloc((size_t)NR);
    d_pf.alloc(P); d_pr.alloc(P); d_ctr.alloc(1);
    D2_HIP(hipMemcpyAsync(d_fb.p, fb.data(), fb.size(), hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemcpyAsync(d_rb.p, rb.data(), rb.size(), hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemcpyAsync(d_fo.p, fo.data(), fo.size() * 8, hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemcpyAsync(d_ro.p, ro.data(), ro.size() * 8, hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemcpyAsync(d_n0F.p, n0F, (size_t)NF * 4, hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemcpyAsync(d_n0R.p, n0R, (size_t)NR * 4, hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemcpyAsync(d_pf.p, pair_f.data(), P * 4, hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemcpyAsync(d_pr.p, pair_r.data(), P * 4, hipMemcpyHostToDevice, Q.s));
    D2_HIP(hipMemsetAsync(d_ctr.p, 0, sizeof(MpCounters), Q.s));
    sync_checked(Q.s);
    st[MR_BYTES_UP] += (int64_t)(fb.size() + rb.size() + (fo.size() + ro.size()) * 8 + (size_t)(NF + NR) * 4 + P * 8);
    add_lap(st[MR_US_UP], t0);
    const MpSeqs Sq{d_fb.p, d_rb.p, d_fo.p, d_ro.p, d_n0F.p, d_n0R.p};
    // mismatches and gaps are penalised heavily so that zero-mismatch merges win (:153-158)
    const int32_t match = 1, mismatch = max_mismatch == 0 ? -64 : -8;
    const long long knob = knobs().merge_chunk;
    const size_t CH = knob > 0 ? (size_t)std::min<long long>(knob, 65536) : 65536;   // 64 pairs to a wave, 65 536 fill the 1 024 SIMDs once
    d_v.alloc(7 * std::min(CH, P)); d_off.alloc(std::min(CH, P));
    std::vector<int32_t> v;
    std::vector<long long> off;
    std::vector<char> arena;
    std::vector<const char *> two;
    for (size_t p0 = 0, p1; p0 < P; p0 = p1) {
      p1 = mp_next_chunk(p0, P, CH);
      const int n = (int)(p1 - p0);
      st[MR_CHUNKS]++;
      // the alignments: unchanged kernels, the moves left where they are
      t0 = clk::now();
      two.resize(2 * (size_t)n);
      size_t maxlen = 0;
      for (int i = 0; i < n; i++) {
        const std::string &a = Fs[(size_t)pair_f[p0 + i]], &b = Rs[(size_t)pair_r[p0 + i]];
        two[2 * (size_t)i] = a.c_str(); two[2 * (size_t)i + 1] = b.c_str();
        maxlen = std::max(maxlen, std::max(a.size(), b.size()));
      }
      dada2hip_sample *s = new dada2hip_sample();
      std::unique_ptr<dada2hip_sample, void (*)(dada2hip_sample *)> guard(s, dada2hip_sample_free);
      const int stride = mp_align_chunk(s, n, two, (int)maxlen, match, mismatch, device);
      add_lap(st[MR_US_ALIGN], t0);
      // the verdicts
      t0 = clk::now();
      const MpPairs Pp{d_pf.p + p0, d_pr.p + p0};
      const MpVerdict V{d_v.p, d_v.p + n, d_v.p + 2 * (size_t)n, d_v.p + 3 * (size_t)n, d_v.p + 4 * (size_t)n, d_v.p + 5 * (size_t)n, d_v.p + 6 * (size_t)n};
      launch_mp_eval(Sq, Pp, n, s->d_moves.p, stride, s->d_nmoves.p, min_overlap, max_mismatch, trim_overhang != 0, V, d_ctr.p, s->stream);
      sync_checked(s->stream);
      add_lap(st[MR_US_EVAL], t0);
      t0 = clk::now();
      v.resize(6 * (size_t)n);
      MpCounters h;
      D2_HIP(hipMemcpyAsync(v.data(), d_v.p, v.size() * 4, hipMemcpyDeviceToHost, s->stream));
      D2_HIP(hipMemcpyAsync(&h, d_ctr.p, sizeof h, hipMemcpyDeviceToHost, s->stream));
      sync_checked(s->stream);
      st[MR_BYTES_DOWN] += (int64_t)v.size() * 4 + (int64_t)sizeof h;
      add_lap(st[MR_US_DOWN], t0);
      if (h.err & MP_ERR_MOVES) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: a move string does not spell its two sequences."};
      // the merged sequences of the accepted pairs (:168, rejects get "", :177)
      t0 = clk::now();
      const int32_t *accept = v.data() + 4 * (size_t)n, *mlen = v.data() + 5 * (size_t)n;
      const long long total = mp_scan_accepted((size_t)n, accept, mlen, off);
      if (total < 0) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: a merged sequence of negative length."};
      arena.resize((size_t)total);
      if (total > 0) {
        d_arena.alloc((size_t)total);
        D2_HIP(hipMemcpyAsync(d_off.p, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, s->stream));
        launch_mp_consensus(Sq, Pp, n, s->d_moves.p, stride, s->d_nmoves.p, V, d_off.p, d_arena.p, s->stream);
        sync_checked(s->stream);
        st[MR_BYTES_UP] += (int64_t)n * 8;
      }
      add_lap(st[MR_US_EVAL], t0);
      t0 = clk::now();
      if (total > 0) {
        D2_HIP(hipMemcpyAsync(arena.data(), d_arena.p, (size_t)total, hipMemcpyDeviceToHost, s->stream));
        sync_checked(s->stream);
        st[MR_BYTES_DOWN] += total;
      }
      for (int i = 0; i < n; i++) {
        const size_t p = p0 + (size_t)i;
        for (int k = 0; k < 5; k++) H->col[MC_NMATCH + k][p] = v[(size_t)k * (size_t)n + (size_t)i];
        if (accept[i]) { seq[p].assign(arena.data() + off[(size_t)i], (size_t)mlen[i]); st[MR_ACCEPTED]++; }
      }
      add_lap(st[MR_US_DOWN], t0);
    }
  }
  H->seq_off.assign(1, 0);
  for (size_t p = 0; p < P; p++) { H->seq_bytes += seq[p]; H->seq_off.push_back((int64_t)H->seq_bytes.size()); }
  finish_stats(st, MR_US_TOTAL, t_call, stats);
  *out = H.release();
}

}  // namespace

int dada2hip_merge_run(int32_t nsamples, const int64_t *nreads, const int32_t *const *derepF_map, const int32_t *const *derepR_map,
                       const int32_t *nuniqF, const int32_t *const *dadaF_map, const int32_t *nuniqR, const int32_t *const *dadaR_map,
                       const int32_t *nclustF, const char *seqF_bytes, const int64_t *seqF_offsets, const int32_t *n0F, const int32_t *nclustR,
                       const char *seqR_bytes, const int64_t *seqR_offsets, const int32_t *n0R, int32_t min_overlap, int32_t max_mismatch,
                       int32_t trim_overhang, int32_t just_concatenate, int32_t device, dada2hip_run_mergers **out, int64_t *stats, char *errbuf,
                       size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    merge_run_body(nsamples, nreads, derepF_map, derepR_map, nuniqF, dadaF_map, nuniqR, dadaR_map, nclustF, seqF_bytes, seqF_offsets, n0F, nclustR,
                   seqR_bytes, seqR_offsets, n0R, min_overlap, max_mismatch, trim_overhang, just_concatenate, device, out, stats);
  });
}

int32_t dada2hip_merge_run_nsamples(const dada2hip_run_mergers *m) { return m ? m->nsamples : 0; }
int64_t dada2hip_merge_run_nrow(const dada2hip_run_mergers *m, int32_t sample) {
  return (m && sample >= 0 && sample < m->nsamples) ? m->row0[(size_t)sample + 1] - m->row0[(size_t)sample] : 0;
}
const int32_t *dada2hip_merge_run_column(const dada2hip_run_mergers *m, int32_t sample, int32_t which) {
  if (!m || sample < 0 || sample >= m->nsamples || which < 0 || which > 7) return nullptr;
  return m->col[which].data() + m->row0[(size_t)sample];
}
const char *dada2hip_merge_run_sequences(const dada2hip_run_mergers *m, int32_t sample, const int64_t **offsets) {
  const bool ok = m && sample >= 0 && sample < m->nsamples;
  if (offsets) *offsets = ok ? m->seq_off.data() + m->row0[(size_t)sample] : nullptr;
  return ok ? m->seq_bytes.data() : nullptr;
}
void dada2hip_merge_run_free(dada2hip_run_mergers *m) { delete m; }
