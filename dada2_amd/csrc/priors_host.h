// priors_host.h — host side of dada2hip_sample_set_prior_seqs (names(uniques) %in% c(priors, pseudo_priors), R/dada.R:335);
// included by driver.cpp inside its extern "C" block, behind primers_host.h.
//
// The prior sequences that can match a unique at all - A/C/G/T only, not empty, no longer than the sample's longest unique - are
// keyed by their first min(32, length) letters, the distinct keys sorted inside key-length groups (stage_plain.h: build_prefix_keys),
// and each is packed once to a 2-bit row on a 16-byte boundary where the kernel reads it: key by key, inside a key in the caller's
// order (pr_build_tables).  Keys, rows and each key's run of rows go
// up, k_prior_match (priors.inc.hip) gives every resident unique a lane, and the flags come back in ONE copy of N bytes into
// h_prior, the mirror the host's p-value replay reads (dada2hip_sample_set_priors keeps it in step the other way round).
#pragma once

namespace {

struct PrTables {
  PrefixKeyTable K;
  std::vector<int32_t> key_row_off, row_woff, row_len, row_seq;
  std::vector<uint32_t> row_words;
};

void pr_build_tables(int32_t n, const char *const *seqs, int maxlen, PrTables &T, int64_t &kept) {
  T = PrTables();
  // the entries kept, with the prefix key of each from its first min(32, length) letters
  std::vector<int32_t> idx, len;
  for (int32_t j = 0; j < n; j++) {
    const char *s = seqs[j];
    if (!s) throw InputError{"dada2hip: bad arguments"};
    const size_t l = strnlen(s, (size_t)maxlen + 1);
    if (l == 0 || l > (size_t)maxlen) continue;
    bool ok = true;
    for (size_t i = 0; i < l && ok; i++) ok = acgt_code(s[i]) >= 0;
    if (!ok) continue;
    idx.push_back(j); len.push_back((int32_t)l);
  }
  kept = (int64_t)idx.size();
  const size_t nr = idx.size();
  std::vector<PrefixKey> kp(nr);
  parallel_for(nr, 1024, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      uint32_t head[2] = {0u, 0u};
      const char *s = seqs[idx[r]];
      const int kl = std::min(len[r], 32);
      for (int i = 0; i < kl; i++) head[i >> 4] |= (uint32_t)acgt_code(s[i]) << (2 * (i & 15));
      kp[r] = prefix_key(head, kl);
    }
  });
  build_prefix_keys(kp, T.K);
  // the rows of every key, in the caller's order inside a key: a counting sort of the entries by key
  const size_t nk = T.K.keys.size();
  T.key_row_off.assign(nk + 1, 0);
  for (int32_t k : T.K.key_of) T.key_row_off[k + 1]++;
  for (size_t k = 0; k < nk; k++) T.key_row_off[k + 1] += T.key_row_off[k];
  std::vector<int32_t> at(T.key_row_off.begin(), T.key_row_off.end() - 1), slot(nr);
  for (size_t r = 0; r < nr; r++) slot[r] = at[T.K.key_of[r]]++;
  T.row_woff.resize(nr); T.row_len.resize(nr); T.row_seq.resize(nr);
  for (size_t r = 0; r < nr; r++) { T.row_len[slot[r]] = len[r]; T.row_seq[slot[r]] = idx[r]; }
  size_t w = 0;                                                  // every row a multiple of 4 words: 16-byte boundaries
  for (size_t t = 0; t < nr; t++) {
    if (w > (size_t)INT32_MAX) throw RuntimeErr{DADA2HIP_ERR_RUNTIME, "dada2hip: the prior sequences are too large for one call."};
    T.row_woff[t] = (int32_t)w;
    w += (size_t)((((T.row_len[t] + 15) / 16) + 3) & ~3);
  }
  // ... and every row packed once, where it stays
  T.row_words.assign(w, 0u);
  parallel_for(nr, 256, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      uint32_t *row = T.row_words.data() + T.row_woff[slot[r]];
      const char *s = seqs[idx[r]];
      for (int i = 0; i < len[r]; i++) row[i >> 4] |= (uint32_t)acgt_code(s[i]) << (2 * (i & 15));
    }
  });
}

void set_prior_seqs_body(dada2hip_sample *s, int32_t n, const char *const *seqs, const uint8_t *or_flags, int32_t *first_match,
                         int32_t *nset) {
  auto t_call = clk::now();
  if (!s || n < 0 || (n > 0 && !seqs)) throw InputError{"dada2hip: bad arguments"};
  int64_t st[DADA2HIP_PRIOR_SEQS_NSTATS] = {0};
  const SampleDev &D = s->D;
  const int N = D.N;
  st[QS_GIVEN] = n;
  PrTables T;
  pr_build_tables(n, seqs, D.maxlen, T, st[QS_KEPT]);
  const int nkeys = (int)T.K.keys.size();
  st[QS_KEYS] = nkeys;
  add_lap(st[QS_US_PACK], t_call);

  auto t_dev = clk::now();
  select_device(s->device);
  hipStream_t q = s->stream;
  DevBuf<unsigned long long> d_keys;
  DevBuf<int32_t> d_groups, d_kro, d_rwo, d_rl, d_rs, d_first;
  DevBuf<uint32_t> d_rw;
  DevBuf<uint8_t> d_or;
  auto up = [&](auto &d, const auto &h) {
    d.alloc(h.size());
    if (!h.empty()) D2_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice, q));
  };
  up(d_keys, T.K.keys); up(d_groups, T.K.groups); up(d_kro, T.key_row_off); up(d_rwo, T.row_woff); up(d_rl, T.row_len); up(d_rs, T.row_seq);
  up(d_rw, T.row_words);
  if (or_flags) { d_or.alloc((size_t)N); D2_HIP(hipMemcpyAsync(d_or.p, or_flags, (size_t)N, hipMemcpyHostToDevice, q)); }
  if (first_match) d_first.alloc((size_t)N);
  PriorKeys K;
  K.keys = d_keys.p; K.groups = d_groups.p; K.ngroups = (int)(T.K.groups.size() / 3); K.nkeys = nkeys;
  K.key_row_off = d_kro.p; K.row_woff = d_rwo.p; K.row_len = d_rl.p; K.row_seq = d_rs.p; K.row_words = d_rw.p;
  const bool lds = nkeys > 0 && nkeys <= std::min(std::max(knobs().priors_lds_keys, 0), PRIOR_LDS_KEYS_MAX);
  const int grid_cap = knobs().priors_grid > 0 ? knobs().priors_grid : 2048;
  st[QS_LDS] = lds ? 1 : 0;
  Events<2> ev;
  const bool timed = knobs().profile;
  if (timed) { ev.create(); D2_HIP(hipEventRecord(ev[0], q)); }
  st[QS_BLOCKS] = launch_prior_match(D, K, lds, grid_cap, or_flags ? d_or.p : nullptr, first_match ? d_first.p : nullptr, q);
  D2_HIP(hipGetLastError());
  if (timed) D2_HIP(hipEventRecord(ev[1], q));
  // the host mirror follows the device array
  D2_HIP(hipMemcpyAsync(s->h_prior.data(), D.prior, (size_t)N, hipMemcpyDeviceToHost, q));
  if (first_match) D2_HIP(hipMemcpyAsync(first_match, d_first.p, (size_t)N * 4, hipMemcpyDeviceToHost, q));
  sync_checked(q);
  if (timed) add_elapsed(st[QS_US_KERNEL], ev[0], ev[1]);
  int64_t set = 0;
  for (int i = 0; i < N; i++) set += s->h_prior[i] != 0;
  st[QS_SET] = set;
  if (nset) *nset = (int32_t)set;
  add_lap(st[QS_US_DEVICE], t_dev);
  st[QS_US_TOTAL] = (int64_t)(ms_since(t_call) * 1e3);
  memcpy(s->prior_seqs_stats, st, sizeof st);
}

}  // namespace

int dada2hip_sample_set_prior_seqs(dada2hip_sample *s, int32_t n, const char *const *seqs, const uint8_t *or_flags, int32_t *first_match,
                                   int32_t *nset, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] { set_prior_seqs_body(s, n, seqs, or_flags, first_match, nset); });
}

void dada2hip_sample_prior_seqs_stats(const dada2hip_sample *s, int64_t *stats) {
  if (s && stats) memcpy(stats, s->prior_seqs_stats, sizeof s->prior_seqs_stats);
}
