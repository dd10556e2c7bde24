// species_host.h — host side of assignSpecies (R/taxonomy.R:264-280; :240-263 and :281-360 are dada2_amd/api.py's); included by
// driver.cpp inside its extern "C" block, behind taxonomy_host.h.
//
// dada2hip_species_open packs the references once (sp_pack_refs: 2-bit words, the plane of letters outside upper-case A/C/G/T,
// every row on a 32-base boundary so that no two rows share a word of either array) and keeps them on the device.  A call folds
// equal queries, and per chunk of distinct queries builds the tables of species.inc.hip (sp_build_tables: the patterns - queries
// and, with try_rc, their reverse complements - packed, their distinct prefix keys sorted inside key-length groups, a CSR list of
// patterns per key), runs the seed kernel over the references and the verify kernel over its candidates, and gathers
// (query, reference) pairs.  The candidate buffer is fixed (DADA2HIP_SPECIES_CAND): the seed kernel counts every hit and stores
// what fits, and a range of references that counted more is halved and run again; a single reference that still counts more
// runs with a buffer of the counted size.  The hit buffer starts at the same size and grows to the counted size.  The pairs are
// sorted and repeats dropped on the host (several positions or both strands in one reference are one hit), then expanded to the
// caller's queries.  stage_common.h: acgt_code, revcomp_acgt, the prefix keys and their groups, Events, the clocks, finish_stats.
#pragma once

struct dada2hip_species {
  int device = 0;
  int nref = 0;
  long long nbases = 0;
  DevBuf<uint32_t> words, nplane;
  DevBuf<long long> woff;
  DevBuf<int32_t> len;
  hipStream_t stream = nullptr;
  mutable std::mutex mu;               // calls on one model take turns (one stream, one set of events)
  ~dada2hip_species() { if (stream) (void)hipStreamDestroy(stream); }
};

struct dada2hip_species_hits {
  std::vector<int64_t> offsets;        // nseq + 1
  std::vector<int32_t> refs;
};

namespace {

constexpr int SP_KEY = 32;             // bases of a prefix key
constexpr int SP_CHUNK_MAX = 8192;     // distinct queries per pass: at most 16 384 keys, two bits each, in the 2^18-bit bitmap (98.6 % of the misses stop there)

struct SpPacked {
  std::vector<uint32_t> words, nplane;
  std::vector<long long> woff;
  std::vector<int32_t> len;
  long long nbases = 0;
};

void sp_pack_refs(int nref, const char *const *refs, SpPacked &P) {
  P.woff.resize(nref); P.len.resize(nref);
  long long w = 0, nb = 0;
  for (int r = 0; r < nref; r++) {
    const size_t l = strlen(refs[r]);
    if (l > (size_t)INT32_MAX - 64) throw InputError{"dada2hip: a reference sequence is too long."};
    P.woff[r] = w; P.len[r] = (int32_t)l;
    w += (long long)((l + 31) / 32) * 2;
    nb += (long long)l;
  }
  P.nbases = nb;
  P.words.assign((size_t)w + 4, 0u);                          // (padding: the kernels read a word or two behind a row)
  P.nplane.assign((size_t)w / 2 + 2, 0u);
  parallel_for((size_t)nref, 64, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      uint32_t *row = P.words.data() + P.woff[r], *pl = P.nplane.data() + P.woff[r] / 2;
      const char *s = refs[r];
      for (int i = 0; i < P.len[r]; i++) {
        const int b = acgt_code(s[i]);
        if (b < 0) pl[i >> 5] |= 1u << (i & 31);
        else row[i >> 4] |= (uint32_t)b << (2 * (i & 15));
      }
    }
  });
}

struct SpTables {
  PrefixKeyTable K;                                             // keys, groups (key_of: per pattern)
  std::vector<int32_t> key_pat_off, key_pats, pat_woff, pat_len, pat_query;
  std::vector<uint32_t> pat_words;
};

// the patterns of the distinct queries [q0, q1) of uq (A/C/G/T only, not empty); a pattern reports under its query's index in uq
void sp_build_tables(const std::vector<std::string> &uq, size_t q0, size_t q1, bool try_rc, SpTables &T) {
  T = SpTables();
  std::vector<PrefixKey> kp;                                    // per pattern
  auto add = [&](const std::string &s, size_t q) {
    const int len = (int)s.size();
    T.pat_woff.push_back((int32_t)T.pat_words.size()); T.pat_len.push_back(len); T.pat_query.push_back((int32_t)q);
    T.pat_words.resize(T.pat_words.size() + (size_t)(len + 15) / 16, 0u);
    uint32_t *w = T.pat_words.data() + T.pat_woff.back();
    for (int i = 0; i < len; i++) w[i >> 4] |= (uint32_t)acgt_code(s[i]) << (2 * (i & 15));
    kp.push_back(prefix_key(w, std::min(len, SP_KEY)));
  };
  for (size_t q = q0; q < q1; q++) {
    const std::string &s = uq[q];
    add(s, q);
    if (try_rc) {
      const std::string rc = revcomp_acgt(s);
      if (rc != s) add(rc, q);
    }
  }
  if (T.pat_words.size() > (size_t)INT32_MAX) throw RuntimeErr{DADA2HIP_ERR_RUNTIME, "dada2hip: a chunk of queries is too large."};
  build_prefix_keys(kp, T.K);
  // the patterns of every key, ascending inside a key: a counting sort of the patterns by key
  T.key_pat_off.assign(T.K.keys.size() + 1, 0); T.key_pats.resize(kp.size());
  for (int32_t k : T.K.key_of) T.key_pat_off[k + 1]++;
  for (size_t k = 0; k < T.K.keys.size(); k++) T.key_pat_off[k + 1] += T.key_pat_off[k];
  std::vector<int32_t> at(T.key_pat_off.begin(), T.key_pat_off.end() - 1);
  for (size_t pat = 0; pat < kp.size(); pat++) T.key_pats[at[T.K.key_of[pat]]++] = (int32_t)pat;
}

void species_open_body(int32_t nref, const char *const *refs, int32_t device, dada2hip_species **out, int64_t *stats) {
  auto t_call = clk::now();
  if (!out) throw InputError{"dada2hip: bad arguments"};
  *out = nullptr;
  if (nref <= 0 || !refs) throw InputError{"dada2hip: no reference sequences provided."};
  for (int r = 0; r < nref; r++) if (!refs[r]) throw InputError{"dada2hip: bad arguments"};
  SpPacked P;
  sp_pack_refs(nref, refs, P);
  select_device(device);
  std::unique_ptr<dada2hip_species> m(new dada2hip_species());
  m->device = device; m->nref = nref; m->nbases = P.nbases;
  D2_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  m->words.alloc(P.words.size()); m->nplane.alloc(P.nplane.size()); m->woff.alloc(nref); m->len.alloc(nref);
  D2_HIP(hipMemcpy(m->words.p, P.words.data(), P.words.size() * 4, hipMemcpyHostToDevice));
  D2_HIP(hipMemcpy(m->nplane.p, P.nplane.data(), P.nplane.size() * 4, hipMemcpyHostToDevice));
  D2_HIP(hipMemcpy(m->woff.p, P.woff.data(), (size_t)nref * 8, hipMemcpyHostToDevice));
  D2_HIP(hipMemcpy(m->len.p, P.len.data(), (size_t)nref * 4, hipMemcpyHostToDevice));
  int64_t st[DADA2HIP_SPECIES_NSTATS] = {0};
  st[SS_REFS] = nref; st[SS_BASES] = P.nbases; st[SS_BYTES] = (int64_t)((P.words.size() + P.nplane.size()) * 4 + (size_t)nref * 12);
  finish_stats(st, SS_US_TOTAL, t_call, stats);
  *out = m.release();
}

void species_match_body(const dada2hip_species *m, int32_t nseq, const char *const *seqs, int32_t try_rc, dada2hip_species_hits **out,
                        int64_t *stats) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_SPECIES_NSTATS] = {0};
  if (!out) throw InputError{"dada2hip: bad arguments"};
  *out = nullptr;
  if (nseq < 0 || (nseq > 0 && !seqs)) throw InputError{"dada2hip: bad arguments"};
  // ---- checks and the fold of equal queries, before any device work ----
  std::vector<std::string> uq;
  std::vector<int32_t> to_uq(nseq);
  {
    std::unordered_map<std::string, int32_t> seen;
    for (int j = 0; j < nseq; j++) {
      if (!seqs[j]) throw InputError{"dada2hip: bad arguments"};
      if (!seqs[j][0]) throw InputError{"dada2hip: an empty query sequence."};
      for (const char *c = seqs[j]; *c; c++)
        if (acgt_code(*c) < 0) throw InputError{"Non-ACGT characters present in the query sequences."};   // taxonomy.R:254
      auto it = seen.emplace(seqs[j], (int32_t)uq.size());
      if (it.second) uq.emplace_back(seqs[j]);
      to_uq[j] = it.first->second;
    }
  }
  if (!m) throw InputError{"dada2hip: no species references."};
  st[SS_REFS] = m->nref; st[SS_BASES] = m->nbases;
  std::vector<unsigned long long> pairs;                       // distinct query << 32 | reference

  if (!uq.empty()) {
    std::lock_guard<std::mutex> lock(m->mu);
    select_device(m->device);
    const size_t chunk = (size_t)std::min(std::max(knobs().species_chunk, 1), SP_CHUNK_MAX);
    const unsigned long long cap0 = (unsigned long long)std::max(knobs().species_cand, 1);
    SpeciesRefs R;
    R.words = m->words.p; R.nplane = m->nplane.p; R.woff = m->woff.p; R.len = m->len.p;
    DevBuf<unsigned long long> d_keys, d_hits, d_counters;
    DevBuf<int32_t> d_groups, d_kpo, d_kp, d_pwo, d_pl, d_pq;
    DevBuf<uint32_t> d_pw, d_bitmap;
    DevBuf<SpCand> d_cand;
    d_counters.alloc(4); d_bitmap.alloc(SP_BITMAP_WORDS); d_cand.alloc((size_t)cap0); d_hits.alloc((size_t)cap0);
    Events<4> ev;
    ev.create();
    hipStream_t s = m->stream;
    unsigned long long cnt[4];
    auto up = [&](auto &d, const auto &h) {
      d.alloc(h.size());
      if (!h.empty()) D2_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice, s));
    };
    auto counted = [&](int e, int word, auto &&launch) {        // a launch between ev[e] and ev[e + 1], the counters back behind it
      D2_HIP(hipEventRecord(ev[e], s));
      launch();
      D2_HIP(hipEventRecord(ev[e + 1], s));
      D2_HIP(hipMemcpyAsync(cnt, d_counters.p, 4 * 8, hipMemcpyDeviceToHost, s));
      sync_checked(s);
      st[SS_LAUNCHES]++;
      add_elapsed(st[word], ev[e], ev[e + 1]);
    };
    SpTables T;
    std::vector<unsigned long long> got;
    for (size_t q0 = 0; q0 < uq.size(); q0 += chunk) {
      sp_build_tables(uq, q0, std::min(uq.size(), q0 + chunk), try_rc != 0, T);
      up(d_keys, T.K.keys); up(d_groups, T.K.groups); up(d_kpo, T.key_pat_off); up(d_kp, T.key_pats); up(d_pwo, T.pat_woff);
      up(d_pl, T.pat_len); up(d_pq, T.pat_query); up(d_pw, T.pat_words);
      SpeciesKeys K;
      K.keys = d_keys.p; K.groups = d_groups.p; K.ngroups = (int)(T.K.groups.size() / 3); K.nkeys = (int)T.K.keys.size();
      K.key_pat_off = d_kpo.p; K.key_pats = d_kp.p; K.pat_woff = d_pwo.p; K.pat_len = d_pl.p; K.pat_query = d_pq.p; K.pat_words = d_pw.p;
      D2_HIP(hipMemsetAsync(d_bitmap.p, 0, SP_BITMAP_WORDS * 4, s));
      launch_species_bitmap(K, d_bitmap.p, s);
      st[SS_LAUNCHES]++;
      std::vector<std::pair<int, int>> ranges(1, std::make_pair(0, m->nref));
      while (!ranges.empty()) {
        const int r0 = ranges.back().first, r1 = ranges.back().second;
        ranges.pop_back();
        // ---- seed ----
        auto t_seed = clk::now();
        D2_HIP(hipMemsetAsync(d_counters.p, 0, 4 * 8, s));
        counted(0, SS_US_SEED_DEV, [&] { launch_species_seed(R, r0, r1, K, d_bitmap.p, d_cand.p, (unsigned long long)d_cand.n, d_counters.p, s); });
        add_lap(st[SS_US_SEED_HOST], t_seed);
        const unsigned long long ncand = cnt[0];
        if (ncand > (unsigned long long)d_cand.n) {            // nothing of this launch is used
          st[SS_RERUNS]++;
          if (r1 - r0 > 1) {
            const int mid = r0 + (r1 - r0) / 2;
            ranges.emplace_back(mid, r1); ranges.emplace_back(r0, mid);
          } else {
            d_cand.alloc((size_t)ncand);
            ranges.emplace_back(r0, r1);
          }
          continue;
        }
        st[SS_WINDOWS] += (int64_t)cnt[1]; st[SS_PAST_BITMAP] += (int64_t)cnt[2]; st[SS_CANDIDATES] += (int64_t)ncand;
        if (ncand == 0) continue;
        // ---- verify ----
        auto t_ver = clk::now();
        for (;;) {
          D2_HIP(hipMemsetAsync(d_counters.p + 3, 0, 8, s));
          counted(2, SS_US_VERIFY_DEV, [&] { launch_species_verify(R, K, d_cand.p, ncand, d_hits.p, (unsigned long long)d_hits.n, d_counters.p, s); });
          if (cnt[3] <= (unsigned long long)d_hits.n) break;
          d_hits.alloc((size_t)cnt[3]);                        // (the candidates are still there: only this kernel runs again)
        }
        if (cnt[3] > 0) {
          got.resize((size_t)cnt[3]);
          D2_HIP(hipMemcpy(got.data(), d_hits.p, (size_t)cnt[3] * 8, hipMemcpyDeviceToHost));
          std::sort(got.begin(), got.end());
          got.erase(std::unique(got.begin(), got.end()), got.end());
          pairs.insert(pairs.end(), got.begin(), got.end());
        }
        add_lap(st[SS_US_VERIFY_HOST], t_ver);
      }
    }
  }
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());

  // ---- per caller's query: the references of its distinct query, ascending ----
  std::vector<int64_t> uoff(uq.size() + 1, 0);
  for (unsigned long long p : pairs) uoff[(size_t)(p >> 32) + 1]++;
  for (size_t q = 0; q < uq.size(); q++) uoff[q + 1] += uoff[q];
  std::unique_ptr<dada2hip_species_hits> H(new dada2hip_species_hits());
  H->offsets.assign((size_t)nseq + 1, 0);
  for (int j = 0; j < nseq; j++) H->offsets[j + 1] = H->offsets[j] + (uoff[to_uq[j] + 1] - uoff[to_uq[j]]);
  H->refs.resize((size_t)H->offsets[nseq]);
  for (int j = 0; j < nseq; j++) {
    int32_t *o = H->refs.data() + H->offsets[j];
    for (int64_t i = uoff[to_uq[j]]; i < uoff[to_uq[j] + 1]; i++) *o++ = (int32_t)(uint32_t)pairs[(size_t)i];
  }
  st[SS_HITS] = H->offsets[nseq];
  finish_stats(st, SS_US_TOTAL, t_call, stats);
  *out = H.release();
}

}  // namespace

int dada2hip_species_open(int32_t nref, const char *const *refs, int32_t device, dada2hip_species **out, int64_t *stats, char *errbuf,
                          size_t errlen) {
  return guarded(errbuf, errlen, [&] { species_open_body(nref, refs, device, out, stats); });
}

void dada2hip_species_free(dada2hip_species *m) { delete m; }

int dada2hip_species_match(const dada2hip_species *m, int32_t nseq, const char *const *seqs, int32_t try_rc, dada2hip_species_hits **out,
                           int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] { species_match_body(m, nseq, seqs, try_rc, out, stats); });
}

const int64_t *dada2hip_species_hits_offsets(const dada2hip_species_hits *h) { return h->offsets.data(); }
const int32_t *dada2hip_species_hits_refs(const dada2hip_species_hits *h) { return h->refs.data(); }
void dada2hip_species_hits_free(dada2hip_species_hits *h) { delete h; }
