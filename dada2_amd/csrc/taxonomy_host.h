// taxonomy_host.h — host side of assignTaxonomy (src/taxonomy.cpp; R/taxonomy.R:65-160 is dada2_amd/api.py's); included by
// driver.cpp inside its extern "C" block, behind collapse_host.h.
//
// The model (taxonomy.cpp:219-270) is built on the host and only the finished table is uploaded: presence counts of every 8-mer
// per genus and in total come sparsely from each reference's distinct k-mers (the reference walks nref x 65 536 bytes), the
// prior is (float)((total + 0.5) / (1.0 + nref)) in double, the entry logf((cnt + prior) / (M_g + 1)) in float - by the HOST's
// logf: the reference's table is libm's logf, a device logf is another function, and the sums of the classifier reproduce the
// reference's bits only over a table that is bit-equal to its table.  cnt is a float the reference increments, exact below 2^24
// references.  On the device the table lies k-mer-major, T[kmer][genus padded to 64] (taxonomy.inc.hip).
// A call of the classifier prepares, per query, its sorted valid k-mers (tax_karray, :55-71) and the replicate positions
// (int)(arraylen * u) with u in the reference's layout (:181-186: query j starts at unifs[j * max_arraylen] - neighbours overlap),
// runs the kernels over chunks of queries, counts `boot` on the host (:189-195).  stage_common.h: acgt_code, Events, the clocks.
#pragma once

struct dada2hip_taxonomy {
  int device = 0;
  int ngenus = 0, nlevel = 0, gpad = 0;
  std::vector<int32_t> genusmat;      // ngenus x nlevel, row-major
  DevBuf<float> T;                    // [65536][gpad]
  hipStream_t stream = nullptr;
  ~dada2hip_taxonomy() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace {

constexpr int TAX_K = 8, TAX_NKMER = 1 << (2 * TAX_K), TAX_NBOOT = 100, TAX_NPASS = TAX_NBOOT + 1, TAX_MIN_LEN = 50;
constexpr int TAX_SLAB_MAX = 512;     // 128 KB of the 160 KB of LDS a workgroup can have

// the valid 8-mer indices of s (of its reverse complement with rc), sorted ascending, duplicates kept; a k-mer with a letter
// outside ACGT in it is skipped (tax_kmer returns -1)
void tax_karray(const char *s, int len, bool rc, std::vector<uint16_t> &out) {
  out.clear();
  uint32_t w = 0;
  int run = 0;
  for (int i = 0; i < len; i++) {
    int b = acgt_code(rc ? s[len - 1 - i] : s[i]);
    if (b < 0) { run = 0; continue; }
    if (rc) b = 3 - b;
    w = ((w << 2) | (uint32_t)b) & (TAX_NKMER - 1);
    if (++run >= TAX_K) out.push_back((uint16_t)w);
  }
  std::sort(out.begin(), out.end());
}

// The generator behind unifs == NULL: value i of the buffer is splitmix64 of (seed + (i + 1) * 0x9E3779B97F4A7C15), its top 53
// bits scaled into [0, 1).  Counter-based, so the buffer need not exist.
inline double tax_unif(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

void taxonomy_train_body(int32_t nref, const char *const *refs, const int32_t *ref_to_genus, int32_t ngenus, int32_t nlevel,
                         const int32_t *genusmat, int32_t device, dada2hip_taxonomy **out, int64_t *stats) {
  auto t_call = clk::now();
  if (!out) throw InputError{"dada2hip: bad arguments"};
  *out = nullptr;
  if (nref <= 0 || !refs || !ref_to_genus) throw InputError{"dada2hip: no reference sequences provided."};
  if (nref >= (1 << 24)) throw InputError{"dada2hip: assignTaxonomy takes fewer than 2^24 references (the counts are floats)."};
  if (ngenus <= 0 || nlevel <= 0 || !genusmat) throw InputError{"dada2hip: the taxonomy has no genus or no level."};
  for (int i = 0; i < nref; i++) {
    if (!refs[i] || strnlen(refs[i], TAX_K) < (size_t)TAX_K) throw InputError{"dada2hip: a reference sequence is shorter than the k-mer size (8)."};
    if (ref_to_genus[i] < 0 || ref_to_genus[i] >= ngenus) throw InputError{"Invalid map from references to genus."};   // taxonomy.cpp:222
  }
  select_device(device);

  // the distinct k-mers of every reference
  std::vector<std::vector<uint16_t>> rk(nref);
  parallel_for((size_t)nref, 8, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      tax_karray(refs[i], (int)strlen(refs[i]), false, rk[i]);
      rk[i].erase(std::unique(rk[i].begin(), rk[i].end()), rk[i].end());
    }
  });
  std::vector<uint32_t> total(TAX_NKMER, 0);
  for (int i = 0; i < nref; i++) for (uint16_t k : rk[i]) total[k]++;
  std::vector<float> prior(TAX_NKMER);
  for (int k = 0; k < TAX_NKMER; k++) prior[k] = (float)(((float)total[k] + 0.5) / (1.0 + (double)(size_t)nref));   // :261
  std::vector<float> mg1(ngenus, 0.0f);                        // M_g + 1 (:227-234)
  std::vector<int32_t> gstart(ngenus + 1, 0), gref(nref);
  for (int i = 0; i < nref; i++) { mg1[ref_to_genus[i]] += 1.0f; gstart[ref_to_genus[i] + 1]++; }
  for (int g = 0; g < ngenus; g++) { mg1[g] += 1.0f; gstart[g + 1] += gstart[g]; }
  {
    std::vector<int32_t> fill(gstart.begin(), gstart.end() - 1);
    for (int i = 0; i < nref; i++) gref[fill[ref_to_genus[i]]++] = i;
  }
  // the column of a genus is, outside its own k-mers, logf(prior / (M_g + 1)): one such column per distinct M_g
  std::vector<float> sizes(mg1);
  std::sort(sizes.begin(), sizes.end());
  sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
  const size_t nsz = sizes.size();
  std::vector<float> zero_col(nsz * TAX_NKMER);
  parallel_for(nsz * 64, 1, [&](size_t lo, size_t hi) {
    for (size_t j = lo; j < hi; j++) {
      const size_t d = j / 64, k0 = (j % 64) * (TAX_NKMER / 64);
      for (size_t k = k0; k < k0 + TAX_NKMER / 64; k++) zero_col[d * TAX_NKMER + k] = logf((0.0f + prior[k]) / sizes[d]);   // :268
    }
  });
  const int gpad = (ngenus + 63) / 64 * 64;
  std::vector<float> T((size_t)TAX_NKMER * gpad, 0.0f);
  // sixteen genera (one cache line of a table row) per piece
  parallel_for((size_t)(ngenus + 15) / 16, 1, [&](size_t lo, size_t hi) {
    std::vector<uint32_t> cnt(TAX_NKMER, 0);
    std::vector<uint16_t> touched;
    for (size_t piece = lo; piece < hi; piece++) {
      const int g0 = (int)piece * 16, g1 = std::min(ngenus, g0 + 16);
      const float *col[16];
      for (int g = g0; g < g1; g++) col[g - g0] = zero_col.data() + (size_t)(std::lower_bound(sizes.begin(), sizes.end(), mg1[g]) - sizes.begin()) * TAX_NKMER;
      for (int k = 0; k < TAX_NKMER; k++)
        for (int g = g0; g < g1; g++) T[(size_t)k * gpad + g] = col[g - g0][k];
      for (int g = g0; g < g1; g++) {
        touched.clear();
        for (int r = gstart[g]; r < gstart[g + 1]; r++)
          for (uint16_t k : rk[gref[r]]) if (cnt[k]++ == 0) touched.push_back(k);
        for (uint16_t k : touched) {
          T[(size_t)k * gpad + g] = logf(((float)cnt[k] + prior[k]) / mg1[g]);   // :268
          cnt[k] = 0;
        }
      }
    }
  });

  std::unique_ptr<dada2hip_taxonomy> m(new dada2hip_taxonomy());
  m->device = device; m->ngenus = ngenus; m->nlevel = nlevel; m->gpad = gpad;
  m->genusmat.assign(genusmat, genusmat + (size_t)ngenus * nlevel);
  D2_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  m->T.alloc(T.size());
  const double ms_host = ms_since(t_call);
  D2_HIP(hipMemcpy(m->T.p, T.data(), T.size() * sizeof(float), hipMemcpyHostToDevice));
  if (stats) {
    memset(stats, 0, DADA2HIP_TAXONOMY_NSTATS * sizeof(int64_t));
    stats[TT_US_HOST] = (int64_t)(ms_host * 1e3); stats[TT_US_UPLOAD] = (int64_t)((ms_since(t_call) - ms_host) * 1e3);
    stats[TT_BYTES] = (int64_t)(T.size() * sizeof(float));
  }
  *out = m.release();
}

struct TaxQuery {
  int32_t id;                          // the caller's index
  std::vector<uint16_t> ka, ka_rc, bpos;
};

// One instance over the queries `list` (indices into Q), in chunks whose per-tile records stay within 64 MB.  rc: the k-mers of
// the reverse complement.  best / ntie / winner: [list.size()][npass].  Returns the device time of the sums kernel in microseconds.
double taxonomy_run(const dada2hip_taxonomy *m, const std::vector<TaxQuery> &Q, const std::vector<int> &list, bool rc, int npass,
                    bool slab, uint64_t seed, std::vector<float> &best, std::vector<int32_t> &ntie, std::vector<int32_t> &winner,
                    int64_t &launches) {
  const int ntiles = m->gpad / 64;
  best.resize(list.size() * npass); ntie.resize(list.size() * npass); winner.resize(list.size() * npass);
  if (list.empty()) return 0.0;
  const size_t per_query = (size_t)npass * ntiles * sizeof(TaxPart);
  const size_t chunk_max = std::max<size_t>(1, std::min<size_t>(((size_t)64 << 20) / per_query, (size_t)INT32_MAX / 2 / ntiles));
  const size_t chunk = knobs().tax_chunk > 0 ? std::min<size_t>((size_t)knobs().tax_chunk, chunk_max) : chunk_max;   // DADA2HIP_TAX_CHUNK
  DevBuf<int32_t> d_koff, d_qid, d_ntie, d_winner;
  DevBuf<uint16_t> d_karr, d_bpos;
  DevBuf<long long> d_boff;
  DevBuf<TaxPart> d_part;
  DevBuf<float> d_best;
  std::vector<int32_t> koff, qid;
  std::vector<long long> boff;
  std::vector<uint16_t> karr, bpos;
  Events<2> ev;
  ev.create();
  double us = 0.0;
  for (size_t c0 = 0; c0 < list.size(); c0 += chunk) {
    const size_t nq = std::min(chunk, list.size() - c0);
    koff.assign(1, 0); qid.clear(); boff.clear(); karr.clear(); bpos.clear();
    int max_a = 0;
    for (size_t i = 0; i < nq; i++) {
      const TaxQuery &q = Q[list[c0 + i]];
      const std::vector<uint16_t> &ka = rc ? q.ka_rc : q.ka;
      karr.insert(karr.end(), ka.begin(), ka.end());
      koff.push_back((int32_t)karr.size());
      qid.push_back(q.id);
      boff.push_back((long long)bpos.size());
      if (npass > 1) bpos.insert(bpos.end(), q.bpos.begin(), q.bpos.end());
      max_a = std::max(max_a, (int)ka.size());
    }
    if (karr.size() > (size_t)INT32_MAX) throw RuntimeErr{DADA2HIP_ERR_RUNTIME, "dada2hip: a chunk of queries is too large."};
    d_koff.alloc(koff.size()); d_qid.alloc(nq); d_boff.alloc(nq); d_karr.alloc(karr.size()); d_bpos.alloc(bpos.size());
    d_part.alloc(nq * npass * ntiles); d_best.alloc(nq * npass); d_ntie.alloc(nq * npass); d_winner.alloc(nq * npass);
    D2_HIP(hipMemcpyAsync(d_koff.p, koff.data(), koff.size() * 4, hipMemcpyHostToDevice, m->stream));
    D2_HIP(hipMemcpyAsync(d_qid.p, qid.data(), nq * 4, hipMemcpyHostToDevice, m->stream));
    D2_HIP(hipMemcpyAsync(d_boff.p, boff.data(), nq * 8, hipMemcpyHostToDevice, m->stream));
    if (!karr.empty()) D2_HIP(hipMemcpyAsync(d_karr.p, karr.data(), karr.size() * 2, hipMemcpyHostToDevice, m->stream));
    if (!bpos.empty()) D2_HIP(hipMemcpyAsync(d_bpos.p, bpos.data(), bpos.size() * 2, hipMemcpyHostToDevice, m->stream));
    TaxJob J;
    J.T = m->T.p; J.gpad = m->gpad; J.ngenus = m->ngenus; J.ntiles = ntiles; J.nq = (int)nq; J.npass = npass;
    J.koff = d_koff.p; J.karr = d_karr.p; J.boff = d_boff.p; J.bpos = d_bpos.p; J.qid = d_qid.p;
    J.seed_lo = (uint32_t)seed; J.seed_hi = (uint32_t)(seed >> 32);
    J.part = d_part.p; J.best = d_best.p; J.ntie = d_ntie.p; J.winner = d_winner.p;
    D2_HIP(hipEventRecord(ev[0], m->stream));
    if (!(slab && launch_tax_sums(J, std::max(max_a, 1), m->stream))) launch_tax_sums(J, 0, m->stream);
    D2_HIP(hipEventRecord(ev[1], m->stream));
    launch_tax_combine(J, m->stream);
    launches += 2;
    D2_HIP(hipMemcpyAsync(best.data() + c0 * npass, d_best.p, nq * npass * 4, hipMemcpyDeviceToHost, m->stream));
    D2_HIP(hipMemcpyAsync(ntie.data() + c0 * npass, d_ntie.p, nq * npass * 4, hipMemcpyDeviceToHost, m->stream));
    D2_HIP(hipMemcpyAsync(winner.data() + c0 * npass, d_winner.p, nq * npass * 4, hipMemcpyDeviceToHost, m->stream));
    sync_checked(m->stream);
    float ms = 0.0f;
    D2_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    us += (double)ms * 1e3;
  }
  return us;
}

void taxonomy_assign_body(const dada2hip_taxonomy *m, int32_t nseq, const char *const *seqs, int32_t try_rc, const double *unifs,
                          uint64_t seed, int32_t *tax, int32_t *boot, int32_t *boot_tax, int32_t *ntie, int64_t *stats) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_TAXONOMY_NSTATS] = {0};
  if (!m) throw InputError{"dada2hip: no taxonomy model."};
  if (nseq <= 0 || !seqs) throw InputError{"No seqs provided to classify."};   // taxonomy.cpp:212
  if (!tax || !boot || !boot_tax || !ntie) throw InputError{"dada2hip: bad arguments"};
  std::vector<int32_t> len(nseq);
  int maxlen = 0;
  for (int j = 0; j < nseq; j++) {
    if (!seqs[j]) throw InputError{"dada2hip: bad arguments"};
    const size_t l = strnlen(seqs[j], (size_t)SEQLEN + 1);
    if (l > (size_t)SEQLEN) throw InputError{"Input sequences exceed the maximum allowed string length."};
    len[j] = (int32_t)l;
    maxlen = std::max(maxlen, (int)l);
  }
  const long long max_arraylen = std::max(0, maxlen - TAX_K + 1);
  const unsigned long long n_unifs = (unsigned long long)nseq * TAX_NBOOT * (unsigned long long)(max_arraylen / 8);   // :284
  const int nlevel = m->nlevel;
  std::fill(tax, tax + nseq, -1);
  std::fill(boot, boot + (size_t)nseq * nlevel, 0);
  std::fill(boot_tax, boot_tax + (size_t)nseq * TAX_NBOOT, -1);
  std::fill(ntie, ntie + (size_t)nseq * TAX_NPASS, 0);

  // ---- per query: k-mer arrays and replicate positions ----
  std::vector<TaxQuery> Q;
  for (int j = 0; j < nseq; j++) if (len[j] >= TAX_MIN_LEN) { Q.emplace_back(); Q.back().id = j; }
  std::atomic<int> bad_unif{0};
  parallel_for(Q.size(), 16, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      TaxQuery &q = Q[i];
      const int j = q.id;
      tax_karray(seqs[j], len[j], false, q.ka);
      if (try_rc) tax_karray(seqs[j], len[j], true, q.ka_rc);   // (as many valid k-mers as forward: :171 cannot fire)
      const int A = (int)q.ka.size(), n = TAX_NBOOT * (A / 8);
      q.bpos.resize(n);
      const unsigned long long u0 = (unsigned long long)j * (unsigned long long)max_arraylen;
      if (n > 0 && u0 + (unsigned long long)n > n_unifs) { bad_unif.store(2); continue; }
      for (int b = 0; b < n; b++) {
        const double u = unifs ? unifs[u0 + b] : tax_unif(seed, u0 + b);
        if (!(u >= 0.0 && u < 1.0)) { bad_unif.store(1); break; }
        q.bpos[b] = (uint16_t)std::min((int)(A * u), A - 1);   // (:185; the clamp only where A * u rounds up to A)
      }
    }
  });
  if (bad_unif.load() == 1) throw InputError{"dada2hip: a bootstrap uniform lies outside [0, 1)."};
  if (bad_unif.load() == 2) throw RuntimeErr{DADA2HIP_ERR_RUNTIME, "dada2hip: the bootstrap uniforms do not cover a query."};
  st[TS_CLASSIFIED] = (int64_t)Q.size();
  add_lap(st[TS_US_PREPARE], t_call);

  select_device(m->device);
  const int slab_max = std::min(std::max(knobs().tax_slab, 0), TAX_SLAB_MAX);
  std::vector<float> best;
  std::vector<int32_t> nt, win;
  std::vector<int> all(Q.size());
  for (size_t i = 0; i < Q.size(); i++) all[i] = (int)i;

  // ---- tryRC (:169-177): the full pass on either strand; the reverse complement's k-mers are used where its maximum is greater ----
  if (try_rc) {
    std::vector<float> best_rc;
    st[TS_US_ORIENT] += (int64_t)taxonomy_run(m, Q, all, false, 1, false, seed, best, nt, win, st[TS_LAUNCHES]);
    st[TS_US_ORIENT] += (int64_t)taxonomy_run(m, Q, all, true, 1, false, seed, best_rc, nt, win, st[TS_LAUNCHES]);
    for (size_t i = 0; i < Q.size(); i++)
      if (best_rc[i] > best[i]) { Q[i].ka.swap(Q[i].ka_rc); st[TS_FLIPPED]++; }
  }

  // ---- all 101 passes, by the instance the query's length asks for ----
  std::vector<int> lists[2];                                    // [1]: the slab instance
  for (size_t i = 0; i < Q.size(); i++) lists[(int)Q[i].ka.size() <= slab_max ? 1 : 0].push_back((int)i);
  st[TS_SLAB] = (int64_t)lists[1].size(); st[TS_GATHER] = (int64_t)lists[0].size();
  for (int inst = 0; inst < 2; inst++) {
    const double us = taxonomy_run(m, Q, lists[inst], false, TAX_NPASS, inst == 1, seed, best, nt, win, st[TS_LAUNCHES]);
    st[inst ? TS_US_SLAB : TS_US_GATHER] += (int64_t)us;
    for (size_t i = 0; i < lists[inst].size(); i++) {
      const int j = Q[lists[inst][i]].id;
      const int32_t *w = win.data() + i * TAX_NPASS;
      memcpy(ntie + (size_t)j * TAX_NPASS, nt.data() + i * TAX_NPASS, TAX_NPASS * sizeof(int32_t));
      tax[j] = w[0];
      const int32_t *gm = m->genusmat.data();
      for (int r = 0; r < TAX_NBOOT; r++) {
        boot_tax[(size_t)j * TAX_NBOOT + r] = w[1 + r];
        for (int l = 0; l < nlevel; l++) {                      // :189-195
          if (gm[(size_t)w[1 + r] * nlevel + l] != gm[(size_t)w[0] * nlevel + l]) break;
          boot[(size_t)j * nlevel + l]++;
        }
      }
    }
  }
  finish_stats(st, TS_US_TOTAL, t_call, stats);
}

}  // namespace

int dada2hip_taxonomy_train(int32_t nref, const char *const *refs, const int32_t *ref_to_genus, int32_t ngenus, int32_t nlevel,
                            const int32_t *genusmat, int32_t device, dada2hip_taxonomy **out, int64_t *stats, char *errbuf,
                            size_t errlen) {
  return guarded(errbuf, errlen, [&] { taxonomy_train_body(nref, refs, ref_to_genus, ngenus, nlevel, genusmat, device, out, stats); });
}

void dada2hip_taxonomy_free(dada2hip_taxonomy *m) { delete m; }

int dada2hip_taxonomy_table(const dada2hip_taxonomy *m, float *out, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (!m || !out) throw InputError{"dada2hip: bad arguments"};
    select_device(m->device);
    std::vector<float> T((size_t)TAX_NKMER * m->gpad);
    D2_HIP(hipMemcpy(T.data(), m->T.p, T.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int g = 0; g < m->ngenus; g++)
      for (int k = 0; k < TAX_NKMER; k++) out[(size_t)g * TAX_NKMER + k] = T[(size_t)k * m->gpad + g];
  });
}

int dada2hip_taxonomy_assign(const dada2hip_taxonomy *m, int32_t nseq, const char *const *seqs, int32_t try_rc, const double *unifs,
                             uint64_t seed, int32_t *tax, int32_t *boot, int32_t *boot_tax, int32_t *ntie, int64_t *stats,
                             char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] { taxonomy_assign_body(m, nseq, seqs, try_rc, unifs, seed, tax, boot, boot_tax, ntie, stats); });
}
