// collapse_host.h — host side of the sequence-table stage (R/multiSample.R:104-160 collapseNoMismatch, R/misc.R:216-225 nweval /
// nwhamming); included by driver.cpp inside its extern "C" block, behind nwvec_any and sample_create.
//
// collapseNoMismatch's pair relation - "the grepl screen passes and the optimal ends-free alignment has neither a mismatch nor
// an internal indel" - does not depend on the state of its greedy loop.  So the loop is cut into batches of queries; for a batch
// the device evaluates the relation for every (query, ref) pair with ref among the columns kept so far or earlier in the batch
// (k_collapse_join: which pairs can pass the screen at all; k_collapse_scan: the screen itself and the bound that settles most
// pairs without a DP; the pair-form lane aligner for the rest, collapse.inc.hip), and the host replays the reference's choice
// from the bulk results: each query joins the FIRST kept column, in kept order, whose pair holds.
// From stage_common.h: require_acgt, the prefix keys and their groups (build_prefix_keys), the clocks and the end of a call.
#pragma once
#include <string_view>
#include <unordered_map>

#include "evalpair.h"

namespace {

// match / mismatch / indel of C_eval_pair on the alignment of every pair; calls of at most 65 536 pairs, as merge.cpp's
void nweval_pairs(size_t n, const char *const *s1, const char *const *s2, int match, int mismatch, int gap_p, int homo_gap_p, int band,
                  int endsfree, bool vec, int device, int32_t *out3) {
  const size_t CH = 65536;
  std::vector<std::vector<char>> bufs;
  std::vector<char *> outs;
  char eb[1024];
  for (size_t p0 = 0; p0 < n; p0 += CH) {
    const size_t m = std::min(CH, n - p0);
    bufs.resize(2 * m); outs.resize(2 * m);
    for (size_t p = 0; p < m; p++) {
      const size_t cap = strlen(s1[p0 + p]) + strlen(s2[p0 + p]) + 1;
      bufs[2 * p].assign(cap, 0); bufs[2 * p + 1].assign(cap, 0);
      outs[2 * p] = bufs[2 * p].data(); outs[2 * p + 1] = bufs[2 * p + 1].data();
    }
    eb[0] = 0;
    const int rc = nwvec_any((int32_t)m, s1 + p0, s2 + p0, match, mismatch, gap_p, homo_gap_p, band, endsfree, device, outs.data(), eb,
                             sizeof eb, vec);
    if (rc != DADA2HIP_OK) throw RuntimeErr{rc, eb};
    parallel_for(m, 256, [&](size_t lo, size_t hi) {
      for (size_t p = lo; p < hi; p++) {
        int32_t *o = out3 + 3 * (p0 + p);
        eval_pair(std::string(outs[2 * p]), std::string(outs[2 * p + 1]), o[0], o[1], o[2]);
      }
    });
  }
}

// {screen, G, m_max, decision} of the (x, y) row pairs of a resident sample, in launches of at most 2^22 pairs
void collapse_scan_pairs(dada2hip_sample *s, const std::vector<int2> &pairs, int min_overlap, int match, int mismatch, bool use_bound,
                         std::vector<int4> &out) {
  out.resize(pairs.size());
  const size_t CH = (size_t)1 << 22;
  DevBuf<int2> d_pairs;
  DevBuf<int4> d_out;
  for (size_t p0 = 0; p0 < pairs.size(); p0 += CH) {
    const size_t m = std::min(CH, pairs.size() - p0);
    d_pairs.alloc(m); d_out.alloc(m);
    D2_HIP(hipMemcpyAsync(d_pairs.p, pairs.data() + p0, m * sizeof(int2), hipMemcpyHostToDevice, s->stream));
    launch_collapse_scan(s->D, d_pairs.p, (int)m, min_overlap, match, mismatch, use_bound ? 1 : 0, d_out.p, s->stream);
    D2_HIP(hipMemcpyAsync(out.data() + p0, d_out.p, m * sizeof(int4), hipMemcpyDeviceToHost, s->stream));
    sync_checked(s->stream);
  }
}

void collapse_body(int32_t nrow, int32_t ncol, const int32_t *mat, const char *const *seqs, int32_t min_overlap, int32_t identical_only,
                   int32_t band, int32_t match, int32_t mismatch, int32_t gap_p, int32_t device, int32_t *into, int64_t *stats) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_COLLAPSE_NSTATS] = {0};
  auto finish = [&] { finish_stats(st, CS_US_TOTAL, t_call, stats); };
  if (nrow < 0 || ncol < 0 || (ncol > 0 && (!seqs || !into || (nrow > 0 && !mat)))) throw InputError{"dada2hip: bad sequence table"};
  if (min_overlap < 1) throw InputError{"dada2hip: minOverlap must be at least 1."};
  if (ncol == 0) { finish(); return; }
  for (int i = 0; i < ncol; i++) if (!seqs[i]) throw InputError{"dada2hip: bad sequence table"};
  const char *too_big = "dada2hip: a column total or a collapsed cell of the sequence table exceeds the integer range (NA in the reference).";

  // ---- duplicate column names are folded into their first occurrence (multiSample.R:105-114) ----
  std::vector<int32_t> rep;                    // the input column of every distinct name, in input order
  std::vector<int32_t> uniq_of(ncol);
  {
    std::unordered_map<std::string_view, int32_t> first;
    first.reserve((size_t)ncol * 2);
    for (int i = 0; i < ncol; i++) {
      auto it = first.find(std::string_view(seqs[i]));
      if (it == first.end()) { first.emplace(std::string_view(seqs[i]), (int32_t)rep.size()); uniq_of[i] = (int32_t)rep.size(); rep.push_back(i); }
      else uniq_of[i] = it->second;
    }
  }
  const int nU = (int)rep.size();
  st[CS_NDEDUP] = nU;
  std::vector<int64_t> cell((size_t)nU * (size_t)nrow, 0);     // the de-duplicated table, column-major
  for (int i = 0; i < ncol; i++)
    for (int r = 0; r < nrow; r++) cell[(size_t)uniq_of[i] * nrow + r] += mat[(size_t)i * nrow + r];
  for (int64_t v : cell) if (v > INT32_MAX) throw InputError{too_big};
  std::vector<int32_t> dest(nU);               // per distinct name: the distinct name it ends up in
  for (int u = 0; u < nU; u++) dest[u] = u;
  auto write_into = [&] { for (int i = 0; i < ncol; i++) into[i] = rep[dest[uniq_of[i]]]; };
  if (identical_only || nU == 1) { write_into(); finish(); return; }

  // ---- sort(getUniques(seqtab), decreasing = TRUE): by total abundance, ties in table order (:118) ----
  std::vector<int64_t> total(nU, 0);
  for (int u = 0; u < nU; u++) {
    for (int r = 0; r < nrow; r++) total[u] += cell[(size_t)u * nrow + r];
    if (total[u] > INT32_MAX) throw InputError{too_big};
  }
  std::vector<int32_t> ord(nU);                // sorted position -> distinct name
  for (int u = 0; u < nU; u++) ord[u] = u;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return total[a] > total[b]; });
  std::vector<const char *> sq(nU);            // the sequences in query order: row p of the resident sample
  for (int p = 0; p < nU; p++) sq[p] = seqs[rep[ord[p]]];
  require_acgt(nU, sq.data(), "collapseNoMismatch");

  select_device(device);
  const Knobs &K = knobs();
  const bool use_join = K.collapse_join != 0, use_bound = K.collapse_scan != 0 && band < 0 && match > 0;
  // a batch costs one aligner call (a throw-away resident sample: tens of milliseconds whatever it aligns) and spends a scan -
  // and, where the bound does not decide, an alignment - on every earlier member of the batch that turns out to have collapsed
  const int batch = K.collapse_batch > 0 ? K.collapse_batch : 4096;
  std::vector<int32_t> ab(nU, 1);
  dada2hip_sample *s = new dada2hip_sample();
  std::unique_ptr<dada2hip_sample, void (*)(dada2hip_sample *)> guard(s, dada2hip_sample_free);
  sample_create(s, nU, sq.data(), ab.data(), nullptr, nullptr, 0, device, /*lite=*/true);

  // ---- the join: which distinct prefix keys occur in which sequence ----
  // key of a sequence = its first min(minOverlap, length, 32) bases as a 64-bit word (base k in bits 2k..2k+1) and that length.
  // substr(q, 1, minOverlap) can occur in r only if key(q) does: (q, r) is a candidate iff key(q) occurs in r or key(r) in q.
  auto t0 = clk::now();
  std::vector<std::vector<int32_t>> keys_in, with_key, of_key;   // keys in sequence p; sequences with key k in them; with key k as theirs
  PrefixKeyTable PK;
  const std::vector<int32_t> &key_of = PK.key_of;
  if (use_join) {
    std::vector<PrefixKey> kp(nU);
    for (int p = 0; p < nU; p++) kp[p] = prefix_key(s->h_seq2.p + (size_t)p * s->D.W2, std::min({(int)min_overlap, s->h_len[p], 32}));
    build_prefix_keys(kp, PK);
    const int nK = (int)PK.keys.size(), KW = (nK + 31) / 32;
    of_key.resize(nK); with_key.resize(nK); keys_in.resize(nU);
    for (int p = 0; p < nU; p++) of_key[key_of[p]].push_back(p);
    DevBuf<unsigned long long> d_keys;
    DevBuf<int32_t> d_groups;
    DevBuf<uint32_t> d_bits;
    d_keys.alloc(nK); d_groups.alloc(PK.groups.size());
    D2_HIP(hipMemcpyAsync(d_keys.p, PK.keys.data(), (size_t)nK * 8, hipMemcpyHostToDevice, s->stream));
    D2_HIP(hipMemcpyAsync(d_groups.p, PK.groups.data(), PK.groups.size() * 4, hipMemcpyHostToDevice, s->stream));
    // the bit matrix in blocks of rows of at most 256 MB
    const size_t rows_per = std::max<size_t>(1, ((size_t)256 << 20) / ((size_t)KW * 4));
    std::vector<uint32_t> h_bits;
    for (size_t r0 = 0; r0 < (size_t)nU; r0 += rows_per) {
      const size_t nr = std::min(rows_per, (size_t)nU - r0);
      d_bits.alloc(nr * KW); h_bits.resize(nr * KW);
      D2_HIP(hipMemsetAsync(d_bits.p, 0, nr * KW * 4, s->stream));
      launch_collapse_join(s->D, (int)r0, (int)nr, d_keys.p, d_groups.p, (int)PK.groups.size() / 3, KW, d_bits.p, s->stream);
      D2_HIP(hipMemcpyAsync(h_bits.data(), d_bits.p, nr * KW * 4, hipMemcpyDeviceToHost, s->stream));
      sync_checked(s->stream);
      for (size_t r = 0; r < nr; r++)
        for (int w = 0; w < KW; w++)
          for (uint32_t b = h_bits[r * KW + w]; b; b &= b - 1) {
            const int k = 32 * w + __builtin_ctz(b);
            keys_in[r0 + r].push_back(k);
            with_key[k].push_back((int32_t)(r0 + r));
          }
    }
  }
  add_lap(st[CS_US_JOIN], t0);

  // ---- the greedy loop (:125-144), a batch of queries at a time ----
  enum : uint8_t { OPEN = 0, KEPT = 1, GONE = 2 };
  std::vector<uint8_t> state(nU, OPEN);
  std::vector<int32_t> joined(nU, -1);         // sorted position of the column a collapsed query was added to
  std::vector<int2> pairs;
  std::vector<int4> scan;
  std::vector<int32_t> cand, ev;
  std::vector<uint8_t> holds;
  std::vector<const char *> a1, a2;
  for (int b0 = 0; b0 < nU; b0 += batch) {
    const int b1 = std::min(nU, b0 + batch);
    st[CS_BATCHES]++;
    pairs.clear();
    for (int q = b0; q < b1; q++) {            // candidates: (q, r), r kept before the batch or earlier in it, ascending r = kept order
      auto ok = [&](int r) { return r < q && (r >= b0 || state[r] == KEPT); };
      if (!use_join) {
        for (int r = 0; r < q; r++) if (ok(r)) pairs.push_back(make_int2(q, r));
        continue;
      }
      cand.clear();
      for (int k : keys_in[q]) for (int r : of_key[k]) { if (r >= q) break; if (ok(r)) cand.push_back(r); }
      for (int r : with_key[key_of[q]]) { if (r >= q) break; if (ok(r)) cand.push_back(r); }
      std::sort(cand.begin(), cand.end());
      cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
      for (int r : cand) pairs.push_back(make_int2(q, r));
    }
    st[CS_CAND] += (int64_t)pairs.size();
    t0 = clk::now();
    collapse_scan_pairs(s, pairs, min_overlap, match, mismatch, use_bound, scan);
    add_lap(st[CS_US_SCAN], t0);
    st[CS_SCANNED] += (int64_t)pairs.size();
    holds.assign(pairs.size(), 0);
    a1.clear(); a2.clear();
    std::vector<size_t> where;
    for (size_t i = 0; i < pairs.size(); i++) {
      const int dec = scan[i].w;
      if (dec == 0) st[CS_SCREENED_OUT]++;
      else if (dec == 1) st[CS_BOUND]++;
      else { where.push_back(i); a1.push_back(sq[pairs[i].x]); a2.push_back(sq[pairs[i].y]); }
    }
    t0 = clk::now();
    if (!where.empty()) {
      ev.resize(3 * where.size());
      nweval_pairs(where.size(), a1.data(), a2.data(), match, mismatch, gap_p, gap_p, band, /*endsfree=*/1, /*vec=*/true, device, ev.data());
      for (size_t t = 0; t < where.size(); t++)
        if (ev[3 * t + 1] + ev[3 * t + 2] == 0) { holds[where[t]] = 1; st[CS_HAM0]++; }
      st[CS_ALIGNED] += (int64_t)where.size();
    }
    add_lap(st[CS_US_ALIGN], t0);
    t0 = clk::now();
    size_t i = 0;
    for (int q = b0; q < b1; q++) {            // the batch in order: a member that collapsed is no ref for the ones behind it
      state[q] = KEPT;
      for (; i < pairs.size() && pairs[i].x == q; i++)
        if (state[q] == KEPT && holds[i] && state[pairs[i].y] == KEPT) { state[q] = GONE; joined[q] = pairs[i].y; }
    }
    add_lap(st[CS_US_RESOLVE], t0);
  }
  for (int p = 0; p < nU; p++) if (joined[p] >= 0) dest[ord[p]] = ord[joined[p]];
  // collapsed[, ref] + seqtab[, query] is integer arithmetic in the reference: NA past INT32_MAX
  {
    std::vector<int64_t> sum((size_t)nU * (size_t)nrow, 0);
    for (int u = 0; u < nU; u++)
      for (int r = 0; r < nrow; r++) {
        int64_t &v = sum[(size_t)dest[u] * nrow + r];
        v += cell[(size_t)u * nrow + r];
        if (v > INT32_MAX) throw InputError{too_big};
      }
  }
  write_into();
  finish();
}

}  // namespace

int dada2hip_collapse_nomismatch(int32_t nrow, int32_t ncol, const int32_t *mat, const char *const *seqs, int32_t min_overlap,
                                 int32_t identical_only, int32_t band, int32_t match, int32_t mismatch, int32_t gap_p,
                                 int32_t device, int32_t *into, int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    collapse_body(nrow, ncol, mat, seqs, min_overlap, identical_only, band, match, mismatch, gap_p, device, into, stats);
  });
}

int dada2hip_collapse_pairs(int32_t n, const char *const *queries, const char *const *refs, int32_t min_overlap, int32_t match,
                            int32_t mismatch, int32_t device, int32_t *out, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (n < 0 || (n > 0 && (!queries || !refs || !out))) throw InputError{"dada2hip: bad arguments"};
    if (min_overlap < 1) throw InputError{"dada2hip: minOverlap must be at least 1."};
    if (n == 0) return;
    require_acgt(n, queries, "collapseNoMismatch");
    require_acgt(n, refs, "collapseNoMismatch");
    select_device(device);
    std::vector<const char *> sq(2 * (size_t)n);
    std::vector<int2> pairs(n);
    for (int i = 0; i < n; i++) { sq[2 * i] = queries[i]; sq[2 * i + 1] = refs[i]; pairs[i] = make_int2(2 * i, 2 * i + 1); }
    std::vector<int32_t> ab(sq.size(), 1);
    dada2hip_sample *s = new dada2hip_sample();
    std::unique_ptr<dada2hip_sample, void (*)(dada2hip_sample *)> guard(s, dada2hip_sample_free);
    sample_create(s, (int32_t)sq.size(), sq.data(), ab.data(), nullptr, nullptr, 0, device, /*lite=*/true);
    std::vector<int4> scan;
    collapse_scan_pairs(s, pairs, min_overlap, match, mismatch, /*use_bound=*/true, scan);
    memcpy(out, scan.data(), (size_t)n * sizeof(int4));
  });
}

int dada2hip_nweval(int32_t n, const char *const *s1, const char *const *s2, int32_t match, int32_t mismatch, int32_t gap_p,
                    int32_t homo_gap_p, int32_t band, int32_t endsfree, int32_t vec, int32_t device, int32_t *out, char *errbuf,
                    size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (n < 0 || (n > 0 && (!s1 || !s2 || !out))) throw InputError{"dada2hip: bad arguments"};
    for (int i = 0; i < n; i++) if (!s1[i] || !s2[i]) throw InputError{"dada2hip: bad arguments"};
    if (vec && homo_gap_p != gap_p) throw InputError{"Homopolymer gap penalties are not implemented in the vectorized aligner."};   // misc.R:183
    if (n == 0) return;
    nweval_pairs((size_t)n, s1, s2, match, mismatch, gap_p, homo_gap_p, band, endsfree, vec != 0, device, out);
  });
}
