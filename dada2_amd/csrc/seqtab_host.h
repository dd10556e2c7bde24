// seqtab_host.h — host side of mergeSequenceTables (seqtab.inc.hip; R/multiSample.R:290-364, validation :206-238); included by
// driver.cpp inside its extern "C" block, behind derep_dev_host.h, on top of stage_common.h and seqtab_plain.h.
//
// The column names of all tables are the "reads" of one DerepDev without qualities (dd_feed through read_pieces.h's two slots):
// a read's index is its running column number, so a unique's smallest index is the sequence's first appearance and a read's
// unique is match().  With tryRC k_st_rc looks every unique's reverse complement up in that table; the flags, the rank of the
// unflagged uniques by first appearance and the row map of the sample names are seqtab_plain.h's.  Then the tables go up one
// after the other and k_st_accumulate adds their cells into the zeroed merged matrix; k_st_colkeys gives the host the sums and
// counts it orders the columns by, k_st_gather writes the matrix in that order, and one copy brings it back.
#pragma once

struct dada2hip_seqtab {
  int32_t nrow = 0, ncol = 0;
  int32_t *cells = nullptr;                    // row-major [nrow x ncol]
  std::string seq_bytes, sam_bytes;
  std::vector<int64_t> seq_off, sam_off;
  ~dada2hip_seqtab() { free(cells); }
};

namespace {

struct StStream {
  hipStream_t s = nullptr;
  void create() { D2_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~StStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};

// the table and the 1-based place inside it of running name c
void st_locate(int32_t ntab, const int32_t *per_table, int64_t c, int32_t &table, int64_t &at) {
  table = 0;
  while (table + 1 < ntab && c >= per_table[table]) c -= per_table[table++];
  at = c + 1;
}

void seqtab_merge_body(int32_t ntab, const int32_t *nrow, const int32_t *ncol, const int32_t *const *cells, const char *col_bytes,
                       const int64_t *col_offsets, const char *row_bytes, const int64_t *row_offsets, int32_t repeats_sum, int32_t order_by,
                       int32_t try_rc, int32_t device, dada2hip_seqtab **out, int32_t *col_map, int64_t *stats) {
  const auto t_call = clk::now();
  int64_t st[DADA2HIP_SEQTAB_NSTATS] = {0};
  if (!out) throw InputError{"dada2hip: bad arguments"};
  *out = nullptr;
  // ---- is.sequence.table (:206-238) and the deviations include/dada2hip.h states ----
  if (ntab < 2) throw InputError{"At least two sequence tables are expected"};
  if (!nrow || !ncol || !cells || !col_bytes || !col_offsets || !row_bytes || !row_offsets) throw InputError{"dada2hip: bad arguments"};
  if (order_by < 0 || order_by > 2) throw InputError{"dada2hip: order_by must be 0 (none), 1 (abundance) or 2 (nsamples)."};
  int64_t ncols = 0, nrows = 0;
  size_t largest = 0;
  for (int32_t t = 0; t < ntab; t++) {
    if (nrow[t] <= 0 || ncol[t] <= 0)
      throw InputError{"dada2hip: sequence table " + std::to_string(t + 1) + " is empty (no rows or no columns)."};
    if (!cells[t]) throw InputError{"dada2hip: bad arguments"};
    ncols += ncol[t]; nrows += nrow[t];
    largest = std::max(largest, (size_t)nrow[t] * (size_t)ncol[t]);
  }
  if (ncols > (int64_t)INT32_MAX || nrows > (int64_t)INT32_MAX) throw InputError{"dada2hip: more than 2^31 - 1 columns or rows to merge."};
  StNames cn, rn;
  cn.n = ncols; cn.bytes = col_bytes; cn.off = col_offsets;
  rn.n = nrows; rn.bytes = row_bytes; rn.off = row_offsets;
  auto blank = [&](const StNames &N, const int32_t *per_table, const char *what) {
    for (int64_t i = 0; i < N.n; i++)
      if (N.off[i + 1] <= N.off[i]) {
        if (N.off[i + 1] < N.off[i]) throw InputError{"dada2hip: bad name offsets."};
        int32_t t; int64_t at;
        st_locate(ntab, per_table, i, t, at);
        throw InputError{std::string("Some ") + what + " names are blank (sequence table " + std::to_string(t + 1) + ")."};
      }
  };
  blank(cn, ncol, "column (sequence)");
  blank(rn, nrow, "row (sample)");
  for (int32_t t = 0; t < ntab; t++) {
    std::atomic<int> neg{0};
    const int32_t *c = cells[t];
    parallel_for((size_t)nrow[t] * (size_t)ncol[t], (size_t)1 << 20, [&](size_t lo, size_t hi) {
      int32_t m = 0;
      for (size_t i = lo; i < hi; i++) m |= c[i];
      if (m < 0) neg.store(1);
    });
    if (neg.load()) throw InputError{"Negative entries (sequence table " + std::to_string(t + 1) + ")."};
  }
  StRows R;
  if (!st_row_map(ntab, nrow, rn, R))
    throw InputError{"Duplicated row (sample) names in sequence table " + std::to_string(R.dup_table + 1) + ": " + st_show(rn[R.dup_row])};
  if (!R.repeated.empty() && !repeats_sum) {
    std::string m = "Duplicated sample names detected in the sequence table row names: ";
    for (size_t i = 0; i < R.repeated.size(); i++) { if (i) m += ", "; m += std::string(rn[R.repeated[i]]); }
    throw InputError{m};
  }
  const int64_t NR = (int64_t)R.first.size();

  // ---- identity: unique(c(sapply(tables, colnames))) (:332) ----
  auto t0 = clk::now();
  DerepDev D;
  dd_open(D, device, 0, 33);
  D.no_qual = true;
  dd_feed(D, ncols, col_bytes, nullptr, col_offsets, nullptr, nullptr);
  const int64_t U = D.nuniq;
  if (U <= 0 || (int64_t)D.ruid.size() != ncols) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator lost a column name."};
  for (int32_t u : D.ruid) if (u < 0 || u >= U) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator lost a column name."};
  StStream S;
  S.create();
  std::vector<uint64_t> first((size_t)U);
  D2_HIP(hipMemcpyAsync(first.data(), D.u_first.p, (size_t)U * 8, hipMemcpyDeviceToHost, S.s));
  sync_checked(S.s);
  for (uint64_t f : first) if (f >= (uint64_t)ncols) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator lost a first appearance."};
  st[SM_BYTES_DOWN] += D.st[DD_BYTES_DOWN] + U * 8;
  const int64_t dup = st_dup_column(ntab, ncol, D.ruid.data(), U);
  if (dup >= 0) {
    int32_t t; int64_t at;
    st_locate(ntab, ncol, dup, t, at);
    throw InputError{"Duplicated column (sequences) names in sequence table " + std::to_string(t + 1) + ": column " + std::to_string(at) + ", " +
                     st_show(cn[dup])};
  }
  add_lap(st[SM_US_IDENTITY], t0);                               // (the names' way up included: a piece is dereplicated under its upload's clock)
  st[SM_BYTES_UP] += D.st[DD_BYTES_UP];

  // ---- tryRC (:333-347): the partners from the device ----
  DevBuf<StCounters> d_ctr;
  d_ctr.alloc(1);
  StCounters h_ctr;
  h_ctr.bad_first = ~0ull; h_ctr.rc_fails = 0; h_ctr.err = 0; h_ctr.pad = 0;
  D2_HIP(hipMemcpyAsync(d_ctr.p, &h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, S.s));
  sync_checked(S.s);
  std::vector<int32_t> partner;
  if (try_rc && U > 1) {
    t0 = clk::now();
    uint8_t comp[256];
    st_comp_table(comp);
    DevBuf<uint8_t> d_comp;
    DevBuf<int32_t> d_partner;
    d_comp.alloc(256); d_partner.alloc((size_t)U);
    partner.resize((size_t)U);
    D2_HIP(hipMemcpyAsync(d_comp.p, comp, 256, hipMemcpyHostToDevice, S.s));
    launch_st_rc(D.state(), (int)U, d_comp.p, d_partner.p, d_ctr.p, S.s);
    D2_HIP(hipMemcpyAsync(partner.data(), d_partner.p, (size_t)U * 4, hipMemcpyDeviceToHost, S.s));
    D2_HIP(hipMemcpyAsync(&h_ctr, d_ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, S.s));
    sync_checked(S.s);
    st[SM_BYTES_UP] += 256; st[SM_BYTES_DOWN] += U * 4 + (int64_t)sizeof h_ctr;
    if (h_ctr.err & ST_ERR_LETTER) {
      if (h_ctr.bad_first >= (uint64_t)ncols) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: a letter was refused in no column."};
      int32_t t; int64_t at;
      st_locate(ntab, ncol, (int64_t)h_ctr.bad_first, t, at);
      throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: mergeSequenceTables with tryRC takes the upper-case letters ACGTMRWSYKVHDBN only: table " +
                                                     std::to_string(t + 1) + ", column " + std::to_string(at) + " (" +
                                                     st_show(cn[(int64_t)h_ctr.bad_first]) + ")."};
    }
    if (h_ctr.err & ST_ERR_WALK) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the reverse complement's table walk reached its bound."};
    for (int32_t p : partner) if (p < -1 || p >= U) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the reverse complement's lookup named no unique."};
    st[SM_RC_FAILS] = (int64_t)h_ctr.rc_fails;
    add_lap(st[SM_US_RC], t0);
  }
  t0 = clk::now();
  StCols P;
  st_plan_columns(U, first.data(), partner.empty() ? nullptr : partner.data(), ncols, D.ruid.data(), P);
  const int64_t NC = (int64_t)P.kept.size();
  add_lap(st[SM_US_IDENTITY], t0);

  // ---- the merged matrix (:349-354), the column keys and the order (:356-362) ----
  const size_t ncell = (size_t)NR * (size_t)NC;
  {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 0; int dv = 0; (void)hipGetDevice(&dv); (void)hipDeviceTotalMem(&fr, dv); }
    const double need = 2.0 * 4.0 * (double)ncell + 4.0 * (double)largest;
    if (need > (double)fr / 2.0)
      throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: the merged table of " + std::to_string(NR) + " x " + std::to_string(NC) + " cells needs " +
                                                     std::to_string((long long)(need / 1048576.0)) + " MiB on the device, more than half of the " +
                                                     std::to_string((long long)(fr >> 20)) + " MiB that are free."};
  }
  std::unique_ptr<dada2hip_seqtab> H(new dada2hip_seqtab());
  H->cells = (int32_t *)malloc(std::max<size_t>(ncell, 1) * 4);
  if (!H->cells) throw RuntimeErr{DADA2HIP_ERR_RUNTIME, "dada2hip: out of memory for the merged table."};
  DevBuf<int32_t> d_merged, d_final, d_cells, d_row_map, d_col_map, d_order, d_npos;
  DevBuf<unsigned long long> d_sum;
  t0 = clk::now();
  d_merged.alloc(ncell); d_cells.alloc(largest); d_row_map.alloc((size_t)nrows); d_col_map.alloc((size_t)ncols);
  D2_HIP(hipMemsetAsync(d_merged.p, 0, ncell * 4, S.s));
  D2_HIP(hipMemcpyAsync(d_row_map.p, R.row_map.data(), (size_t)nrows * 4, hipMemcpyHostToDevice, S.s));
  D2_HIP(hipMemcpyAsync(d_col_map.p, P.col_map.data(), (size_t)ncols * 4, hipMemcpyHostToDevice, S.s));
  sync_checked(S.s);
  st[SM_BYTES_UP] += (nrows + ncols) * 4;
  add_lap(st[SM_US_UP], t0);
  int64_t r0 = 0, c0 = 0;
  for (int32_t t = 0; t < ntab; t++) {                           // one table at a time: its upload, then its adds
    t0 = clk::now();
    const size_t n = (size_t)nrow[t] * (size_t)ncol[t];
    D2_HIP(hipMemcpyAsync(d_cells.p, cells[t], n * 4, hipMemcpyHostToDevice, S.s));
    sync_checked(S.s);
    st[SM_BYTES_UP] += (int64_t)n * 4;
    add_lap(st[SM_US_UP], t0);
    t0 = clk::now();
    launch_st_accumulate(d_cells.p, nrow[t], ncol[t], d_row_map.p + r0, d_col_map.p + c0, d_merged.p, NC, d_ctr.p, S.s);
    sync_checked(S.s);                                           // (the next table's upload overwrites d_cells)
    add_lap(st[SM_US_ACCUM], t0);
    r0 += nrow[t]; c0 += ncol[t];
  }
  t0 = clk::now();
  D2_HIP(hipMemcpyAsync(&h_ctr, d_ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, S.s));
  sync_checked(S.s);
  if (h_ctr.err & ST_ERR_OVERFLOW)
    throw InputError{"dada2hip: a merged cell of the sequence tables exceeds the integer range (NA in the reference)."};
  std::vector<int32_t> order;
  bool identity = true;
  if (order_by != 0) {
    std::vector<uint64_t> sum((size_t)NC);
    std::vector<int32_t> npos((size_t)NC);
    d_sum.alloc((size_t)NC); d_npos.alloc((size_t)NC);
    D2_HIP(hipMemsetAsync(d_sum.p, 0, (size_t)NC * 8, S.s));
    D2_HIP(hipMemsetAsync(d_npos.p, 0, (size_t)NC * 4, S.s));
    launch_st_colkeys(d_merged.p, NR, NC, d_sum.p, d_npos.p, S.s);
    D2_HIP(hipMemcpyAsync(sum.data(), d_sum.p, (size_t)NC * 8, hipMemcpyDeviceToHost, S.s));
    D2_HIP(hipMemcpyAsync(npos.data(), d_npos.p, (size_t)NC * 4, hipMemcpyDeviceToHost, S.s));
    sync_checked(S.s);
    st[SM_BYTES_DOWN] += NC * 12;
    identity = st_order(NC, sum.data(), npos.data(), order_by, order);
    if (!identity) {
      d_order.alloc((size_t)NC); d_final.alloc(ncell);
      D2_HIP(hipMemcpyAsync(d_order.p, order.data(), (size_t)NC * 4, hipMemcpyHostToDevice, S.s));
      launch_st_gather(d_merged.p, NR, NC, d_order.p, d_final.p, S.s);
      sync_checked(S.s);
      st[SM_BYTES_UP] += NC * 4;
    }
  } else {
    st_order(NC, nullptr, nullptr, 0, order);
  }
  add_lap(st[SM_US_ACCUM], t0);
  t0 = clk::now();
  D2_HIP(hipMemcpyAsync(H->cells, identity ? d_merged.p : d_final.p, ncell * 4, hipMemcpyDeviceToHost, S.s));
  sync_checked(S.s);
  st[SM_BYTES_DOWN] += (int64_t)ncell * 4;
  add_lap(st[SM_US_DOWN], t0);

  // ---- the names of the result, and where every input column went ----
  H->nrow = (int32_t)NR; H->ncol = (int32_t)NC;
  H->seq_off.assign(1, 0); H->sam_off.assign(1, 0);
  for (int64_t k = 0; k < NC; k++) {
    const std::string_view s = cn[(int64_t)first[(size_t)P.kept[(size_t)order[(size_t)k]]]];
    H->seq_bytes.append(s.data(), s.size());
    H->seq_off.push_back((int64_t)H->seq_bytes.size());
  }
  for (int64_t r = 0; r < NR; r++) {
    const std::string_view s = rn[R.first[(size_t)r]];
    H->sam_bytes.append(s.data(), s.size());
    H->sam_off.push_back((int64_t)H->sam_bytes.size());
  }
  if (col_map) {
    std::vector<int32_t> place((size_t)NC);
    for (int64_t k = 0; k < NC; k++) place[(size_t)order[(size_t)k]] = (int32_t)k;
    for (int64_t c = 0; c < ncols; c++) col_map[c] = place[(size_t)P.col_map[(size_t)c]];
  }
  st[SM_TABLES] = ntab; st[SM_COLS_IN] = ncols; st[SM_DISTINCT] = U; st[SM_FLAGGED] = P.nflag; st[SM_ROWS] = NR; st[SM_COLS] = NC;
  st[SM_CAPACITY] = (int64_t)D.cap; st[SM_REBUILDS] = D.st[DD_REBUILDS]; st[SM_ROUNDS] = D.st[DD_ROUNDS]; st[SM_PIECES] = D.st[DD_PIECES];
  finish_stats(st, SM_US_TOTAL, t_call, stats);
  *out = H.release();
}

}  // namespace

int dada2hip_seqtab_merge(int32_t ntab, const int32_t *nrow, const int32_t *ncol, const int32_t *const *cells, const char *col_bytes,
                          const int64_t *col_offsets, const char *row_bytes, const int64_t *row_offsets, int32_t repeats_sum,
                          int32_t order_by, int32_t try_rc, int32_t device, dada2hip_seqtab **out, int32_t *col_map, int64_t *stats,
                          char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    seqtab_merge_body(ntab, nrow, ncol, cells, col_bytes, col_offsets, row_bytes, row_offsets, repeats_sum, order_by, try_rc, device, out,
                      col_map, stats);
  });
}

int32_t dada2hip_seqtab_nrow(const dada2hip_seqtab *t) { return t ? t->nrow : 0; }
int32_t dada2hip_seqtab_ncol(const dada2hip_seqtab *t) { return t ? t->ncol : 0; }
const int32_t *dada2hip_seqtab_cells(const dada2hip_seqtab *t) { return t ? t->cells : nullptr; }
const char *dada2hip_seqtab_sequences(const dada2hip_seqtab *t, const int64_t **offsets) {
  if (offsets) *offsets = t ? t->seq_off.data() : nullptr;
  return t ? t->seq_bytes.data() : nullptr;
}
const char *dada2hip_seqtab_samples(const dada2hip_seqtab *t, const int64_t **offsets) {
  if (offsets) *offsets = t ? t->sam_off.data() : nullptr;
  return t ? t->sam_bytes.data() : nullptr;
}
void dada2hip_seqtab_free(dada2hip_seqtab *t) { delete t; }
