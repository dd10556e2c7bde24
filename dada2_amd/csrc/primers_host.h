// primers_host.h — host side of removePrimers' per-read verdicts (R/filter.R:81-233); included by driver.cpp inside its extern "C"
// block, behind filter_host.h.  The file-level entry (dada2hip_primers_fastq) is derep.cpp's, where the FASTQ reader and writer
// are; it calls dada2hip_primers_reads per chunk.
//
// The call turns the primers into the four patterns of primers.inc.hip (the forward primer, the reverse primer, the reverse
// complement of each), every letter a byte of plane selectors: the letter's IUPAC set for a primer with a letter beyond A/C/G/T
// (fixed = FALSE, :111-112), the "is exactly this base" plane for a primer of A/C/G/T only.  Both rules are symmetric under
// complement, so the reverse complement of a pattern is matched by the same rule and the read is never reverse-complemented.
// The reads go up as dada2hip_filter_reads' do - pieces of at most PR_PIECE_READS reads / PR_PIECE_BYTES bytes
// (DADA2HIP_PRIMERS_PIECE, DADA2HIP_PRIMERS_PIECE_BYTES: fewer, for the tests), two slots with pinned staging, device buffers and
// a stream each, the copy of piece k + 1 under the kernel of piece k - but only the sequence bytes and the offsets; 32 bytes per
// read come back, and 32 more when the starts are asked for.
#pragma once

namespace {

constexpr int64_t PR_PIECE_READS = 1 << 16;
constexpr int64_t PR_PIECE_BYTES = 32 << 20;

enum { PS_IN = 0, PS_KEPT, PS_CODE1, PS_FLIPPED = 6, PS_MULTI, PS_HITS_FWD, PS_HITS_REV, PS_PIECES, PS_TILES, PS_BYTES, PS_US_UP, PS_US_KERNEL,
       PS_US_DOWN, PS_US_PARSE, PS_US_DEFLATE, PS_US_WRITE, PS_US_TOTAL };

struct PrSlot {
  PinBuf<uint8_t> h_seq;
  PinBuf<long long> h_off;
  PinBuf<PrimerOut> h_out;
  PinBuf<int32_t> h_starts;
  DevBuf<uint8_t> d_seq;
  DevBuf<long long> d_off;
  DevBuf<PrimerOut> d_out;
  DevBuf<int32_t> d_starts;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  int64_t first = 0, count = 0;
  bool busy = false;
  ~PrSlot() {
    if (busy && st) (void)hipStreamSynchronize(st);
    for (int i = 0; i < 2; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (st) (void)hipStreamDestroy(st);
  }
};

// the IUPAC set of a letter over A C G T = 1 2 4 8 (Biostrings' IUPAC_CODE_MAP); 0 for anything else
inline int pr_iupac(char c) {
  static const char *codes = "ACMGRSVTWYHKDBN";                 // the letter of set 1, 2, ... 15
  const char *p = c ? strchr(codes, c) : nullptr;
  return p ? (int)(p - codes) + 1 : 0;
}
inline char pr_complement(char c) {                             // A<->T C<->G: a set's bits in reverse order
  const int m = pr_iupac(c), r = ((m & 1) << 3) | ((m & 2) << 1) | ((m & 4) >> 1) | ((m & 8) >> 3);
  return "ACMGRSVTWYHKDBN"[r - 1];
}

void primer_args(const dada2hip_primer_params *P, PrimerArgs &A) {
  if (!P) throw InputError{"dada2hip: bad arguments"};
  if (P->allow_indels) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: allow.indels = TRUE is not supported (primers are matched without indels)."};
  if (!P->primer_fwd) throw InputError{"Primer sequences must be provided as base R strings."};   // :104
  if (P->max_mismatch < 0) throw InputError{"dada2hip: max.mismatch must not be negative."};
  if (P->max_mismatch > PR_MAXMM) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: max.mismatch above 15 is not supported."};
  memset(&A, 0, sizeof A);
  const char *prim[2] = {P->primer_fwd, P->primer_rev};
  for (int k = 0; k < 2; k++) {
    if (!prim[k]) continue;
    const size_t L = strlen(prim[k]);
    if (L == 0) throw InputError{"dada2hip: a primer must have at least one letter."};
    if (L > (size_t)PR_MAXL) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: a primer of more than 128 letters is not supported."};
    if ((size_t)P->max_mismatch >= L) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: max.mismatch must be below the primer's length."};
    bool fixed = true;                                          // C_isACGT, :111-112
    for (size_t i = 0; i < L; i++) {
      const int m = pr_iupac(prim[k][i]);
      if (m == 0) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: a primer may hold the upper-case IUPAC codes ACGTMRWSYKVHDBN only."};
      if (m != 1 && m != 2 && m != 4 && m != 8) fixed = false;
    }
    A.len[k] = A.len[k + 2] = (int32_t)L;
    for (size_t i = 0; i < L; i++) {
      const int m = pr_iupac(prim[k][i]), mc = pr_iupac(pr_complement(prim[k][L - 1 - i]));
      A.sel[k][i] = (uint8_t)(fixed ? m << 4 : m);
      A.sel[k + 2][i] = (uint8_t)(fixed ? mc << 4 : mc);
    }
  }
  A.has_rev = P->primer_rev ? 1 : 0; A.orient = P->orient ? 1 : 0; A.trim_fwd = P->trim_fwd ? 1 : 0; A.trim_rev = P->trim_rev ? 1 : 0;
  A.mm = P->max_mismatch;
  while ((1 << A.nbits) < A.mm + 1) A.nbits++;                  // the counter starts at 2^nbits - 1 - mm
  for (int k = 0; k < 4; k++) {
    if ((k & 1) && !A.has_rev) { A.len[k] = 0; continue; }
    if (k >= 2 && !A.orient) { A.len[k] = 0; continue; }
    A.act[A.nact++] = k;
  }
  const long long t = knobs().primers_tile;
  A.tile = t > 0 ? (int)std::min<long long>(t, PR_TILE_MAX) : PR_TILE_MAX;
}

void primers_reads_body(int64_t n, const char *seq, const int64_t *offsets, const dada2hip_primer_params *P, int32_t device,
                        int32_t *code, int32_t *flip, int32_t *first, int32_t *last, int32_t *hits, int32_t *starts, int64_t *stats) {
  auto t_call = clk::now();
  int64_t st[DADA2HIP_PRIMERS_NSTATS] = {0};
  PrimerArgs A;
  primer_args(P, A);
  if (n < 0 || (n > 0 && (!seq || !offsets))) throw InputError{"dada2hip: bad arguments"};
  int lmin = PR_MAXL;
  for (int a = 0; a < A.nact; a++) lmin = std::min(lmin, (int)A.len[A.act[a]]);
  for (int64_t r = 0; r < n; r++) {
    const int64_t l = offsets[r + 1] - offsets[r];
    if (l < 0 || l > (int64_t)1 << 30) throw InputError{"dada2hip: bad read offsets."};
    // (the host's count of the kernel's tiles: the chunks of 64 that hold the starts -mm .. l - lmin + mm)
    const int64_t nstart = std::max<int64_t>(0, l - lmin + 2 * (int64_t)A.mm + 1), nchunk = (nstart + 63) / 64;
    st[PS_TILES] += nchunk > 0 ? (nchunk + A.tile - 1) / A.tile : 1;
  }
  st[PS_IN] = n;
  select_device(device);
  PrSlot slot[2];
  for (PrSlot &S : slot) {
    D2_HIP(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) D2_HIP(hipEventCreate(&S.ev[i]));
  }
  int64_t bad_read = -1;
  auto harvest = [&](PrSlot &S) {
    if (!S.busy) return;
    auto t0 = clk::now();
    D2_HIP(hipStreamSynchronize(S.st));
    S.busy = false;
    D2_HIP(hipGetLastError());
    float ms = 0.0f;
    D2_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[1])); st[PS_US_KERNEL] += (int64_t)((double)ms * 1e3);
    const int64_t f = S.first, c = S.count;
    const PrimerOut *o = S.h_out.p;
    for (int64_t i = 0; i < c; i++) {
      const PrimerOut &x = o[i];
      if (code) code[f + i] = x.code;
      if (flip) flip[f + i] = x.flip;
      if (first) first[f + i] = x.first;
      if (last) last[f + i] = x.last;
      if (hits) memcpy(hits + 4 * (f + i), x.hits, sizeof x.hits);
      if (x.code == 0) st[PS_KEPT]++; else st[PS_CODE1 + x.code - 1]++;
      if (x.code == 4 && bad_read < 0) bad_read = f + i;
      st[PS_FLIPPED] += x.flip;
      st[PS_MULTI] += (x.hits[0] > 1 || x.hits[1] > 1 || x.hits[2] > 1 || x.hits[3] > 1) ? 1 : 0;
      st[PS_HITS_FWD] += x.hits[0]; st[PS_HITS_REV] += x.hits[1];
    }
    if (starts) memcpy(starts + 8 * f, S.h_starts.p, (size_t)c * 8 * sizeof(int32_t));
    st[PS_US_DOWN] += (int64_t)(ms_since(t0) * 1e3);
  };

  const int64_t piece_reads = knobs().primers_piece > 0 ? std::min<int64_t>(knobs().primers_piece, PR_PIECE_READS) : PR_PIECE_READS;
  const int64_t piece_bytes = knobs().primers_piece_bytes > 0 ? std::min<int64_t>(knobs().primers_piece_bytes, PR_PIECE_BYTES) : PR_PIECE_BYTES;
  int64_t r0 = 0;
  for (int piece = 0; r0 < n; piece++) {
    int64_t r1 = r0 + 1;
    while (r1 < n && r1 - r0 < piece_reads && offsets[r1 + 1] - offsets[r0] <= piece_bytes) r1++;
    PrSlot &S = slot[piece & 1];
    harvest(S);
    auto t_up = clk::now();
    const int64_t c = r1 - r0, base = offsets[r0], bytes = offsets[r1] - base;
    S.h_seq.alloc((size_t)bytes); S.h_off.alloc((size_t)c + 1); S.h_out.alloc((size_t)c);
    S.d_seq.alloc((size_t)bytes); S.d_off.alloc((size_t)c + 1); S.d_out.alloc((size_t)c);
    if (starts) { S.h_starts.alloc((size_t)c * 8); S.d_starts.alloc((size_t)c * 8); }
    parallel_for((size_t)bytes, (size_t)1 << 20, [&](size_t lo, size_t hi) { memcpy(S.h_seq.p + lo, seq + base + lo, hi - lo); });
    for (int64_t i = 0; i <= c; i++) S.h_off.p[i] = (long long)(offsets[r0 + i] - base);
    if (bytes > 0) D2_HIP(hipMemcpyAsync(S.d_seq.p, S.h_seq.p, (size_t)bytes, hipMemcpyHostToDevice, S.st));
    D2_HIP(hipMemcpyAsync(S.d_off.p, S.h_off.p, (size_t)(c + 1) * 8, hipMemcpyHostToDevice, S.st));
    D2_HIP(hipEventRecord(S.ev[0], S.st));
    launch_primers(A, (int)c, S.d_seq.p, S.d_off.p, S.d_out.p, starts ? S.d_starts.p : nullptr, S.st);
    D2_HIP(hipEventRecord(S.ev[1], S.st));
    D2_HIP(hipMemcpyAsync(S.h_out.p, S.d_out.p, (size_t)c * sizeof(PrimerOut), hipMemcpyDeviceToHost, S.st));
    if (starts) D2_HIP(hipMemcpyAsync(S.h_starts.p, S.d_starts.p, (size_t)c * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, S.st));
    S.first = r0; S.count = c; S.busy = true;
    st[PS_BYTES] += bytes + (c + 1) * 8; st[PS_PIECES]++;
    st[PS_US_UP] += (int64_t)(ms_since(t_up) * 1e3);
    r0 = r1;
  }
  harvest(slot[0]); harvest(slot[1]);
  st[PS_US_TOTAL] = (int64_t)(ms_since(t_call) * 1e3);
  if (stats) memcpy(stats, st, sizeof st);
  if (bad_read >= 0)
    throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, "dada2hip: read " + std::to_string(bad_read + 1) +
                                                   " holds a letter outside the upper-case IUPAC codes ACGTMRWSYKVHDBN."};
}

}  // namespace

int dada2hip_primers_reads(int64_t n, const char *seq, const int64_t *offsets, const dada2hip_primer_params *params, int32_t device,
                           int32_t *code, int32_t *flip, int32_t *first, int32_t *last, int32_t *hits, int32_t *starts,
                           int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] { primers_reads_body(n, seq, offsets, params, device, code, flip, first, last, hits, starts, stats); });
}
