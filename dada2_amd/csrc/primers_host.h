// primers_host.h — host side of removePrimers' per-read verdicts (R/filter.R:81-233); included by driver.cpp inside its extern "C"
// block, behind filter_host.h.  The file-level entry (dada2hip_primers_fastq) is derep.cpp's, where the FASTQ reader and writer
// are; it calls dada2hip_primers_reads per chunk.
//
// The call turns the primers into the four patterns of primers.inc.hip (the forward primer, the reverse primer, the reverse
// complement of each), every letter a byte of plane selectors: the letter's IUPAC set for a primer with a letter beyond A/C/G/T
// (fixed = FALSE, :111-112), the "is exactly this base" plane for a primer of A/C/G/T only.  Both rules are symmetric under
// complement, so the reverse complement of a pattern is matched by the same rule and the read is never reverse-complemented.
// The reads go up through read_pieces.h's two-slot pipeline (DADA2HIP_PRIMERS_PIECE, DADA2HIP_PRIMERS_PIECE_BYTES: smaller pieces,
// for the tests), only the sequence bytes and the offsets, the slots made per call; the stage supplies the one kernel and the
// scatter (32 bytes per read come back, 32 more when the starts are asked for).  From stage_common.h: the clocks, the end of a call.
#pragma once

namespace {

using PrSlot = PieceSlot<PrimerOut, 2>;   // aux: the eight starts

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
  for (PrSlot &S : slot) S.create();
  int64_t bad_read = -1;
  auto launch = [&](PrSlot &S, int c) {
    launch_primers(A, c, S.d_seq.p, S.d_off.p, S.d_out.p, starts ? S.d_aux.p : nullptr, S.st);
    st[PS_PIECES]++;
  };
  auto scatter = [&](PrSlot &S) {
    add_elapsed(st[PS_US_KERNEL], S.ev[0], S.ev[1]);
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
    if (starts) memcpy(starts + 8 * f, S.h_aux.p, (size_t)c * 8 * sizeof(int32_t));
  };
  run_pieces(slot, n, seq, nullptr, offsets, knobs().primers_piece, knobs().primers_piece_bytes, starts ? 8 : 0, st, PS_BYTES, PS_US_UP,
             PS_US_DOWN, launch, scatter);
  finish_stats(st, PS_US_TOTAL, t_call, stats);
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
