// collapse.inc.hip — the device side of collapseNoMismatch (R/multiSample.R:104-160); included by kernels.hip, inside namespace d2,
// behind seqkeys.inc.hip (bases16, the window key and the search of a key group).
//
// The reference walks, for every column of a sequence table, the columns it has kept so far; each step is two grepl() calls
// (does the first minOverlap bases of one sequence occur in the other?) and, where either says yes, an unbanded ends-free
// alignment reduced to "mismatches + internal indels == 0" (nwhamming, R/misc.R:216).  That relation of a PAIR does not depend
// on the state of the greedy loop, so it is evaluated in bulk here and the loop is replayed on the host (collapse_host.h):
//   k_collapse_join   which of the distinct prefix keys occur in which sequence: a necessary condition of the grepl screen that
//                     keeps 10^5 columns from costing 5 x 10^9 pair scans
//   k_collapse_scan   per (query, ref) pair, over all len_q + len_r - 1 gapless diagonals: the grepl screen itself, exactly; G, the
//                     best score of a gapless diagonal; m_max, the longest diagonal without a mismatch.  An alignment without
//                     mismatch or internal indel lies on one diagonal and scores match x (its overlap) <= match x m_max, and the
//                     optimum of the unbanded ends-free DP is at least G: with G > match x m_max no optimal alignment is exact,
//                     whatever the traceback's tie-breaking does.  Every other screened pair goes to the lane aligner
//                     (k_nw_gen<pair>, through nwvec_any) - the ties are real.
// Neither is an aligner instance: no entry in the launch ledger.

constexpr int CL_MAXW = (SEQLEN + 15) / 16;   // 2-bit words of the longest row a resident sample takes (reads < SEQLEN)

// One wave per sequence, a lane per window position; rows [row0, row0 + nrows) of the sample, bits[row - row0][KW] preset to 0.
// keys: the distinct (length, first bases) prefix keys, ascending inside each length's group; groups[g] = {length, first key,
// number of keys}.  A window that equals key k sets bit k of its sequence's row.
__global__ __launch_bounds__(256) void k_collapse_join(SampleDev S, int row0, int nrows, const unsigned long long *__restrict__ keys,
                                                        const int32_t *__restrict__ groups, int ngroups, int KW,
                                                        uint32_t *__restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((gridDim.x * blockDim.x) >> 6);
  for (int rr = wave; rr < nrows; rr += nwaves) {
    const int sq = row0 + rr, L = S.len[sq], nw = (L + 15) >> 4;
    const uint32_t *row = S.seq2 + (size_t)sq * S.W2;
    for (int g = 0; g < ngroups; g++) {
      const int kl = groups[3 * g], first = groups[3 * g + 1], cnt = groups[3 * g + 2];
      const unsigned long long mask = key_mask(kl);
      for (int p = lane; p + kl <= L; p += 64) {
        const unsigned long long w = window_key(row, nw, p, mask);
        const int lo = key_lower_bound(keys, first, cnt, w);
        if (lo < first + cnt && keys[lo] == w) atomicOr(&bits[(size_t)rr * KW + (lo >> 5)], 1u << (lo & 31));
      }
    }
  }
}

void launch_collapse_join(const SampleDev &S, int row0, int nrows, const unsigned long long *d_keys, const int32_t *d_groups,
                          int ngroups, int KW, uint32_t *d_bits, hipStream_t st) {
  if (nrows <= 0 || ngroups <= 0) return;
  hipLaunchKernelGGL(k_collapse_join, dim3(std::min((nrows + 3) / 4, 2048)), dim3(256), 0, st, S, row0, nrows, d_keys, d_groups, ngroups,
                     KW, d_bits);
}

// One wave per pair (query = pairs[i].x, ref = pairs[i].y, rows of the sample), both 2-bit rows staged in LDS, a lane per diagonal:
// on diagonal s, q[i] faces r[i - s]; the overlap is i in [max(0, s), min(len_q, len_r + s)).  out[i] = {screen, G, m_max, decision}:
//   screen    bit 0: substr(q, 1, minOverlap) occurs in r (a diagonal s <= 0 whose first min(minOverlap, len_q) columns match);
//             bit 1: substr(r, 1, minOverlap) occurs in q (s >= 0, min(minOverlap, len_r) columns)
//   G         max over the diagonals of match (m - mm) + mismatch mm, m the overlap and mm its mismatches
//   m_max     the longest overlap with mm == 0, 0 if there is none
//   decision  0 screened out, 1 rejected by the bound (use_bound and G > match m_max), 2 needs the alignment
__global__ __launch_bounds__(64) void k_collapse_scan(SampleDev S, const int2 *__restrict__ pairs, int npairs, int min_overlap, int match,
                                                       int mismatch, int use_bound, int4 *__restrict__ out) {
  __shared__ uint32_t s_q[CL_MAXW], s_r[CL_MAXW];
  const int lane = threadIdx.x;
  for (int pi = blockIdx.x; pi < npairs; pi += gridDim.x) {
    const int2 pr = pairs[pi];
    const int lq = S.len[pr.x], lr = S.len[pr.y];
    const int wq = (lq + 15) >> 4, wr = (lr + 15) >> 4;
    __syncthreads();                                       // (the previous pair's rows are no longer read)
    for (int w = lane; w < wq; w += 64) s_q[w] = S.seq2[(size_t)pr.x * S.W2 + w];
    for (int w = lane; w < wr; w += 64) s_r[w] = S.seq2[(size_t)pr.y * S.W2 + w];
    __syncthreads();
    const int plq = min(min_overlap, lq), plr = min(min_overlap, lr);
    int best = -2147483647 - 1, mmax = 0, screen = 0;
    const int nd = lq + lr - 1;
    for (int d = lane; d < nd; d += 64) {
      const int s = d - (lr - 1);
      const int i0 = max(0, s), i1 = min(lq, lr + s);
      int mm = 0, lead = -1;                               // lead: matching columns before the overlap's first mismatch
      for (int w = i0 >> 4; w <= (i1 - 1) >> 4; w++) {
        const uint32_t x = s_q[w] ^ bases16(s_r, wr, 16 * w - s);
        const int lo = max(i0 - 16 * w, 0), hi = min(i1 - 16 * w, 16);   // the word's bases [lo, hi) lie in the overlap
        const uint32_t keep = (hi >= 16 ? ~0u : ((1u << (2 * hi)) - 1u)) & ~((1u << (2 * lo)) - 1u);
        const uint32_t f = (x | (x >> 1)) & 0x55555555u & keep;          // one bit per mismatching base
        if (f != 0u && lead < 0) lead = 16 * w + (__builtin_ctz(f) >> 1) - i0;
        mm += __popc(f);
      }
      const int m = i1 - i0;
      if (lead < 0) lead = m;
      best = max(best, match * (m - mm) + mismatch * mm);
      if (mm == 0) mmax = max(mmax, m);
      if (s <= 0 && lead >= plq) screen |= 1;
      if (s >= 0 && lead >= plr) screen |= 2;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      best = max(best, __shfl_xor(best, o, 64));
      mmax = max(mmax, __shfl_xor(mmax, o, 64));
      screen |= __shfl_xor(screen, o, 64);
    }
    if (lane == 0) {
      const int dec = screen == 0 ? 0 : ((use_bound && best > match * mmax) ? 1 : 2);
      out[pi] = make_int4(screen, best, mmax, dec);
    }
  }
}

void launch_collapse_scan(const SampleDev &S, const int2 *d_pairs, int npairs, int min_overlap, int match, int mismatch, int use_bound,
                          int4 *d_out, hipStream_t st) {
  if (npairs <= 0) return;
  hipLaunchKernelGGL(k_collapse_scan, dim3(std::min(npairs, 16384)), dim3(64), 0, st, S, d_pairs, npairs, min_overlap, match, mismatch,
                     use_bound, d_out);
}
