// primers.inc.hip — the device side of removePrimers (R/filter.R:81-233: vmatchPattern(primer, reads, max.mismatch, with.indels =
// FALSE, fixed = C_isACGT(primer)) on the reads and, with orient, on their reverse complements; the first forward and the last
// reverse match; flip, keep and the window); included by kernels.hip, inside namespace d2, behind filter.inc.hip.
//
//   k_primers   a block of two waves per read.  A read is swept in tiles of `tile` chunks of 64 match starts.
//     planes    a wave takes 64 positions at a time and builds, from four ballots, the planes "the letter's IUPAC set holds A / C /
//               G / T", and from them the planes "the letter IS that base" (plane & ~the other three) for the fixed rule; a fifth
//               ballot, "no IUPAC letter", is the read's error flag.  The eight words go to LDS; a tile holds its chunks and two
//               more, the L - 1 positions its last starts look at.  A position outside the read has zero planes: it matches
//               nothing under either rule, which is the out-of-limits rule with nothing written for it.
//     search    a lane takes one (pattern, chunk of 64 starts).  For primer letter i the word of the starts whose letter at
//               start + i matches is the OR of the selected planes, shifted by i across two adjacent words; its complement is added
//               into a bit-sliced counter of ceil(log2(mm + 1)) planes that starts at 2^bits - 1 - mm, so that the carry out of its
//               top plane is "more than mm mismatches": that word is sticky and masks later additions, nothing wraps.  After L
//               letters the hits are the starts without the sticky bit, inside the pattern's range of starts.
//     verdict   count, smallest and largest start per pattern come together in LDS; thread 0 settles the read.
// The bit of start st is st - lo of the word sequence, lo being the smallest start of any pattern: the range of starts is
// pr_start_range's, and nowhere else.

// THE range of match starts (0-based, inclusive) of a pattern of L letters in a read of n: up to mm positions of a match may lie
// outside the read, where they count as mismatches (Biostrings' "out of limits" matches)
__device__ __forceinline__ void pr_start_range(int n, int L, int mm, int &lo, int &hi) { lo = -mm; hi = n - L + mm; }

// the IUPAC set of a letter over A C G T = 1 2 4 8; 0 for anything else
__device__ __forceinline__ int pr_mask(uint8_t c) {
  const unsigned i = (unsigned)c - (unsigned)'A';
  if (i >= 26u) return 0;
  const unsigned long long tab = i < 16u ? 0x00F30C00B400D2E1ull : 0x0A09708650ull;   // A-P, Q-Z, a nibble a letter
  return (int)((tab >> ((i & 15u) * 4u)) & 15ull);
}

// 64 bits of the plane (cur, next) from bit s on, 0 <= s < 64
__device__ __forceinline__ unsigned long long pr_from(unsigned long long cur, unsigned long long next, int s) {
  return s == 0 ? cur : ((cur >> s) | (next << (64 - s)));
}

__global__ __launch_bounds__(PR_THREADS) void k_primers(PrimerArgs A, int n, const uint8_t *__restrict__ seq,
                                                         const long long *__restrict__ off, PrimerOut *__restrict__ out,
                                                         int32_t *__restrict__ starts) {
  __shared__ unsigned long long s_pl[8][PR_TILE_MAX + 2];
  __shared__ uint8_t s_sel[4][PR_MAXL];
  __shared__ int s_cnt[4], s_min[4], s_max[4], s_bad;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 4 * PR_MAXL; i += PR_THREADS) s_sel[i / PR_MAXL][i % PR_MAXL] = A.sel[i / PR_MAXL][i % PR_MAXL];
  const int T = A.tile, mm = A.mm, nb = A.nbits;
  const unsigned init = (1u << nb) - 1u - (unsigned)mm;        // the counter's first value: mm + 1 additions carry out of it
  // (everything that steers a loop with a barrier in it is the same on all threads of the block: offsets and arguments)
  for (int r = (int)blockIdx.x; r < n; r += (int)gridDim.x) {
    const long long b = off[r];
    const int len = (int)(off[r + 1] - b);
    if (tid < 4) { s_cnt[tid] = 0; s_min[tid] = INT32_MAX; s_max[tid] = INT32_MIN; }
    if (tid == 0) s_bad = 0;
    int lo_all = INT32_MAX, hi_all = INT32_MIN;
    for (int a = 0; a < A.nact; a++) {
      int lo, hi;
      pr_start_range(len, A.len[A.act[a]], mm, lo, hi);
      lo_all = min(lo_all, lo); hi_all = max(hi_all, hi);
    }
    const int nstart = hi_all >= lo_all ? hi_all - lo_all + 1 : 0;   // bit s of the word sequence is start lo_all + s
    const int nchunk = (nstart + 63) >> 6;
    const int ntile = nchunk > 0 ? (nchunk + T - 1) / T : 1;    // (a read too short for any start is still looked at for its letters)
    for (int tile = 0; tile < ntile; tile++) {
      const int c0 = tile * T, tc = min(T, nchunk - c0), nw = tc + 2;
      __syncthreads();                                           // the search of the tile before is through with the planes
      for (int w = wave; w < nw; w += PR_THREADS / 64) {
        const long long p = (long long)(c0 + w) * 64 + lane + lo_all;
        int m = 0, bad = 0;
        if (p >= 0 && p < (long long)len) { m = pr_mask(seq[b + p]); bad = m == 0; }
        const unsigned long long pa = __ballot(m & 1), pc = __ballot(m & 2), pg = __ballot(m & 4), pt = __ballot(m & 8);
        const unsigned long long pb = __ballot(bad);
        if (lane == 0) {
          s_pl[0][w] = pa; s_pl[1][w] = pc; s_pl[2][w] = pg; s_pl[3][w] = pt;
          s_pl[4][w] = pa & ~(pc | pg | pt); s_pl[5][w] = pc & ~(pa | pg | pt);
          s_pl[6][w] = pg & ~(pa | pc | pt); s_pl[7][w] = pt & ~(pa | pc | pg);
          if (pb != 0ull) atomicOr(&s_bad, 1);
        }
      }
      __syncthreads();
      for (int t = tid; t < A.nact * tc; t += PR_THREADS) {
        const int a = t / tc, c = t - a * tc, k = A.act[a], L = A.len[k];
        int lo, hi;
        pr_start_range(len, L, mm, lo, hi);
        const long long s_base = (long long)(c0 + c) * 64;      // bit 0 of this chunk is start lo_all + s_base
        const long long v0 = (long long)lo - lo_all - s_base, v1 = (long long)hi - lo_all - s_base;   // its valid bits: v0 .. v1
        if (v1 < 0 || v0 > 63) continue;
        unsigned long long valid = ~0ull;
        if (v0 > 0) valid &= ~0ull << v0;
        if (v1 < 63) valid &= ~0ull >> (63 - v1);
        unsigned long long cnt[4], dead = 0ull;
#pragma unroll
        for (int j = 0; j < 4; j++) cnt[j] = ((init >> j) & 1u) ? ~0ull : 0ull;
        for (int i = 0; i < L; i++) {
          const int sel = s_sel[k][i], w = c + (i >> 6);
          unsigned long long cur = 0ull, nxt = 0ull;
#pragma unroll
          for (int pl = 0; pl < 8; pl++)
            if (sel & (1 << pl)) { cur |= s_pl[pl][w]; nxt |= s_pl[pl][w + 1]; }
          unsigned long long carry = ~pr_from(cur, nxt, i & 63) & ~dead;
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (j < nb) { const unsigned long long x = cnt[j] & carry; cnt[j] ^= carry; carry = x; }
          dead |= carry;
        }
        const unsigned long long h = ~dead & valid;
        if (h != 0ull) {
          const int st0 = (int)(s_base + lo_all);
          atomicAdd(&s_cnt[k], __popcll(h));
          atomicMin(&s_min[k], st0 + __builtin_ctzll(h));
          atomicMax(&s_max[k], st0 + 63 - __builtin_clzll(h));
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      PrimerOut o;
      int st[8];
      const bool bad = s_bad != 0;
      for (int k = 0; k < 4; k++) {
        const int h = bad ? 0 : s_cnt[k], L = A.len[k];
        o.hits[k] = h;
        // (a start of rc(P) on the read is the start len - L - st of P on the reverse complement: its first is the other's last)
        if (h == 0) { st[2 * k] = PR_NA; st[2 * k + 1] = PR_NA; }
        else if (k < 2) { st[2 * k] = s_min[k] + 1; st[2 * k + 1] = s_max[k] + 1; }
        else { st[2 * k] = len - L - s_max[k] + 1; st[2 * k + 1] = len - L - s_min[k] + 1; }
      }
      const int flip = (A.orient && o.hits[0] == 0 && o.hits[2] > 0) ? 1 : 0;   // :181
      const int kf = flip ? 2 : 0, kr = flip ? 3 : 1;
      int code = 0, first = 0, last = 0;
      if (bad) code = 4;
      else if (o.hits[kf] == 0) code = 1;                        // :193
      else if (A.has_rev && o.hits[kr] == 0) code = 2;           // :194
      else {
        first = A.trim_fwd ? st[2 * kf] + A.len[kf] : 1;         // :201-205: end(first forward match) + 1
        last = (A.has_rev && A.trim_rev) ? st[2 * kr + 1] - 1 : len;   // :206-210: start(last reverse match) - 1
        if (!(last > first)) code = 3;                           // :211
      }
      o.code = code; o.flip = flip; o.first = first; o.last = last;
      out[r] = o;
      if (starts)
        for (int i = 0; i < 8; i++) starts[(size_t)r * 8 + i] = st[i];
    }
    __syncthreads();                                             // the next read's counters are set behind this
  }
}

void launch_primers(const PrimerArgs &A, int n, const uint8_t *d_seq, const long long *d_off, PrimerOut *d_out, int32_t *d_starts,
                    hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_primers, dim3((unsigned)std::min(n, PR_GRID)), dim3(PR_THREADS), 0, st, A, n, d_seq, d_off, d_out, d_starts);
}
