// readqc.inc.hip — the device side of the read diagnostics (R/plot-methods.R:163-243 plotQualityProfile on ShortRead qa()'s
// perCycle$quality; R/filter.R:1248-1275 seqComplexity with a window, R/plot-methods.R:293-299 plotComplexity); included by
// kernels.hip, inside namespace d2, behind primers.inc.hip.  Integers only in the table's kernel; the one floating-point sum of the
// windowed complexity is H = sum(-y log y), whose exp, cap and NaN rule are the host's.
//
//   k_qprofile        a block owns the tile of 64 cycles blockIdx.y and every gridDim.x-th group of sixteen reads from blockIdx.x on:
//                     a wave takes a read, lane j reads byte c0 + j of its qualities - a coalesced row of 64 bytes - and bumps
//                     cell (j, letter - '!') of the block's LDS table by an LDS atomic.  A lane past the read's end counts
//                     nothing; a letter outside '!'..'~' counts nothing and marks the read.  At the end the block adds its
//                     non-zero cells into the batch's 64-bit table.
//   k_complexity_win  a block of one wave per read.  A window's 2-bit codes and its "not A/C/G/T" plane are three ballots per 64
//                     positions, as in k_filter_scan; the lane of k-mer p shifts the planes of this chunk and the next together,
//                     so a k-mer costs no further load.  The window's 4^k histogram is in LDS; its H is summed over the bins by a
//                     lane each and a butterfly.  Two numbers per read come back (engine.h: ComplexityOut), which keeps a batch
//                     independent of the longest read of the CALL: the host decides whether the last window counts.

__global__ __launch_bounds__(QP_THREADS) void k_qprofile(int n, const uint8_t *__restrict__ qual, const long long *__restrict__ off,
                                                          unsigned long long *__restrict__ tab, int32_t *__restrict__ bad) {
  __shared__ unsigned int s_tab[QP_TILE * QP_ROW];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < QP_TILE * QP_ROW; i += QP_THREADS) s_tab[i] = 0u;
  __syncthreads();
  const int c0 = (int)blockIdx.y * QP_TILE, c = c0 + lane;
  constexpr int NW = QP_THREADS / 64, UNROLL = 4;
  const long long step = (long long)gridDim.x * NW;
  // (four reads of a wave in flight: their offsets, then their bytes, then the atomics)
  for (long long r0 = (long long)blockIdx.x * NW + wave; r0 < n; r0 += step * UNROLL) {
    long long b[UNROLL];
    int len[UNROLL];
    unsigned q[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const long long r = r0 + step * u;
      b[u] = 0; len[u] = 0;
      if (r < n) { b[u] = off[r]; len[u] = (int)(off[r + 1] - b[u]); }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) q[u] = c < len[u] ? (unsigned)qual[b[u] + c] - 33u : 0u;
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      if (c >= len[u]) continue;
      if (q[u] < (unsigned)QP_NSCORE) atomicAdd(&s_tab[lane * QP_ROW + (int)q[u]], 1u);
      else bad[r0 + step * u] = 1;
    }
  }
  __syncthreads();
  for (int i = tid; i < QP_TILE * QP_NSCORE; i += QP_THREADS) {
    const int j = i / QP_NSCORE, s = i - j * QP_NSCORE;
    const unsigned int v = s_tab[j * QP_ROW + s];
    if (v != 0u) atomicAdd(&tab[(size_t)(c0 + j) * QP_NSCORE + s], (unsigned long long)v);
  }
}

void launch_qprofile(int n, int ncyc_pad, const uint8_t *d_qual, const long long *d_off, unsigned long long *d_tab, int32_t *d_bad,
                     hipStream_t st) {
  if (n <= 0 || ncyc_pad <= 0) return;
  const unsigned gx = (unsigned)std::min((n + QP_SLICE - 1) / QP_SLICE, QP_GRID_X), gy = (unsigned)(ncyc_pad / QP_TILE);
  hipLaunchKernelGGL(k_qprofile, dim3(gx, gy), dim3(QP_THREADS), 0, st, n, d_qual, d_off, d_tab, d_bad);
}

__global__ __launch_bounds__(64) void k_complexity_win(int n, int k, int window, int by, const uint8_t *__restrict__ seq,
                                                        const long long *__restrict__ off, const double *__restrict__ ylogy,
                                                        ComplexityOut *__restrict__ out) {
  extern __shared__ double cw_tab[];                             // [window - k + 2]
  __shared__ int32_t s_h[256];
  const int lane = (int)threadIdx.x;
  const int full = window - k + 1, nb = 1 << (2 * k);            // the k-mers of a window; the bins
  const unsigned long long kmask = (1ull << k) - 1ull;
  for (int i = lane; i <= full; i += 64) cw_tab[i] = ylogy[i];
  for (int i = lane; i < nb; i += 64) s_h[i] = 0;
  __syncthreads();
  const double inf = (double)INFINITY, nan = (double)NAN;
  // (everything that steers a loop with a barrier in it is the same on all lanes: offsets, arguments and ballots)
  for (int r = (int)blockIdx.x; r < n; r += (int)gridDim.x) {
    const long long b = off[r];
    const int len = (int)(off[r + 1] - b);
    double lo = inf, last = inf;
    for (long long s = 0; s + window <= (long long)len; s += by) {
      const uint8_t *w = seq + b + s;
      int tot = 0;
      unsigned long long c0 = 0, c1 = 0, cn = 0, n0 = 0, n1 = 0, nn = 0;
      for (int p0 = -64; p0 < full; p0 += 64) {                  // the planes of chunk p0 + 64 are taken, the k-mers of chunk p0 counted
        c0 = n0; c1 = n1; cn = nn;
        const int p = p0 + 64 + lane;
        const int cd = p < window ? ft_code(w[p]) : 0;
        n0 = __ballot(cd & 1); n1 = __ballot(cd & 2); nn = __ballot(cd & 4);
        if (p0 < 0) continue;
        const int j = p0 + lane;
        const bool ok = j < full && (ft_from(cn, nn, lane) & kmask) == 0ull;
        tot += __popcll(__ballot(ok));
        if (ok) {
          const unsigned long long w0 = ft_from(c0, n0, lane), w1 = ft_from(c1, n1, lane);
          int idx = 0;
          for (int t = 0; t < k; t++) idx = idx * 4 + (int)(((w0 >> t) & 1ull) | (((w1 >> t) & 1ull) << 1));
          atomicAdd(&s_h[idx], 1);
        }
      }
      __syncthreads();
      double acc = 0.0;
      for (int i = lane; i < nb; i += 64) {
        const int c = s_h[i];
        s_h[i] = 0;
        if (c > 0) {
          if (tot == full) acc += cw_tab[c];
          else { const double y = (double)c / (double)tot; acc += -y * log(y); }
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
      const double H = tot > 0 ? acc : nan;
      if (s + window < (long long)len) { if (H < lo || H != H) lo = H; }   // (a NaN stays: nothing is below it)
      else last = H;
      __syncthreads();                                           // the next window's counts go into cleared bins
    }
    if (lane == 0) { ComplexityOut o; o.lo = lo; o.last = last; out[r] = o; }
  }
}

void launch_complexity_win(int n, int k, int window, int by, const uint8_t *d_seq, const long long *d_off, const double *d_ylogy,
                           ComplexityOut *d_out, hipStream_t st) {
  if (n <= 0) return;
  const size_t lds = (size_t)(window - k + 2) * sizeof(double);
  hipLaunchKernelGGL(k_complexity_win, dim3((unsigned)std::min(n, CW_GRID)), dim3(64), lds, st, n, k, window, by, d_seq, d_off, d_ylogy,
                     d_out);
}
