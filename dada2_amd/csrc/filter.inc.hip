// filter.inc.hip — the device side of filterAndTrim (R/filter.R:613-730 fastqFilter, :1180-1187 isPhiX, :1248-1275 seqComplexity;
// src/filter.cpp:7-32 C_matchRef, :35-49 C_matrixEE); included by kernels.hip, inside namespace d2, behind species.inc.hip.
//
// A batch of reads lies on the device as it was parsed: the sequence bytes, the quality bytes and the offsets.
//   k_filter_scan   a wave per read.  The window arithmetic of stages 1-3 and 5-6 is scalar; the truncQ cut (trimTails(fq, 1,
//                   truncQ), :677) is a ballot over 64 positions at a time and the first set bit.  One pass over the kept window,
//                   64 positions at a time, then gives the letters that are not upper-case A/C/G/T (a popcount of a ballot), the
//                   minimum quality (a lane minimum, reduced at the end) and three bit planes of the chunk: bit 0 and bit 1 of
//                   every base's 2-bit code and "not A/C/G/T".  The lane of window j shifts the planes of this chunk and the next
//                   one together, so its key - the two planes of its wordSize bases side by side - costs no memory access and no
//                   staging of the read: a read of any length takes the same path.  The key is searched in the sorted word table
//                   (both strands in one array, two flag bits per word), which the block keeps in LDS when it fits.  The hit bits
//                   of the 64 windows come back as two ballots, and the greedy count of C_matchRef (:24-29: a hit at j makes
//                   j + wordSize + 1 the next window tested - `j += word_size` and then the loop's `j++`) is a walk over set
//                   bits, the same on every lane.  The two strands are counted apart and never summed (:1184-1186).
//   k_filter_ee     a thread per read: ee = 0.0; ee += tab[q] in read order (:41-45), tab computed by the host's pow.  Nothing is
//                   reduced across lanes: twenty Q10 bases are 2.0000000000000004 in this order and 2.0 in a tree, and maxEE = 2
//                   tells them apart.  Then stages 9 (ee <= maxEE, :692) and 10 (either count >= minMatches).
//   k_filter_kmers  a block of one wave per read: the k-mer histogram of seqComplexity in LDS, integer counts out; the Shannon
//                   number is the host's (libm's log and exp, in bin order).
//   k_filter_orient orient.fwd (:648-658): a wave per read, the barcode against the read's first letters and its complement against
//                   the read's last letters backwards, 64 letters per ballot; one byte per read into FilterOut::pad.  The three
//                   kernels above have an ORIENT instance each that reads it and traverses a flipped read from its end, letters
//                   complemented; the instances without it are what the un-oriented entries launch, unchanged.
// Codes: 0 kept, 1 maxLen, 2 trimLeft, 3 trimRight, 4 truncQ left nothing, 5 truncLen, 6 minLen, 7 maxN, 8 minQ, 9 maxEE, 10 phiX
// (11, the complexity, is the host's; 12, the oriented instances only: in neither orientation).  A read that fails a stage 1-6
// reports an empty window and no counts.

__device__ __forceinline__ int ft_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// the flags of key k, 0 if it is no word of the reference
__device__ __forceinline__ int ft_lookup(const unsigned long long *keys, const uint8_t *flags, int n, unsigned long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return (lo < n && keys[lo] == k) ? (int)flags[lo] : 0;
}

// 64 bits of the plane (cur, next) from bit s on, 0 <= s < 64
__device__ __forceinline__ unsigned long long ft_from(unsigned long long cur, unsigned long long next, int s) {
  return s == 0 ? cur : ((cur >> s) | (next << (64 - s)));
}

// C_matchRef's count over the hit bits m of windows p0 .. p0 + 63 (uniform over the wave); next: the first window still tested
__device__ __forceinline__ void ft_count(unsigned long long m, int p0, int step, bool non_overlapping, int &count, int &next) {
  if (!non_overlapping) { count += __popcll(m); return; }
  int s = next - p0;
  if (s >= 64) return;
  if (s > 0) m &= ~0ull << s;
  while (m != 0ull) {
    const int j = __builtin_ctzll(m);
    count++;
    next = p0 + j + step;
    s = j + step;
    if (s >= 64) break;
    m &= ~0ull << s;
  }
}

// ORIENT: the instance for dada2hip_filter_reads_oriented.  out[r].pad holds k_filter_orient's verdict, the same on every lane of the
// read's wave; position p of a flipped read is letter L - 1 - p with its 2-bit code complemented (3 - code; "other" stays other), so
// the truncQ ballot, the planes, the window keys and the greedy walk are those of the reverse complement read from ITS left end.
template <bool LDS, bool ORIENT>
__global__ __launch_bounds__(FT_THREADS) void k_filter_scan(FilterTable T, FilterArgs A, int n, const uint8_t *__restrict__ seq,
                                                             const uint8_t *__restrict__ qual, const long long *__restrict__ off,
                                                             FilterOut *__restrict__ out) {
  extern __shared__ unsigned long long ft_lds[];
  const unsigned long long *keys = T.keys;
  const uint8_t *flags = T.flags;
  if (LDS) {                                                   // keys[nkeys], then flags[nkeys]
    uint8_t *sf = (uint8_t *)(ft_lds + T.nkeys);
    for (int i = (int)threadIdx.x; i < T.nkeys; i += (int)blockDim.x) { ft_lds[i] = T.keys[i]; sf[i] = T.flags[i]; }
    __syncthreads();
    keys = ft_lds; flags = sf;
  }
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((gridDim.x * blockDim.x) >> 6);
  const int W = T.word_size;
  const unsigned long long wmask = W >= 32 ? 0xFFFFFFFFull : ((1ull << W) - 1ull);
  const bool screen = T.nkeys > 0;
  // (everything below that steers a branch is the same on all lanes of the wave: offsets, arguments and ballots)
  for (int r = wave; r < n; r += nwaves) {
    const long long b = off[r];
    const int L = (int)(off[r + 1] - b);
    int code = 0, w = 0;
    const int ori = ORIENT ? out[r].pad : 0;
    const bool flip = ORIENT && ori == 1;
    if (ORIENT && ori >= 2) code = FT_CODE_ORIENT;             // :655-657: in neither set
    else if (A.max_len > 0 && L > A.max_len) code = 1;         // :660
    else if (L < A.skip + 1) code = 2;                         // :662
    else {
      w = L - A.skip;                                          // :663
      if (A.trim_right > 0) {                                  // :665-668
        if (w > A.trim_right) w -= A.trim_right; else code = 3;
      }
    }
    const uint8_t *s = seq + b + A.skip, *q = qual + b + A.skip;
    const uint8_t *se = seq + b + L - 1 - A.skip, *qe = qual + b + L - 1 - A.skip;   // (flipped: position p is se[-p], p < w <= L - skip)
    auto qv = [&](int p) -> int { return flip ? (int)qe[-p] : (int)q[p]; };
    auto cdv = [&](int p) -> int {
      if (!flip) return ft_code(s[p]);
      const int c = ft_code(se[-p]);
      return c < 4 ? 3 - c : 4;
    };
    if (code == 0) {                                           // :677, then the reads left with nothing
      for (int p0 = 0; p0 < w; p0 += 64) {
        const int p = p0 + lane;
        const unsigned long long m = __ballot(p < w && qv(p) <= A.cut_char);
        if (m != 0ull) { w = p0 + __builtin_ctzll(m); break; }
      }
      if (w == 0) code = 4;
    }
    if (code == 0 && A.trunc_end > 0) {                        // :680-682
      if (w < A.trunc_end) code = 5; else w = A.trunc_end;
    }
    if (code == 0 && w < A.min_len) code = 6;                  // :684
    int nother = 0, mq = 255, hf = 0, hr = 0;
    if (code == 0) {
      const int nwin = (screen && w >= W) ? w - W + 1 : 0;
      int next_f = 0, next_r = 0;
      unsigned long long c0 = 0, c1 = 0, cn = 0, n0 = 0, n1 = 0, nn = 0;
      for (int p0 = -64; p0 < w; p0 += 64) {                   // the planes of chunk p0 + 64 are taken, the windows of chunk p0 are looked up
        c0 = n0; c1 = n1; cn = nn;
        const int p = p0 + 64 + lane;
        int cd = 0;
        if (p < w) {
          cd = cdv(p);
          mq = min(mq, qv(p));
        }
        n0 = __ballot(cd & 1); n1 = __ballot(cd & 2); nn = __ballot(cd & 4);
        nother += __popcll(nn);
        if (p0 < 0 || p0 >= nwin) continue;
        int f = 0;
        const int j = p0 + lane;
        if (j < nwin && (ft_from(cn, nn, lane) & wmask) == 0ull) {
          const unsigned long long key = (ft_from(c0, n0, lane) & wmask) | ((ft_from(c1, n1, lane) & wmask) << 32);
          f = ft_lookup(keys, flags, T.nkeys, key);
        }
        const unsigned long long mf = __ballot(f & 1), mr = __ballot(f & 2);
        ft_count(mf, p0, W + 1, A.non_overlapping != 0, hf, next_f);
        ft_count(mr, p0, W + 1, A.non_overlapping != 0, hr, next_r);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mq = min(mq, __shfl_xor(mq, o, 64));
      if (nother > A.max_n) code = 7;                          // :687
      else if (A.minq_on && !(mq > A.minq_char)) code = 8;     // :690
    }
    if (lane == 0) {
      FilterOut o;
      o.code = code; o.off = A.skip; o.len = ((code >= 1 && code <= 6) || (ORIENT && code == FT_CODE_ORIENT)) ? 0 : w; o.nother = nother; o.minq = mq; o.hits_f = hf; o.hits_r = hr;
      o.pad = ori; o.ee = 0.0;
      out[r] = o;
    }
  }
}

template <bool ORIENT>
__global__ __launch_bounds__(256) void k_filter_ee(FilterArgs A, int n, const uint8_t *__restrict__ qual, const long long *__restrict__ off,
                                                   const double *__restrict__ ee_tab, FilterOut *__restrict__ out) {
  __shared__ double s_tab[256];
  s_tab[threadIdx.x] = ee_tab[threadIdx.x];
  __syncthreads();
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (r >= n) return;
  int code = out[r].code;
  const int len = out[r].len;
  if (len <= 0) return;
  const uint8_t *q = qual + off[r] + out[r].off;
  double ee = 0.0;
  if (ORIENT && out[r].pad == 1) {                             // the reverse complement's qualities, in ITS order
    const uint8_t *qe = qual + off[r + 1] - 1 - out[r].off;
    for (int j = 0; j < len; j++) ee += s_tab[qe[-j]];
  } else
  for (int j = 0; j < len; j++) ee += s_tab[q[j]];             // src/filter.cpp:41-45, in this order
  out[r].ee = ee;
  if (code == 0) {
    if (A.ee_on && !(ee <= A.max_ee)) code = 9;                // :692
    else if (A.rm_phix && (out[r].hits_f >= A.min_matches || out[r].hits_r >= A.min_matches)) code = 10;   // :1186
    if (code != 0) out[r].code = code;
  }
}

// a block of 64 threads per read; 4^k <= 256 bins
template <bool ORIENT>
__global__ __launch_bounds__(64) void k_filter_kmers(int n, int k, const uint8_t *__restrict__ seq, const long long *__restrict__ off,
                                                     const FilterOut *__restrict__ out, int32_t *__restrict__ counts) {
  __shared__ int32_t s_h[256];
  const int nb = 1 << (2 * k);
  for (int r = (int)blockIdx.x; r < n; r += (int)gridDim.x) {
    for (int i = (int)threadIdx.x; i < nb; i += 64) s_h[i] = 0;
    __syncthreads();
    const int len = out[r].len;
    const uint8_t *s = seq + off[r] + out[r].off;
    const bool flip = ORIENT && out[r].pad == 1;
    const uint8_t *se = seq + off[r + 1] - 1 - out[r].off;
    for (int p = (int)threadIdx.x; p + k <= len; p += 64) {
      int idx = 0, bad = 0;
      for (int t = 0; t < k; t++) {
        int cd = ft_code(flip ? se[-(p + t)] : s[p + t]);
        if (flip && cd < 4) cd = 3 - cd;
        bad |= cd & 4;
        idx = idx * 4 + (cd & 3);
      }
      if (!bad) atomicAdd(&s_h[idx], 1);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < nb; i += 64) counts[(size_t)r * nb + i] = s_h[i];
    __syncthreads();
  }
}

// orient.fwd: a wave per read; the barcode against the read's first letters and (unless forward_only) its complement against the
// read's last letters read backwards, 64 letters per ballot
__global__ __launch_bounds__(256) void k_filter_orient(FilterBarcode B, int forward_only, int n, const uint8_t *__restrict__ seq,
                                                       const long long *__restrict__ off, FilterOut *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((gridDim.x * blockDim.x) >> 6);
  for (int r = wave; r < n; r += nwaves) {
    const long long b = off[r];
    const int L = (int)(off[r + 1] - b);
    int flag = 3;                                              // narrow(x, 1, barlen) on a shorter read
    if (L >= B.len) {
      bool bad_f = false, bad_r = forward_only != 0;
      for (int c0 = 0; c0 < B.len && !(bad_f && bad_r); c0 += 64) {
        const int i = c0 + lane;
        const bool in = i < B.len;
        if (!bad_f) bad_f = __ballot(in && seq[b + i] != B.fwd[i]) != 0ull;            // :653
        if (!bad_r) bad_r = __ballot(in && seq[b + L - 1 - i] != B.comp[i]) != 0ull;   // :652, :654
      }
      flag = !bad_f ? 0 : !bad_r ? 1 : 2;                      // :654 `& !keepF`: both ends match -> as given
    }
    if (lane == 0) out[r].pad = flag;
  }
}

template <bool ORIENT>
void launch_filter_scan_t(const FilterTable &T, const FilterArgs &A, int n, const uint8_t *d_seq, const uint8_t *d_qual,
                          const long long *d_off, FilterOut *d_out, hipStream_t st) {
  if (n <= 0) return;
  const unsigned grid = (unsigned)std::min((n + FT_THREADS / 64 - 1) / (FT_THREADS / 64), 512);
  const size_t lds = (size_t)T.nkeys * 9 + 8;
  if (T.nkeys > 0 && lds <= (size_t)FT_LDS_MAX) {
    // (more than 64 KiB of dynamic LDS has to be asked for, per device; a part that refuses searches global memory)
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)k_filter_scan<true, ORIENT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      hipLaunchKernelGGL((k_filter_scan<false, ORIENT>), dim3(grid), dim3(FT_THREADS), 0, st, T, A, n, d_seq, d_qual, d_off, d_out);
      return;
    }
    hipLaunchKernelGGL((k_filter_scan<true, ORIENT>), dim3(grid), dim3(FT_THREADS), lds, st, T, A, n, d_seq, d_qual, d_off, d_out);
  } else {
    hipLaunchKernelGGL((k_filter_scan<false, ORIENT>), dim3(grid), dim3(FT_THREADS), 0, st, T, A, n, d_seq, d_qual, d_off, d_out);
  }
}
void launch_filter_scan(const FilterTable &T, const FilterArgs &A, int n, const uint8_t *d_seq, const uint8_t *d_qual,
                        const long long *d_off, FilterOut *d_out, hipStream_t st) {
  launch_filter_scan_t<false>(T, A, n, d_seq, d_qual, d_off, d_out, st);
}
void launch_filter_scan_oriented(const FilterTable &T, const FilterArgs &A, int n, const uint8_t *d_seq, const uint8_t *d_qual,
                                 const long long *d_off, FilterOut *d_out, hipStream_t st) {
  launch_filter_scan_t<true>(T, A, n, d_seq, d_qual, d_off, d_out, st);
}
void launch_filter_ee(const FilterArgs &A, int n, const uint8_t *d_qual, const long long *d_off, const double *d_ee_tab, FilterOut *d_out,
                      hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_filter_ee<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, n, d_qual, d_off, d_ee_tab, d_out);
}
void launch_filter_ee_oriented(const FilterArgs &A, int n, const uint8_t *d_qual, const long long *d_off, const double *d_ee_tab,
                               FilterOut *d_out, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_filter_ee<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, n, d_qual, d_off, d_ee_tab, d_out);
}
void launch_filter_kmers(int n, int k, const uint8_t *d_seq, const long long *d_off, const FilterOut *d_out, int32_t *d_counts,
                         hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_filter_kmers<false>, dim3((unsigned)std::min(n, 16384)), dim3(64), 0, st, n, k, d_seq, d_off, d_out, d_counts);
}
void launch_filter_kmers_oriented(int n, int k, const uint8_t *d_seq, const long long *d_off, const FilterOut *d_out, int32_t *d_counts,
                                  hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_filter_kmers<true>, dim3((unsigned)std::min(n, 16384)), dim3(64), 0, st, n, k, d_seq, d_off, d_out, d_counts);
}
void launch_filter_orient(const FilterBarcode &B, int forward_only, int n, const uint8_t *d_seq, const long long *d_off, FilterOut *d_out,
                          hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_filter_orient, dim3((unsigned)std::min((n + 3) / 4, 4096)), dim3(256), 0, st, B, forward_only, n, d_seq, d_off, d_out);
}
