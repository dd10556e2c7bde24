// priors.inc.hip — priors given as sequences, matched against the resident uniques of a sample (names(uniques) %in% c(priors,
// pseudo_priors), R/dada.R:335); included by kernels.hip, inside namespace d2, behind seqkeys.inc.hip (the window key, the key
// mask and the search of a key group).
//
// The host (priors_host.h) packs the prior sequences like the uniques (2-bit words, every row on a 16-byte boundary and zero
// behind its last base), sorts their distinct prefix keys - the first min(32, length) bases - inside key-length groups and lays
// the rows out key by key, the rows of one key in the order the caller gave them.
//   k_prior_match   a lane per resident unique: its prefix key, the group of its key length, the lower bound inside the group -
//                   out of LDS where the keys fit the budget (DADA2HIP_PRIORS_LDS_KEYS), out of global memory otherwise -, then
//                   the rows of an equal key one after the other: equal length, and every word equal under the mask of the
//                   unique's last, partial word (neither side is trusted to be zero behind its last base), read 16 bytes at a time.
//                   The first row that holds is the caller's SMALLEST index of an equal sequence: R's match().
// The flag and, where asked for, the index are plain vector stores, one per lane.

// the bits of word w of a row of L bases that hold bases
__device__ __forceinline__ uint32_t prior_word_mask(int w, int L) {
  const int nw = (L + 15) >> 4, r = L & 15;
  return w < nw - 1 ? ~0u : (w == nw - 1 ? (r ? ((1u << (2 * r)) - 1u) : ~0u) : 0u);
}

// rows a and b (16-byte aligned, at least 4 * ceil(nw / 4) words each) hold the same L bases
__device__ __forceinline__ bool prior_rows_equal(const uint32_t *a, const uint32_t *b, int L) {
  const int nq = (((L + 15) >> 4) + 3) >> 2;
  const uint4 *qa = reinterpret_cast<const uint4 *>(a), *qb = reinterpret_cast<const uint4 *>(b);
  uint32_t diff = 0u;
  for (int c = 0; c < nq && diff == 0u; c++) {
    const uint4 x = qa[c], y = qb[c];
    diff |= (x.x ^ y.x) & prior_word_mask(4 * c, L);
    diff |= (x.y ^ y.y) & prior_word_mask(4 * c + 1, L);
    diff |= (x.z ^ y.z) & prior_word_mask(4 * c + 2, L);
    diff |= (x.w ^ y.w) & prior_word_mask(4 * c + 3, L);
  }
  return diff == 0u;
}

// prior[i] = (or_flags ? or_flags[i] != 0 : 0) | matched; first_match[i] (optional) = the caller's index of the first equal entry, -1
template <bool LDS>
__global__ __launch_bounds__(256) void k_prior_match(int N, int W2, const uint32_t *__restrict__ seq2, const int32_t *__restrict__ len, PriorKeys K,
                                                     const uint8_t *__restrict__ or_flags, uint8_t *__restrict__ prior,
                                                     int32_t *__restrict__ first_match) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_prior_keys[];
  const unsigned long long *keys = K.keys;
  if (LDS) {
    for (int k = (int)threadIdx.x; k < K.nkeys; k += (int)blockDim.x) s_prior_keys[k] = K.keys[k];
    __syncthreads();
    keys = s_prior_keys;
  }
  const long long stride = (long long)gridDim.x * blockDim.x;   // (64-bit: i + stride may pass INT_MAX before the loop ends)
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)N; i += stride) {
    const int L = len[i], kl = min(32, L);
    const uint32_t *row = seq2 + (size_t)i * W2;
    int hit = -1;
    int first = 0, cnt = 0;
    for (int g = 0; g < K.ngroups; g++)
      if (K.groups[3 * g] == kl) { first = K.groups[3 * g + 1]; cnt = K.groups[3 * g + 2]; }
    if (cnt > 0) {
      const unsigned long long w = window_key(row, W2, 0, key_mask(kl));
      const int lo = key_lower_bound(keys, first, cnt, w);
      if (lo < first + cnt && keys[lo] == w)
        for (int r = K.key_row_off[lo]; r < K.key_row_off[lo + 1] && hit < 0; r++)
          if (K.row_len[r] == L && prior_rows_equal(row, K.row_words + (size_t)K.row_woff[r], L)) hit = K.row_seq[r];
    }
    prior[i] = (uint8_t)(((or_flags && or_flags[i]) || hit >= 0) ? 1 : 0);
    if (first_match) first_match[i] = hit;
  }
}

// Returns the blocks launched.  lds: stage the keys in LDS (the caller has checked that they fit); grid_cap: at most that many blocks.
int launch_prior_match(const SampleDev &S, const PriorKeys &K, bool lds, int grid_cap, const uint8_t *d_or_flags, int32_t *d_first_match,
                       hipStream_t st) {
  if (S.N <= 0) return 0;
  const int blocks = std::max(1, std::min((S.N + 255) / 256, grid_cap));
  if (lds)
    hipLaunchKernelGGL(k_prior_match<true>, dim3((unsigned)blocks), dim3(256), (size_t)K.nkeys * 8, st, S.N, S.W2, S.seq2, S.len, K, d_or_flags,
                       S.prior, d_first_match);
  else
    hipLaunchKernelGGL(k_prior_match<false>, dim3((unsigned)blocks), dim3(256), 0, st, S.N, S.W2, S.seq2, S.len, K, d_or_flags, S.prior,
                       d_first_match);
  return blocks;
}
