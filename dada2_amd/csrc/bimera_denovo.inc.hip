// bimera_denovo.inc.hip — isBimeraDenovo on a resident lite sample (R/chimeras.R:105-154, C_is_bimera: src/chimera.cpp:18-59);
// included by kernels.hip, inside namespace d2, behind priors.inc.hip.
//
// The host (bimera_denovo_host.h, bimera_plain.h) ranks the sequences of one row of abundances (descending) and gives every query
// j one integer: its parents are the ranks [0, P[j]).  The parents are visited in windows of ranks, most abundant first; between
// the host and the device go the ranking and P once per row, one word per window and n flag bytes at the end.
//   k_bimera_worklist  a lane per work slot of a launch: nq live queries x wr ranks from rank r0.  Slot (q, r) names the parent
//                      rank[r] while r < P[q] and q is not flagged yet, -1 otherwise; every `per` slots - one chunk of the
//                      aligner, all of one query - get the query as their chunk centre.  These are the d_chunk_centre / d_work
//                      arrays of the bimera-mode aligners (launch_nw_ad_lr; launch_nw + launch_bimera_lr), which leave five words
//                      per slot: left, right, left_oo, right_oo, hamming.
//   k_bimera_fold      a wave per live query of the launch: its wr slots reduced to six maxima (chimera.cpp:29-41: a parent with
//                      left + right >= len is tossed; the one-off maxima take parents of hamming >= min_one_off_par_dist only),
//                      merged into the query's running maxima in device memory, the three completion tests (:44-50), the flag
//                      byte.  On the window's last launch over these queries (`last`) the queries still unflagged with ranks
//                      left behind the window go into the next window's live list, whose length is counted up in *n_next.
// The maxima only grow, so the order of the parents and the early stop of the reference's loop (:25) do not change an answer.
// Every store is a plain vector store or an atomic add of one lane.

__global__ __launch_bounds__(256) void k_bimera_worklist(const int32_t *__restrict__ live, int nq, int r0, int wr, int per,
                                                         const int32_t *__restrict__ rank, const int32_t *__restrict__ P,
                                                         const uint8_t *__restrict__ flags, int32_t *__restrict__ chunk_centre,
                                                         int32_t *__restrict__ work) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)nq * wr) return;
  const int ql = (int)(t / wr), o = (int)(t - (long long)ql * wr);
  const int q = live[ql], r = r0 + o;
  work[t] = (r < P[q] && !flags[q]) ? rank[r] : -1;
  if (o % per == 0) chunk_centre[t / per] = q;
}

__global__ __launch_bounds__(256) void k_bimera_fold(BimeraFold F) {
  const int lane = (int)(threadIdx.x & 63);
  const int ql = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (ql >= F.nq) return;                                      // (wave-uniform)
  const int q = F.live[ql], L = F.len[q];
  int m[6] = {0, 0, 0, 0, 0, 0}, cnt = 0;
  for (int o = lane; o < F.wr; o += 64) {
    const size_t slot = (size_t)ql * F.wr + o;
    if (F.work[slot] < 0) continue;
    cnt++;
    const int32_t *b = F.rec + slot * 5;
    const int left = b[0], right = b[1];
    if (left + right >= L) continue;                           // id / pure-shift / internal-indel "parents"
    m[0] = max(m[0], left); m[1] = max(m[1], right);
    if (F.allow_one_off && b[4] >= F.min_one_off_par_dist) {
      m[2] = max(m[2], left); m[3] = max(m[3], right);
      m[4] = max(m[4], b[2]); m[5] = max(m[5], b[3]);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int k = 0; k < 6; k++) m[k] = max(m[k], __shfl_xor(m[k], d, 64));
    cnt += __shfl_xor(cnt, d, 64);
  }
  if (lane != 0) return;
  int32_t *run = F.maxima + (size_t)q * 6;
#pragma unroll
  for (int k = 0; k < 6; k++) { m[k] = max(m[k], run[k]); run[k] = m[k]; }
  bool bim = F.flags[q] != 0;
  if (m[0] + m[1] >= L) bim = true;
  if (F.allow_one_off && (m[2] + m[5] >= L || m[4] + m[3] >= L)) bim = true;
  F.flags[q] = bim ? 1 : 0;
  if (cnt) atomicAdd(F.aligned, (unsigned long long)cnt);
  if (F.last && !bim && F.P[q] > F.r0 + F.wr) F.next_live[atomicAdd(F.n_next, 1)] = q;
}

void launch_bimera_worklist(const int32_t *d_live, int nq, int r0, int wr, int per, const int32_t *d_rank, const int32_t *d_P,
                            const uint8_t *d_flags, int32_t *d_chunk_centre, int32_t *d_work, hipStream_t st) {
  const long long n = (long long)nq * wr;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_bimera_worklist, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_live, nq, r0, wr, per, d_rank, d_P, d_flags,
                     d_chunk_centre, d_work);
}

void launch_bimera_fold(const BimeraFold &F, hipStream_t st) {
  if (F.nq <= 0) return;
  hipLaunchKernelGGL(k_bimera_fold, dim3((unsigned)((F.nq + 3) / 4)), dim3(256), 0, st, F);
}
