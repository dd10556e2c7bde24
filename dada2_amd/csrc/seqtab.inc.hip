// seqtab.inc.hip — the device side of mergeSequenceTables (R/multiSample.R:290-364); included by kernels.hip, inside namespace d2,
// behind derep_dev.inc.hip, whose table, arena and per-unique words it reads.  The column names of all tables have gone through
// the dereplicator without qualities (seqtab_host.h), so a unique is a distinct sequence and u_first its first appearance.
//   k_st_rc          a wave per unique looks its reverse complement up in the table, which no launch changes any more
//   k_st_accumulate  a lane per cell of one table adds it into the merged matrix at (row map, column map)
//   k_st_colkeys     the 64-bit sum and the number of positive cells of every merged column
//   k_st_gather      the merged matrix with its columns in the final order
// The rule in front of derep_dev.inc.hip holds here: equality is decided on bytes, no lane waits for another, every loop is bounded.
// Integers only; the adds are order-free.

constexpr int ST_THREADS = 256, ST_WAVES = ST_THREADS / 64;
constexpr int ST_GRID_Y = 32768;              // rows of a launch's second dimension; a block walks the rows beyond in steps of it
constexpr int ST_KEY_ROWS = 256;              // rows per block of k_st_colkeys

// The hash of a string is a sum over its positions (k_dd_hash), so the reverse complement's needs no second string: the lane that
// holds position p adds the term of position len - 1 - p with the complemented byte.
__global__ __launch_bounds__(ST_THREADS) void k_st_rc(DdState T, int nuniq, const uint8_t *__restrict__ comp, int32_t *__restrict__ partner,
                                                      StCounters *ctr) {
  const int lane = (int)threadIdx.x & 63, u = (int)blockIdx.x * ST_WAVES + ((int)threadIdx.x >> 6);
  if (u >= nuniq) return;                                        // (the same for every lane of the wave)
  const int len = T.u_len[u];
  const uint8_t *mine = T.arena + T.u_off[u];
  unsigned long long h = 0;
  int bad = 0;
  for (int p = lane; p < len; p += 64) {
    const unsigned c = comp[mine[p]];
    bad |= c == 0u;
    h += dd_mix(((unsigned long long)(len - 1 - p) << 8) | (unsigned long long)c);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) h += __shfl_xor(h, o, 64);
  if (__any(bad)) {                                              // a letter without a complement: the host names the column
    if (lane == 0) { partner[u] = -1; atomicMin(&ctr->bad_first, T.u_first[u]); atomicOr(&ctr->err, (int)ST_ERR_LETTER); }
    return;
  }
  h = dd_mix(h ^ ((unsigned long long)(unsigned)len * 0x9E3779B97F4A7C15ull)) & T.hmask;
  const int mask = T.cap - 1;
  int s = (int)(h & (unsigned long long)mask), found = -1, fails = 0, step = 0;
  for (; step < T.cap; step++) {
    const int v = T.tab[s];                                      // (one address for the wave, and nothing writes the table: wave-uniform)
    if (v < 0) break;                                            // a free slot ends the walk (no claim outlives its round)
    if (T.u_hash[v] == h) {
      if (T.u_len[v] == len) {
        const uint8_t *other = T.arena + T.u_off[v];             // the occupant forward against this unique backward and complemented
        int differ = 0;
        for (int p = lane; p < len; p += 64) differ |= other[p] != comp[mine[len - 1 - p]];
        if (!__any(differ)) { found = v; break; }
        fails++;
      }
    }
    s = (s + 1) & mask;
  }
  if (lane != 0) return;
  partner[u] = found;
  if (fails) atomicAdd(&ctr->rc_fails, (unsigned long long)fails);
  if (step >= T.cap) atomicOr(&ctr->err, (int)ST_ERR_WALK);      // (a full table: the host keeps it at most half full)
}

// Cells collide only where two rows or two columns of the inputs share a target.  The add that takes a cell past INT32_MAX sees
// it in what the add returns, and every add behind it finds the cell negative.
__global__ __launch_bounds__(ST_THREADS) void k_st_accumulate(const int32_t *__restrict__ cells, int nrow, int ncol,
                                                              const int32_t *__restrict__ row_map, const int32_t *__restrict__ col_map,
                                                              int32_t *merged, long long out_cols, StCounters *ctr) {
  const long long c = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (c >= ncol) return;
  const long long dc = col_map[c];
  for (long long r = blockIdx.y; r < nrow; r += gridDim.y) {
    const int32_t v = cells[r * ncol + c];
    if (v <= 0) continue;                                        // (the host has refused negative cells)
    const int32_t old = atomicAdd(&merged[(long long)row_map[r] * out_cols + dc], v);
    if (old < 0 || old > INT32_MAX - v) atomicOr(&ctr->err, (int)ST_ERR_OVERFLOW);
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_st_colkeys(const int32_t *__restrict__ merged, long long nrow, long long ncol,
                                                           unsigned long long *sum, int32_t *npos) {
  const long long c = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (c >= ncol) return;
  unsigned long long s = 0;
  int n = 0;
  for (long long r0 = (long long)blockIdx.y * ST_KEY_ROWS; r0 < nrow; r0 += (long long)gridDim.y * ST_KEY_ROWS) {
    const long long r1 = r0 + ST_KEY_ROWS < nrow ? r0 + ST_KEY_ROWS : nrow;
    for (long long r = r0; r < r1; r++) {
      const int32_t v = merged[r * ncol + c];
      s += (unsigned long long)v;
      n += v > 0;
    }
  }
  if (s) atomicAdd(&sum[c], s);
  if (n) atomicAdd(&npos[c], n);
}

// a block writes 256 neighbouring cells of a row: the writes are coalesced, the reads follow the order inside that row
__global__ __launch_bounds__(ST_THREADS) void k_st_gather(const int32_t *__restrict__ merged, long long nrow, long long ncol,
                                                          const int32_t *__restrict__ order, int32_t *__restrict__ out) {
  const long long k = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (k >= ncol) return;
  const long long from = order[k];
  for (long long r = blockIdx.y; r < nrow; r += gridDim.y) out[r * ncol + k] = merged[r * ncol + from];
}

void launch_st_rc(const DdState &T, int nuniq, const uint8_t *d_comp, int32_t *d_partner, StCounters *d_ctr, hipStream_t st) {
  if (nuniq <= 0) return;
  hipLaunchKernelGGL(k_st_rc, dim3((unsigned)((nuniq + ST_WAVES - 1) / ST_WAVES)), dim3(ST_THREADS), 0, st, T, nuniq, d_comp, d_partner, d_ctr);
}

void launch_st_accumulate(const int32_t *d_cells, int nrow, int ncol, const int32_t *d_row_map, const int32_t *d_col_map, int32_t *d_merged,
                          long long out_cols, StCounters *d_ctr, hipStream_t st) {
  if (nrow <= 0 || ncol <= 0) return;
  const dim3 grid((unsigned)((ncol + ST_THREADS - 1) / ST_THREADS), (unsigned)std::min(nrow, ST_GRID_Y));
  hipLaunchKernelGGL(k_st_accumulate, grid, dim3(ST_THREADS), 0, st, d_cells, nrow, ncol, d_row_map, d_col_map, d_merged, out_cols, d_ctr);
}

void launch_st_colkeys(const int32_t *d_merged, long long nrow, long long ncol, unsigned long long *d_sum, int32_t *d_npos, hipStream_t st) {
  if (nrow <= 0 || ncol <= 0) return;
  const dim3 grid((unsigned)((ncol + ST_THREADS - 1) / ST_THREADS), (unsigned)std::min<long long>((nrow + ST_KEY_ROWS - 1) / ST_KEY_ROWS, ST_GRID_Y));
  hipLaunchKernelGGL(k_st_colkeys, grid, dim3(ST_THREADS), 0, st, d_merged, nrow, ncol, d_sum, d_npos);
}

void launch_st_gather(const int32_t *d_merged, long long nrow, long long ncol, const int32_t *d_order, int32_t *d_out, hipStream_t st) {
  if (nrow <= 0 || ncol <= 0) return;
  const dim3 grid((unsigned)((ncol + ST_THREADS - 1) / ST_THREADS), (unsigned)std::min<long long>(nrow, ST_GRID_Y));
  hipLaunchKernelGGL(k_st_gather, grid, dim3(ST_THREADS), 0, st, d_merged, nrow, ncol, d_order, d_out);
}
