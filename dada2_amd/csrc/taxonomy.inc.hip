// taxonomy.inc.hip — the device side of assignTaxonomy (src/taxonomy.cpp:73-110 get_best_genus, :153-197 the per-query loop);
// included by kernels.hip, inside namespace d2.
//
// The reference makes, per query, 101 passes over every genus (the full k-mer array, then 100 bootstrap replicates of an eighth
// of it), each a gather-and-sum of float log-probabilities out of lgk[genus][kmer], and keeps the genus with the largest sum.
// Here the table lies transposed, T[kmer][genus padded to 64] (taxonomy_host.h), so the 64 lanes of a wave read 64 consecutive
// genera of one k-mer in one 256-byte access, and a block owns one (query, tile of 64 genera):
//   k_tax_sums<true>   stages the slab S[pos][lane] = T[karray[pos]][genus] of the query's k-mers in LDS once and sums all passes
//                      out of it: the table is read from memory once per query and tile, not 13.5 times
//   k_tax_sums<false>  gathers every addend straight from T (queries whose slab, arraylen x 256 B, does not fit the LDS budget)
//   k_tax_combine      folds the per-tile records of a (query, pass) into its maximum, the size of its tied set and its winner
// A lane adds its genus's terms ONE AFTER THE OTHER in float, in the reference's order (sorted k-mers for the full pass, draw
// order for a replicate): the sums are the reference's bits.  Its early exit (:93) is not needed for that: every addend is <= 0,
// so a partial sum below the running maximum stays below it.  Ties at the maximum go to the genus with the smallest 32-bit hash
// of (seed, query, pass, genus), the genus index breaking equal hashes - uniform over the tied set, the same whatever the tiling
// or the order of the reduction.

__host__ __device__ __forceinline__ uint32_t tax_fmix(uint32_t h) {   // (the finaliser of MurmurHash3: public domain)
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
// hash of (seed, query, pass), to be folded with the genus by tax_hash_genus
__host__ __device__ __forceinline__ uint32_t tax_hash_pass(uint32_t seed_lo, uint32_t seed_hi, uint32_t query, uint32_t pass) {
  uint32_t h = tax_fmix(seed_lo ^ 0x9E3779B9u);
  h = tax_fmix(h ^ seed_hi);
  h = tax_fmix(h ^ query);
  return tax_fmix(h ^ pass);
}
__host__ __device__ __forceinline__ uint32_t tax_hash_genus(uint32_t hpass, uint32_t genus) { return tax_fmix(hpass ^ genus); }

// One block per (query, tile): blockIdx.x = query * ntiles + tile; lane = genus of the tile; the waves of the block take the passes
// in turn.  part[(query * npass + pass) * ntiles + tile] = {max sum of the tile, genera of the tile at it, hash and genus of the
// tile's winner}.  Dynamic LDS (SLAB): 256 B per k-mer of the longest query of the launch.
template <bool SLAB>
__global__ __launch_bounds__(TAX_THREADS) void k_tax_sums(TaxJob J) {
  extern __shared__ float tax_slab[];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6), nwave = (int)(blockDim.x >> 6);
  const int q = (int)(blockIdx.x / (unsigned)J.ntiles), tile = (int)(blockIdx.x - (unsigned)q * (unsigned)J.ntiles);
  const int k0 = J.koff[q], A = J.koff[q + 1] - k0, n8 = A >> 3;
  const uint16_t *ka = J.karr + k0;
  const int g = tile * 64 + lane;                       // (< gpad: the padding columns are there, and never win)
  const float *Tg = J.T + g;
  if (SLAB) {
    for (int pos = wave; pos < A; pos += nwave) tax_slab[pos * 64 + lane] = Tg[(size_t)ka[pos] * J.gpad];
    __syncthreads();
  }
  const uint16_t *bp = J.npass > 1 ? J.bpos + J.boff[q] : nullptr;
  const bool valid = g < J.ngenus;
  for (int p = wave; p < J.npass; p += nwave) {
    float s = 0.0f;
    if (p == 0) {
      for (int pos = 0; pos < A; pos++) s += SLAB ? tax_slab[pos * 64 + lane] : Tg[(size_t)ka[pos] * J.gpad];
    } else {
      const uint16_t *b = bp + (size_t)(p - 1) * n8;
      for (int i = 0; i < n8; i++) {
        const int pos = b[i];
        s += SLAB ? tax_slab[pos * 64 + lane] : Tg[(size_t)ka[pos] * J.gpad];
      }
    }
    float m = valid ? s : -INFINITY;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const bool tied = valid && s == m;
    const int ntie = __popcll(__ballot(tied));
    const uint32_t hp = tax_hash_pass(J.seed_lo, J.seed_hi, (uint32_t)J.qid[q], (uint32_t)p);
    unsigned long long key = tied ? (((unsigned long long)tax_hash_genus(hp, (uint32_t)g)) << 32) | (uint32_t)g : ~0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other < key ? other : key;
    }
    if (lane == 0) {
      TaxPart r;
      r.maxlogp = m; r.ntie = ntie; r.hash = (uint32_t)(key >> 32); r.genus = (int32_t)(uint32_t)key;
      J.part[((size_t)q * J.npass + p) * J.ntiles + tile] = r;
    }
  }
}

// one thread per (query, pass)
__global__ __launch_bounds__(256) void k_tax_combine(TaxJob J) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)J.nq * J.npass) return;
  const TaxPart *p = J.part + idx * J.ntiles;
  TaxPart best = p[0];
  for (int t = 1; t < J.ntiles; t++) {
    const TaxPart r = p[t];
    if (r.maxlogp > best.maxlogp) best = r;
    else if (r.maxlogp == best.maxlogp) {
      const int n = best.ntie + r.ntie;
      if (r.hash < best.hash || (r.hash == best.hash && r.genus < best.genus)) best = r;
      best.ntie = n;
    }
  }
  J.best[idx] = best.maxlogp; J.ntie[idx] = best.ntie; J.winner[idx] = best.genus;
}

// slab_positions > 0: the slab instance, with LDS for that many k-mers (every query of the job has at most as many); 0: the gather
// instance.  Returns false where the device does not take the slab's LDS (the caller then sends the job to the gather instance).
bool launch_tax_sums(const TaxJob &J, int slab_positions, hipStream_t st) {
  if (J.nq <= 0) return true;
  const dim3 grid((unsigned)((size_t)J.nq * J.ntiles)), block(TAX_THREADS);
  if (slab_positions > 0) {
    const size_t lds = (size_t)slab_positions * 256;
    static size_t attr_set[64] = {0};
    int dev_ = 0;
    (void)hipGetDevice(&dev_);
    if (lds > attr_set[dev_ & 63]) {
      if (hipFuncSetAttribute((const void *)k_tax_sums<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      attr_set[dev_ & 63] = lds;
    }
    hipLaunchKernelGGL(k_tax_sums<true>, grid, block, lds, st, J);
  } else {
    hipLaunchKernelGGL(k_tax_sums<false>, grid, block, 0, st, J);
  }
  return true;
}
void launch_tax_combine(const TaxJob &J, hipStream_t st) {
  const size_t n = (size_t)J.nq * J.npass;
  if (n == 0) return;
  hipLaunchKernelGGL(k_tax_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, J);
}
