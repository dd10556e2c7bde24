// species.inc.hip — the device side of assignSpecies (R/taxonomy.R:264-280: PDict + vcountPDict > 0 per chunk of equal-length
// queries, a second time over the reverse complements with tryRC); included by kernels.hip, inside namespace d2, behind
// seqkeys.inc.hip (bases16, the window key and the search of a key group).
//
// The reference asks, for every (query, reference) pair, "does the query occur in the reference as a substring", fixed = TRUE:
// a reference position with any letter other than upper-case A/C/G/T matches nothing.  Here the references are resident
// (species_host.h: 2-bit words, a 1-bit plane of the other letters, every row starting on a 32-base boundary) and a call is
//   k_species_bitmap  two bits per prefix key (the first min(length, 32) bases of a pattern as a 64-bit word, k_collapse_join's
//                     key form) at two hashes of the key, in a 32 KB presence bitmap
//   k_species_seed    a wave per reference, a lane per window position: the window's key, dropped where it touches the plane or
//                     would run past the end of ITS reference, is looked up in the bitmap - staged in LDS, so the miss, which is
//                     almost every window, costs no trip to memory - and only the survivors search the sorted keys (through L2:
//                     at most 2 x the query chunk of 8-byte words).  A hit appends (reference, position, key) to the candidate
//                     buffer, one atomic add per wave; every hit is COUNTED, only what fits is stored (the host re-runs the range
//                     in pieces, species_host.h)
//   k_species_verify  a thread per candidate, over the patterns that carry its key (CSR): the span inside the reference, no plane
//                     bit over the whole span, bases 32.. equal word by word -> (query, reference), counted and stored likewise
// The host sorts the pairs and drops repeats: several positions, or both strands, in one reference are one hit.

__device__ __forceinline__ uint32_t sp_hash(unsigned long long key, int kl) {
  uint32_t h = (uint32_t)key * 0x9E3779B1u ^ (uint32_t)(key >> 32) * 0x85EBCA6Bu ^ (uint32_t)kl * 0xC2B2AE35u;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
  return h;
}
// the two bits of a key in the bitmap (a Bloom filter of two probes: at 10 000 keys 0.5 % of the misses get past it, with one
// probe 3.7 % - and a wave waits for the search of its survivors if any of its 64 lanes has one)
__device__ __forceinline__ uint32_t sp_bit_a(uint32_t h) { return h >> (32 - SP_BITMAP_LOG2); }
__device__ __forceinline__ uint32_t sp_bit_b(uint32_t h) { return (h * 0x45D9F3B5u) >> (32 - SP_BITMAP_LOG2); }
// 32 bits of the plane from bit b on (the plane is padded by two words behind the last row)
__device__ __forceinline__ uint32_t sp_bits32(const uint32_t *plane, long long b) {
  const long long w = b >> 5;
  return (uint32_t)(((((uint64_t)plane[w + 1]) << 32) | plane[w]) >> (int)(b & 31));
}

// one thread per key; bitmap[SP_BITMAP_WORDS] preset to 0
__global__ __launch_bounds__(256) void k_species_bitmap(SpeciesKeys K, uint32_t *__restrict__ bitmap) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= K.nkeys) return;
  int kl = 0;
  for (int g = 0; g < K.ngroups; g++)
    if (i >= K.groups[3 * g + 1] && i < K.groups[3 * g + 1] + K.groups[3 * g + 2]) kl = K.groups[3 * g];
  const uint32_t h = sp_hash(K.keys[i], kl), a = sp_bit_a(h), b = sp_bit_b(h);
  atomicOr(&bitmap[a >> 5], 1u << (a & 31));
  atomicOr(&bitmap[b >> 5], 1u << (b & 31));
}

// References [r0, r1).  counters: [0] candidates (all of them, stored or not), [1] windows looked up, [2] windows past the bitmap.
__global__ __launch_bounds__(256) void k_species_seed(SpeciesRefs R, int r0, int r1, SpeciesKeys K, const uint32_t *__restrict__ bitmap,
                                                       SpCand *__restrict__ cand, unsigned long long cap, unsigned long long *counters) {
  __shared__ uint32_t s_bm[SP_BITMAP_WORDS];
  for (int i = (int)threadIdx.x; i < SP_BITMAP_WORDS; i += (int)blockDim.x) s_bm[i] = bitmap[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((gridDim.x * blockDim.x) >> 6);
  unsigned long long nwin = 0, npast = 0;
  for (int r = r0 + wave; r < r1; r += nwaves) {
    const int L = R.len[r], nw = (L + 15) >> 4;
    const long long wo = R.woff[r];
    const uint32_t *row = R.words + wo;
    for (int g = 0; g < K.ngroups; g++) {
      const int kl = K.groups[3 * g], first = K.groups[3 * g + 1], cnt = K.groups[3 * g + 2];
      const unsigned long long mask = key_mask(kl);
      const uint32_t pmask = kl >= 32 ? ~0u : ((1u << kl) - 1u);
      const int npos = L - kl + 1;                           // windows that end inside this reference
      for (int p0 = 0; p0 < npos; p0 += 64) {                // (uniform over the wave: the ballot below is taken by all lanes)
        const int p = p0 + lane;
        bool hit = false;
        int ki = 0;
        if (p < npos && (sp_bits32(R.nplane, wo * 16 + p) & pmask) == 0u) {
          nwin++;
          const unsigned long long w = window_key(row, nw, p, mask);
          const uint32_t h = sp_hash(w, kl), ba = sp_bit_a(h), bb = sp_bit_b(h);
          if ((s_bm[ba >> 5] >> (ba & 31)) & (s_bm[bb >> 5] >> (bb & 31)) & 1u) {
            npast++;
            const int lo = key_lower_bound(K.keys, first, cnt, w);
            hit = lo < first + cnt && K.keys[lo] == w;
            ki = lo;
          }
        }
        const unsigned long long b = __ballot(hit);
        if (b != 0ull) {
          unsigned long long base = 0;
          if (lane == 0) base = atomicAdd(&counters[0], (unsigned long long)__popcll(b));
          base = __shfl(base, 0, 64);
          const unsigned long long i = base + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
          if (hit && i < cap) { SpCand c; c.ref = r; c.pos = p; c.key = ki; cand[i] = c; }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { nwin += __shfl_xor(nwin, o, 64); npast += __shfl_xor(npast, o, 64); }
  if (lane == 0 && nwin != 0ull) { atomicAdd(&counters[1], nwin); atomicAdd(&counters[2], npast); }
}

// One thread per candidate.  counters[3]: the (query, reference) pairs found (all of them); hits[i] = query << 32 | reference for
// the first hit_cap.
__global__ __launch_bounds__(256) void k_species_verify(SpeciesRefs R, SpeciesKeys K, const SpCand *__restrict__ cand, unsigned long long ncand,
                                                         unsigned long long *__restrict__ hits, unsigned long long hit_cap,
                                                         unsigned long long *counters) {
  const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncand) return;
  const SpCand c = cand[idx];
  const int L = R.len[c.ref], nw = (L + 15) >> 4;
  const long long wo = R.woff[c.ref];
  const uint32_t *row = R.words + wo;
  for (int j = K.key_pat_off[c.key]; j < K.key_pat_off[c.key + 1]; j++) {
    const int pt = K.key_pats[j], pl = K.pat_len[pt];
    if ((long long)c.pos + pl > (long long)L) continue;
    bool ok = true;
    for (int o = 0; o < pl && ok; o += 32) {                 // the plane over the whole span
      const int n = min(32, pl - o);
      ok = (sp_bits32(R.nplane, wo * 16 + c.pos + o) & (n >= 32 ? ~0u : ((1u << n) - 1u))) == 0u;
    }
    const uint32_t *pw = K.pat_words + K.pat_woff[pt];
    for (int o = 32; o < pl && ok; o += 16) {                // bases 32.. (the key is bases 0..31)
      const int n = min(16, pl - o);
      ok = ((pw[o >> 4] ^ bases16(row, nw, c.pos + o)) & (n >= 16 ? ~0u : ((1u << (2 * n)) - 1u))) == 0u;
    }
    if (ok) {
      const unsigned long long i = atomicAdd(&counters[3], 1ull);
      if (i < hit_cap) hits[i] = (((unsigned long long)(uint32_t)K.pat_query[pt]) << 32) | (uint32_t)c.ref;
    }
  }
}

void launch_species_bitmap(const SpeciesKeys &K, uint32_t *d_bitmap, hipStream_t st) {
  if (K.nkeys <= 0) return;
  hipLaunchKernelGGL(k_species_bitmap, dim3((unsigned)((K.nkeys + 255) / 256)), dim3(256), 0, st, K, d_bitmap);
}
void launch_species_seed(const SpeciesRefs &R, int r0, int r1, const SpeciesKeys &K, const uint32_t *d_bitmap, SpCand *d_cand,
                         unsigned long long cap, unsigned long long *d_counters, hipStream_t st) {
  if (r1 <= r0 || K.ngroups <= 0) return;
  hipLaunchKernelGGL(k_species_seed, dim3((unsigned)std::min((r1 - r0 + 3) / 4, 2048)), dim3(256), 0, st, R, r0, r1, K, d_bitmap, d_cand,
                     cap, d_counters);
}
void launch_species_verify(const SpeciesRefs &R, const SpeciesKeys &K, const SpCand *d_cand, unsigned long long ncand,
                           unsigned long long *d_hits, unsigned long long hit_cap, unsigned long long *d_counters, hipStream_t st) {
  if (ncand == 0) return;
  hipLaunchKernelGGL(k_species_verify, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, st, R, K, d_cand, ncand, d_hits, hit_cap,
                     d_counters);
}
