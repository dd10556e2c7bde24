// derep_dev.inc.hip — the device side of the dereplicator (derepFastq, R/sequenceIO.R:45-183, on reads that are already on the
// device); included by kernels.hip, inside namespace d2, behind readqc.inc.hip.  engine.h: DdState, what outlives a piece, and
// DdPiece, the reads of one.  Integers only: the sums are of raw quality characters, so the order of the adds does not matter.
//
// A piece goes through k_dd_hash once and then through ROUNDS of four launches, until every read has its unique:
//   k_dd_claim    a lane per unsettled read walks from its slot over the slots whose occupant has ANOTHER hash (an occupant with
//                 another hash has other bytes) and stops at the first that is free - which it tries to claim by a compare-and-swap
//                 with its own number, looking at what the swap returns if it lost - or whose occupant has its hash.
//   k_dd_verify   a wave per unsettled read compares its bytes with the occupant's: a unique's in the arena, a claimant's where it
//                 lies in the piece.  Equal: the read has its unique, or its claimant.  Unequal - a true collision of the hash -:
//                 the read moves one slot on and waits for the NEXT round.
//   k_dd_publish  a lane per claimant draws the unique's number and its place in the arena and puts the number in the slot.
//   k_dd_settle   a wave per read settled in this round (r_ref says so; the next round's k_dd_claim clears it): a claimant copies
//                 its bytes into the arena; the count, the smallest read index and the quality characters are added to the
//                 unique's by vector atomics.  No lane reads in a launch what another lane of its wave writes in it.
// A piece with a null `qual` is dereplicated without qualities (seqtab_host.h: the column names of sequence tables): k_dd_hash
// takes no minimum and k_dd_settle adds no quality characters; the branch is uniform over the launch.
// Equality is decided on bytes, never on the hash.  No lane waits for another inside a launch: what a launch needs from another
// lane was written by an EARLIER launch (the hashes, the claims, the numbers), and the one value that changes under a launch, a
// slot going from free to claimed, is only ever acted on through the compare-and-swap's own answer.  Every loop is bounded by the
// table's capacity (the host keeps the table at most half full); a walk that reaches the bound sets ctr->err.
// All reads of a piece with the same bytes start at the same slot and move alike, so they end at the same slot in every round,
// and a unique put in earlier lies in front of the first free slot of its walk: it is found before anything is claimed.

__device__ __forceinline__ unsigned long long dd_mix(unsigned long long x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

constexpr int DD_THREADS = 256, DD_WAVES = DD_THREADS / 64;

// the hash of (length, bytes), the first slot, and the smallest quality character of the reads Auto asks about
__global__ __launch_bounds__(DD_THREADS) void k_dd_hash(DdState T, DdPiece P) {
  const int lane = (int)threadIdx.x & 63, j = (int)blockIdx.x * DD_WAVES + ((int)threadIdx.x >> 6);
  if (j >= P.m) return;                                          // (the same for every lane of the wave)
  const DdRead R = P.rec[j];
  unsigned long long h = 0;
  int mn = 255;
  const bool want_min = P.qual != nullptr && R.idx < P.auto_reads;   // (a piece without qualities: no minimum)
  for (int p = lane; p < R.len; p += 64) {
    h += dd_mix(((unsigned long long)p << 8) | (unsigned long long)P.seq[R.start + p]);
    if (want_min) mn = min(mn, (int)P.qual[R.start + p]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    h += __shfl_xor(h, o, 64);
    mn = min(mn, __shfl_xor(mn, o, 64));
  }
  if (lane != 0) return;
  h = dd_mix(h ^ ((unsigned long long)(unsigned)R.len * 0x9E3779B97F4A7C15ull)) & T.hmask;
  P.r_hash[j] = h;
  P.r_slot[j] = (int)(h & (unsigned long long)(T.cap - 1));
  P.r_uid[j] = R.len > 0 ? DD_PENDING : DD_SKIP;
  P.r_ref[j] = -1;
  if (want_min && mn < 255) atomicMin(&T.ctr->minq, mn);
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_claim(DdState T, DdPiece P) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= P.m) return;
  if (P.r_uid[j] != DD_PENDING) { P.r_ref[j] = -1; return; }     // (settled in an earlier round: k_dd_settle passes it by)
  const unsigned long long h = P.r_hash[j];
  const int mask = T.cap - 1;
  int s = P.r_slot[j];
  for (int step = 0; step < T.cap; step++) {
    int v = T.tab[s];
    if (v == DD_EMPTY) v = atomicCAS(&T.tab[s], DD_EMPTY, -(j + 2));   // (returns what was there: DD_EMPTY when the claim is ours)
    if (v == DD_EMPTY) { P.r_slot[j] = s; return; }
    const unsigned long long hv = v >= 0 ? T.u_hash[v] : P.r_hash[-(v + 2)];
    if (hv == h) { P.r_slot[j] = s; return; }
    s = (s + 1) & mask;
  }
  T.ctr->err = 1;                                                // (a full table: the host never lets it come to that)
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_verify(DdState T, DdPiece P) {
  const int lane = (int)threadIdx.x & 63, j = (int)blockIdx.x * DD_WAVES + ((int)threadIdx.x >> 6);
  if (j >= P.m || P.r_uid[j] != DD_PENDING) return;             // (wave-uniform)
  const DdRead R = P.rec[j];
  const int s = P.r_slot[j], v = T.tab[s];
  if (v == -(j + 2)) { if (lane == 0) P.r_ref[j] = j; return; }  // the claimant itself
  const uint8_t *mine = P.seq + R.start, *other;
  int olen;
  if (v >= 0) { other = T.arena + T.u_off[v]; olen = T.u_len[v]; }
  else if (v <= -2) { const DdRead C = P.rec[-(v + 2)]; other = P.seq + C.start; olen = C.len; }
  else { if (lane == 0) T.ctr->err = 2; return; }                // (a free slot behind the claims: cannot be)
  int differ = olen != R.len;
  if (!differ)
    for (int p = lane; p < R.len; p += 64) differ |= mine[p] != other[p];
  differ = __any(differ);
  if (lane != 0) return;
  if (!differ) {
    P.r_ref[j] = v >= 0 ? -(v + 3) : -(v + 2);                    // an earlier unique v as -(v + 3); or the claimant, for its number
  } else {
    P.r_slot[j] = (s + 1) & (T.cap - 1);                         // a true collision: one slot on, in the next round
    atomicAdd(&T.ctr->pending, 1);
  }
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_publish(DdState T, DdPiece P) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= P.m || P.r_uid[j] != DD_PENDING || P.r_ref[j] != j) return;
  const DdRead R = P.rec[j];
  const int u = atomicAdd(&T.ctr->nuniq, 1);
  const unsigned long long at = atomicAdd(&T.ctr->arena_used, (unsigned long long)R.len);
  T.u_hash[u] = P.r_hash[j]; T.u_off[u] = (long long)at; T.u_len[u] = R.len;
  T.u_count[u] = 0ull; T.u_first[u] = ~0ull;
  T.tab[P.r_slot[j]] = u;
  P.r_uid[j] = u;
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_settle(DdState T, DdPiece P) {
  const int lane = (int)threadIdx.x & 63, j = (int)blockIdx.x * DD_WAVES + ((int)threadIdx.x >> 6);
  if (j >= P.m) return;
  const int ref = P.r_ref[j];
  if (ref == -1) return;                                         // nothing settled for this read in this round (wave-uniform)
  const int u = ref >= 0 ? P.r_uid[ref] : -(ref + 3);            // (a claimant's number is k_dd_publish's)
  const DdRead R = P.rec[j];
  const long long at = T.u_off[u];
  if (ref == j)
    for (int p = lane; p < R.len; p += 64) T.arena[at + p] = P.seq[R.start + p];
  if (P.qual != nullptr && T.sums != nullptr)                    // (wave-uniform; a piece without qualities adds none)
    for (int p = lane; p < R.len; p += 64) atomicAdd(&T.sums[at + p], (unsigned long long)P.qual[R.start + p]);
  if (lane == 0) {
    atomicAdd(&T.u_count[u], 1ull);
    atomicMin(&T.u_first[u], (unsigned long long)R.idx);
    if (ref != j) P.r_uid[j] = u;                                // (no lane of this launch reads it: the next round's k_dd_claim clears r_ref)
  }
}

// every unique into a fresh table: a lane per unique walks from its slot to the first free one it can claim
__global__ __launch_bounds__(DD_THREADS) void k_dd_rebuild(DdState T, int nuniq) {
  const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (u >= nuniq) return;
  const int mask = T.cap - 1;
  int s = (int)(T.u_hash[u] & (unsigned long long)mask);
  for (int step = 0; step < T.cap; step++) {
    if (T.tab[s] == DD_EMPTY && atomicCAS(&T.tab[s], DD_EMPTY, u) == DD_EMPTY) return;
    s = (s + 1) & mask;
  }
  T.ctr->err = 3;
}

void launch_dd_hash(const DdState &T, const DdPiece &P, hipStream_t st) {
  if (P.m <= 0) return;
  hipLaunchKernelGGL(k_dd_hash, dim3((unsigned)((P.m + DD_WAVES - 1) / DD_WAVES)), dim3(DD_THREADS), 0, st, T, P);
}

void launch_dd_round(const DdState &T, const DdPiece &P, hipStream_t st) {
  if (P.m <= 0) return;
  const dim3 per_lane((unsigned)((P.m + DD_THREADS - 1) / DD_THREADS)), per_wave((unsigned)((P.m + DD_WAVES - 1) / DD_WAVES));
  hipLaunchKernelGGL(k_dd_claim, per_lane, dim3(DD_THREADS), 0, st, T, P);
  hipLaunchKernelGGL(k_dd_verify, per_wave, dim3(DD_THREADS), 0, st, T, P);
  hipLaunchKernelGGL(k_dd_publish, per_lane, dim3(DD_THREADS), 0, st, T, P);
  hipLaunchKernelGGL(k_dd_settle, per_wave, dim3(DD_THREADS), 0, st, T, P);
}

void launch_dd_rebuild(const DdState &T, int nuniq, hipStream_t st) {
  if (nuniq <= 0) return;
  hipLaunchKernelGGL(k_dd_rebuild, dim3((unsigned)((nuniq + DD_THREADS - 1) / DD_THREADS)), dim3(DD_THREADS), 0, st, T, nuniq);
}
