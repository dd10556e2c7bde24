// merge.inc.hip — the device side of the run-level mergePairs (R/paired.R:92-201; merge_host.h); included by kernels.hip, inside
// namespace d2.  The alignments themselves are k_nw_gen<pair>'s, unchanged; what is here stands in front of and behind them.
//   k_mp_tally      a lane per read pair of one sample: f = dadaF.map[derepF.map[i]], r likewise, the pair (f, r) counted in the
//                   sample's table with its first read (unique(pairdf) and table(), :125 and :175)
//   k_mp_compact    the occupied slots of the table as records, in no order (the host orders a sample's few thousand)
//   k_mp_eval       a wave per unique pair on the move string the aligner left on the device: C_eval_pair's three counts
//                   (evaluate.cpp:73-114, restated in evalpair.h), prefer and accept (:165-166), the merged length
//   k_mp_consensus  a wave per accepted pair: C_pair_consensus (evaluate.cpp:124-174) into the chunk's arena
// No lane waits for another: a key is claimed with one compare-and-swap and is final from then on, counts are integer adds, first
// reads integer minima - every order of arrival gives the same table.  Every loop is bounded.
//
// A move string is recorded from the END of the alignment backwards: column c of n is moves[n - 1 - c]; 1 is a diagonal move (a
// base of each string), 2 a gap in the forward string (a base of the reverse one alone), 3 a gap in the reverse string.

constexpr int MP_THREADS = 256, MP_WAVES = MP_THREADS / 64;

__device__ __forceinline__ unsigned long long mp_mix(unsigned long long x) {   // (splitmix64's finaliser)
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// One key, n read pairs, the first of them: walk from the key's slot to the key or to a free slot that the swap makes the key's.
__device__ __forceinline__ void mp_insert(const MpTable &T, unsigned long long k, int n, int first, MpCounters *ctr) {
  const long long mask = T.cap - 1;
  long long s = (long long)(mp_mix(k) & T.hmask) & mask, step = 0;
  for (; step < T.cap; step++) {
    unsigned long long cur = T.key[s];                            // (a key never changes once set: a stale MP_EMPTY is what the swap settles)
    if (cur == MP_EMPTY) {
      cur = atomicCAS(&T.key[s], MP_EMPTY, k);
      if (cur == MP_EMPTY) cur = k;
    }
    if (cur == k) {
      atomicAdd(&T.count[s], n);
      atomicMin(&T.first[s], (uint32_t)first);
      break;
    }
    s = (s + 1) & mask;
  }
  if (step) atomicAdd(&ctr->collisions, (unsigned long long)step);
  if (step >= T.cap) atomicOr(&ctr->err, (int)MP_ERR_FULL);       // (a full table: the host keeps it at most half full)
}

// The top pair of a real sample is a large share of its reads, so the lanes of a wave that hold one key send ONE insert: the wave
// takes the key of its first unserved lane, ballots who shares it, and that lane - whose read is the smallest of them - inserts
// the group.  As many trips as the wave has distinct keys.
__global__ __launch_bounds__(MP_THREADS) void k_mp_tally(MpSample S, MpTable T, MpCounters *ctr) {
  const int lane = (int)threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * MP_THREADS + threadIdx.x;
  const bool mine = i < S.nreads;
  int f = 0, r = 0, uf = -1, ur = -1, bad = MP_BAD_NONE;          // f, r: 0 is NA
  if (mine) {
    uf = S.derepF[i]; ur = S.derepR[i];                           // (negative: NA, whatever the value)
    if (uf >= S.nuniqF) bad = MP_BAD_DEREP_F;
    else if (ur >= S.nuniqR) bad = MP_BAD_DEREP_R;
    else {
      const int vf = uf >= 0 ? S.dadaF[uf] : 0, vr = ur >= 0 ? S.dadaR[ur] : 0;   // (<= 0: NA)
      if (vf > S.nclustF) bad = MP_BAD_DADA_F;
      else if (vr > S.nclustR) bad = MP_BAD_DADA_R;
      else { f = vf > 0 ? vf : 0; r = vr > 0 ? vr : 0; }
    }
    if (bad) atomicMin(&ctr->bad_first, ((unsigned long long)i << 3) | (unsigned long long)bad);
  }
  int mf = uf < 0 ? -1 : uf, mr = ur < 0 ? -1 : ur;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { mf = max(mf, __shfl_xor(mf, o, 64)); mr = max(mr, __shfl_xor(mr, o, 64)); }
  const bool live = mine && !bad && f > 0 && r > 0;
  const unsigned long long dropped = __ballot(mine && !bad && !live);
  if (lane == 0) {
    if (mf >= 0) atomicMax(&ctr->max_f, mf);
    if (mr >= 0) atomicMax(&ctr->max_r, mr);
    if (dropped) atomicAdd(&ctr->na, (unsigned long long)__popcll(dropped));
  }
  const unsigned long long key = ((unsigned long long)(unsigned)f << 32) | (unsigned long long)(unsigned)r;
  unsigned long long todo = __ballot(live);
  while (todo) {                                                  // (wave-uniform)
    const int leader = __builtin_ctzll(todo);
    const unsigned long long k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(live && key == k);
    if (lane == leader) mp_insert(T, k, __popcll(same), (int)i, ctr);
    todo &= ~same;
  }
}

__global__ __launch_bounds__(MP_THREADS) void k_mp_compact(MpTable T, MpRec *rec, int max_rec, MpCounters *ctr) {
  const long long s = (long long)blockIdx.x * MP_THREADS + threadIdx.x;
  if (s >= T.cap) return;
  const unsigned long long k = T.key[s];
  if (k == MP_EMPTY) return;
  const int at = atomicAdd(&ctr->nrec, 1);
  if (at >= max_rec) { atomicOr(&ctr->err, (int)MP_ERR_RECORDS); return; }
  rec[at].key = k; rec[at].count = T.count[s]; rec[at].first = (int32_t)T.first[s];
}

// What both kernels below know of a pair.  The run of one gap kind at either end of the alignment is what C_eval_pair steps over:
// `start` columns of the kind of column 0 in front, `trail` of the kind of the last column behind (0 where that column is a
// diagonal move), counted in tiles of 64 columns until a tile holds another kind.
struct MpPairView {
  const uint8_t *mv, *sf, *sr;
  int n, lf, lr, start, trail, kind0, kindn;
};

__device__ __forceinline__ int mp_kind(const MpPairView &v, int c) { return c < v.n ? (int)v.mv[v.n - 1 - c] : 0; }

__device__ __forceinline__ MpPairView mp_view(const MpSeqs &Q, const MpPairs &P, int p, const uint8_t *moves, int stride, const int32_t *nmoves,
                                              int lane) {
  MpPairView v;
  const int gf = P.f[p], gr = P.r[p];
  v.sf = Q.f_bytes + Q.f_off[gf]; v.lf = (int)(Q.f_off[gf + 1] - Q.f_off[gf]);
  v.sr = Q.r_bytes + Q.r_off[gr]; v.lr = (int)(Q.r_off[gr + 1] - Q.r_off[gr]);
  v.mv = moves + (size_t)p * stride;
  v.n = nmoves[p];
  if (v.n < 0 || v.n > stride || v.n > v.lf + v.lr) v.n = -1;     // not a move string of this pair: the caller flags it
  v.start = v.trail = v.kind0 = v.kindn = 0;
  if (v.n <= 0) return v;
  v.kind0 = v.mv[v.n - 1]; v.kindn = v.mv[0];
  if (v.kind0 != 1)
    for (int c0 = 0; c0 < v.n; c0 += 64) {
      const unsigned long long other = __ballot(c0 + lane < v.n && mp_kind(v, c0 + lane) != v.kind0);
      if (other) { v.start = c0 + __builtin_ctzll(other); break; }
      v.start = min(c0 + 64, v.n);
    }
  if (v.kindn != 1)
    for (int t0 = 0; t0 < v.n; t0 += 64) {                        // (from the back: the move string's own order)
      const unsigned long long other = __ballot(t0 + lane < v.n && v.mv[t0 + lane] != v.kindn);
      if (other) { v.trail = t0 + __builtin_ctzll(other); break; }
      v.trail = min(t0 + 64, v.n);
    }
  return v;
}

// A tile of 64 columns: the lane's column kind, and the position of its column in either string from the ballots of the three
// kinds - the bases in front of the tile (af, ar) and the population count of the lanes below.
__device__ __forceinline__ void mp_tile(const MpPairView &v, int c0, int lane, int &af, int &ar, int &kind, int &pf, int &pr) {
  kind = mp_kind(v, c0 + lane);
  const unsigned long long b1 = __ballot(kind == 1), b2 = __ballot(kind == 2), b3 = __ballot(kind == 3);
  const unsigned long long below = (1ull << lane) - 1ull;
  pf = af + __popcll((b1 | b3) & below);
  pr = ar + __popcll((b1 | b2) & below);
  af += __popcll(b1 | b3);
  ar += __popcll(b1 | b2);
}

__global__ __launch_bounds__(MP_THREADS) void k_mp_eval(MpSeqs Q, MpPairs P, int npairs, const uint8_t *__restrict__ moves, int stride,
                                                        const int32_t *__restrict__ nmoves, int min_overlap, int max_mismatch, int trim_overhang,
                                                        MpVerdict V, MpCounters *ctr) {
  const int lane = (int)threadIdx.x & 63, p = (int)blockIdx.x * MP_WAVES + ((int)threadIdx.x >> 6);
  if (p >= npairs) return;                                        // (the same for every lane of the wave)
  const MpPairView v = mp_view(Q, P, p, moves, stride, nmoves, lane);
  // C_eval_pair: start is the first column behind the leading run; end the last one in front of the trailing run, but not below
  // start - 1; what lies between them is counted
  const int start = v.start, end = max(v.n - 1 - v.trail, start - 1);
  int nmatch = 0, nmismatch = 0, nindel = 0, af = 0, ar = 0;
  for (int c0 = 0; c0 < v.n; c0 += 64) {
    int kind, pf, pr;
    mp_tile(v, c0, lane, af, ar, kind, pf, pr);
    const int c = c0 + lane;
    const bool in = c >= start && c <= end;
    bool eq = false;
    if (in && kind == 1 && pf < v.lf && pr < v.lr) eq = v.sf[pf] == v.sr[pr];
    nmatch += __popcll(__ballot(in && kind == 1 && eq));
    nmismatch += __popcll(__ballot(in && kind == 1 && !eq));
    nindel += __popcll(__ballot(in && kind != 1));
  }
  if (lane != 0) return;
  if (v.n < 0 || af != v.lf || ar != v.lr) atomicOr(&ctr->err, (int)MP_ERR_MOVES);   // the moves do not spell the two strings
  const int gf = P.f[p], gr = P.r[p];
  const int lead = (trim_overhang && v.kind0 == 2) ? v.start : 0, tail = (trim_overhang && v.kindn == 3) ? v.trail : 0;
  V.nmatch[p] = nmatch; V.nmismatch[p] = nmismatch; V.nindel[p] = nindel;
  V.prefer[p] = 1 + (Q.r_n0[gr] > Q.f_n0[gf] ? 1 : 0);
  V.accept[p] = (nmatch >= min_overlap && nmismatch + nindel <= max_mismatch) ? 1 : 0;
  V.mlen[p] = max(v.n, 0) - lead - tail;                         // (the two runs are of different kinds: they do not overlap)
  V.lead[p] = lead;
}

// C_pair_consensus leaves no gap in its output, so column c writes byte c - lead: where the strings agree, or one has a gap, the
// base there is; where they differ, the preferred string's.
__global__ __launch_bounds__(MP_THREADS) void k_mp_consensus(MpSeqs Q, MpPairs P, int npairs, const uint8_t *__restrict__ moves, int stride,
                                                             const int32_t *__restrict__ nmoves, MpVerdict V, const long long *__restrict__ off,
                                                             uint8_t *__restrict__ arena) {
  const int lane = (int)threadIdx.x & 63, p = (int)blockIdx.x * MP_WAVES + ((int)threadIdx.x >> 6);
  if (p >= npairs) return;
  if (!V.accept[p]) return;                                       // (one word for the wave)
  MpPairView v;
  const int gf = P.f[p], gr = P.r[p];
  v.sf = Q.f_bytes + Q.f_off[gf]; v.lf = (int)(Q.f_off[gf + 1] - Q.f_off[gf]);
  v.sr = Q.r_bytes + Q.r_off[gr]; v.lr = (int)(Q.r_off[gr + 1] - Q.r_off[gr]);
  v.mv = moves + (size_t)p * stride;
  v.n = nmoves[p];
  if (v.n < 0 || v.n > stride) return;                            // (k_mp_eval has flagged it)
  const int lead = V.lead[p], mlen = V.mlen[p], prefer = V.prefer[p];
  uint8_t *out = arena + off[p];
  int af = 0, ar = 0;
  for (int c0 = 0; c0 < v.n; c0 += 64) {
    int kind, pf, pr;
    mp_tile(v, c0, lane, af, ar, kind, pf, pr);
    const int c = c0 + lane, at = c - lead;
    if (c >= v.n || at < 0 || at >= mlen) continue;               // (no cross-lane operation behind this line)
    const bool hf = kind != 2 && pf < v.lf, hr = kind != 3 && pr < v.lr;
    const uint8_t bf = hf ? v.sf[pf] : (uint8_t)'N', br = hr ? v.sr[pr] : (uint8_t)'N';
    out[at] = kind == 2 ? br : kind == 3 ? bf : (bf == br || prefer == 1) ? bf : br;
  }
}

void launch_mp_tally(const MpSample &S, const MpTable &T, MpCounters *d_ctr, hipStream_t st) {
  if (S.nreads <= 0) return;
  hipLaunchKernelGGL(k_mp_tally, dim3((unsigned)(((long long)S.nreads + MP_THREADS - 1) / MP_THREADS)), dim3(MP_THREADS), 0, st, S, T, d_ctr);
}

void launch_mp_compact(const MpTable &T, void *d_rec, int max_rec, MpCounters *d_ctr, hipStream_t st) {
  hipLaunchKernelGGL(k_mp_compact, dim3((unsigned)((T.cap + MP_THREADS - 1) / MP_THREADS)), dim3(MP_THREADS), 0, st, T, (MpRec *)d_rec, max_rec, d_ctr);
}

void launch_mp_eval(const MpSeqs &Q, const MpPairs &P, int npairs, const uint8_t *d_moves, int stride, const int32_t *d_nmoves, int min_overlap,
                    int max_mismatch, int trim_overhang, const MpVerdict &V, MpCounters *d_ctr, hipStream_t st) {
  if (npairs <= 0) return;
  hipLaunchKernelGGL(k_mp_eval, dim3((unsigned)((npairs + MP_WAVES - 1) / MP_WAVES)), dim3(MP_THREADS), 0, st, Q, P, npairs, d_moves, stride,
                     d_nmoves, min_overlap, max_mismatch, trim_overhang, V, d_ctr);
}

void launch_mp_consensus(const MpSeqs &Q, const MpPairs &P, int npairs, const uint8_t *d_moves, int stride, const int32_t *d_nmoves,
                         const MpVerdict &V, const long long *d_off, uint8_t *d_arena, hipStream_t st) {
  if (npairs <= 0) return;
  hipLaunchKernelGGL(k_mp_consensus, dim3((unsigned)((npairs + MP_WAVES - 1) / MP_WAVES)), dim3(MP_THREADS), 0, st, Q, P, npairs, d_moves, stride,
                     d_nmoves, V, d_off, d_arena);
}
