// seqkeys.inc.hip — device helpers over packed 2-bit rows that collapse.inc.hip and species.inc.hip share; included by
// kernels.hip, inside namespace d2, ahead of both.  The prefix keys and their groups are stage_plain.h's.

// sixteen bases (bits 2k..2k+1 = base b + k) of a packed row of nw words, from base b on; bases outside [0, 16 nw) read as zero
__device__ __forceinline__ uint32_t bases16(const uint32_t *row, int nw, int b) {
  const int w = b >> 4, sh = (b & 15) * 2;
  const uint32_t lo = (w >= 0 && w < nw) ? row[w] : 0u;
  const uint32_t hi = (w + 1 >= 0 && w + 1 < nw) ? row[w + 1] : 0u;
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh);
}
// the bits of a key of kl bases, and the key of the window of that many bases at position p of a row
__device__ __forceinline__ unsigned long long key_mask(int kl) { return kl >= 32 ? ~0ull : ((1ull << (2 * kl)) - 1ull); }
__device__ __forceinline__ unsigned long long window_key(const uint32_t *row, int nw, int p, unsigned long long mask) {
  return ((((unsigned long long)bases16(row, nw, p + 16)) << 32) | bases16(row, nw, p)) & mask;
}
// the first key >= w of the group keys[first, first + cnt): w is a key of the group iff the result is inside it and equals w
__device__ __forceinline__ int key_lower_bound(const unsigned long long *keys, int first, int cnt, unsigned long long w) {
  int lo = first, hi = first + cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < w) lo = mid + 1; else hi = mid;
  }
  return lo;
}
