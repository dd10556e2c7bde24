// derep_resident.inc.hip — the device dereplicator's uniques into a resident sample's rows, where they lie; included by
// kernels.hip, inside namespace d2, behind derep_dev.inc.hip (whose DdState it reads).  engine.h: DrRecord, launch_dd_to_sample.
//
// k_dd_to_sample writes, for output rank r, the rows of device unique u = order[r] (derep_dev_plain.h's order, uploaded at four
// bytes per unique) exactly as sample_create's upload leaves them (driver.cpp; hostsimd.cpp's marshal_rows):
//   len[r], reads[r]    the length and the count, as words
//   seq2[r][0 .. W2)    pack_row_2bit's words out of the arena's bytes: A C G T = 0 1 2 3, base k of a word in bits 2k, 2k + 1, a
//                       letter outside ACGT packs as 0 and sets the record's bad_base; every word behind the read is zero, out to
//                       the row's stride.  A lane packs the sixteen bases of one word
//   qual[r][0 .. LQ)    the 64-bit sums less count x offset through derep_resident_plain.h's integer rule (the byte marshal_rows'
//                       round() gives the double mean), zero from len on; a mean that rounds into no byte stores 0 and sets bad_qual
// A wave takes a row; the grid is capped (DADA2HIP_DD_SAMPLE_BLOCKS) and strides over the rows.  What a wave has seen - the two
// flags, its largest byte, its largest ceil(mean) - is reduced over its lanes by shuffles and added ONCE, behind its last row, to
// the record by vector atomics from lane 0.  No LDS, no barrier; no lane reads what another lane writes; every loop is bounded by
// the row geometry.  Bounds: r < nuniq rows of W2 words / LQ bytes are the sample's allocations (driver.cpp, sample_shell);
// order[r] < nuniq and u_off[u] + u_len[u] <= the arena's use are the dereplicator's.
#include "derep_resident_plain.h"

constexpr int DR_THREADS = 256, DR_WAVES = DR_THREADS / 64;

__global__ __launch_bounds__(DR_THREADS) void k_dd_to_sample(DdState T, const int32_t *__restrict__ order, int nuniq, int offset, SampleDev S,
                                                             DrRecord *rec) {
  const int lane = (int)threadIdx.x & 63, wave = (int)blockIdx.x * DR_WAVES + ((int)threadIdx.x >> 6), nwave = (int)gridDim.x * DR_WAVES;
  int bad_base = 0, bad_qual = 0, qmax = 0;
  long long cmax = INT32_MIN;
  for (int r = wave; r < nuniq; r += nwave) {                      // (wave-uniform)
    const int u = order[r];
    const int len = T.u_len[u];
    const long long at = T.u_off[u], cnt = (long long)T.u_count[u];
    if (lane == 0) { S.len[r] = len; S.reads[r] = (uint32_t)cnt; }
    const uint8_t *__restrict__ bytes = T.arena + at;
    uint32_t *__restrict__ row = S.seq2 + (size_t)r * S.W2;
    for (int w = lane; w < S.W2; w += 64) {
      const int p0 = w << 4, e = min(16, max(len - p0, 0));
      uint32_t word = 0;
      for (int k = 0; k < e; k++) {
        const uint32_t c = bytes[p0 + k];
        const bool ok = c == 'A' || c == 'C' || c == 'G' || c == 'T';
        bad_base |= !ok;
        word |= (ok ? ((c >> 1) ^ (c >> 2)) & 3u : 0u) << (k << 1);
      }
      row[w] = word;
    }
    const unsigned long long *__restrict__ sums = T.sums + at;
    uint8_t *__restrict__ q = S.qual + (size_t)r * S.LQ;
    const long long off = (long long)offset * cnt;
    for (int p = lane; p < S.LQ; p += 64) {
      int b = 0;
      if (p < len) {
        const long long t = (long long)sums[p] - off;
        b = dr_round_byte(t, cnt);
        if (b < 0) { bad_qual = 1; b = 0; }
        qmax = max(qmax, b);
        const long long c = (long long)dr_ceil_mean(t, cnt);
        cmax = c > cmax ? c : cmax;
      }
      q[p] = (uint8_t)b;
    }
  }
  bad_base = __any(bad_base);
  bad_qual = __any(bad_qual);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    qmax = max(qmax, __shfl_xor(qmax, o, 64));
    const long long c = __shfl_xor(cmax, o, 64);
    cmax = c > cmax ? c : cmax;
  }
  if (lane != 0 || wave >= nuniq) return;                          // (a wave without a row has nothing to add)
  if (bad_base) atomicOr(&rec->bad_base, 1);
  if (bad_qual) atomicOr(&rec->bad_qual, 1);
  atomicMax(&rec->qmax, qmax);
  atomicMax(&rec->ceil_max, (int)cmax);                            // (a mean of bytes less an offset lies in [-64, 255])
}

// blocks: the grid's cap (at least 1); returns the blocks launched
int launch_dd_to_sample(const DdState &T, const int32_t *d_order, int nuniq, int offset, const SampleDev &S, DrRecord *d_rec, int blocks,
                        hipStream_t st) {
  if (nuniq <= 0) return 0;
  const int grid = std::max(1, std::min((nuniq + DR_WAVES - 1) / DR_WAVES, blocks));
  hipLaunchKernelGGL(k_dd_to_sample, dim3((unsigned)grid), dim3(DR_THREADS), 0, st, T, d_order, nuniq, offset, S, d_rec);
  return grid;
}
