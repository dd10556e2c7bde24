// tools/micro/qprofile_shape.hip — k_qprofile's launch shape (readqc.inc.hip) swept on one piece of 65 536 reads x 250
// cycles: threads per block, reads in flight per wave, reads per block of the grid's first dimension.  A copy of the kernel with
// the three as parameters; the table's total is checked.  Not part of the library.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/micro/qprofile_shape tools/micro/qprofile_shape.hip && tools/micro/qprofile_shape
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
constexpr int NS = 94, TILE = 64, ROW = 95;
template <int THREADS, int UNROLL>
__global__ __launch_bounds__(THREADS) void k(int n, const uint8_t *__restrict__ qual, const long long *__restrict__ off,
                                             unsigned long long *__restrict__ tab, int32_t *__restrict__ bad) {
  __shared__ unsigned int s_tab[TILE * ROW];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < TILE * ROW; i += THREADS) s_tab[i] = 0u;
  __syncthreads();
  const int c0 = (int)blockIdx.y * TILE, c = c0 + lane;
  constexpr int NW = THREADS / 64;
  const long long step = (long long)gridDim.x * NW;
  for (long long r0 = (long long)blockIdx.x * NW + wave; r0 < n; r0 += step * UNROLL) {
    long long b[UNROLL]; int len[UNROLL]; unsigned q[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) { const long long r = r0 + step * u; b[u] = 0; len[u] = 0; if (r < n) { b[u] = off[r]; len[u] = (int)(off[r + 1] - b[u]); } }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) q[u] = c < len[u] ? (unsigned)qual[b[u] + c] - 33u : 0u;
#pragma unroll
    for (int u = 0; u < UNROLL; u++) { if (c >= len[u]) continue; if (q[u] < (unsigned)NS) atomicAdd(&s_tab[lane * ROW + (int)q[u]], 1u); else bad[r0 + step * u] = 1; }
  }
  __syncthreads();
  for (int i = tid; i < TILE * NS; i += THREADS) {
    const int j = i / NS, s = i - j * NS;
    const unsigned int v = s_tab[j * ROW + s];
    if (v != 0u) atomicAdd(&tab[(size_t)(c0 + j) * NS + s], (unsigned long long)v);
  }
}
template <int THREADS, int UNROLL>
int run(int n, int len, int slice, const uint8_t *dq, const long long *doff, unsigned long long *dtab, int32_t *dbad) {
  const int ncyc = (len + 63) / 64 * 64;
  const unsigned gx = (unsigned)std::min((n + slice - 1) / slice, 4096), gy = ncyc / 64;
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  float best = 1e9f;
  for (int rep = 0; rep < 12; rep++) {
    CK(hipMemset(dtab, 0, (size_t)ncyc * NS * 8));
    CK(hipEventRecord(a));
    hipLaunchKernelGGL((k<THREADS, UNROLL>), dim3(gx, gy), dim3(THREADS), 0, 0, n, dq, doff, dtab, dbad);
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    if (rep >= 2) best = std::min(best, ms);
  }
  std::vector<unsigned long long> h((size_t)ncyc * NS);
  CK(hipMemcpy(h.data(), dtab, h.size() * 8, hipMemcpyDeviceToHost));
  unsigned long long tot = 0; for (auto v : h) tot += v;
  printf("threads %4d unroll %d slice %4d grid %4u x %u : %.1f us, %.0f GB/s, total %llu %s\n", THREADS, UNROLL, slice, gx, gy, best * 1e3,
         (double)n * len / (best * 1e-3) / 1e9, tot, tot == (unsigned long long)n * len ? "ok" : "WRONG");
  return 0;
}
int main() {
  const int n = 65536, len = 250;
  std::vector<uint8_t> q((size_t)n * len); std::vector<long long> off(n + 1);
  uint32_t x = 12345; for (auto &c : q) { x = x * 1664525u + 1013904223u; c = (uint8_t)(35 + (x >> 24) % 39); }
  for (int i = 0; i <= n; i++) off[i] = (long long)i * len;
  uint8_t *dq; long long *doff; unsigned long long *dtab; int32_t *dbad;
  CK(hipMalloc(&dq, q.size() + 64)); CK(hipMalloc(&doff, (n + 1) * 8)); CK(hipMalloc(&dtab, 256 * NS * 8)); CK(hipMalloc(&dbad, n * 4));
  CK(hipMemcpy(dq, q.data(), q.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(doff, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
  CK(hipMemset(dbad, 0, n * 4));
  for (int slice : {1024, 512, 256, 128, 64}) {
    if (run<256, 4>(n, len, slice, dq, doff, dtab, dbad)) return 1;
    if (run<256, 8>(n, len, slice, dq, doff, dtab, dbad)) return 1;
    if (run<512, 4>(n, len, slice, dq, doff, dtab, dbad)) return 1;
    if (run<1024, 4>(n, len, slice, dq, doff, dtab, dbad)) return 1;
  }
  return 0;
}
