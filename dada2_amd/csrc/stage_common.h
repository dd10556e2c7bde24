// stage_common.h — what the host sides of the five stages (collapse_, taxonomy_, species_, filter_, primers_host.h) share; included
// by driver.cpp ahead of them, with C++ linkage.  stage_stats.h and stage_plain.h, and what needs HIP or driver.cpp's types.
#pragma once
#include "stage_plain.h"
#include "stage_stats.h"

namespace {

void require_acgt(int n, const char *const *seqs, const char *what) {
  for (int i = 0; i < n; i++) {
    if (!seqs[i]) throw InputError{"dada2hip: bad arguments"};
    for (const char *c = seqs[i]; *c; c++)
      if (acgt_code(*c) < 0) throw RuntimeErr{DADA2HIP_ERR_UNSUPPORTED, std::string("dada2hip: ") + what + " on the device takes A/C/G/T only."};
  }
}

// N events, created on the selected device by create() and destroyed with their owner
template <int N> struct Events {
  hipEvent_t e[N] = {};
  Events() {}
  Events(const Events &) = delete;
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  void create() { for (hipEvent_t &x : e) D2_HIP(hipEventCreate(&x)); }
  hipEvent_t operator[](int i) const { return e[i]; }
};

// microseconds into a stats word, truncated: the host's since t0, the device's between two events of a synchronised stream
inline void add_lap(int64_t &word, clk::time_point t0) { word += (int64_t)(ms_since(t0) * 1e3); }
inline void add_elapsed(int64_t &word, hipEvent_t from, hipEvent_t to) {
  float ms = 0.0f;
  D2_HIP(hipEventElapsedTime(&ms, from, to));
  word += (int64_t)((double)ms * 1e3);
}
inline void sync_checked(hipStream_t s) { D2_HIP(hipStreamSynchronize(s)); D2_HIP(hipGetLastError()); }
// the end of a call: its total, and the words out to the caller who asked for them
template <size_t N> void finish_stats(int64_t (&st)[N], int total_word, clk::time_point t_call, int64_t *stats) {
  st[total_word] = (int64_t)(ms_since(t_call) * 1e3);
  if (stats) memcpy(stats, st, sizeof st);
}

}  // namespace
