// tests/golden/taxonomy_ref_wrap.cpp — TEST INFRASTRUCTURE ONLY (tests/golden/make_taxonomy_golden.py, tools/taxonomy_bench.py).
//
// Compiles the reference's src/taxonomy.cpp UNMODIFIED and in place (the compile line puts its src directory and oracle/shim on
// the include path) behind one C entry.  The shim lacks one thing the file uses, Rcpp::runif(n): it is defined here and hands
// out the caller's buffer, so that a run's bootstrap draws are the caller's.  The shim's four externals are defined here too, so
// the wrapper links against nothing of the oracle.  Nothing built from this file is committed.
#include <cfloat>
#include <cstring>
#include <thread>
#include <vector>

#include <Rcpp.h>

extern "C" {
int dada2_shim_verbose = 0;
int dada2_shim_nthreads = 1;
double dada2_oracle_ppois(double, double, int) { return 0.0; }   // (not reached from taxonomy.cpp)
void dada2_shim_parallel_for(std::size_t begin, std::size_t end, std::size_t chunk, void (*fn)(void *, std::size_t, std::size_t), void *ctx) {
  (void)chunk;
  const std::size_t n = end - begin, nt = (std::size_t)dada2_shim_nthreads;
  std::vector<std::thread> th;
  for (std::size_t t = 0; t < nt; t++) {
    const std::size_t b = begin + n * t / nt, e = begin + n * (t + 1) / nt;
    if (b < e) th.emplace_back([=] { fn(ctx, b, e); });
  }
  for (auto &x : th) x.join();
}
}

static const double *g_unifs = nullptr;
static std::size_t g_nunifs = 0;
namespace Rcpp {
inline NumericVector runif(std::size_t n) {
  if (n != g_nunifs) stop("taxonomy_ref_wrap: the call draws %d uniforms, the caller supplied %d.", (int)n, (int)g_nunifs);
  return NumericVector(g_unifs, g_unifs + n);
}
}  // namespace Rcpp

#include "taxonomy.cpp"

// ref_to_genus 1-based and genusmat ngenus x nlevel ROW-major in; tax[nseq], boot[nseq][nlevel], boot_tax[nseq][100] out, 0-based
// (-1 = NA) and row-major.  Returns 0, or 1 with the reference's message in err.
extern "C" int taxonomy_ref_run(int nseq, const char *const *seqs, const char *const *rcs, int nref, const char *const *refs,
                                const int *ref_to_genus, int ngenus, int nlevel, const int *genusmat, int try_rc, const double *unifs,
                                long long nunifs, int nthreads, int *tax, int *boot, int *boot_tax, char *err, std::size_t errlen) {
  try {
    dada2_shim_nthreads = nthreads < 1 ? 1 : nthreads;
    g_unifs = unifs; g_nunifs = (std::size_t)nunifs;
    std::vector<std::string> s(seqs, seqs + nseq), r(rcs, rcs + nseq), rf(refs, refs + nref);
    std::vector<int> r2g(ref_to_genus, ref_to_genus + nref);
    Rcpp::IntegerMatrix gm(ngenus, nlevel);
    for (int g = 0; g < ngenus; g++) for (int l = 0; l < nlevel; l++) gm(g, l) = genusmat[g * nlevel + l];
    Rcpp::List res = C_assign_taxonomy2(s, r, rf, r2g, gm, try_rc != 0, false);
    const Rcpp::RObj *t = res.obj->get("tax"), *b = res.obj->get("boot"), *bt = res.obj->get("boot_tax");
    for (int j = 0; j < nseq; j++) {
      tax[j] = t->iv[j] == NA_INTEGER ? -1 : t->iv[j] - 1;
      for (int l = 0; l < nlevel; l++) boot[j * nlevel + l] = b->iv[(std::size_t)l * nseq + j];
      for (int k = 0; k < 100; k++) {
        const int v = bt->iv[(std::size_t)k * nseq + j];
        boot_tax[j * 100 + k] = v == NA_INTEGER ? -1 : v - 1;
      }
    }
    return 0;
  } catch (const std::exception &e) {
    if (err && errlen) snprintf(err, errlen, "%s", e.what());
    return 1;
  }
}
