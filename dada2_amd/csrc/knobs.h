// knobs.h — the library's run-time knobs: ONE place that reads the environment.
//
// Every DADA2HIP_* variable is parsed here, into one immutable snapshot, when a boundary call (include/dada2hip.h) is entered
// (knobs_reload(), called by the C-ABI entry points); everything below the boundary reads `knobs()`.  Nothing else in the
// library calls getenv.  The supported set is listed in include/dada2hip.h ("Environment"); all default to "off" / automatic,
// and none changes a result - they choose engines, kernel families and buffer sizes, which the parity tests sweep.
// The variables read are exactly the ones named beside the fields of Knobs below (DESIGN.md has the same list as a table).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

namespace d2 {

enum { NWK_AUTO = 0, NWK_LANE = 1, NWK_COOP = 2, NWK_WIDE = 3 };   // Knobs::nw_kernel

struct Knobs {
  // ---- which engine / kernel family (tests cross-check them) ----
  bool engine_classic = false;        // DADA2HIP_ENGINE=classic        round 1's engine: one centre per round, host round trip per decision
  int nw_kernel = 0;                  // DADA2HIP_NW_KERNEL=lane|coop|wide   (1 / 2 / 3; 0 = automatic)
  bool ad_homo = true;                // DADA2HIP_AD_HOMO=0             homopolymer-gap aligner back on the lane kernels + classic engine
  bool no_speculation = false;        // DADA2HIP_NO_SPECULATION        classic engine: the reference's plain loop
  bool no_autobirth = false;          // DADA2HIP_NO_AUTOBIRTH          classic engine: every bud decision on the host
  // ---- round engine v2 ----
  int v2_nbuf = 0;                    // DADA2HIP_V2_NBUF               cached batch buffers (0 = automatic: <= 64, <= 1/8 of the device)
  int v2_depth = 0;                   // DADA2HIP_V2_DEPTH              rounds / super-chains enqueued ahead (0 = automatic: 2)
  int v2_chain = 0;                   // DADA2HIP_V2_CHAIN              shuffle calls per launch chain (0 = automatic: 4)
  int v2_lite = -1;                   // DADA2HIP_V2_LITE=0|1           chains expected to hit the cache go out without the compare launches
  int v2_align = -1;                  // DADA2HIP_V2_ALIGN=commit|batch when the pairs of a batch are aligned (1 / 0; -1 = automatic)
  int v2_filter = -1;                 // DADA2HIP_V2_FILTER=0|1         later shuffle calls visit only the uniques the previous call can have unsettled
  int v2_grid_shuffle = 0;            // DADA2HIP_V2_GRID_SHUFFLE       block cap of k2_shuffle (0 = 2048)
  int v2_grid_pupdate = 0;            // DADA2HIP_V2_GRID_PUPDATE       block cap of k2_pupdate (0 = 1024)
  int v2_mov_inline = 0;              // DADA2HIP_V2_MOV_INLINE         movers that ride inline with a result block (tests: pauses / long lists)
  bool v2_tail_chain = false;         // DADA2HIP_V2_TAIL=chain         the round tail as launch chains instead of the persistent kernel
  int v3_grid = 0;                    // DADA2HIP_V3_GRID               blocks of the persistent launch (tests: several blocks on a small sample)
  int v3_ring = 0;                    // DADA2HIP_V3_RING               result blocks the device may be ahead of the host (tests: a host that lags)
  int v3_overlap = -1;                // DADA2HIP_V3_OVERLAP=0|1        the next batch's compare under the persistent tail, on a second stream (-1 = automatic)
  int v3_pf_wait_us = -1;             // DADA2HIP_V3_PF_WAIT_US         how long the tail spins for a prefetched compare before it leaves the launch
  int v3_pf_early = -1;               // DADA2HIP_V3_PF_EARLY=n         (tuning) plan the next prefetch n positions into the batch before the newest (0-8)
  int v3_pf_gate_us = -1;             // DADA2HIP_V3_PF_GATE_US         how long the gate of a prefetch chain enqueued ahead waits for its plan (0 = no chain ahead: the host launches a compare when it sees the plan)
  int v3_xbar = -1;                   // DADA2HIP_V3_XBAR=0|1           XCD-hierarchical grid barriers inside a persistent launch (default: from 48 blocks on)
  int v3_spec = 1;                     // DADA2HIP_V3_SPEC=0|1           the round's evaluation rides on its shuffle calls (0: a phase of its own behind them, round 4's form)
  int v3_spec_max = -1;               // DADA2HIP_V3_SPEC_MAX=n         (tuning) ... only behind a call that moved at most n uniques
  int v3_pf_sync = 0;                 // DADA2HIP_V3_PF_SYNC=1          (measurement) every prefetch is waited for at the next serial end, the tail resident and idle
  int replay_radix_min = 4096;        // DADA2HIP_REPLAY_RADIX_MIN=n    test knob: mover lists from n entries on are ordered by the radix sort of the host's replay (1 = always)
  int v3_slots = 3;                   // DADA2HIP_V3_SLOTS=n            persistent launches of this process side by side on one device (several samples in flight; 1 = their rounds take turns)
  int v3_mirror = 1;                  // DADA2HIP_V3_MIRROR=0           the persistent tail reads every unique's partition / flags from global memory in each sweep (no LDS mirror)
  int v3_fail_entry = 0;              // DADA2HIP_V3_FAIL_ENTRY=n       test knob: the n-th persistent launch fails its entry barrier (-> launch chains)
  bool v2_debug = false;              // DADA2HIP_V2_DEBUG              per-block trace on stderr
  bool v2_summary = false;            // DADA2HIP_V2_SUMMARY            per-pass summary on stderr
  bool v2_trace_on = false;           // DADA2HIP_V2_TRACE=<round>[:file]   in-kernel phase stamps of one round (tools/trace_round.py)
  int v2_trace_seq = -1;
  std::string v2_trace_file;
  // ---- measurement / plumbing ----
  bool profile = false;               // DADA2HIP_PROFILE=1             event-time every launch (dev_ms_* in the stats)
  long long node_cap = 0;             // DADA2HIP_NODE_CAP              first allocation of the comparison store (tests: the growth path)
  bool wait_block = false;            // DADA2HIP_WAIT=block            blocking synchronisation instead of spinning
  double wait_timeout_s = 600.0;      // DADA2HIP_WAIT_TIMEOUT_S        bound on every host-side device wait
  long long ad_fcap = 0;              // DADA2HIP_AD_FCAP               rows of k_ad_product's offset buffer (tests: the in-kernel product)
  int screen_bits = 1;                // DADA2HIP_SCREEN_BITS=0         no 5-mer presence bitmaps: the batch screen walks every unique's k-mer record
  int ad_fast = 1;                    // DADA2HIP_AD_FAST=0             batch compares on the full aligner only (no pointer-free first pass)
  long long nw_ring = 0;              // DADA2HIP_NW_RING=n             waves of the lane aligners' scratch ring (a multiple of 4, at least 4; at most, and unset, the automatic size; tests: a wave's second and third chunk in a reused slot)
  long long upload_chunk_rows = 0;    // DADA2HIP_UPLOAD_CHUNK_ROWS=n   test knob: rows per chunk of the boundary's upload (rounded up to a multiple of 512; unset: about 16 MB of quality bytes; tests: chunk borders on small samples)
  int alloc_poison = -1;              // DADA2HIP_ALLOC_POISON=<0..255> test knob: every block the allocation cache hands out, fresh or recycled, device or pinned, is filled with that byte over its whole size class first (hostpar.h; unset: handed out as it lies; tests: kernels and host passes that rely on what a buffer held before)
  int ad_debug = 0;                   // DADA2HIP_AD_DEBUG             profiling build only (make prof): skips phases of k_nw_ad, results void
  bool bimera_times = false;          // DADA2HIP_BIMERA_TIMES=1        stderr: host / device split of a bimera call
  long long bimera_slots = 0;         // DADA2HIP_BIMERA_SLOTS=n        isBimeraDenovo: work slots per launch (at least one chunk of the aligner; at most, and unset, what a bimera call's launch holds; tests: a window in several launches at small sizes)
  int collapse_batch = 0;             // DADA2HIP_COLLAPSE_BATCH=n      collapseNoMismatch: queries per batch (0 = automatic: 4 096)
  int collapse_scan = 1;              // DADA2HIP_COLLAPSE_SCAN=0       ... every screened pair is aligned (the diagonal bound is not used)
  int collapse_join = 1;              // DADA2HIP_COLLAPSE_JOIN=0       ... every (query, ref) pair is scanned (no prefix-key join)
  int tax_slab = 256;                 // DADA2HIP_TAX_SLAB=n            assignTaxonomy: queries of at most n k-mers are summed out of an LDS slab (0 = every query gathers from the table; at most 512)
  long long tax_chunk = 0;            // DADA2HIP_TAX_CHUNK=n           ... queries per chunk of a pass (at least 1; at most, and unset, what keeps the per-tile records within 64 MB)
  long long filter_piece = 0;         // DADA2HIP_FILTER_PIECE=n        filterAndTrim: reads per piece of a call (at least 1; at most, and unset, 65 536)
  long long filter_piece_bytes = 0;   // DADA2HIP_FILTER_PIECE_BYTES=n  ... bases per piece (at least 1; at most, and unset, 32 MiB; a longer read is a piece of its own)
  long long primers_piece = 0;        // DADA2HIP_PRIMERS_PIECE=n       removePrimers: reads per piece of a call (at least 1; at most, and unset, 65 536)
  long long primers_piece_bytes = 0;  // DADA2HIP_PRIMERS_PIECE_BYTES=n ... bases per piece (at least 1; at most, and unset, 32 MiB; a longer read is a piece of its own)
  long long primers_tile = 0;         // DADA2HIP_PRIMERS_TILE=n        ... chunks of 64 match starts per tile of a read (at least 1; at most, and unset, 64)
  long long readqc_piece = 0;         // DADA2HIP_READQC_PIECE=n        read diagnostics: reads per piece of a call (at least 1; at most, and unset, 65 536)
  long long readqc_piece_bytes = 0;   // DADA2HIP_READQC_PIECE_BYTES=n  ... bases per piece (at least 1; at most, and unset, 32 MiB; a longer read is a piece of its own)
  long long derep_piece = 0;          // DADA2HIP_DEREP_PIECE=n         device dereplicator: reads per piece of a dada2hip_derep_reads call (at least 1; at most, and unset, 65 536)
  long long derep_piece_bytes = 0;    // DADA2HIP_DEREP_PIECE_BYTES=n   ... bases per piece (at least 1; at most, and unset, 32 MiB; a longer read is a piece of its own)
  long long derep_table = 0;          // DADA2HIP_DEREP_TABLE=n         ... slots of the table at the start (rounded up to a power of two, at least 8; unset: 131 072; tests: the rebuild)
  int derep_hash_bits = 64;           // DADA2HIP_DEREP_HASH_BITS=k     ... the hash masked to k bits (0..64; tests: true collisions, 0 = every read with every other)
  int dd_sample_blocks = 0;           // DADA2HIP_DD_SAMPLE_BLOCKS=n    ... block cap of k_dd_to_sample, the uniques into a resident sample's rows (0 = 4 096; tests: waves that stride on a few hundred uniques)
  int merge_hash_bits = 64;           // DADA2HIP_MERGE_HASH_BITS=k     run-level mergePairs: the pair table's hash masked to k bits (0..64; tests: true collisions, 0 = every pair walks from slot 0)
  long long merge_chunk = 0;          // DADA2HIP_MERGE_CHUNK=n         ... unique pairs per chunk of the aligner (at least 1; at most, and unset, 65 536; tests: chunk borders inside and between samples)
  int species_cand = 1 << 20;         // DADA2HIP_SPECIES_CAND=n       assignSpecies: records of the candidate buffer and of the hit buffer (a launch that counts more is re-run in pieces)
  int species_chunk = 8192;           // DADA2HIP_SPECIES_CHUNK=n       ... distinct queries per pass over the references (at most 8 192: the presence bitmap is sized for it)
  int priors_lds_keys = 4096;         // DADA2HIP_PRIORS_LDS_KEYS=n     priors by sequence: up to n distinct prefix keys are searched in LDS, more in global memory (at most 6 144; 0 = always global; tests: the global path on a small set)
  int priors_grid = 0;                // DADA2HIP_PRIORS_GRID=n         ... block cap of k_prior_match (0 = 2048; tests: blocks that stride on a small sample)
  bool derep_zlib = false;           // DADA2HIP_DEREP_INFLATE=zlib    .gz files through zlib's streaming inflate even where libdeflate is installed
  bool derep_times = false;           // DADA2HIP_DEREP_TIMES=1         stderr: phases of a dada2hip_derep_fastq / dada2hip_derep_combine call
  // (read once per process, when the host pool / the allocation cache are created: DADA2HIP_HOST_THREADS, DADA2HIP_ALLOC_CACHE,
  //  DADA2HIP_ALLOC_CACHE_GB)
  int host_threads = 0;
  int alloc_cache = -1;
  long long alloc_cache_gb = -1;
  // what the environment said: "NAME=text" of every variable from_env looked up and found set, in lookup order.  Two snapshots
  // are the same settings exactly when these strings are equal (knobs_reload) - nothing to keep in step when a knob is added.
  std::string env_text;

  static Knobs from_env() {
    Knobs k;
    auto S = [&k](const char *n) -> const char * {   // every lookup goes through here, and leaves its text in env_text
      const char *e = std::getenv(n);
      if (e) k.env_text.append(n).append(1, '=').append(e).append(1, '\n');
      return e;
    };
    auto I = [&](const char *n, int dflt) -> int { const char *e = S(n); return e ? std::atoi(e) : dflt; };
    auto B = [&](const char *n) -> bool { const char *e = S(n); return e && std::atoi(e) != 0; };
    auto T = [&](const char *n) -> int { const char *e = S(n); return e ? (std::atoi(e) != 0 ? 1 : 0) : -1; };   // tri-state
    if (const char *e = S("DADA2HIP_ENGINE")) k.engine_classic = !std::strcmp(e, "classic");
    if (const char *e = S("DADA2HIP_NW_KERNEL")) k.nw_kernel = !std::strcmp(e, "lane") ? 1 : (!std::strcmp(e, "coop") ? 2 : (!std::strcmp(e, "wide") ? 3 : 0));
    if (const char *e = S("DADA2HIP_AD_HOMO")) k.ad_homo = std::strcmp(e, "0") != 0;
    k.no_speculation = S("DADA2HIP_NO_SPECULATION") != nullptr;
    k.no_autobirth = S("DADA2HIP_NO_AUTOBIRTH") != nullptr;
    k.v2_nbuf = I("DADA2HIP_V2_NBUF", 0); k.v2_depth = I("DADA2HIP_V2_DEPTH", 0); k.v2_chain = I("DADA2HIP_V2_CHAIN", 0);
    k.v2_lite = T("DADA2HIP_V2_LITE");
    if (const char *e = S("DADA2HIP_V2_ALIGN")) k.v2_align = !std::strcmp(e, "commit") ? 1 : 0;
    k.v2_filter = T("DADA2HIP_V2_FILTER");
    k.v2_grid_shuffle = I("DADA2HIP_V2_GRID_SHUFFLE", 0); k.v2_grid_pupdate = I("DADA2HIP_V2_GRID_PUPDATE", 0);
    k.v2_mov_inline = I("DADA2HIP_V2_MOV_INLINE", 0);
    if (const char *e = S("DADA2HIP_V2_TAIL")) k.v2_tail_chain = !std::strcmp(e, "chain");
    k.v3_grid = I("DADA2HIP_V3_GRID", 0); k.v3_ring = I("DADA2HIP_V3_RING", 0);
    k.v3_overlap = T("DADA2HIP_V3_OVERLAP"); k.v3_pf_wait_us = I("DADA2HIP_V3_PF_WAIT_US", -1);
    k.v3_fail_entry = I("DADA2HIP_V3_FAIL_ENTRY", 0); k.v3_spec = I("DADA2HIP_V3_SPEC", 1); k.v3_xbar = T("DADA2HIP_V3_XBAR"); k.v3_spec_max = I("DADA2HIP_V3_SPEC_MAX", -1);
    k.v3_pf_early = I("DADA2HIP_V3_PF_EARLY", -1); k.v3_pf_sync = I("DADA2HIP_V3_PF_SYNC", 0); k.v3_pf_gate_us = I("DADA2HIP_V3_PF_GATE_US", -1);
    k.v3_mirror = I("DADA2HIP_V3_MIRROR", 1);
    k.v3_slots = I("DADA2HIP_V3_SLOTS", 3);
    k.replay_radix_min = I("DADA2HIP_REPLAY_RADIX_MIN", 4096);
    k.v2_debug = S("DADA2HIP_V2_DEBUG") != nullptr; k.v2_summary = S("DADA2HIP_V2_SUMMARY") != nullptr;
    if (const char *e = S("DADA2HIP_V2_TRACE")) {
      k.v2_trace_on = true; k.v2_trace_seq = std::atoi(e);
      const char *colon = std::strchr(e, ':');
      k.v2_trace_file = colon ? colon + 1 : "dada2hip_trace.bin";
    }
    k.profile = B("DADA2HIP_PROFILE");
    if (const char *e = S("DADA2HIP_NODE_CAP")) k.node_cap = std::atoll(e);
    if (const char *e = S("DADA2HIP_WAIT")) k.wait_block = !std::strcmp(e, "block");
    if (const char *e = S("DADA2HIP_WAIT_TIMEOUT_S")) k.wait_timeout_s = std::atof(e);
    if (const char *e = S("DADA2HIP_AD_FCAP")) k.ad_fcap = std::atoll(e);
    k.ad_debug = I("DADA2HIP_AD_DEBUG", 0); k.ad_fast = I("DADA2HIP_AD_FAST", 1); k.screen_bits = I("DADA2HIP_SCREEN_BITS", 1);
    if (const char *e = S("DADA2HIP_BIMERA_TIMES")) k.bimera_times = !std::strcmp(e, "1");
    k.collapse_batch = I("DADA2HIP_COLLAPSE_BATCH", 0); k.collapse_scan = I("DADA2HIP_COLLAPSE_SCAN", 1);
    k.collapse_join = I("DADA2HIP_COLLAPSE_JOIN", 1);
    k.tax_slab = I("DADA2HIP_TAX_SLAB", 256);
    auto P = [&](const char *n) -> long long { const char *e = S(n); return e ? std::max(1ll, std::atoll(e)) : 0ll; };   // a size: 0 = unset
    k.tax_chunk = P("DADA2HIP_TAX_CHUNK"); k.filter_piece = P("DADA2HIP_FILTER_PIECE"); k.filter_piece_bytes = P("DADA2HIP_FILTER_PIECE_BYTES");
    k.upload_chunk_rows = P("DADA2HIP_UPLOAD_CHUNK_ROWS");
    if (const char *e = S("DADA2HIP_ALLOC_POISON")) k.alloc_poison = *e ? std::max(0, std::min(255, std::atoi(e))) : -1;
    k.nw_ring = P("DADA2HIP_NW_RING"); k.bimera_slots = P("DADA2HIP_BIMERA_SLOTS");
    k.primers_piece = P("DADA2HIP_PRIMERS_PIECE"); k.primers_piece_bytes = P("DADA2HIP_PRIMERS_PIECE_BYTES"); k.primers_tile = P("DADA2HIP_PRIMERS_TILE");
    k.readqc_piece = P("DADA2HIP_READQC_PIECE"); k.readqc_piece_bytes = P("DADA2HIP_READQC_PIECE_BYTES");
    k.derep_piece = P("DADA2HIP_DEREP_PIECE"); k.derep_piece_bytes = P("DADA2HIP_DEREP_PIECE_BYTES"); k.derep_table = P("DADA2HIP_DEREP_TABLE");
    k.derep_hash_bits = std::max(0, std::min(64, I("DADA2HIP_DEREP_HASH_BITS", 64)));
    k.dd_sample_blocks = std::max(0, I("DADA2HIP_DD_SAMPLE_BLOCKS", 0));
    k.merge_hash_bits = std::max(0, std::min(64, I("DADA2HIP_MERGE_HASH_BITS", 64))); k.merge_chunk = P("DADA2HIP_MERGE_CHUNK");
    k.species_cand = I("DADA2HIP_SPECIES_CAND", 1 << 20); k.species_chunk = I("DADA2HIP_SPECIES_CHUNK", 8192);
    k.priors_lds_keys = I("DADA2HIP_PRIORS_LDS_KEYS", 4096); k.priors_grid = I("DADA2HIP_PRIORS_GRID", 0);
    if (const char *e = S("DADA2HIP_DEREP_INFLATE")) k.derep_zlib = !std::strcmp(e, "zlib");
    if (const char *e = S("DADA2HIP_DEREP_TIMES")) k.derep_times = !std::strcmp(e, "1");
    k.host_threads = I("DADA2HIP_HOST_THREADS", 0);
    k.alloc_cache = T("DADA2HIP_ALLOC_CACHE");
    if (const char *e = S("DADA2HIP_ALLOC_CACHE_GB")) k.alloc_cache_gb = std::atoll(e);
    return k;
  }
};

namespace knobs_detail {
inline std::mutex &mu() { static std::mutex m; return m; }          // serialises reloads only
inline std::atomic<const Knobs *> &cur() { static std::atomic<const Knobs *> p{nullptr}; return p; }
}  // namespace knobs_detail

// Re-read the environment (every C-ABI entry point does, once, before anything else).  A snapshot that differs from the current
// one replaces it; old snapshots are never freed (a few hundred bytes each, and only when the environment changed), so a
// reference obtained from knobs() by another thread stays valid.
// The ONE variable the library SETS (once, when it is loaded, and only if the caller has not): the HIP runtime maps a process's
// streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) when it initialises.  A run uses three streams (rounds, side copies,
// prefetch compares) and several samples in flight use three each; streams that share a queue run one behind the other - a
// persistent launch at the head of a queue holds back whatever else was mapped onto it.  With 8: configs[3] on one GPU 204 -> 190 ms
// at two slots (profiles/r10i_*, r10j_*); the single-sample call reads the same with 4, 8 or 16 (151-158 ms, profiles/r11b_*).  No effect if the runtime
// is already up (torch initialised first): dada2_amd/_lib.py and bench.py set it before either is.
inline void knobs_process_defaults() { (void)setenv("GPU_MAX_HW_QUEUES", "8", /*overwrite=*/0); }

inline void knobs_reload() {
  Knobs k = Knobs::from_env();
  std::lock_guard<std::mutex> g(knobs_detail::mu());
  const Knobs *c = knobs_detail::cur().load(std::memory_order_relaxed);
  if (!c || c->env_text != k.env_text) knobs_detail::cur().store(new Knobs(std::move(k)), std::memory_order_release);
}
// (an acquire load: knobs() is called from polling loops and per-round paths of several host threads - no lock on the read side)
inline const Knobs &knobs() {
  const Knobs *c = knobs_detail::cur().load(std::memory_order_acquire);
  if (c) return *c;
  knobs_reload();
  return *knobs_detail::cur().load(std::memory_order_acquire);
}

}  // namespace d2
