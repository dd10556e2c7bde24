/*
 * dada2hip.h — C ABI of libdada2hip.so, the MI355X (gfx950) implementation of DADA2's
 * divisive-denoising hot path.  This is the drop-in boundary: these entry points are what
 * the reference's Rcpp glue for the path would bind (INTEGRATION.md shows the 40-line
 * Rcpp translation unit that re-exports `_dada2_dada_uniques`, `_dada2_C_nwalign` and
 * `_dada2_C_nwvec` on top of them, so R/dada.R and R/misc.R call the new path unchanged).
 *
 * Reference interfaces replaced (all paths relative to /root/reference):
 *   dada2hip_dada_uniques   <- dada_uniques()      src/Rmain.cpp:30-295  (.Call `_dada2_dada_uniques`,
 *                                                   src/RcppExports.cpp:18-53, R/RcppExports.R:8-10)
 *   dada2hip_sample_* / _run<- the same call split so reads/qualities/k-mer tables stay resident in
 *                              HBM across the selfConsist passes of R/dada.R:256-405 (only `err` changes)
 *   dada2hip_nwalign        <- C_nwalign()         src/evaluate.cpp:18-62    (`_dada2_C_nwalign`, RcppExports.cpp:94)
 *   dada2hip_nwvec          <- C_nwvec()           src/nwalign_vectorized.cpp:321-343 (`_dada2_C_nwvec`, :227)
 *   dada2hip_result_*       <- the Rcpp::List of six objects built at src/Rmain.cpp:254-294 and src/error.cpp
 *   dada2hip_table_bimera2  <- C_table_bimera2()   src/chimera.cpp:192-208   (`_dada2_C_table_bimera2`; R/chimeras.R:236)
 *   dada2hip_is_bimera      <- C_is_bimera()       src/chimera.cpp:18-59     (`_dada2_C_is_bimera`; R/chimeras.R:44)
 *   dada2hip_merge_pairs    <- mergePairs()        R/paired.R:92-201 on C_nwalign / C_eval_pair / C_pair_consensus
 *                                                   (src/evaluate.cpp:18-62, :73-114, :124-174)
 *   dada2hip_collapse_nomismatch <- collapseNoMismatch()  R/multiSample.R:104-160 (grepl screen + nwhamming per pair)
 *   dada2hip_seqtab_merge   <- mergeSequenceTables()   R/multiSample.R:290-364 (validation :206-238)
 *   dada2hip_merge_run      <- mergePairs() over the samples of a run  R/paired.R:92-201 (the pairs tallied, judged and merged on the device)
 *   dada2hip_nweval         <- nweval() / nwhamming()  R/misc.R:216-225
 *   dada2hip_taxonomy_*     <- C_assign_taxonomy2() src/taxonomy.cpp:206-338  (`_dada2_C_assign_taxonomy2`; R/taxonomy.R:135), split into
 *                              the model (:219-270, built once, resident in HBM) and the classification of queries (:113-200)
 *   dada2hip_derep_*        <- derepFastq() / qtables2()  R/sequenceIO.R:45-124, :150-183 (host-side C++, zlib)
 *   dada2hip_derep_combine  <- combineDereps2()    R/multiSample.R:165-203 (dada(pool = TRUE), R/dada.R:189-192; host-side C++)
 *   dada2hip_sample_set_prior_seqs <- names(uniques) %in% c(priors, pseudo_priors)  R/dada.R:335, on the resident uniques
 *   dada2hip_filter_*       <- filterAndTrim() / fastqFilter() / fastqPairedFilter() / isPhiX() / seqComplexity()  R/filter.R:402-1275 on
 *                              C_matchRef / C_matrixEE (src/filter.cpp:7-49)
 *   dada2hip_primers_*      <- removePrimers()  R/filter.R:81-233 (vmatchPattern without indels, restated)
 *   dada2hip_qprofile_*     <- the data of plotQualityProfile()  R/plot-methods.R:163-243 (ShortRead qa()'s perCycle$quality, restated)
 *   dada2hip_complexity_*   <- seqComplexity() with window / by, plotComplexity()'s data  R/filter.R:1248-1275, R/plot-methods.R:293-299
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every call returns 0 on success or a
 * non-zero code with a NUL-terminated message in `errbuf` (the reference's Rcpp::stop texts are
 * kept where one exists).  Inputs are borrowed for the duration of the call only.  A result is
 * owned by the library until dada2hip_result_free().  There is NO CPU fallback: every entry point
 * that computes fails with DADA2HIP_ERR_DEVICE when no gfx950 device is usable.
 *
 * Environment.  The library reads its DADA2HIP_* variables in ONE place (dada2_amd/csrc/knobs.h), once per boundary call,
 * into an immutable snapshot; none of them changes a result.  Supported (the parity tests sweep them):
 *   DADA2HIP_ENGINE=classic            one centre per round, a host round trip per decision (round 1's engine)
 *   DADA2HIP_V2_TAIL=chain             the round tail as launch chains instead of the persistent kernel
 *   DADA2HIP_V3_OVERLAP=0|1            the next batch's compare under the persistent tail on a second stream (default: on)
 *   DADA2HIP_V3_SPEC=0|1               the evaluation of a round rides on its shuffle calls (default: on; 0 = a phase of its own)
 *   DADA2HIP_V3_MIRROR=0|1             the persistent tail keeps the per-unique facts its sweeps ask for in LDS (default: on)
 *   DADA2HIP_V3_SLOTS=<n>              persistent launches of this process side by side on a device (default 3; 1 = the rounds of
 *                                      several samples in flight take turns)
 * The library SETS one variable when it is loaded, unless the caller has: GPU_MAX_HW_QUEUES=8 (the HIP runtime's hardware queues
 * per process, 4 by default; a run uses three streams, several samples in flight three each).
 *   DADA2HIP_NW_KERNEL=lane|coop|wide  force one aligner family;  DADA2HIP_AD_HOMO=0  homopolymer gaps on the lane kernels
 *   DADA2HIP_NW_RING=<n>               waves of the lane aligners' scratch ring (a multiple of 4, at least 4; default and at most
 *                                      the automatic size: 4 096 waves, halved down to 64 while the pointers would pass 6 GiB)
 *   DADA2HIP_UPLOAD_CHUNK_ROWS=<n>     rows per chunk of the boundary's upload (rounded up to a multiple of 512; default: about 16 MB of
 *                                      quality bytes; tests: chunk borders on small samples)
 *   DADA2HIP_ALLOC_POISON=<0..255>     test knob: every block the allocation cache hands out (device and pinned, fresh or recycled) is
 *                                      first filled with that byte over its whole size class, on a stream of the cache's own (default:
 *                                      unset, blocks are handed out as they lie; dada2hip_alloc_poison_stats counts the fills)
 *   DADA2HIP_WAIT=block, DADA2HIP_WAIT_TIMEOUT_S=<s>   sleep instead of spin while waiting; bound of every device wait
 *   DADA2HIP_HOST_THREADS=<n>, DADA2HIP_ALLOC_CACHE=0, DADA2HIP_ALLOC_CACHE_GB=<n>   marshalling pool, allocation cache
 *   DADA2HIP_DEREP_INFLATE=zlib        dada2hip_derep_fastq, dada2hip_filter_fastq: .gz files through zlib's streaming inflate even where libdeflate is installed
 *   DADA2HIP_COLLAPSE_BATCH=<n>        dada2hip_collapse_nomismatch: queries per batch (default 0 = automatic)
 *   DADA2HIP_COLLAPSE_SCAN=0           ... every screened pair is aligned (the bound of the diagonal scan is not used)
 *   DADA2HIP_COLLAPSE_JOIN=0           ... every (query, ref) pair is scanned (no prefix-key join)
 *   DADA2HIP_TAX_SLAB=<n>              dada2hip_taxonomy_assign: queries of at most n valid k-mers are summed out of an LDS slab, longer
 *                                      ones gather from the table (default 256, at most 512; 0 = every query gathers)
 *   DADA2HIP_TAX_CHUNK=<n>             ... queries per chunk of a pass (at least 1; default and at most what keeps the per-tile records
 *                                      within 64 MB)
 *   DADA2HIP_SPECIES_CAND=<n>          dada2hip_species_match: records of the candidate and hit buffers (default 1 048 576; a launch
 *                                      that counts more is run again in pieces)
 *   DADA2HIP_SPECIES_CHUNK=<n>         ... distinct queries per pass over the references (default and at most 8 192)
 *   DADA2HIP_FILTER_PIECE=<n>          dada2hip_filter_reads: reads per piece of a call (at least 1; default and at most 65 536)
 *   DADA2HIP_FILTER_PIECE_BYTES=<n>    ... bases per piece (at least 1; default and at most 32 MiB; a longer read is a piece of its own)
 *   DADA2HIP_PRIMERS_PIECE=<n>         dada2hip_primers_reads: reads per piece of a call (at least 1; default and at most 65 536)
 *   DADA2HIP_PRIMERS_PIECE_BYTES=<n>   ... bases per piece (at least 1; default and at most 32 MiB; a longer read is a piece of its own)
 *   DADA2HIP_PRIMERS_TILE=<n>          ... chunks of 64 match starts per tile of a read (at least 1; default and at most 64)
 *   DADA2HIP_READQC_PIECE=<n>          dada2hip_qprofile_reads, dada2hip_complexity_reads: reads per piece of a call (at least 1; default and at most 65 536)
 *   DADA2HIP_READQC_PIECE_BYTES=<n>    ... bases per piece (at least 1; default and at most 32 MiB; a longer read is a piece of its own)
 *   DADA2HIP_DEREP_PIECE=<n>           dada2hip_derep_reads: reads per piece of a call (at least 1; default and at most 65 536)
 *   DADA2HIP_DEREP_PIECE_BYTES=<n>     ... bases per piece (at least 1; default and at most 32 MiB; a longer read is a piece of its own)
 *   DADA2HIP_DEREP_TABLE=<n>           the device dereplicator: slots of its table at the start (a power of two from 8 on; default 131 072)
 *   DADA2HIP_DEREP_HASH_BITS=<k>       ... its hash masked to k bits (0..64; default 64; 0: every read collides with every other)
 *   DADA2HIP_DD_SAMPLE_BLOCKS=<n>      dada2hip_derep_reads_resident and the fused _resident entries: block cap of the kernel that writes the
 *                                      sample's rows (default 4 096; a small value makes its waves stride over the uniques)
 *   DADA2HIP_MERGE_HASH_BITS=<k>       dada2hip_merge_run: the pair table's hash masked to k bits (0..64; default 64; 0: every pair walks from slot 0)
 *   DADA2HIP_MERGE_CHUNK=<n>           ... unique pairs per chunk of the aligner (at least 1; default and at most 65 536)
 *   DADA2HIP_PRIORS_LDS_KEYS=<n>       dada2hip_sample_set_prior_seqs: up to n distinct prefix keys are searched in LDS, more in global
 *                                      memory (default 4 096, at most 6 144; 0 = always global memory)
 *   DADA2HIP_BIMERA_SLOTS=<n>          dada2hip_bimera_denovo: work slots per launch (at least one chunk of the aligner; default and at most
 *                                      what a launch of dada2hip_table_bimera2 holds)
 *   DADA2HIP_PROFILE=1, DADA2HIP_V2_SUMMARY, DADA2HIP_V2_DEBUG   per-launch device times in the stats; traces on stderr
 * Test / tuning knobs (sizes of rings and grids, forced growth paths, injected failures) are listed with their meaning in
 * knobs.h and DESIGN.md §10b; they are not part of the interface.
 */
#ifndef DADA2HIP_H
#define DADA2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DADA2HIP_OK            0
#define DADA2HIP_ERR_INPUT     1   /* validation failure (messages of src/Rmain.cpp:52-78) */
#define DADA2HIP_ERR_DEVICE    2   /* no usable GPU / HIP runtime error */
#define DADA2HIP_ERR_RUNTIME   3   /* runtime error of the algorithm ("Bad lambda." ...) */
#define DADA2HIP_ERR_UNSUPPORTED 4 /* input outside what the device path represents (N / IUPAC codes in nwalign, band 0 in nwvec) */
#define DADA2HIP_ERR_ABORTED   5   /* should_abort() returned non-zero (Rcpp::checkUserInterrupt analogue) */
#define DADA2HIP_ERR_INTERNAL  6   /* a bound the library sets for itself was reached (the device dereplicator's rounds, its table) */

#define DADA2HIP_NA_INTEGER (-2147483647 - 1)   /* R's NA_integer_ */

/* The 23 scalars dada_uniques takes positionally (src/Rmain.cpp:33-47); doubles first so the
 * struct has no padding (112 bytes).  Defaults and normalisation: R/dada.R:1-27, :222-237. */
typedef struct dada2hip_opts {
  double kdist_cutoff, omegaA, omegaP, omegaC, min_fold;
  int32_t match, mismatch, gap, homo_gap, band_size, max_clust, min_hamming, min_abund;
  int32_t use_kmers, detect_singletons, use_quals, final_consensus, vectorized_alignment;
  int32_t multithread, verbose, SSE, gapless, greedy;
} dada2hip_opts;

/* Optional host callbacks (replace Rprintf and Rcpp::checkUserInterrupt, src/Rmain.cpp:317-333). */
typedef struct dada2hip_hooks {
  void (*log)(const char *msg, void *user);
  int (*should_abort)(void *user);   /* polled once per divisive round */
  void *user;
} dada2hip_hooks;

typedef struct dada2hip_sample dada2hip_sample;   /* uniques of one sample, resident in HBM */
typedef struct dada2hip_result dada2hip_result;

/* Counters of one run (the reference's nalign/nshroud, src/dada.h:113-114, plus device timings). */
typedef struct dada2hip_stats {
  uint64_t ncompare;     /* raws offered to b_compare over all rounds (nraw x rounds)            */
  uint64_t nskipped;     /* greedy skips: reads > centre reads, or locked (cluster.cpp:127-130)  */
  uint64_t nshroud;      /* k-mer screened out (nwalign_endsfree.cpp:51-53)                      */
  uint64_t ngapless;     /* gapless pairings (:54-55)                                            */
  uint64_t nnw;          /* banded NW alignments incl. the final-subs pass (:57-64)              */
  uint64_t nshuffle;     /* b_shuffle2 calls                                                     */
  uint64_t nstored;      /* Comparisons kept (cluster.cpp:189-199)                               */
  uint32_t rounds;       /* b_compare rounds = final number of partitions                        */
  uint32_t kernel_times_sampled;  /* 1: nw/screen_kernel_ms are EXTRAPOLATED from sampled launches (round 0, every 8th
                                     round, the final pass); 0: every launch was event-timed (DADA2HIP_PROFILE=1)  */
  /* host wall-clock split of the call: upload = sample creation (marshalling + H2D + k-mer build), screen = enqueue
   * of the compare kernels, bookkeep = round tails incl. waiting for the device, final = final pass + outputs */
  double ms_total, ms_upload, ms_screen, ms_nw, ms_gapless, ms_bookkeep, ms_pval, ms_final;
  double nw_kernel_ms;   /* HIP-event time of the NW kernel launches (see kernel_times_sampled)  */
  uint64_t nw_kernel_launches;
  uint64_t nw_cells;     /* DP cells those launches filled (algorithmic work)      */
  double screen_kernel_ms;
  uint64_t screen_kernel_launches;
  uint64_t screen_bytes; /* algorithmic bytes the screen launches had to read                     */
  /* device time per kernel class, summed over every launch; filled only under DADA2HIP_PROFILE=1 (else 0) */
  double dev_ms_screen, dev_ms_nw, dev_ms_shuffle, dev_ms_pval, dev_ms_birth, dev_ms_final;
  /* host side of the device-driven round loop: waiting for published round results (= the device is the bottleneck),
   * replaying moves / births on the host mirror, enqueuing launches; uniques moved by b_shuffle2 over the run */
  double ms_wait_device, ms_replay, ms_enqueue;
  uint64_t nmoves, batch_compares;
  /* pairs the aligner processed for the rounds' batch compares (device-driven rounds align a whole batch - up to eight
   * coming centres - in one launch, as of the screen: a pair the greedy rule skips when its round commits, or whose batch
   * position is never used, is aligned in vain; nnw / ngapless above stay the reference's counts) */
  uint64_t nnw_run, ngapless_run;
  /* rounds enqueued without the launches of a batch compare because their centre was expected to be cached, and how many
   * of those guesses were wrong (the device then halts and the host sends the full chain) */
  uint64_t lite_chains, lite_misses;
  /* persistent round tail (one launch runs rounds back to back until the next batch compare is due): launches, blocks of the
   * launch, pauses (a round whose mover lists did not fit its result block), shuffle calls; under DADA2HIP_PROFILE=1 also the
   * device time of those launches and what block 0 of them spent in each phase (barriers = waiting for the other blocks,
   * which includes the serial end of the round run by the last arriver) */
  uint64_t tail_launches, tail_pauses, tail_levels;
  uint32_t tail_blocks;
  uint32_t tail_fallbacks;   /* persistent launches whose entry barrier failed (blocks not co-resident): the run went on on the launch chains */
  double dev_ms_tail, tail_ms_entry, tail_ms_shuffle0, tail_ms_shuffle_more, tail_ms_pupdate, tail_ms_barriers, tail_ms_birth,
      tail_ms_publish, tail_ms_release;
  /* the NEXT batch's compare under the persistent tail (second stream): prefetch compares launched; rounds whose centre came out
   * of a prefetched batch; how often the tail had to spin for a prefetch still in flight / left its launch for one; centres
   * prefetched; threads per block of the tail; 1 if the overlap was on.  Under DADA2HIP_PROFILE=1: device time of the
   * prefetch compares' screen and aligner launches (they run INSIDE the interval of dev_ms_tail) */
  uint64_t pf_compares, pf_hits, pf_waits, pf_exits, pf_centres;
  uint32_t tail_threads, overlap_on;
  double dev_ms_pf_screen, dev_ms_pf_nw;
  uint32_t tail_xcd_barrier;   /* 1: the persistent launches of the run used the XCD-hierarchical grid barrier */
  uint32_t tail_mirror;        /* 1: ... and kept the per-unique facts their sweeps ask for in LDS for the life of a launch (DADA2HIP_V3_MIRROR) */
  /* host wall of what stands in front of the rounds: setup = state buffers, memsets, the host mirror of b_init; round0 = the
   * comparison of every unique with the first centre (Rmain.cpp:309-310) up to the first enqueue of the rounds */
  double ms_setup, ms_round0;
  /* under DADA2HIP_PROFILE=1: what the serial end of the rounds spent spinning for a prefetch compare still in flight, and
   * planning the next prefetch (both are part of tail_ms_birth) */
  double tail_ms_pf_wait, tail_ms_pf_plan;
  /* batch compares on the default scores run a pointer-free first pass of the aligner (k_nw_ad<.., FAST>): the pairs it could
   * not finish - walks with an interior gap - and handed to the full kernel, and the pairs the pass looked at (of nnw_run: the pass
   * switches itself off for the rest of a run once more than a quarter came back) */
  uint64_t nnw_retry, nnw_fast;
  /* batch screens with the 5-mer presence bitmaps: uniques (summed over the batch screens, each up to 8 centres) whose class
   * word the 128-byte bound did not settle, i.e. that went through the exact k-mer walk */
  uint64_t screen_stage2;
  /* NW pairs the rounds committed (nnw without round 0, the final pass and the birth pairs): nnw_run - nnw_rounds were aligned in
   * vain - their batch position was never used, or a greedy skip dropped the pair when its round committed */
  uint64_t nnw_rounds;
} dada2hip_stats;

/* ---- whole-call form: exactly dada_uniques (src/Rmain.cpp:30) ---------------------------------
 * seqs       nraw NUL-terminated ACGT strings (abundance-sorted, R/sequenceIO.R:98)
 * abundances nraw ints; priors nraw bytes (0/1) or NULL
 * err        16 x err_ncol doubles, COLUMN-major (R NumericMatrix), rows A2A,A2C,..,T2T
 * quals      quals_nrow x nraw doubles, column-major: positions are rows, uniques are columns
 *            (src/Rmain.cpp:69,113); quals_nrow must equal the longest sequence.  Required: the
 *            reference dereferences it unconditionally (src/error.cpp:158) and R always passes it.
 * device     HIP device ordinal (the reference has no such notion; the R glue passes 0). */
int dada2hip_dada_uniques(int32_t nraw, const char *const *seqs, const int32_t *abundances,
                          const uint8_t *priors, const double *err, int32_t err_ncol, const double *quals,
                          int32_t quals_nrow, const dada2hip_opts *opts, int32_t device,
                          const dada2hip_hooks *hooks, dada2hip_result **out, char *errbuf, size_t errlen);

/* ---- batch form: the per-sample loop of dada() (R/dada.R:266-366 calls dada_uniques once per sample, serially)
 * spread over the GPUs of one node.  Samples only share `err`, so sample i simply runs on
 * device_ids[i % n_devices], one host thread per entry of device_ids, the samples of a thread in order; out[i]
 * receives sample i's result (all NULL on failure; errbuf then names the first failing sample).  The caller sums
 * the results' $subqual matrices (accumulateTrans, R/errorModels.R:462-471).  n_devices <= 0: device 0 only. */
typedef struct dada2hip_sample_input {
  int32_t nraw;
  int32_t quals_nrow;
  const char *const *seqs;
  const int32_t *abundances;
  const uint8_t *priors;      /* may be NULL */
  const double *quals;
} dada2hip_sample_input;
int dada2hip_run_multi(int32_t n_samples, const dada2hip_sample_input *samples, const double *err, int32_t err_ncol,
                       const dada2hip_opts *opts, int32_t n_devices, const int32_t *device_ids, dada2hip_result **out,
                       char *errbuf, size_t errlen);

/* Device and pinned-host allocations are cached per process between calls (the "per-device context cache" of a
 * drop-in replacement: back-to-back dada_uniques calls do not pay hipMalloc / hipFree again); this hands every cached
 * block back to the runtime.  DADA2HIP_ALLOC_CACHE=0 disables the cache. */
void dada2hip_trim_cache(void);

/* Test hook.  What DADA2HIP_ALLOC_POISON has filled since the process started: out[0] device blocks, out[1] device bytes, out[2]
 * pinned blocks, out[3] pinned bytes (all 0 while the knob has never been set: a test reads from it that its knob was live). */
void dada2hip_alloc_poison_stats(int64_t out[4]);

/* ---- resident form --------------------------------------------------------------------------- */
int dada2hip_sample_create(int32_t nraw, const char *const *seqs, const int32_t *abundances,
                           const uint8_t *priors, const double *quals, int32_t quals_nrow, int32_t device,
                           dada2hip_sample **out, char *errbuf, size_t errlen);
int dada2hip_sample_set_priors(dada2hip_sample *s, const uint8_t *priors, char *errbuf, size_t errlen);
/* Priors given as SEQUENCES - names(uniques) %in% c(priors, pseudo_priors), R/dada.R:335 - matched on the device against the resident
 * uniques: the flag of unique i becomes (or_flags ? or_flags[i] != 0 : 0) | (its sequence is one of seqs).  Entries of seqs with a
 * letter outside upper-case A/C/G/T, or empty, match nothing and are no error (%in% does not mind them); duplicates are allowed.
 * first_match (optional, N entries): R's match(uniques, seqs) - 1, the SMALLEST index of an equal entry, -1 for none.  nset
 * (optional): the flags set after the call.  n == 0 clears the flags, or leaves exactly or_flags.  A sharded sample flags all N
 * uniques, as dada2hip_sample_set_priors does.  dada2hip_sample_prior_seqs_stats: the words of the sample's LAST such call
 * (DADA2HIP_PRIOR_SEQS_NSTATS int64): [0] entries given, [1] entries kept, [2] distinct prefix keys, [3] 1 = the keys were staged in
 * LDS (DADA2HIP_PRIORS_LDS_KEYS), [4] flags set, [5] blocks launched, [6] host packing and tables, [7] the host's wall time from the first upload to the end of the
 * copy back (the kernel inside it), [8] the kernel by device events (DADA2HIP_PROFILE=1 only), [9] the whole call; [6]-[9] microseconds. */
#define DADA2HIP_PRIOR_SEQS_NSTATS 16
int dada2hip_sample_set_prior_seqs(dada2hip_sample *s, int32_t n, const char *const *seqs, const uint8_t *or_flags,
                                   int32_t *first_match, int32_t *nset, char *errbuf, size_t errlen);
void dada2hip_sample_prior_seqs_stats(const dada2hip_sample *s, int64_t *stats);
int dada2hip_sample_run(dada2hip_sample *s, const double *err, int32_t err_ncol, const dada2hip_opts *opts,
                        const dada2hip_hooks *hooks, dada2hip_result **out, char *errbuf, size_t errlen);
void dada2hip_sample_free(dada2hip_sample *s);

/* ---- one sample over several GPUs (last row: "intra-sample sharding") --------------
 * The reference has no counterpart: a sample is one serial dada_uniques call (R/dada.R:266).  Here every rank (one
 * process per GPU) holds the whole sample's sequences, qualities and k-mer records, and does the per-unique work of
 * run_dada - b_compare (src/cluster.cpp:90-204), b_shuffle2's arg-max (:229-239), b_p_update (src/pval.cpp:14-40), the
 * first stage of b_bud (src/cluster.cpp:284-308), the final alignments (src/Rmain.cpp:172-236) - for ONE contiguous
 * block of the uniques, [nraw * rank / world, nraw * (rank + 1) / world).  What the reference's serial bookkeeping
 * shares between uniques is exchanged through `exchange` at fixed points, the same sequence on every rank:
 *   per b_shuffle2 call   the (unique, from, to) triples that moved  (all ranks replay all of them in the reference's order:
 *                         partition reads, member slots and the arg-max snapshot of the next call stay identical everywhere)
 *   per b_bud             the candidate records of each rank's best key and its near ties (48 B each)
 *   at the end            p-value / correction / substitution count of every unique, the transition and quality sums
 * and every rank returns the complete, identical result.  The round loop runs host-driven (one centre per round, every
 * decision on the host): the exchanges sit between its kernels.
 *   kind 0  all-gather: every rank contributes send_bytes bytes (the same count on all ranks); recv receives
 *           world * send_bytes bytes in rank order
 *   kind 1  all-reduce(sum) of send_bytes / 8 int64 values; send == recv (in place)
 * `exchange` returns 0 on success; anything else aborts the run with DADA2HIP_ERR_RUNTIME on that rank.
 * Failure protocol: every exchange point opens with an 8-byte kind-0 gather of a size; a rank that has failed between two points
 * contributes -1 at the next one (one extra call of `exchange`, not made once the run's last exchange point is behind it), and
 * its peers return DADA2HIP_ERR_RUNTIME there.  A collective that never completes - a rank that died, a transport that is gone -
 * is `exchange`'s own to time out: the library never waits for a peer by itself. */
typedef struct dada2hip_shard {
  int32_t rank, world;
  int (*exchange)(void *user, int32_t kind, const void *send, int64_t send_bytes, void *recv);
  void *user;
} dada2hip_shard;
int dada2hip_sample_run_sharded(dada2hip_sample *s, const double *err, int32_t err_ncol, const dada2hip_opts *opts,
                                const dada2hip_hooks *hooks, const dada2hip_shard *shard, dada2hip_result **out,
                                char *errbuf, size_t errlen);
int32_t dada2hip_sample_nraw(const dada2hip_sample *s);
int32_t dada2hip_sample_maxlen(const dada2hip_sample *s);

/* ---- result access (library-owned arrays, valid until dada2hip_result_free) -------------------
 * $clustering (src/error.cpp:121-126): one row per partition. */
int32_t dada2hip_result_nclust(const dada2hip_result *r);
int32_t dada2hip_result_nraw(const dada2hip_result *r);
int32_t dada2hip_result_maxlen(const dada2hip_result *r);
int32_t dada2hip_result_ncol(const dada2hip_result *r);          /* columns of $subqual */
int32_t dada2hip_result_nbirth_subs(const dada2hip_result *r);
const char *dada2hip_result_sequence(const dada2hip_result *r, int32_t i);
const int32_t *dada2hip_result_abundance(const dada2hip_result *r);
const int32_t *dada2hip_result_n0(const dada2hip_result *r);
const int32_t *dada2hip_result_n1(const dada2hip_result *r);
const int32_t *dada2hip_result_nunq(const dada2hip_result *r);
const double *dada2hip_result_clust_pval(const dada2hip_result *r);
const int32_t *dada2hip_result_birth_from(const dada2hip_result *r);   /* 1-based, NA for row 0 */
const double *dada2hip_result_birth_pval(const dada2hip_result *r);
const double *dada2hip_result_birth_fold(const dada2hip_result *r);
const int32_t *dada2hip_result_birth_ham(const dada2hip_result *r);
const double *dada2hip_result_birth_qave(const dada2hip_result *r);
const int32_t *dada2hip_result_center(const dada2hip_result *r);       /* 0-based unique index of each centre (extra) */
/* $birth_subs (src/error.cpp:299) */
const int32_t *dada2hip_result_bs_pos(const dada2hip_result *r);       /* 1-based */
const char *dada2hip_result_bs_ref(const dada2hip_result *r);          /* one char per row */
const char *dada2hip_result_bs_sub(const dada2hip_result *r);
const double *dada2hip_result_bs_qual(const dada2hip_result *r);
const int32_t *dada2hip_result_bs_clust(const dada2hip_result *r);     /* 1-based */
/* $subqual 16 x ncol int32 column-major; $clusterquals maxlen x nclust double column-major (NA past the
 * centre's length); $map nraw int32 (1-based or NA); $pval nraw double. */
const int32_t *dada2hip_result_subqual(const dada2hip_result *r);
const double *dada2hip_result_clusterquals(const dada2hip_result *r);
const int32_t *dada2hip_result_map(const dada2hip_result *r);
const double *dada2hip_result_pval(const dada2hip_result *r);
void dada2hip_result_stats(const dada2hip_result *r, dada2hip_stats *out);
void dada2hip_result_free(dada2hip_result *r);

/* ---- pairwise alignment exports ---------------------------------------------------------------
 * dada2hip_nwalign == C_nwalign(s1, s2, match, mismatch, gap_p, homo_gap_p, band, endsfree)
 * (src/evaluate.cpp:18): ACGT in, two gapped strings out (capacity >= len1+len2+1 each).
 * dada2hip_nwvec == C_nwvec (src/nwalign_vectorized.cpp:321): n pairs at once; out[2*i], out[2*i+1]
 * are caller buffers of capacity >= len1_i+len2_i+1.  Both run the device NW kernel, and all of C_nwalign's aligners
 * are there: nwalign_endsfree (src/nwalign_endsfree.cpp:76-216), nwalign_endsfree_homo when homo_gap_p != gap_p
 * (:220-396: a gap opposite a base of a homopolymer run of >= 3 costs homo_gap_p) and, with endsfree = 0, the global
 * nwalign (:403-537; C_nwvec: nwalign_vectorized2 with end_gap_p = gap_p, src/nwalign_vectorized.cpp:333). */
int dada2hip_nwalign(const char *s1, const char *s2, int32_t match, int32_t mismatch, int32_t gap_p,
                     int32_t homo_gap_p, int32_t band, int32_t endsfree, int32_t device, char *out0, char *out1,
                     char *errbuf, size_t errlen);
int dada2hip_nwvec(int32_t n, const char *const *s1, const char *const *s2, int32_t match, int32_t mismatch,
                   int32_t gap_p, int32_t band, int32_t endsfree, int32_t device, char *const *out,
                   char *errbuf, size_t errlen);

/* ---- bimera identification: the step after dada() ------------------------------------------
 * dada2hip_table_bimera2 == C_table_bimera2(mat, seqs, min_fold, min_abund, allow_one_off, min_one_off_par_dist, match,
 * mismatch, gap_p, max_shift) (src/chimera.cpp:192): mat is the nrow (samples) x ncol (sequences) integer table, column-major
 * as R holds it; nflag[ncol] / nsam[ncol] receive the two columns of the returned data.frame.  Every (sequence, more abundant
 * parent) alignment the table asks for runs on the device NW kernel (band = max_shift, ends-free: the denoising path's
 * aligner, chimera.cpp:122), get_lr / get_ham_endsfree (:211-293) on the device too.
 * dada2hip_is_bimera == C_is_bimera (src/chimera.cpp:18): *out = 1 / 0. */
int dada2hip_table_bimera2(int32_t nrow, int32_t ncol, const int32_t *mat, const char *const *seqs, double min_fold,
                           int32_t min_abund, int32_t allow_one_off, int32_t min_one_off_par_dist, int32_t match,
                           int32_t mismatch, int32_t gap_p, int32_t max_shift, int32_t device, int32_t *nflag, int32_t *nsam,
                           char *errbuf, size_t errlen);
int dada2hip_is_bimera(const char *sq, int32_t npars, const char *const *pars, int32_t allow_one_off,
                       int32_t min_one_off_par_dist, int32_t match, int32_t mismatch, int32_t gap_p, int32_t max_shift,
                       int32_t device, int32_t *out, char *errbuf, size_t errlen);
/* dada2hip_bimera_pairs: the quantities the two entry points above reduce to a decision, for n (query, parent) pairs:
 * out[5 i .. 5 i + 4] = left, right, left_oo, right_oo of get_lr (src/chimera.cpp:243-293) and get_ham_endsfree (:211-239) on the
 * alignment nwalign_vectorized2(query, parent, match, mismatch, gap_p, 0, max_shift) (chimera.cpp:26,122).  The reference keeps
 * them inside C_is_bimera / BimeraTableParallel; this entry exists so that parity can be checked per alignment and not only
 * per flagged sequence (tests/, oracle_bimera_pairs). */
int dada2hip_bimera_pairs(int32_t n, const char *const *queries, const char *const *parents, int32_t allow_one_off,
                          int32_t match, int32_t mismatch, int32_t gap_p, int32_t max_shift, int32_t device, int32_t *out,
                          char *errbuf, size_t errlen);

/* dada2hip_bimera_denovo == isBimeraDenovo (R/chimeras.R:105-154) on every row of an integer table, the sequences resident once:
 * mat is nrow x ncol, column-major as for dada2hip_table_bimera2 (nrow = 1: a uniques vector); flags[i + j * nrow] = 1 when
 * sequence j is a bimera of row i's more abundant sequences.  The parents of query j in a row are the sequences k with
 * mat[k] > min_fold * mat[j] and mat[k] > min_parent_abund (:127: both compared as doubles, both strict); fewer than two parents
 * give 0 without an alignment (:128).  That set is a prefix of the row's ranking by abundance, so the device is told the ranking
 * and one integer per query, visits the parents in windows of ranks - most abundant first - and drops a query from the work as
 * soon as a model is complete (C_is_bimera's running maxima, src/chimera.cpp:29-50, only grow: the answer is the reference's).
 * skip_zero: queries of abundance 0 get 0 without work (removeBimeraDenovo's "per-sample" zeroes those cells anyway).
 * Abundances must not be negative; the sequences are A/C/G/T only and max_shift is not 0, as for dada2hip_table_bimera2.
 * stats (optional, DADA2HIP_BIMERA_DENOVO_NSTATS int64): [0] sequences, [1] rows, [2] queries with at least two parents,
 * [3] pairs possible (the sum of their parents), [4] pairs aligned, [5] windows, [6] launches of the aligner, [7] flags set,
 * [8] the aligner's route (1 = k_nw_ad in its bimera mode, 2 = the lane kernel + k_bimera_lr), [9] slots per chunk of the aligner,
 * [10] the slot budget of a launch, [11] us of ranking and packing, [12] us of device work as the host sees it, [13] us of kernels
 * (event-timed under DADA2HIP_PROFILE=1, else 0), [14] us in total. */
#define DADA2HIP_BIMERA_DENOVO_NSTATS 16
int dada2hip_bimera_denovo(int32_t nrow, int32_t ncol, const int32_t *mat, const char *const *seqs, double min_fold,
                           double min_parent_abund, int32_t allow_one_off, int32_t min_one_off_par_dist, int32_t match,
                           int32_t mismatch, int32_t gap_p, int32_t max_shift, int32_t skip_zero, int32_t device, uint8_t *flags,
                           int64_t *stats, char *errbuf, size_t errlen);

/* The two kernels of dada2hip_bimera_denovo on arrays the caller makes up, so that they can be held to restatements on hand-made
 * records (tests/).  n sequences; nq live queries `live`, parent ranks [r0, r0 + wr), wr a multiple of per, nq * wr <= 2^23.
 * worklist_probe: rank[n], P[n], flags[n] in; chunk_centre[nq * wr / per] and work[nq * wr] out (slot (q, r): rank[r] while
 * r < P[q] and flags[q] == 0, else -1).  fold_probe: work[nq * wr], rec[5 * nq * wr] (left, right, left_oo, right_oo, hamming of
 * each slot that names a parent), len[n], P[n] in; maxima[6 n] and flags[n] in and out; with last != 0 the queries still unflagged
 * with P > r0 + wr go to next_live (any order; the rest of its nq entries is -1) and are counted in *n_next; *aligned = the slots
 * that named a parent. */
int dada2hip_bimera_worklist_probe(int32_t n, const int32_t *rank, const int32_t *P, const uint8_t *flags, int32_t nq,
                                   const int32_t *live, int32_t r0, int32_t wr, int32_t per, int32_t device, int32_t *chunk_centre,
                                   int32_t *work, char *errbuf, size_t errlen);
int dada2hip_bimera_fold_probe(int32_t n, const int32_t *len, const int32_t *P, int32_t nq, const int32_t *live, int32_t r0,
                               int32_t wr, const int32_t *work, const int32_t *rec, int32_t allow_one_off,
                               int32_t min_one_off_par_dist, int32_t last, int32_t device, int32_t *maxima, uint8_t *flags,
                               int32_t *next_live, int32_t *n_next, int64_t *aligned, char *errbuf, size_t errlen);

/* ---- dereplication front-end: the step before dada() ----------------------------------------
 * dada2hip_derep_fastq == derepFastq(fl, n = chunk_reads, qualityType = "Auto" | offset) (R/sequenceIO.R:45-124 on top of
 * qtables2, :150-183): reads one FASTQ file (plain or gzip), dereplicates it and returns the `derep-class` content:
 *   seqs[nuniques]        the unique sequences, by decreasing abundance (ties: first chunk seen, then C-locale lexical)
 *   abundances[nuniques]  $uniques
 *   quals                 $quals as nuniques rows of maxlen doubles (row u = mean quality per position of unique u, NA past
 *                         its length) — which IS the column-major maxlen x nuniques matrix dada2hip_dada_uniques takes
 *   map[nreads]           $map, 0-BASED unique index per read (DADA2HIP_NA_INTEGER for zero-length reads)
 * chunk_reads <= 0 means the reference's default 1e6; qual_offset 33 / 64, or 0 for "Auto" (ShortRead's rule: a character
 * below ';' anywhere in the first chunk => Phred+33, else +64).  Host-side: no device is touched.
 * dada2hip_sample_from_derep uploads the object as a resident sample without another host copy. */
typedef struct dada2hip_derep dada2hip_derep;
int dada2hip_derep_fastq(const char *path, int64_t chunk_reads, int32_t qual_offset, dada2hip_derep **out, char *errbuf,
                         size_t errlen);
int32_t dada2hip_derep_nuniques(const dada2hip_derep *d);
int64_t dada2hip_derep_nreads(const dada2hip_derep *d);
int32_t dada2hip_derep_maxlen(const dada2hip_derep *d);
const char *const *dada2hip_derep_seqs(const dada2hip_derep *d);
const int32_t *dada2hip_derep_abundances(const dada2hip_derep *d);
const double *dada2hip_derep_quals(const dada2hip_derep *d);   /* NULL for an object without a matrix (dada2hip_derep_has_quals) */
const int32_t *dada2hip_derep_map(const dada2hip_derep *d);
void dada2hip_derep_free(dada2hip_derep *d);
int dada2hip_sample_from_derep(const dada2hip_derep *d, const uint8_t *priors, int32_t device, dada2hip_sample **out,
                               char *errbuf, size_t errlen);
/* An object from a _resident entry (below) has no quality matrix: dada2hip_derep_has_quals is 0, dada2hip_derep_quals is NULL,
 * and dada2hip_sample_from_derep, dada2hip_derep_combine (for a view with quals == NULL) return DADA2HIP_ERR_INPUT with one
 * message that says so.  dada2hip_derep_qmax is ceiling(max(derep$quals, na.rm = TRUE)) (R/dada.R:290) of either kind of object:
 * from the matrix, or the word the device stored. */
int32_t dada2hip_derep_has_quals(const dada2hip_derep *d);
int32_t dada2hip_derep_qmax(const dada2hip_derep *d);

/* ---- dereplication on the device: reads in memory, or the reads filterAndTrim keeps, to a derep object ------------------
 * dada2hip_derep_reads: n reads in the layout of dada2hip_filter_reads (read r is seq / qual[offsets[r] .. offsets[r + 1]))
 * to an ordinary dada2hip_derep - every accessor above, dada2hip_sample_from_derep and dada2hip_derep_combine take it - that
 * equals in every field what dada2hip_derep_fastq returns for a file of these reads: chunks of chunk_reads (<= 0: 1e6), new
 * uniques of a chunk in C-locale lexical order behind those of earlier chunks, the stable order by decreasing abundance, means
 * as integer sums divided by the count, NA past a unique's length, map 0-based with NA for zero-length reads; sequences are
 * compared as bytes.  qual_offset 33, 64 or 0 = Auto, judged on the FIRST chunk only (a character below ';' anywhere in it:
 * +33, else +64): the raw quality characters are summed in 64-bit words and count x offset is taken off at the end.  n above
 * 2^31 - 1 and a read above 2^31 - 129 bytes are DADA2HIP_ERR_INPUT; only zero-length reads (or none): DADA2HIP_ERR_INPUT
 * "Only zero-length sequences detected during dereplication.".  The reads go up in pieces (DADA2HIP_DEREP_PIECE, _PIECE_BYTES);
 * the table of uniques, their bytes and their sums stay on the device until the call's end, when one row per unique and one
 * word per read come back; the order, the division and the map's renumbering are the host's.  A round bound or a full table
 * reached is DADA2HIP_ERR_INTERNAL, never another round.
 * stats (optional, DADA2HIP_DEREP_NSTATS int64 words): [0] reads in, [1] uniques, [2] the table's capacity at the end, [3] its
 * rebuilds, [4] collision rounds (rounds of a piece beyond its first: a read that met other bytes under its own hash moved one
 * slot on), [5] pieces, [6] bytes copied to the device, [7] bytes copied back, [8] host microseconds of the upload, [9] device
 * microseconds of the derep kernels, [10] host microseconds of the download at the end, [11] of the finalisation, [12] of the
 * whole call. */
#define DADA2HIP_DEREP_NSTATS 16
int dada2hip_derep_reads(int64_t n, const char *seq, const char *qual, const int64_t *offsets, int64_t chunk_reads,
                         int32_t qual_offset, int32_t device, dada2hip_derep **out, int64_t *stats, char *errbuf, size_t errlen);

/* ---- ... and straight to a resident sample ------------------------------------------------------------------------------
 * dada2hip_derep_reads_resident takes dada2hip_derep_reads' arguments and returns the derep object AND the resident sample that
 * dada2hip_sample_from_derep would make of it (no priors) - without the quality sums leaving the device.  At the end of the call
 * the device holds the uniques' letters, a 64-bit sum per base and the counts: 28 bytes per unique and the letters come down
 * (for the order, the strings, the abundances and the map), the order goes up at 4 bytes per unique, and one kernel writes the
 * sample's rows where the data lies: the letters packed into 2-bit words, the sums less count x offset rounded to the byte
 * that round(mean) gives (on integers: half away from zero, a mean that rounds below 0 or above 255 is the reference's
 * "Quality values must be positive integers."), every pad word and byte zero.  The rows are byte for byte those of the host
 * route; the k-mer records are built behind them and the packed rows come down once, into the sample's host mirror.
 * *out is a derep object WITHOUT a quality matrix (above): sequences, abundances, map, maxlen, nreads and dada2hip_derep_qmax are
 * those of dada2hip_derep_reads' object.  The sample is an ordinary one: dada2hip_sample_run, _set_priors, _set_prior_seqs, _free.
 * Errors: dada2hip_derep_reads', and the input errors of dada2hip_sample_create with its texts and in its order (a read at or
 * above the maximum length, a read of at most five bases, a letter outside A/C/G/T, a mean that is no byte).  On any error the
 * call returns NEITHER object - dada2hip_derep_reads would have returned the derep object, and dada2hip_sample_from_derep failed.
 * resident_stats (optional, DADA2HIP_RESIDENT_NSTATS int64 words, the finish alone): [0] bytes copied down (the rows, the host
 * mirror, the tallies), [1] bytes copied up (the order), [2] host microseconds of the rows' download, [3] of the order, the object
 * and the order's upload, [4] device microseconds of the kernel, [5] of the k-mer build, [6] of the mirror's download, [7] blocks
 * the kernel was launched with (DADA2HIP_DD_SAMPLE_BLOCKS caps them), [8] uniques.  stats: dada2hip_derep_reads' words. */
#define DADA2HIP_RESIDENT_NSTATS 16
int dada2hip_derep_reads_resident(int64_t n, const char *seq, const char *qual, const int64_t *offsets, int64_t chunk_reads,
                                  int32_t qual_offset, int32_t device, dada2hip_derep **out, dada2hip_sample **sample,
                                  int64_t *stats, int64_t *resident_stats, char *errbuf, size_t errlen);
/* The rows of a resident sample as they lie on the device, padding included (any of the four may be NULL):
 * geometry[DADA2HIP_SAMPLE_ROWS_NGEOM] = uniques N, W2, LQ, maxlen, minlen, qmax (the largest quality byte), 0, 0;
 * seq2[N * W2] the 2-bit words, len[N], reads[N], qual[N * LQ] the rounded quality bytes.  Ask for the geometry first. */
#define DADA2HIP_SAMPLE_ROWS_NGEOM 8
int dada2hip_sample_rows(dada2hip_sample *s, int32_t *geometry, uint32_t *seq2, int32_t *len, uint32_t *reads, uint8_t *qual,
                         char *errbuf, size_t errlen);

/* ---- pooling: the samples' derep objects into one (combineDereps2, R/multiSample.R:165-203; dada(pool = TRUE), R/dada.R:189-192) ----
 * A view is one sample as the accessors above expose it, or as the caller holds it.  dada2hip_derep_combine returns an ordinary
 * dada2hip_derep - every accessor above and dada2hip_sample_from_derep take it - that equals combineDereps2 field for field:
 *   seqs        the union of the samples' uniques: order of first appearance over the samples as given, each sample's uniques in
 *               their own order, then ordered by decreasing summed abundance, stably (R's order(decreasing = TRUE))
 *   abundances  int32 sums; a sum past INT32_MAX is DADA2HIP_ERR_INPUT (R: NA and a warning)
 *   quals       per pooled unique and position acc = 0.0; acc = acc + q * (double)abundance for each contributing sample in sample
 *               order - a multiply and an add, each rounded, never fused -; acc / (double)sum.  NA past the unique's length and past
 *               the maxlen of a contributing sample that is narrower (the cbind(..., NA) of :184); maxlen is the widest sample's
 *   map         the samples' maps one after the other, renumbered to the pooled rows; DADA2HIP_NA_INTEGER stays
 * unique_to_pool (optional; sum of nuniques entries, sample after sample): the 0-based pooled row of every unique of every sample -
 * what the split of a pooled result back into samples needs (R/dada.R:454, :467).  A sample that holds one sequence twice, an empty
 * sequence, a negative abundance or a map entry that names no unique is DADA2HIP_ERR_INPUT.  Host-side: no device is touched. */
typedef struct dada2hip_derep_view {
  int32_t nuniques, maxlen;
  int64_t nreads;
  const char *const *seqs;
  const int32_t *abundances;
  const double *quals;           /* nuniques rows of maxlen doubles, NA past a unique's length */
  const int32_t *map;            /* nreads entries, 0-based, DADA2HIP_NA_INTEGER allowed; may be NULL when nreads == 0 */
} dada2hip_derep_view;
int dada2hip_derep_combine(int32_t nsamples, const dada2hip_derep_view *in, dada2hip_derep **out, int32_t *unique_to_pool,
                           char *errbuf, size_t errlen);

/* ---- mergePairs: denoised forward + reverse reads -> merged amplicons -------------------------
 * dada2hip_merge_pairs == the per-sample body of mergePairs(dadaF, derepF, dadaR, derepR, minOverlap, maxMismatch,
 * returnRejects=TRUE, justConcatenate, trimOverhang) (R/paired.R:113-190).  fwd[i] / rev[i] = dadaF$map[derepF$map][i] /
 * dadaR$map[derepR$map][i]: the 1-BASED denoised-sequence index of read pair i, or DADA2HIP_NA_INTEGER.  seqsF / n0F
 * (seqsR / n0R) are dadaF$clustering$sequence / $n0.  Every unique (forward, reverse) pair is aligned on the device as
 * R's nwalign(F, rc(R), band=-1) does (C_nwalign -> nwalign_endsfree, unbanded, scores 1/-64/-64 when maxMismatch == 0
 * else 1/-8/-8, paired.R:152-159), then C_eval_pair / C_pair_consensus (src/evaluate.cpp:73,124) on the host.
 * Rows come back in the reference's order (first appearance, stably sorted by decreasing abundance) INCLUDING the rejects
 * (accept == 0, sequence ""): returnRejects=FALSE is a filter on `accept`.  prefer is NA with just_concatenate. */
typedef struct dada2hip_mergers dada2hip_mergers;
int dada2hip_merge_pairs(int64_t nreads, const int32_t *fwd, const int32_t *rev, int32_t nF, const char *const *seqsF,
                         const int32_t *n0F, int32_t nR, const char *const *seqsR, const int32_t *n0R, int32_t min_overlap,
                         int32_t max_mismatch, int32_t trim_overhang, int32_t just_concatenate, int32_t device,
                         dada2hip_mergers **out, char *errbuf, size_t errlen);
int32_t dada2hip_mergers_nrow(const dada2hip_mergers *m);
const char *dada2hip_mergers_sequence(const dada2hip_mergers *m, int32_t i);
const int32_t *dada2hip_mergers_abundance(const dada2hip_mergers *m);
const int32_t *dada2hip_mergers_forward(const dada2hip_mergers *m);
const int32_t *dada2hip_mergers_reverse(const dada2hip_mergers *m);
const int32_t *dada2hip_mergers_nmatch(const dada2hip_mergers *m);
const int32_t *dada2hip_mergers_nmismatch(const dada2hip_mergers *m);
const int32_t *dada2hip_mergers_nindel(const dada2hip_mergers *m);
const int32_t *dada2hip_mergers_prefer(const dada2hip_mergers *m);
const int32_t *dada2hip_mergers_accept(const dada2hip_mergers *m);
void dada2hip_mergers_free(dada2hip_mergers *m);

/* ---- the sequence-table stage: collapseNoMismatch, nweval / nwhamming ---------------------------------------------------
 * dada2hip_collapse_nomismatch == the decisions of collapseNoMismatch(seqtab, minOverlap, identicalOnly = identical_only,
 * band = band) (R/multiSample.R:104-160).  mat is the nrow (samples) x ncol (sequences) integer table, column-major as R holds
 * it, seqs its column names.  into[ncol] receives, per input column, the 0-BASED input column its counts end up in: the column
 * itself when it is kept, else the kept column it was added to (a duplicate name goes where its first occurrence goes, so
 * into[into[i]] == into[i]).  The sums, the removal of the other columns and the two column orders (orderBy, then total
 * abundance) are the caller's, from `into`.  identical_only != 0 folds duplicate names only (no device work).
 * Otherwise the columns are processed by decreasing total abundance (stable) in batches; per batch the device decides, for
 * every (query, kept-or-earlier-in-the-batch ref) pair that can pass the reference's prefix screen, whether it passes it and
 * whether its gapless diagonals already rule out an alignment without mismatch or internal indel (collapse.inc.hip); the
 * pairs left are aligned by the pair-form lane aligner as nwalign(query, ref, match, mismatch, gap_p, band = band,
 * endsfree = TRUE) and reduced by C_eval_pair on the host, and the host replays the greedy choice.  With band >= 0 every
 * screened pair is aligned.  Letters outside A/C/G/T: DADA2HIP_ERR_UNSUPPORTED.  A column total or a collapsed cell above
 * INT32_MAX (NA in the reference) is DADA2HIP_ERR_INPUT.
 * stats (optional, DADA2HIP_COLLAPSE_NSTATS int64 words): [0] columns after de-duplication, [1] candidate pairs after the
 * join, [2] pairs scanned, [3] of them screened out, [4] rejected by the bound, [5] pairs aligned, [6] aligned pairs with
 * mismatch + indel == 0, [7] batches, [8..11] host wall time in microseconds of join / scan / align / resolve, [12] of the
 * whole call; the rest 0.
 * dada2hip_collapse_pairs: what the scan kernel computes, for n (query, ref) pairs: out[4 i .. 4 i + 3] = screen (bit 0:
 * substr(query, 1, min_overlap) occurs in ref, bit 1: substr(ref, 1, min_overlap) occurs in query), G (the best score of a
 * gapless diagonal), m_max (the longest diagonal without a mismatch, 0 if none), decision (0 screened out, 1 rejected by
 * G > match * m_max, 2 needs the alignment).
 * dada2hip_nweval == nweval(s1, s2, match, mismatch, gap_p, homo_gap_p, band, endsfree, vec) (R/misc.R:222-225), vectorised:
 * out[3 i .. 3 i + 2] = match, mismatch, indel of C_eval_pair on the alignment of pair i (vec != 0: C_nwvec, else C_nwalign);
 * nwhamming is mismatch + indel. */
#define DADA2HIP_COLLAPSE_NSTATS 16
int dada2hip_collapse_nomismatch(int32_t nrow, int32_t ncol, const int32_t *mat, const char *const *seqs, int32_t min_overlap,
                                 int32_t identical_only, int32_t band, int32_t match, int32_t mismatch, int32_t gap_p,
                                 int32_t device, int32_t *into, int64_t *stats, char *errbuf, size_t errlen);
int dada2hip_collapse_pairs(int32_t n, const char *const *queries, const char *const *refs, int32_t min_overlap, int32_t match,
                            int32_t mismatch, int32_t device, int32_t *out, char *errbuf, size_t errlen);
int dada2hip_nweval(int32_t n, const char *const *s1, const char *const *s2, int32_t match, int32_t mismatch, int32_t gap_p,
                    int32_t homo_gap_p, int32_t band, int32_t endsfree, int32_t vec, int32_t device, int32_t *out,
                    char *errbuf, size_t errlen);

/* ---- mergeSequenceTables (R/multiSample.R:290-364, validation :206-238) ----------------------------------------------------------
 * dada2hip_seqtab_merge merges ntab >= 2 sequence tables.  Table t is nrow[t] (samples) x ncol[t] (sequences) cells, ROW-major
 * int32, at cells[t].  The names of all tables lie table after table: column c of the whole call (the running column number) is
 * col_bytes[col_offsets[c] .. col_offsets[c + 1]), row r is row_bytes[row_offsets[r] .. row_offsets[r + 1]); both offset arrays
 * have one entry more than names.  repeats_sum 0: a sample name in more than one table is DADA2HIP_ERR_INPUT ("Duplicated sample
 * names detected in the sequence table row names: a, b"); otherwise such rows are summed at the name's first place.  order_by 0:
 * the columns stay in order of first appearance; 1: stably by decreasing column sum; 2: by decreasing number of positive cells.
 * try_rc (used when there is more than one distinct sequence): a sequence whose reverse complement appears EARLIER among the distinct
 * sequences is renamed to it in every table and leaves the result; a palindrome never is.  Every letter must then be one of
 * ACGTMRWSYKVHDBN, complemented as Biostrings does; anything else is DADA2HIP_ERR_UNSUPPORTED naming table and column.  Without
 * try_rc names are compared as bytes and may hold anything.
 * DADA2HIP_ERR_INPUT: fewer than two tables; an empty table; a negative cell; a blank name; one name twice among a table's columns or
 * among its rows (the reference only warns); a merged cell above INT32_MAX (NA in the reference).  The sums that order the columns
 * are 64-bit and never an error.  DADA2HIP_ERR_UNSUPPORTED: two merged matrices and the largest table do not fit in half of the
 * device's free memory.
 * The distinct sequences are found by the device dereplicator (DADA2HIP_DEREP_TABLE, _HASH_BITS, _PIECE, _PIECE_BYTES apply), the
 * reverse complements are looked up in its table, and the cells are added, keyed and reordered on the device.
 * col_map (optional, one entry per input column, table after table): the 0-based column of the result an input column went to.
 * stats (optional, DADA2HIP_SEQTAB_NSTATS int64 words): [0] tables, [1] input columns, [2] distinct sequences, [3] sequences
 * flagged as a reverse complement, [4] rows and [5] columns of the result, [6] the table's capacity, [7] its rebuilds, [8] collision
 * rounds, [9] reverse-complement lookups that compared bytes and found them different, [10] pieces, [11] bytes copied to the
 * device, [12] bytes copied back, host microseconds of [13] the uploads of the maps and the cells, [14] the identity of the names
 * (their upload included) and the plans, [15] the reverse-complement lookup, [16] accumulate + column keys + gather, [17] the
 * download, [18] the whole call.
 * The result is owned by the handle until dada2hip_seqtab_free: cells row-major [nrow x ncol]; the names as bytes and offsets. */
#define DADA2HIP_SEQTAB_NSTATS 24
typedef struct dada2hip_seqtab dada2hip_seqtab;
int dada2hip_seqtab_merge(int32_t ntab, const int32_t *nrow, const int32_t *ncol, const int32_t *const *cells, const char *col_bytes,
                          const int64_t *col_offsets, const char *row_bytes, const int64_t *row_offsets, int32_t repeats_sum,
                          int32_t order_by, int32_t try_rc, int32_t device, dada2hip_seqtab **out, int32_t *col_map, int64_t *stats,
                          char *errbuf, size_t errlen);
int32_t dada2hip_seqtab_nrow(const dada2hip_seqtab *t);
int32_t dada2hip_seqtab_ncol(const dada2hip_seqtab *t);
const int32_t *dada2hip_seqtab_cells(const dada2hip_seqtab *t);
const char *dada2hip_seqtab_sequences(const dada2hip_seqtab *t, const int64_t **offsets);   /* ncol + 1 offsets into the bytes */
const char *dada2hip_seqtab_samples(const dada2hip_seqtab *t, const int64_t **offsets);     /* nrow + 1 offsets */
void dada2hip_seqtab_free(dada2hip_seqtab *t);

/* ---- mergePairs over a run (R/paired.R:92-201) -------------------------------------------------------------------------------
 * dada2hip_merge_run == lapply(seq_along(dadaF), ...) of mergePairs() for nsamples samples in one call; dada2hip_merge_pairs above
 * is the one-sample entry and is unchanged.  Per sample s: nreads[s] read pairs; derepF_map[s] / derepR_map[s] the derep-class
 * maps (0-BASED unique of every read; any negative value is NA); dadaF_map[s] / dadaR_map[s] the dada-class maps of nuniqF[s] /
 * nuniqR[s] uniques (1-BASED denoised sequence; <= 0, NA_INTEGER included, is NA).  The clustering tables of all samples stand
 * one behind the other: sample s has nclustF[s] forward sequences, sequence i of the run is seqF_bytes[seqF_offsets[i] ..
 * seqF_offsets[i + 1]) with n0F[i]; the reverse side alike.
 * On the device: a lane per read pair gathers f = dadaF_map[derepF_map[i]] and r, drops the pair when either step is NA and counts
 * (f, r) in the sample's own open-addressing table with the first read that had it (unique(pairdf), table(): :125, :175); the
 * unique pairs of ALL samples are aligned in chunks by the pair-form lane aligner as nwalign(F, rc(R), band = -1) with the scores
 * of :153-158; C_eval_pair (nmatch, nmismatch, nindel), prefer, accept (:165-166) and C_pair_consensus are computed from the move
 * strings where the aligner left them.  Six integers per pair and the accepted sequences come back.  With just_concatenate
 * nothing is aligned (:140-148).  Rows per sample in the reference's order: first appearance, stably by decreasing abundance.
 * Errors.  DADA2HIP_ERR_INPUT: a map of more than INT32_MAX reads; the reference's "Non-corresponding derep-class and dada-class
 * objects." where the largest entry of a derep map is not the last unique of the dada-class object (:116-119; an empty map or one
 * of NAs alone included), with the sample (counted from 1); the same message for an index past either table, with the sample and
 * the first read (counted from 0) that holds one.  DADA2HIP_ERR_UNSUPPORTED: a denoised sequence that is empty or has a letter
 * outside A/C/G/T (dada() produces none), unless just_concatenate.
 * stats (optional, DADA2HIP_MERGE_NSTATS int64 words): [0] samples, [1] read pairs in, [2] of them dropped as NA, [3] unique pairs,
 * [4] chunks, [5] pairs accepted, [6] the largest table's capacity, [7] slots walked past by inserts, [8] bytes copied to the
 * device, [9] bytes copied back, host microseconds of [10] the uploads, [11] the tally (tables, records, order), [12] the
 * alignments (the throw-away sample included), [13] eval + consensus, [14] the downloads, [15] the whole call.
 * The result is owned by the handle until dada2hip_merge_run_free.  dada2hip_merge_run_column: `which` 0..7 = abundance, forward,
 * reverse, nmatch, nmismatch, nindel, prefer (NA_INTEGER with just_concatenate), accept - nrow(sample) entries, rejects included.
 * dada2hip_merge_run_sequences: the bytes of the whole run and, through `offsets`, the nrow(sample) + 1 offsets of the sample's rows
 * into them ("" for a reject). */
#define DADA2HIP_MERGE_NSTATS 16
typedef struct dada2hip_run_mergers dada2hip_run_mergers;
int dada2hip_merge_run(int32_t nsamples, const int64_t *nreads, const int32_t *const *derepF_map, const int32_t *const *derepR_map,
                       const int32_t *nuniqF, const int32_t *const *dadaF_map, const int32_t *nuniqR, const int32_t *const *dadaR_map,
                       const int32_t *nclustF, const char *seqF_bytes, const int64_t *seqF_offsets, const int32_t *n0F, const int32_t *nclustR,
                       const char *seqR_bytes, const int64_t *seqR_offsets, const int32_t *n0R, int32_t min_overlap, int32_t max_mismatch,
                       int32_t trim_overhang, int32_t just_concatenate, int32_t device, dada2hip_run_mergers **out, int64_t *stats, char *errbuf,
                       size_t errlen);
int32_t dada2hip_merge_run_nsamples(const dada2hip_run_mergers *m);
int64_t dada2hip_merge_run_nrow(const dada2hip_run_mergers *m, int32_t sample);
const int32_t *dada2hip_merge_run_column(const dada2hip_run_mergers *m, int32_t sample, int32_t which);
const char *dada2hip_merge_run_sequences(const dada2hip_run_mergers *m, int32_t sample, const int64_t **offsets);
void dada2hip_merge_run_free(dada2hip_run_mergers *m);

/* ---- assignTaxonomy: the naive-Bayes 8-mer classifier -----------------------------------------------
 * dada2hip_taxonomy_train builds the model of C_assign_taxonomy2 (src/taxonomy.cpp:219-270) from nref reference sequences,
 * ref_to_genus[nref] (0-BASED) and genusmat (ngenus x nlevel integer level codes, ROW-major; only their equality is used) and
 * keeps it on `device`: per genus g and 8-mer w, logf((cnt[g][w] + prior[w]) / (M_g + 1)) with cnt the references of g that
 * contain w, prior[w] = (float)((references that contain w + 0.5) / (1.0 + nref)) and M_g the references of g.  The table is
 * computed on the host (counts from each reference's distinct k-mers, the logarithm by the host's logf) and is bit-equal to the
 * reference's; on the device it lies k-mer-major with the genera padded to a multiple of 64.  DADA2HIP_ERR_INPUT: a reference
 * shorter than 8, ref_to_genus out of range, ngenus == 0, nref >= 2^24.  stats (optional, DADA2HIP_TAXONOMY_NSTATS int64 words):
 * [0] host microseconds of the build, [1] of the upload, [2] bytes of the table.
 * dada2hip_taxonomy_table (diagnostic) reads the table back: out[g * 65536 + w], ngenus x 65536 floats.
 *
 * dada2hip_taxonomy_assign classifies nseq queries as AssignParallel does (src/taxonomy.cpp:143-199).  Outputs are 0-BASED and
 * ROW-major: tax[nseq] the best genus, boot_tax[j * 100 + r] the best genus of bootstrap replicate r, boot[j * nlevel + l] the
 * replicates whose genus agrees with tax[j] on levels 0..l, ntie[j * 101 + p] the number of genera whose sum equals the maximum
 * of pass p (0: the full pass, 1 + r: replicate r).  A query shorter than 50 gets tax = -1, boot = 0, boot_tax = -1, ntie = 0 (NA
 * in the reference); one longer than 9999 is DADA2HIP_ERR_INPUT.  K-mers with a letter outside A/C/G/T are skipped.
 * Each sum is taken sequentially in float in the reference's order (the sorted k-mers; the draws of a replicate), over the
 * reference's table: the sums are the reference's bits, so the maximum and the set of genera at it are the reference's.  Inside
 * that set the reference draws from std::random_device; here the winner is the genus with the smallest 32-bit hash of (seed,
 * query, pass, genus), equal hashes going to the smaller genus - uniform over the set, deterministic for a seed.  The hash is
 * f(f(f(f(f(lo ^ 0x9E3779B9) ^ hi) ^ query) ^ pass) ^ genus) with lo / hi the halves of seed and f MurmurHash3's 32-bit finaliser.
 * Replicate r of query j draws k-mer (int)(arraylen * u) of its sorted array, arraylen / 8 times, with u taken in the
 * reference's layout (:181-186): query j starts at unifs[j * max_arraylen] and consumes 100 * (arraylen / 8) values in a row,
 * max_arraylen = max(length) - 7 over ALL queries; neighbouring queries overlap, as in the reference.  unifs holds
 * nseq * 100 * (max_arraylen / 8) doubles in [0, 1) (what Rcpp::runif returns there); with unifs == NULL value i of that buffer
 * is z = seed + (i + 1) * 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 * z ^= z >> 31; u = (z >> 11) * 2^-53 (splitmix64), in 64-bit unsigned arithmetic.
 * try_rc != 0 (:169-177): the full pass also runs on the reverse complement's k-mers; where its maximum is strictly greater as a
 * float, its k-mers serve the query's 101 passes.
 * stats (optional, DADA2HIP_TAXONOMY_NSTATS int64 words): [0] queries classified, [1] of them by the slab instance, [2] by the
 * gather instance, [3] queries that took their reverse complement, [4] kernel launches, [5] host microseconds of the
 * preparation, [6] device microseconds in the slab instance, [7] in the gather instance, [8] in the try_rc passes, [9] host
 * microseconds of the whole call. */
#define DADA2HIP_TAXONOMY_NSTATS 16
typedef struct dada2hip_taxonomy dada2hip_taxonomy;
int dada2hip_taxonomy_train(int32_t nref, const char *const *refs, const int32_t *ref_to_genus, int32_t ngenus, int32_t nlevel,
                            const int32_t *genusmat, int32_t device, dada2hip_taxonomy **out, int64_t *stats, char *errbuf,
                            size_t errlen);
void dada2hip_taxonomy_free(dada2hip_taxonomy *m);
int dada2hip_taxonomy_table(const dada2hip_taxonomy *m, float *out, char *errbuf, size_t errlen);
int dada2hip_taxonomy_assign(const dada2hip_taxonomy *m, int32_t nseq, const char *const *seqs, int32_t try_rc, const double *unifs,
                             uint64_t seed, int32_t *tax, int32_t *boot, int32_t *boot_tax, int32_t *ntie, int64_t *stats,
                             char *errbuf, size_t errlen);

/* ---- assignSpecies: exact matching against a species reference (R/taxonomy.R:240-289) ------------------------------------------
 * What is matched is R/taxonomy.R:264-280: per chunk of equal-length queries a PDict, vcountPDict(...) > 0 over every reference,
 * and with tryRC the same over the references' reverse complements - query q hits reference r exactly when q (with try_rc: q or
 * its reverse complement) occurs in r as a substring.  The match is fixed = TRUE: a reference position holding any letter other
 * than upper-case A/C/G/T (N, IUPAC codes, lower case) matches nothing, so an occurrence must lie on A/C/G/T only.  Nothing here
 * is approximate and there are no ties: the hit lists are the reference's bit for bit.  The id parsing, mapHits, matchGenera and
 * addSpecies (:251-263, :163-185, :281-360) are dada2_amd/api.py's.
 *
 * dada2hip_species_open packs nref reference sequences (2-bit words, a 1-bit plane of the other letters, row offsets and
 * lengths) and keeps them on `device`; a reference may be empty.  DADA2HIP_ERR_INPUT: nref == 0.  stats as below ([0], [1], [12],
 * [13] are set).
 * dada2hip_species_match reports, per query, the 0-based indices of the references it hits, ascending, each once however many
 * positions or strands match: offsets[nseq + 1] into refs.  Equal queries are matched once.  A query longer than every reference
 * has no hits.  DADA2HIP_ERR_INPUT, checked before any device work: a query with a letter other than upper-case A/C/G/T
 * ("Non-ACGT characters present in the query sequences.", :254), an empty query.  Calls on one handle take turns.
 * stats (optional, DADA2HIP_SPECIES_NSTATS int64 words): [0] references, [1] their bases, [2] windows looked up in the presence
 * bitmap (windows inside one reference that touch no other letter, per key length and query chunk), [3] of them past the bitmap,
 * [4] candidates (windows equal to a prefix key), [5] launches of the seed kernel thrown away because they counted more
 * candidates than DADA2HIP_SPECIES_CAND holds and run again in pieces, [6] entries of refs, [7] kernel launches, [8] host and
 * [9] device microseconds of the seed kernel, [10] host and [11] device microseconds of the verification, [12] host
 * microseconds of the whole call, [13] (open) bytes resident on the device. */
#define DADA2HIP_SPECIES_NSTATS 16
typedef struct dada2hip_species dada2hip_species;
int dada2hip_species_open(int32_t nref, const char *const *refs, int32_t device, dada2hip_species **out, int64_t *stats, char *errbuf,
                          size_t errlen);
void dada2hip_species_free(dada2hip_species *m);
typedef struct dada2hip_species_hits dada2hip_species_hits;
int dada2hip_species_match(const dada2hip_species *m, int32_t nseq, const char *const *seqs, int32_t try_rc,
                           dada2hip_species_hits **out, int64_t *stats, char *errbuf, size_t errlen);
const int64_t *dada2hip_species_hits_offsets(const dada2hip_species_hits *h);   /* nseq + 1 */
const int32_t *dada2hip_species_hits_refs(const dada2hip_species_hits *h);      /* 0-based, ascending per query */
void dada2hip_species_hits_free(dada2hip_species_hits *h);

/* ---- filterAndTrim: read filtering and the phiX screen (R/filter.R:402-1120, src/filter.cpp) ----------------------------------
 * A read is its sequence bytes and its quality bytes.  The stages run in fastqFilter's order (R/filter.R:659-706), with
 * start = max(1, trim_left + 1); a read reports the FIRST stage it fails as its code:
 *   1 max_len (> 0: raw width <= max_len)      2 trim_left (width >= start, then start - 1 bases dropped)
 *   3 trim_right (> 0: width > trim_right, then that many dropped from the end)
 *   4 trunc_q (cut at the first quality <= trunc_q; a read left with nothing is dropped)
 *   5 trunc_len (>= start: width >= trunc_len - start + 1, then cut to it)          6 min_len (width >= min_len)
 *   7 max_n (letters other than upper-case A/C/G/T <= max_n)     8 min_q (only if min_q > trunc_q: min(q) > min_q, strict)
 *   9 max_ee (only if finite: the in-order fp64 sum of pow(10.0, -q / 10.0), C_matrixEE's bits, <= max_ee)
 *  10 rm_phix (isPhiX: C_matchRef's count against the reference or the count against its reverse complement >= min_matches;
 *     the counts are never summed; with non_overlapping a hit at window j makes j + word_size + 1 the next window tested;
 *     a window with a letter other than upper-case A/C/G/T matches nothing; the reference is circular)
 *  11 rm_lowcomplex (> 0: seqComplexity(read, kmer_size) >= rm_lowcomplex; a read with no valid k-mer is dropped)
 * and 0 when it is kept.  qual_offset is 33, 64 or 0 = Auto (dada2hip_derep_fastq's rule: the smallest quality character of the
 * call - of the first chunk, for a file - below ';' means 33, otherwise 64).
 *
 * dada2hip_filter_open builds the screen's word table from `ref` (upper-case A/C/G/T only, else DADA2HIP_ERR_UNSUPPORTED; shorter
 * than word_size: DADA2HIP_ERR_INPUT; word_size outside 1..32: DADA2HIP_ERR_UNSUPPORTED) and keeps it on `device`.  The library
 * ships no reference sequence.  ref == NULL: a context without a screen (rm_phix != 0 is then DADA2HIP_ERR_INPUT).
 * dada2hip_filter_reads: n reads, read r being seq / qual[offsets[r] .. offsets[r + 1]).  Outputs (each optional): code[n];
 * window[2 r], [2 r + 1] the kept window's offset and length inside the read (length 0 for codes 1-6); ee[n] (0 for codes 1-6);
 * hits[2 r], [2 r + 1] the two counts of the screen; kmer_counts[r * 4^k + bin] the k-mers of the kept window that are A/C/G/T
 * only, first letter most significant; complexity[n] = exp(sum(-y log y)) over the bins with y > 0, in bin order, by the host's
 * libm (NaN without a valid k-mer).  kmer_size 0 means 2; outside 0..4: DADA2HIP_ERR_UNSUPPORTED.
 * dada2hip_filter_fastq filters a FASTQ file (plain or gzip) into `out` in chunks of chunk_reads records (<= 0: 100 000):
 * records as `@id\nseq\n+\nqual\n`, ids unchanged, input order; compress != 0: every chunk is deflated in pieces over the host
 * pool, each piece a gzip member of its own.  in == out is DADA2HIP_ERR_INPUT ("The output and input files must be different.").
 * An existing `out` is removed first; when nothing passes no file is left (:724-727).  dada2hip_filter_fastq_paired keeps a pair
 * when both reads pass their own parameters; files of unequal read counts are DADA2HIP_ERR_INPUT ("Mismatched forward and
 * reverse sequence files: ...").  A truncated or corrupt input is a read error, as in dada2hip_derep_fastq.
 * stats (optional, DADA2HIP_FILTER_NSTATS int64 words): [0] reads in, [1] reads kept, [2..12] reads dropped at stage 1..11,
 * [13] keys in the word table, [14] 1 when the table is searched in LDS, [15] bytes copied to the device, [16] host
 * microseconds of the upload, [17] device microseconds of the scan kernel, [18] of the EE kernel, [19] of the k-mer kernel,
 * [20] host microseconds of the download, [21] of parsing (on a thread of its own, under the previous chunk's work), [22] of
 * deflate, [23] of writing, [24] of the whole call, [25] of opening the inputs (a gzip file that libdeflate takes is inflated
 * there, in one go). */
#define DADA2HIP_FILTER_NSTATS 32
typedef struct dada2hip_filter dada2hip_filter;
typedef struct dada2hip_filter_params {
  int32_t trunc_q, trunc_len, trim_left, trim_right;
  int32_t max_len;                 /* <= 0: no limit (maxLen = Inf) */
  int32_t min_len, max_n, min_q;
  double max_ee;                   /* not finite: not applied */
  double rm_lowcomplex;            /* <= 0: not applied */
  int32_t rm_phix, min_matches, non_overlapping, kmer_size, qual_offset, reserved;
} dada2hip_filter_params;
int dada2hip_filter_open(const char *ref, int32_t word_size, int32_t device, dada2hip_filter **out, int64_t *stats, char *errbuf,
                         size_t errlen);
void dada2hip_filter_free(dada2hip_filter *ctx);
int dada2hip_filter_reads(dada2hip_filter *ctx, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                          const dada2hip_filter_params *params, int32_t *code, int32_t *window, double *ee, int32_t *hits,
                          int32_t *kmer_counts, double *complexity, int64_t *stats, char *errbuf, size_t errlen);
int dada2hip_filter_fastq(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params,
                          int32_t compress, int64_t chunk_reads, int64_t *reads_in, int64_t *reads_out, int64_t *stats,
                          char *errbuf, size_t errlen);
int dada2hip_filter_fastq_paired(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f, const char *out_r,
                                 const dada2hip_filter_params *params_f, const dada2hip_filter_params *params_r, int32_t compress,
                                 int64_t chunk_reads, int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf,
                                 size_t errlen);

/* ---- filter and dereplicate in one pass ---------------------------------------------------------------------------------------------
 * dada2hip_filter_derep_fastq does everything dada2hip_filter_fastq does, and the kept window of every kept read also goes, from
 * the slot of the filter's pipeline it already lies in and before that slot takes another piece, into the device dereplicator
 * of dada2hip_derep_reads.  out == NULL: no file is written, deflated or formatted; otherwise the file is byte for byte
 * dada2hip_filter_fastq's.  *derep is in every field what dada2hip_derep_fastq(out, derep_chunk_reads, derep_qual_offset) returns
 * for that file: its Auto is judged on the kept windows of the first derep_chunk_reads kept reads (not the filter's own decision,
 * which is params->qual_offset's), its map has *reads_out entries in file order.  When nothing passes, *derep is NULL, the
 * return code is DADA2HIP_OK and no file is left.  The pieces are the filter's (DADA2HIP_FILTER_PIECE, _PIECE_BYTES).
 * dada2hip_filter_derep_fastq_paired is dada2hip_filter_fastq_paired with two derep objects: a pair goes into both or into
 * neither, so the two maps are equally long and in step (what dada2hip_merge_pairs asks).  A pair's verdict is known only when
 * both files' pieces have been judged, so the kept windows of a chunk go up once more, through dada2hip_derep_reads' pieces.
 * stats (optional, DADA2HIP_FILTER_DEREP_NSTATS int64 words): the DADA2HIP_FILTER_NSTATS words of dada2hip_filter_fastq, then
 * the DADA2HIP_DEREP_NSTATS words of dada2hip_derep_reads (of the forward object, for a pair; the clocks of both added). */
#define DADA2HIP_FILTER_DEREP_NSTATS (DADA2HIP_FILTER_NSTATS + DADA2HIP_DEREP_NSTATS)
int dada2hip_filter_derep_fastq(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params,
                                int32_t compress, int64_t chunk_reads, int64_t derep_chunk_reads, int32_t derep_qual_offset,
                                dada2hip_derep **derep, int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf,
                                size_t errlen);
int dada2hip_filter_derep_fastq_paired(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f,
                                       const char *out_r, const dada2hip_filter_params *params_f,
                                       const dada2hip_filter_params *params_r, int32_t compress, int64_t chunk_reads,
                                       int64_t derep_chunk_reads, int32_t derep_qual_offset, dada2hip_derep **derep_f,
                                       dada2hip_derep **derep_r, int64_t *reads_in, int64_t *reads_out, int64_t *stats,
                                       char *errbuf, size_t errlen);
/* The same two with dada2hip_derep_reads_resident's end: every derep object comes without a quality matrix and with its resident
 * sample.  When nothing passes, the objects and the samples are NULL and the return code is DADA2HIP_OK.  An input error of a
 * sample fails the call: no object, no sample, no file.  resident_stats (optional): DADA2HIP_RESIDENT_NSTATS words; for a
 * pair twice as many, the forward sample's and then the reverse sample's. */
int dada2hip_filter_derep_fastq_resident(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params,
                                         int32_t compress, int64_t chunk_reads, int64_t derep_chunk_reads, int32_t derep_qual_offset,
                                         dada2hip_derep **derep, dada2hip_sample **sample, int64_t *reads_in, int64_t *reads_out,
                                         int64_t *stats, int64_t *resident_stats, char *errbuf, size_t errlen);
int dada2hip_filter_derep_fastq_paired_resident(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f,
                                                const char *out_r, const dada2hip_filter_params *params_f,
                                                const dada2hip_filter_params *params_r, int32_t compress, int64_t chunk_reads,
                                                int64_t derep_chunk_reads, int32_t derep_qual_offset, dada2hip_derep **derep_f,
                                                dada2hip_derep **derep_r, dada2hip_sample **sample_f, dada2hip_sample **sample_r,
                                                int64_t *reads_in, int64_t *reads_out, int64_t *stats, int64_t *resident_stats,
                                                char *errbuf, size_t errlen);

/* ---- filterAndTrim's orient.fwd, matchIDs, id.sep and id.field (R/filter.R:648-658, :940-1007) --------------------------------------
 * The entries above stay as they are; these take the four arguments they do not have.
 * orient_fwd: 1..256 upper-case A/C/G/T (empty: DADA2HIP_ERR_INPUT; another letter: DADA2HIP_ERR_INPUT "Non-ACGT characters
 * detected in orient.fwd"; longer: DADA2HIP_ERR_UNSUPPORTED).  A read shorter than it fails the call (narrow() in the reference):
 * DADA2HIP_ERR_INPUT naming the read.
 * dada2hip_filter_reads_oriented, orient_mode 0 (single-end): orient[r] is 0 when read r starts with orient_fwd, 1 when only its
 * reverse complement does, 2 when neither does (3 for the read that failed the call).  A read with 1 goes through every stage AS
 * its reverse complement - the truncQ cut, the in-order EE sum, the screen's greedy walk and the k-mers are those of the flipped
 * read - and its window[2 r] counts from the read's END; hits[2 r] is the flipped read's count against the reference.  A read
 * with 2 has code 12, an empty window and no counts.  Results are in input order (the order of a chunk's output, every 0 and
 * then every 1, is the file level's).  orient_mode 1 (the paired form): the forward test alone, orient[r] 0 or 2, code[r] 0 or
 * 12, nothing else is judged or written and `qual` and `params` are not looked at.
 * dada2hip_filter_fastq_oriented: dada2hip_filter_fastq with orient_fwd; per chunk the reads as given in input order, then the
 * flipped ones in input order (letters complemented as Biostrings does, qualities reversed, ids unchanged): the output depends on
 * chunk_reads, as the reference's does on n.
 * dada2hip_filter_fastq_paired_ex: orient_fwd may be NULL.  With it, a pair whose forward read starts with it stays; one whose
 * reverse read does (and whose forward read does not) is SWAPPED - each read is judged by, and written to, the other direction -
 * and the swapped pairs follow the others of their chunk; the rest is dropped.  match_ids != 0: per chunk, with the unmatched
 * tails of the chunks before in front, the forward records whose id occurs among the reverse ids are kept, and the reverse
 * records likewise; everything behind a side's last match is carried over.  The id is the header line without '@', split at
 * id_sep (NULL or "\\s": one of space \t \n \v \f \r; else exactly one literal character) by strsplit's rules, field id_field
 * (1-based; 0: detected from the first forward id - the one field with 6 colons, else the one with 4, whose forward ids then lose
 * their '#...' tail and whose reverse ids, as in the reference, do not).  Kept lists of unequal length (duplicate ids) are
 * DADA2HIP_ERR_INPUT.  Without match_ids unequal chunks are the "Mismatched ..." error of dada2hip_filter_fastq_paired.
 * stats: the words above and [26] reads (pairs) dropped by orientation, [27] reads flipped (pairs swapped), [28] forward records
 * without a partner by id, [29] device microseconds of the orientation kernel, [30] host microseconds of the id join. */
int dada2hip_filter_reads_oriented(dada2hip_filter *ctx, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                                   const dada2hip_filter_params *params, const char *orient_fwd, int32_t orient_mode, int32_t *code,
                                   int32_t *window, double *ee, int32_t *hits, int32_t *kmer_counts, double *complexity, int8_t *orient,
                                   int64_t *stats, char *errbuf, size_t errlen);
int dada2hip_filter_fastq_oriented(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params,
                                   const char *orient_fwd, int32_t compress, int64_t chunk_reads, int64_t *reads_in, int64_t *reads_out,
                                   int64_t *stats, char *errbuf, size_t errlen);
int dada2hip_filter_fastq_paired_ex(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f, const char *out_r,
                                    const dada2hip_filter_params *params_f, const dada2hip_filter_params *params_r, const char *orient_fwd,
                                    int32_t match_ids, const char *id_sep, int32_t id_field, int32_t compress, int64_t chunk_reads,
                                    int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen);

/* ---- removePrimers: primer search on both strands, orientation and trimming (R/filter.R:81-233) ----------------------------------
 * A match of a primer of L letters in a read of n letters is a start st (0-based here, reported 1-based) at which at most
 * max_mismatch of the positions st .. st + L - 1 mismatch; st runs over -max_mismatch .. n - L + max_mismatch and a position outside
 * the read is a mismatch (vmatchPattern(primer, reads, max.mismatch, with.indels = FALSE) with its "out of limits" matches, as
 * documented; DESIGN.md §8e says what of this is unverified).  A primer of upper-case A/C/G/T only is matched byte for byte (fixed
 * = TRUE: an N in the read mismatches); any other primer by IUPAC sets, both letters read as sets over {A,C,G,T} that match when
 * they intersect.  The forward primer uses its FIRST match, the reverse primer its LAST (:159-177).  With orient the same searches
 * run on the read's reverse complement (A<->T C<->G M<->K R<->Y V<->B H<->D; W S N themselves), and a read is flipped only when it
 * has no forward match as given and at least one on its reverse complement (:181).  In the kept orientation a read needs a forward
 * match and, if primer_rev is given, a reverse match (:192-194); first = end of the forward match + 1 if trim_fwd else 1, last =
 * start of the reverse match - 1 if primer_rev && trim_rev else n, and the read is kept when last > first, strictly (:201-211).
 * code: 0 kept, 1 no forward primer, 2 no reverse primer, 3 nothing left, 4 a letter outside the fifteen upper-case IUPAC codes.
 * Refused with DADA2HIP_ERR_UNSUPPORTED: allow_indels != 0, a primer of more than 128 letters, max_mismatch above 15 or not below
 * a primer's length, a primer or read letter outside ACGTMRWSYKVHDBN (the message names the read).
 * dada2hip_primers_reads: n reads, read r being seq[offsets[r] .. offsets[r + 1]).  Outputs (each optional): code[n], flip[n],
 * first[n], last[n] (1-based, inclusive, in the kept orientation; 0 for codes 1, 2 and 4); hits[4 r + k] the matches of k = 0 the
 * forward primer, 1 the reverse primer, 2 the forward primer on the reverse complement, 3 the reverse primer on it (2 and 3 are 0
 * without orient); starts[8 r + 2 k], [+ 1] the first and the last start of k, 1-based on the strand k stands for, INT32_MIN
 * without a match.  It applies no whole-file rule.
 * dada2hip_primers_fastq: a FASTQ file (plain or gzip) into `out`, in chunks of chunk_reads records (<= 0: 100 000), with the reader,
 * the writer and the gzip members of dada2hip_filter_fastq.  A kept record is `@id`, letters first..last, `+`, their qualities; of
 * a flipped read the reverse complement's letters and the reversed qualities.  The whole-file rule (:157-158) is applied at the
 * end: when no read of the file has a forward match AS GIVEN (or, with primer_rev, none a reverse match as given), what was written
 * is removed and reads_out is 0, even where orient would have flipped every read.  in == out is DADA2HIP_ERR_INPUT; an existing
 * `out` is removed first; no file is left when nothing passes or the call fails.
 * stats (optional, DADA2HIP_PRIMERS_NSTATS int64 words): [0] reads in, [1] reads kept, [2..5] reads with code 1..4, [6] reads
 * flipped, [7] reads with more than one match of a pattern (the reference's "Multiple matches" message), [8] and [9] the forward
 * and the reverse primer's matches on the reads as given, summed, [10] pieces, [11] tiles, [12] bytes copied to the device,
 * [13] host microseconds of the upload, [14] device microseconds of the kernel, [15] host microseconds of the download, [16] of
 * parsing, [17] of deflate, [18] of writing, [19] of the whole call, [20] of opening the input. */
#define DADA2HIP_PRIMERS_NSTATS 24
typedef struct dada2hip_primer_params {
  const char *primer_fwd;
  const char *primer_rev;          /* NULL: none */
  int32_t max_mismatch, trim_fwd, trim_rev, orient, allow_indels, reserved;
} dada2hip_primer_params;
int dada2hip_primers_reads(int64_t n, const char *seq, const int64_t *offsets, const dada2hip_primer_params *params, int32_t device,
                           int32_t *code, int32_t *flip, int32_t *first, int32_t *last, int32_t *hits, int32_t *starts,
                           int64_t *stats, char *errbuf, size_t errlen);
int dada2hip_primers_fastq(const char *in, const char *out, const dada2hip_primer_params *params, int32_t compress,
                           int64_t chunk_reads, int32_t device, int64_t *reads_in, int64_t *reads_out, int64_t *stats,
                           char *errbuf, size_t errlen);

/* ---- read diagnostics: the data of plotQualityProfile and plotComplexity (R/plot-methods.R:163-243, :293-299; R/filter.R:1248-1275) ----
 * Nothing is drawn here; dada2_amd/readqc.py restates the statistics of the R code on these numbers.
 * dada2hip_qprofile_reads: n reads' quality strings, read r being qual[offsets[r] .. offsets[r + 1]).  counts[c * 94 + letter - 33],
 * c < ncycle, is SET to the number of reads whose quality letter at cycle c + 1 is `letter` ('!' .. '~'; ShortRead qa()'s
 * perCycle$quality before an offset is taken off); cycles from the longest read on stay 0.  A letter outside '!'..'~' is
 * DADA2HIP_ERR_INPUT and the message names the read; a read longer than ncycle, or than 262 144, is refused.
 * dada2hip_qprofile_fastq: the table of a FASTQ file (plain or gzip), read in chunks of chunk_reads records (<= 0: 100 000) with
 * the reader of dada2hip_filter_fastq, the next chunk parsed under this chunk's kernel.  The first max_reads records are profiled
 * (0: all of them; the reference profiles a random sample of that size), the whole file is counted.  qual_offset 33, 64 or 0 =
 * Auto (dada2hip_derep_fastq's rule, on the first chunk).  Accessors: _ncycle the longest profiled read, _counts the table
 * [ncycle x 94] as above, _reads the records of the file (the reference's rc), _profiled those counted in the table,
 * _qual_offset the offset settled.
 * dada2hip_complexity_reads: seqComplexity(seqs, kmerSize, window, by) of n sequences, sequence r being seq[offsets[r] ..
 * offsets[r + 1]).  window 0 is window = NULL: dada2hip_filter_reads' complexity of the whole sequence.  Otherwise the R loop with
 * its quirks: the value starts at 4^k; window starts i = 1, 1 + by, ... <= max(width) - window, the maximum over the sequences of
 * THE CALL; a sequence is tested at i only if it is at least i + window - 1 long - so one shorter than the window keeps 4^k, and
 * one of the maximal length never has its last window tested; k-mers with a letter other than upper-case A/C/G/T are not counted,
 * and a tested window without a countable k-mer makes the value NaN for good.  kmer_size 0 means 2.  DADA2HIP_ERR_INPUT:
 * kmer_size >= window ("The window over which kmer frequency is calculated must be larger than the kmerSize."), max(width) -
 * window < 1 (R's seq() stops), by < 1.  DADA2HIP_ERR_UNSUPPORTED: kmer_size outside 0..4, window above 1 024.
 * dada2hip_complexity_fastq: the same of the first max_reads records of a file (0: all), the maximum taken over those records;
 * *out is an array of *nout doubles for dada2hip_complexity_free.
 * stats (optional, DADA2HIP_READQC_NSTATS int64 words): [0] reads in (of a file: its records), [1] reads profiled, [2] pieces,
 * [3] cycles of the table (complexity: the longest sequence), [4] bytes copied to the device, [5] host microseconds of the upload,
 * [6] device microseconds of the kernel, [7] host microseconds of the download, [8] of parsing, [9] of the whole call, [10] of
 * opening the input. */
#define DADA2HIP_READQC_NSTATS 16
#define DADA2HIP_QPROFILE_NSCORE 94
typedef struct dada2hip_qprofile dada2hip_qprofile;
int dada2hip_qprofile_reads(int64_t n, const char *qual, const int64_t *offsets, int32_t device, int32_t ncycle, int64_t *counts,
                            int64_t *stats, char *errbuf, size_t errlen);
int dada2hip_qprofile_fastq(const char *path, int64_t chunk_reads, int64_t max_reads, int32_t qual_offset, int32_t device,
                            dada2hip_qprofile **out, int64_t *stats, char *errbuf, size_t errlen);
int32_t dada2hip_qprofile_ncycle(const dada2hip_qprofile *p);
const int64_t *dada2hip_qprofile_counts(const dada2hip_qprofile *p);
int64_t dada2hip_qprofile_reads_total(const dada2hip_qprofile *p);
int64_t dada2hip_qprofile_profiled(const dada2hip_qprofile *p);
int32_t dada2hip_qprofile_qual_offset(const dada2hip_qprofile *p);
void dada2hip_qprofile_free(dada2hip_qprofile *p);
int dada2hip_complexity_reads(int64_t n, const char *seq, const int64_t *offsets, int32_t kmer_size, int32_t window, int32_t by,
                              int32_t device, double *complexity, int64_t *stats, char *errbuf, size_t errlen);
int dada2hip_complexity_fastq(const char *path, int64_t chunk_reads, int64_t max_reads, int32_t kmer_size, int32_t window, int32_t by,
                              int32_t device, double **out, int64_t *nout, int64_t *stats, char *errbuf, size_t errlen);
void dada2hip_complexity_free(double *values);

/* One b_compare round exposed for kernel-level parity tests and for bench.py's roofline leg:
 * compares every unique of `s` against unique `centre` exactly as CompareParallel does
 * (src/cluster.cpp:90-149) with the given k-mer cutoff and greedy-skip mask (skip[i] != 0 => NULL
 * sub); writes lambda[nraw], hamming[nraw] (0xFFFFFFFF for NULL subs) and cls[nraw]
 * (0 skipped, 1 shrouded, 2 gapless, 3 NW). */
int dada2hip_sample_compare(dada2hip_sample *s, int32_t centre, const double *err, int32_t err_ncol,
                            const dada2hip_opts *opts, double kdist_cutoff, const uint8_t *skip,
                            double *lambda, uint32_t *hamming, uint8_t *cls, dada2hip_stats *stats,
                            char *errbuf, size_t errlen);

/* Diagnostic: the launch ledger.  Every launcher of an aligner or gapless kernel ORs one bit into a process-wide mask at the
 * place where it chooses the compiled instance (host side, one relaxed atomic OR per launch; no device work, no effect on any
 * result).  Copies min(nwords, 2) 64-bit words to `mask` (further words are zeroed), clears the ledger when clear != 0 and
 * returns the number of words the ledger has (2).  Bit b lives in word b / 64 at position b % 64; gl = 0 / 1 / 2 for 21 / 32 / 64
 * lanes per alignment, EDGE = the band fills the lane group (cross-group neighbours are masked):
 *   0 + 8 gl + 4 EDGE + mode   k_nw_ad, mode 0 default scores, 1 generic scores, 2 homopolymer gaps, 3 FAST (pointer-free pass)
 *  32 + 4 gl + 2 EDGE + g      k_nw_ad in bimera mode (LR), g = 0 default / 1 generic scores
 *  64 + 2 gl + g               k_nw_adw (wide band), g as above
 *  72 + 3 c + form             k_nw<WMAX>, c = 0..4 for WMAX 33 / 65 / 129 / 193 / 257; form 0 plain, 1 non-plain (homopolymer
 *                              gaps or global ends), 2 a centre per pair (nwvec, merge)
 *  88 + p                      k_nw_gen, p = 1 with a centre per pair
 *  96, 97                      k_gapless, k_gapless_batch */
int32_t dada2hip_launch_ledger(uint64_t *mask, int32_t nwords, int32_t clear);

/* Diagnostic, beside the ledger and in its style (host side, one relaxed atomic max per launch; no device work, no effect on any
 * result): the most trips through its chunk loop any launch of the lane aligners (k_nw<WMAX>, k_nw_gen) was sized for since
 * the last clear - ceil(chunks of 64 alignments / waves launched).  The chunks come from the host's bound on the launch's work:
 * the count itself for the pair-form calls (nwvec, nwalign, merge, collapse, the bimera table) and for a compare with the k-mer
 * screen off, the number of uniques where the device counts the work.  1: every wave had one chunk at most; from 2 on a wave
 * went back to the slot of the scratch ring it had used (DADA2HIP_NW_RING makes the ring small).  Clears when clear != 0. */
int32_t dada2hip_nw_ring_trips(int32_t clear);

/* Diagnostic (tests): the work list of the sample's last run's final pass as it lies on the device - `work`: partitions in index
 * order, each padded with -1 to whole chunks of `per` slots; `chunk_centre`: one centre per chunk.  info[0..3] = slots, chunks, per,
 * 1 if the list was built on the device (0: by the host - a sharded run, or the scratch of the device's sort too large).  An
 * array is filled only if its capacity (in entries) holds it: call with nulls for the sizes first.  No effect on any result. */
int dada2hip_sample_final_worklist(dada2hip_sample *s, int32_t *work, int64_t work_cap, int32_t *chunk_centre, int64_t chunk_cap,
                                   int64_t *info, char *errbuf, size_t errlen);

/* Poisson tail used for the abundance p-value: calc_pA (src/pval.cpp:44-64) evaluated by the
 * device kernel for n (reads, E) pairs — for parity tests against the oracle. */
int dada2hip_calc_pA(int32_t n, const int32_t *reads, const double *E_reads, const uint8_t *prior, int32_t device,
                     double *out, char *errbuf, size_t errlen);

const char *dada2hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DADA2HIP_H */
