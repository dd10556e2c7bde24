// stage_stats.h — the words of the stages' `stats` arrays (include/dada2hip.h says what each holds), named once.  Plain C++:
// driver.cpp takes it through stage_common.h, derep.cpp - whose file-level entries add the calls' words up over the chunks of a
// file - directly.  A word's position is ABI: a new word goes in front of its enum's *_COUNT, never between two others.
#pragma once
#include "../../include/dada2hip.h"

enum { CS_NDEDUP = 0, CS_CAND, CS_SCANNED, CS_SCREENED_OUT, CS_BOUND, CS_ALIGNED, CS_HAM0, CS_BATCHES, CS_US_JOIN, CS_US_SCAN, CS_US_ALIGN,
       CS_US_RESOLVE, CS_US_TOTAL, CS_COUNT };
enum { TT_US_HOST = 0, TT_US_UPLOAD, TT_BYTES, TT_COUNT };     // dada2hip_taxonomy_train
enum { TS_CLASSIFIED = 0, TS_SLAB, TS_GATHER, TS_FLIPPED, TS_LAUNCHES, TS_US_PREPARE, TS_US_SLAB, TS_US_GATHER, TS_US_ORIENT, TS_US_TOTAL,
       TS_COUNT };
enum { SS_REFS = 0, SS_BASES, SS_WINDOWS, SS_PAST_BITMAP, SS_CANDIDATES, SS_RERUNS, SS_HITS, SS_LAUNCHES, SS_US_SEED_HOST, SS_US_SEED_DEV,
       SS_US_VERIFY_HOST, SS_US_VERIFY_DEV, SS_US_TOTAL, SS_BYTES, SS_COUNT };
// FS_STAGE1 .. + 10: the reads dropped at stage 1..11; PS_CODE1 .. + 3: those with code 1..4.  *_US_PARSE and behind: the file level's.
enum { FS_IN = 0, FS_KEPT, FS_STAGE1, FS_KEYS = 13, FS_LDS, FS_BYTES, FS_US_UP, FS_US_SCAN, FS_US_EE, FS_US_KMERS, FS_US_DOWN, FS_US_PARSE,
       FS_US_DEFLATE, FS_US_WRITE, FS_US_TOTAL, FS_US_INFLATE, FS_COUNT };
// the words of the oriented / id-matching entries, behind the filter's: reads (pairs) in neither orientation, reads flipped (pairs
// swapped), forward records that found no partner by id, device microseconds of k_filter_orient, host microseconds of the id join
enum { FO_DROPPED_ORIENT = FS_COUNT, FO_FLIPPED, FO_DROPPED_IDS, FO_US_ORIENT, FO_US_IDJOIN, FO_COUNT };
static_assert(FS_COUNT == 26 && FO_COUNT <= DADA2HIP_FILTER_NSTATS, "stats words");
enum { PS_IN = 0, PS_KEPT, PS_CODE1, PS_FLIPPED = 6, PS_MULTI, PS_HITS_FWD, PS_HITS_REV, PS_PIECES, PS_TILES, PS_BYTES, PS_US_UP, PS_US_KERNEL,
       PS_US_DOWN, PS_US_PARSE, PS_US_DEFLATE, PS_US_WRITE, PS_US_TOTAL, PS_US_INFLATE, PS_COUNT };
enum { QS_GIVEN = 0, QS_KEPT, QS_KEYS, QS_LDS, QS_SET, QS_BLOCKS, QS_US_PACK, QS_US_DEVICE, QS_US_KERNEL, QS_US_TOTAL, QS_COUNT };   // dada2hip_sample_set_prior_seqs
static_assert(QS_COUNT <= DADA2HIP_PRIOR_SEQS_NSTATS, "stats words");
// dada2hip_bimera_denovo: BD_ROUTE 1 = k_nw_ad in its bimera mode, 2 = the lane kernel + k_bimera_lr; BD_PER: slots to a chunk of the aligner
enum { BD_SEQS = 0, BD_ROWS, BD_QUERIES, BD_PAIRS_POSSIBLE, BD_PAIRS_ALIGNED, BD_WINDOWS, BD_LAUNCHES, BD_FLAGGED, BD_ROUTE, BD_PER, BD_SLOTS,
       BD_US_PACK, BD_US_DEVICE, BD_US_KERNEL, BD_US_TOTAL, BD_COUNT };
static_assert(BD_COUNT <= DADA2HIP_BIMERA_DENOVO_NSTATS, "stats words");
// the read diagnostics (dada2hip_qprofile_*, dada2hip_complexity_*): RQ_US_PARSE and behind are the file level's
enum { RQ_IN = 0, RQ_PROFILED, RQ_PIECES, RQ_CYCLES, RQ_BYTES, RQ_US_UP, RQ_US_KERNEL, RQ_US_DOWN, RQ_US_PARSE, RQ_US_TOTAL, RQ_US_INFLATE,
       RQ_COUNT };
static_assert(RQ_COUNT <= DADA2HIP_READQC_NSTATS && RQ_IN == FS_IN && RQ_PROFILED == FS_KEPT, "stats words; reads in and profiled where a file's reads in and kept are");
enum { RQ_CALL_FIRST = RQ_PIECES, RQ_CALL_LAST = RQ_US_DOWN };   // the words of a chunk's call that a file adds up (RQ_CYCLES: the largest)
// the device dereplicator (dada2hip_derep_reads; behind the filter's words in dada2hip_filter_derep_fastq's stats)
enum { DD_IN = 0, DD_UNIQUES, DD_CAPACITY, DD_REBUILDS, DD_ROUNDS, DD_PIECES, DD_BYTES_UP, DD_BYTES_DOWN, DD_US_UP, DD_US_KERNEL, DD_US_DOWN,
       DD_US_FINAL, DD_US_TOTAL, DD_COUNT };
static_assert(DD_COUNT <= DADA2HIP_DEREP_NSTATS, "stats words");
// ... its resident form's own words (dada2hip_derep_reads_resident and the fused entries: resident_stats)
enum { DR_BYTES_DOWN = 0, DR_BYTES_UP, DR_US_ROWS, DR_US_ORDER, DR_US_KERNEL, DR_US_KMERS, DR_US_MIRROR, DR_BLOCKS, DR_UNIQUES, DR_COUNT };
static_assert(DR_COUNT <= DADA2HIP_RESIDENT_NSTATS, "stats words");
// dada2hip_seqtab_merge
enum { SM_TABLES = 0, SM_COLS_IN, SM_DISTINCT, SM_FLAGGED, SM_ROWS, SM_COLS, SM_CAPACITY, SM_REBUILDS, SM_ROUNDS, SM_RC_FAILS, SM_PIECES,
       SM_BYTES_UP, SM_BYTES_DOWN, SM_US_UP, SM_US_IDENTITY, SM_US_RC, SM_US_ACCUM, SM_US_DOWN, SM_US_TOTAL, SM_COUNT };
static_assert(SM_COUNT <= DADA2HIP_SEQTAB_NSTATS, "stats words");
// dada2hip_merge_run
enum { MR_SAMPLES = 0, MR_PAIRS_IN, MR_NA, MR_UNIQUE, MR_CHUNKS, MR_ACCEPTED, MR_CAPACITY, MR_COLLISIONS, MR_BYTES_UP, MR_BYTES_DOWN, MR_US_UP,
       MR_US_TALLY, MR_US_ALIGN, MR_US_EVAL, MR_US_DOWN, MR_US_TOTAL, MR_COUNT };
static_assert(MR_COUNT <= DADA2HIP_MERGE_NSTATS, "stats words");
// How a file adds its chunks' calls up.  Filter: the words of the context are taken, the call's total is the file's own, every other
// word adds; of a pair's second file only the bytes and the call's clocks add.  Primers: every word of the call adds.
enum { FS_TAKEN_FIRST = FS_KEYS, FS_TAKEN_LAST = FS_LDS, FS_CLOCK_FIRST = FS_BYTES, FS_CLOCK_LAST = FS_US_DOWN, PS_CALL_LAST = PS_US_DOWN };

static_assert(CS_COUNT <= DADA2HIP_COLLAPSE_NSTATS && TT_COUNT <= DADA2HIP_TAXONOMY_NSTATS && TS_COUNT <= DADA2HIP_TAXONOMY_NSTATS &&
              SS_COUNT <= DADA2HIP_SPECIES_NSTATS && FS_COUNT <= DADA2HIP_FILTER_NSTATS && PS_COUNT <= DADA2HIP_PRIMERS_NSTATS, "stats words");
static_assert(FS_STAGE1 + 11 == FS_KEYS && PS_CODE1 + 4 == PS_FLIPPED, "the per-stage and per-code counts fill the gap left for them");
static_assert(FS_TAKEN_LAST + 1 == FS_CLOCK_FIRST && FS_CLOCK_LAST + 1 == FS_US_PARSE, "filter: taken words, call clocks, file clocks in a row");
static_assert(PS_CALL_LAST + 1 == PS_US_PARSE && FS_IN == PS_IN && FS_KEPT == PS_KEPT, "primers: the file's words follow the call's; reads in and kept as filter's");
