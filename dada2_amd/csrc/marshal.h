// marshal.h — the row work of the boundary's fused upload pass (hostsimd.cpp), in plain C++: no HIP header, so that
// tools/upload_fused_check.cpp can run it under the host sanitizers.  driver.cpp (sample_create) cuts the rows into pieces,
// owns the buffers and queues the copies; what is done to a row is here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace d2 {

// The caller's inputs and the buffers one pass fills.  stride = the stated row length of the quality matrix (quals_nrow): the
// geometry of the rows (W2 words of 2-bit codes, LQ quality bytes) derives from it, not from the lengths the pass finds.
struct MarshalRows {
  const char *const *seqs;
  const int32_t *abund;
  const uint8_t *priors;         // may be null
  const double *quals;           // [n][stride]
  int stride, W2, LQ;
  int len_cap;                   // lengths are measured up to len_cap + 1 (SEQLEN: a row of at least len_cap is an error)
  int32_t *len;                  // [n]
  uint32_t *reads;               // [n]
  uint8_t *prior;                // [n]
  uint32_t *packed;              // [n][W2]
  uint8_t *qbytes;               // [n][LQ]
};

// what a piece found (the pieces' tallies are merged by the caller)
struct MarshalTally {
  int maxlen = 0, minlen = 0x7FFFFFFF;
  uint64_t reads = 0;
  uint32_t bad_base = 0;         // a byte other than A C G T inside a read
  int bad_qual = 0;              // a quality that does not round into 0..255 inside a read
  int qmax = 0;
};

// Rows [lo, hi): length (strnlen up to len_cap + 1), abundance and prior of every row; then, for a row that fits its stride
// (len <= stride and len < len_cap), its 2-bit words and its rounded quality bytes, zero behind the read's end.  A row that does
// not fit is only recorded - nothing of it is packed or converted, and nothing is written past a row's W2 words / LQ bytes.
void marshal_rows(const MarshalRows &m, size_t lo, size_t hi, MarshalTally *t);

}  // namespace d2
