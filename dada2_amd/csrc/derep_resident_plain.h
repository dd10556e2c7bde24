// derep_resident_plain.h — the rounding of a resident sample's quality bytes, on integers: no HIP, no doubles.  Included by
// derep_resident.inc.hip (k_dd_to_sample, a lane per position) and alone by tools/derep_resident_plain_check.cpp.
//
// The host route divides first and rounds later: x = (double)(S - offset * n) / (double)n (dd_quality_row, derep_dev_plain.h),
// then marshal_rows' round() (hostsimd.cpp) - half away from zero, a rounded value below 0 or above 255 is bad_qual, -0.0 passes
// as 0.  With T = S - offset * n (which may be negative: offset 64 forced on Phred+33 characters) the same byte is
//   T >= 0:  (2 T + n) / (2 n), bad above 255          (floor(T / n + 1/2); a tie k + 1/2 goes up, away from zero)
//   T <  0:  bad exactly when 2 |T| >= n, else 0       (x <= -1/2 rounds to -1 or below; -1/2 < x < 0 rounds to -0.0)
// and ceiling(max(derep$quals)) (R/dada.R:290) is the largest ceil(T / n).
// Why the doubles agree: |T| < 2^39 and n < 2^31, so T and n are exact as doubles and the one rounding of the division errs by
// less than 2^-45 relative to a quotient below 2^8; a quotient that is not exactly k + 1/2 (or exactly an integer, for the ceiling)
// lies at least 1 / (2 n) > 2^-32 from it, and an exact k + 1/2 or integer is representable, so the division returns it.
// tools/derep_resident_plain_check.cpp does not take that on trust: it compares the two rules value by value.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define D2_DR_FN __host__ __device__ inline
#else
#define D2_DR_FN inline
#endif

// the byte of a mean T / n (n >= 1): 0..255, or -1 for a mean that does not round into a byte (bad_qual; the byte kept is 0)
D2_DR_FN int dr_round_byte(int64_t T, int64_t n) {
  if (T >= 0) {
    const int64_t b = (2 * T + n) / (2 * n);
    return b > 255 ? -1 : (int)b;
  }
  return 2 * (-T) >= n ? -1 : 0;
}

// ceil(T / n) (n >= 1): C's division truncates towards zero, which is the ceiling of a negative quotient
D2_DR_FN int64_t dr_ceil_mean(int64_t T, int64_t n) {
  const int64_t q = T / n;
  return q + (T % n > 0 ? 1 : 0);
}

#undef D2_DR_FN
