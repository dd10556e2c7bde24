// evalpair.h — C_eval_pair (evaluate.cpp:73-114) on the host: what mergePairs (merge.cpp) and nweval / nwhamming /
// collapseNoMismatch (collapse_host.h) reduce an alignment to.
#pragma once
#include <cstdint>
#include <string>

namespace d2 {

// the internal part of the alignment is what lies between the end gaps of either string
inline void eval_pair(const std::string &s1, const std::string &s2, int32_t &match, int32_t &mismatch, int32_t &indel) {
  const int n = (int)s1.size();
  bool g1 = true, g2 = true;
  int start = -1;
  do {
    start++;
    g1 = g1 && start < n && s1[start] == '-';
    g2 = g2 && start < n && s2[start] == '-';
  } while ((g1 || g2) && start < n);
  g1 = g2 = true;
  int end = n;
  do {
    end--;
    if (end < 0) break;
    g1 = g1 && s1[end] == '-';
    g2 = g2 && s2[end] == '-';
  } while ((g1 || g2) && end >= start);
  match = mismatch = indel = 0;
  for (int i = start; i <= end; i++) {
    if (s1[i] == '-' || s2[i] == '-') indel++;
    else if (s1[i] == s2[i]) match++;
    else mismatch++;
  }
}

}  // namespace d2
