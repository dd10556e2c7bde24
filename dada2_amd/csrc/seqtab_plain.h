// seqtab_plain.h — the host's part of mergeSequenceTables (seqtab_host.h, seqtab.inc.hip; R/multiSample.R:290-364) in plain C++: no
// HIP, no host pool, no driver.cpp types.  tools/seqtab_plain_check.cpp includes this header alone.
//   st_comp_table     Biostrings' complement of the fifteen IUPAC letters; 0 marks a letter that has none
//   st_row_map        the sample names of all tables -> the rows of the result: first appearance, a repeated name one row (:321-331)
//   st_dup_column     a table that holds one sequence twice (refused; the reference only warns, :231)
//   st_plan_columns   the flags and targets of tryRC from the device's partners, the rank of the unflagged uniques by their first
//                     appearance (unique(), :332, less rc.seqs, :345), and every input column's merged column
//   st_order          order(colSums(.), decreasing = TRUE), stable (:356-362)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace {

inline void st_comp_table(uint8_t *t) {
  memset(t, 0, 256);
  const char *from = "ACGTMRWSYKVHDBN", *to = "TGCAKYWSRMBDHVN";
  for (int i = 0; from[i]; i++) t[(uint8_t)from[i]] = (uint8_t)to[i];
}

// n names: name i is bytes[off[i] .. off[i + 1])
struct StNames {
  int64_t n = 0;
  const char *bytes = nullptr;
  const int64_t *off = nullptr;
  std::string_view operator[](int64_t i) const { return std::string_view(bytes + off[i], (size_t)(off[i + 1] - off[i])); }
};

// a name for a message, cut at 60 letters
inline std::string st_show(std::string_view s) { return s.size() <= 60 ? std::string(s) : std::string(s.substr(0, 57)) + "..."; }

struct StRows {
  std::vector<int32_t> row_map;                // input row (running over the tables) -> row of the result
  std::vector<int64_t> first;                  // row of the result -> the input row its name first stood at
  std::vector<int64_t> repeated;               // input rows whose name an EARLIER table had, one per such name, in order (:325)
  int32_t dup_table = -1;                      // the first table that holds one name twice, and the second of the two rows
  int64_t dup_row = -1;
};

// false: a table holds a row name twice (R.dup_table, R.dup_row)
inline bool st_row_map(int32_t ntab, const int32_t *nrow, const StNames &names, StRows &R) {
  struct Seen { int32_t row, table; bool listed; };
  std::unordered_map<std::string_view, Seen> seen;
  seen.reserve((size_t)names.n * 2);
  R.row_map.assign((size_t)names.n, 0);
  R.first.clear(); R.repeated.clear();
  int64_t r = 0;
  for (int32_t t = 0; t < ntab; t++)
    for (int32_t i = 0; i < nrow[t]; i++, r++) {
      auto it = seen.find(names[r]);
      if (it == seen.end()) {
        seen.emplace(names[r], Seen{(int32_t)R.first.size(), t, false});
        R.row_map[(size_t)r] = (int32_t)R.first.size();
        R.first.push_back(r);
        continue;
      }
      if (it->second.table == t) { R.dup_table = t; R.dup_row = r; return false; }
      it->second.table = t;
      if (!it->second.listed) { it->second.listed = true; R.repeated.push_back(r); }
      R.row_map[(size_t)r] = it->second.row;
    }
  return true;
}

// the running column number of a column whose table already holds its unique, -1 if there is none; uid[c]: column c's unique
inline int64_t st_dup_column(int32_t ntab, const int32_t *ncol, const int32_t *uid, int64_t nuniq) {
  std::vector<int32_t> last((size_t)nuniq, -1);
  int64_t c = 0;
  for (int32_t t = 0; t < ntab; t++)
    for (int32_t i = 0; i < ncol[t]; i++, c++) {
      if (last[(size_t)uid[c]] == t) return c;
      last[(size_t)uid[c]] = t;
    }
  return -1;
}

struct StCols {
  std::vector<int32_t> kept;                   // merged column (order of first appearance) -> unique
  std::vector<int32_t> col_of;                 // unique -> merged column (a flagged unique: its partner's)
  std::vector<int32_t> col_map;                // input column -> merged column
  int64_t nflag = 0;
};

// first[u]: the running column number unique u first stood at (distinct, below ncols); partner: null without tryRC, else per
// unique the unique that is its reverse complement, itself for a palindrome, -1 for none.  Of a pair only the later one is
// flagged, and its partner, being earlier, is not: no chains.
inline void st_plan_columns(int64_t nuniq, const uint64_t *first, const int32_t *partner, int64_t ncols, const int32_t *uid, StCols &P) {
  std::vector<int32_t> at((size_t)ncols, -1);
  for (int64_t u = 0; u < nuniq; u++) at[(size_t)first[u]] = (int32_t)u;
  auto flagged = [&](int64_t u) {
    if (!partner) return false;
    const int32_t p = partner[u];
    return p >= 0 && p != u && first[p] < first[u];
  };
  P.kept.clear(); P.nflag = 0;
  P.col_of.assign((size_t)nuniq, -1);
  for (int64_t c = 0; c < ncols; c++) {
    const int32_t u = at[(size_t)c];
    if (u < 0) continue;
    if (flagged(u)) { P.nflag++; continue; }
    P.col_of[(size_t)u] = (int32_t)P.kept.size();
    P.kept.push_back(u);
  }
  for (int64_t u = 0; u < nuniq; u++)
    if (P.col_of[(size_t)u] < 0) P.col_of[(size_t)u] = P.col_of[(size_t)partner[u]];
  P.col_map.resize((size_t)ncols);
  for (int64_t c = 0; c < ncols; c++) P.col_map[(size_t)c] = P.col_of[(size_t)uid[c]];
}

// order_by 1: by decreasing sum; 2: by decreasing number of positive cells; ties stay in column order.  True when the order is 0, 1, 2, ...
inline bool st_order(int64_t ncol, const uint64_t *sum, const int32_t *npos, int order_by, std::vector<int32_t> &order) {
  order.resize((size_t)ncol);
  for (int64_t k = 0; k < ncol; k++) order[(size_t)k] = (int32_t)k;
  if (order_by == 1) std::stable_sort(order.begin(), order.end(), [sum](int32_t a, int32_t b) { return sum[a] > sum[b]; });
  else if (order_by == 2) std::stable_sort(order.begin(), order.end(), [npos](int32_t a, int32_t b) { return npos[a] > npos[b]; });
  for (int64_t k = 0; k < ncol; k++) if (order[(size_t)k] != (int32_t)k) return false;
  return true;
}

}  // namespace
