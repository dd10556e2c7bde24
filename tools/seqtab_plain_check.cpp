// tools/seqtab_plain_check.cpp — check program for the host's part of mergeSequenceTables (dada2_amd/csrc/seqtab_plain.h: the row
// map of the sample names, the refusal of a name twice in one table, the flags and targets of tryRC, the rank of the unflagged
// uniques by first appearance, the stable column order) without a device: plain host C++ that includes the header alone and
// links nothing else, built with the sanitizers and run by tests/test_seqtables.py:
//   hipcc -O1 -g -std=c++17 -Wall -Xarch_host -fsanitize=address,undefined -x c++ tools/seqtab_plain_check.cpp -o seqtab_plain_check
//   seqtab_plain_check <tables file>
// The tables file: a line "<tables> <repeats_sum> <order_by> <try_rc>", then per table a line "<rows> <columns>", its row names and
// its column names one per line, and its cells row by row.  A stand-in for the device makes what the header is given: the
// uniques numbered in an order that has nothing to do with arrival (descending hash), their first appearances, every column's
// unique, with try_rc every unique's partner by a lookup of its reverse complement; and what the kernels do behind it: the adds
// into the merged matrix with the overflow check, the column keys, the gather.  The checks of seqtab_host.h stand here too.
// Output: "<rows> <columns>", the sample names, the sequences, the cells row by row, the column map on one line.
// Exit status: 0; 2 = usage or a bad file; 3 = refused, with "error <code> <message>" printed.
#include "../dada2_amd/csrc/seqtab_plain.h"

#include <cstdio>
#include <cstdlib>
#include <functional>

static bool read_line(FILE *f, std::string &s) {
  s.clear();
  int c;
  while ((c = fgetc(f)) != EOF && c != '\n') s.push_back((char)c);
  return c != EOF || !s.empty();
}

static int refuse(int code, const std::string &m) { printf("error %d %s\n", code, m.c_str()); return 3; }

static void locate(const std::vector<int32_t> &per_table, int64_t c, int &table, long long &at) {
  table = 0;
  while (table + 1 < (int)per_table.size() && c >= per_table[(size_t)table]) c -= per_table[(size_t)table++];
  at = c + 1;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: seqtab_plain_check <tables file>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string line;
  int ntab = 0, repeats_sum = 0, order_by = 0, try_rc = 0;
  if (!read_line(f, line) || sscanf(line.c_str(), "%d %d %d %d", &ntab, &repeats_sum, &order_by, &try_rc) != 4 || ntab < 0) { fclose(f); return 2; }
  std::vector<int32_t> nrow((size_t)ntab), ncol((size_t)ntab);
  std::vector<std::vector<int32_t>> cells((size_t)ntab);
  std::string row_bytes, col_bytes;
  std::vector<int64_t> row_off(1, 0), col_off(1, 0);
  for (int t = 0; t < ntab; t++) {
    int r = 0, c = 0;
    if (!read_line(f, line) || sscanf(line.c_str(), "%d %d", &r, &c) != 2 || r < 0 || c < 0) { fclose(f); return 2; }
    nrow[(size_t)t] = r; ncol[(size_t)t] = c;
    for (int i = 0; i < r; i++) { read_line(f, line); row_bytes += line; row_off.push_back((int64_t)row_bytes.size()); }
    for (int i = 0; i < c; i++) { read_line(f, line); col_bytes += line; col_off.push_back((int64_t)col_bytes.size()); }
    cells[(size_t)t].resize((size_t)r * (size_t)c);
    for (size_t i = 0; i < cells[(size_t)t].size(); i++)
      if (fscanf(f, "%d", &cells[(size_t)t][i]) != 1) { fclose(f); return 2; }
    if (r > 0 && c > 0) read_line(f, line);                          // (the rest of the last line of cells)
  }
  fclose(f);
  // ---- seqtab_host.h's checks ----
  if (ntab < 2) return refuse(1, "At least two sequence tables are expected");
  for (int t = 0; t < ntab; t++)
    if (nrow[(size_t)t] <= 0 || ncol[(size_t)t] <= 0) return refuse(1, "dada2hip: sequence table " + std::to_string(t + 1) + " is empty (no rows or no columns).");
  StNames cn, rn;
  cn.n = (int64_t)col_off.size() - 1; cn.bytes = col_bytes.data(); cn.off = col_off.data();
  rn.n = (int64_t)row_off.size() - 1; rn.bytes = row_bytes.data(); rn.off = row_off.data();
  int tb; long long at;
  for (int64_t i = 0; i < cn.n; i++)
    if (cn[i].empty()) { locate(ncol, i, tb, at); return refuse(1, "Some column (sequence) names are blank (sequence table " + std::to_string(tb + 1) + ")."); }
  for (int64_t i = 0; i < rn.n; i++)
    if (rn[i].empty()) { locate(nrow, i, tb, at); return refuse(1, "Some row (sample) names are blank (sequence table " + std::to_string(tb + 1) + ")."); }
  for (int t = 0; t < ntab; t++)
    for (int32_t v : cells[(size_t)t]) if (v < 0) return refuse(1, "Negative entries (sequence table " + std::to_string(t + 1) + ").");
  // ---- the header under test: the rows ----
  StRows R;
  if (!st_row_map(ntab, nrow.data(), rn, R))
    return refuse(1, "Duplicated row (sample) names in sequence table " + std::to_string(R.dup_table + 1) + ": " + st_show(rn[R.dup_row]));
  if (!R.repeated.empty() && !repeats_sum) {
    std::string m = "Duplicated sample names detected in the sequence table row names: ";
    for (size_t i = 0; i < R.repeated.size(); i++) { if (i) m += ", "; m += std::string(rn[R.repeated[i]]); }
    return refuse(1, m);
  }
  // ---- the stand-in for the dereplicator and k_st_rc ----
  std::unordered_map<std::string_view, int32_t> seen;
  std::vector<std::string_view> uniq;
  for (int64_t c = 0; c < cn.n; c++) if (seen.emplace(cn[c], 0).second) uniq.push_back(cn[c]);
  std::sort(uniq.begin(), uniq.end(), [](std::string_view a, std::string_view b) {
    const size_t ha = std::hash<std::string_view>()(a), hb = std::hash<std::string_view>()(b);
    return ha != hb ? ha > hb : a > b;
  });
  const int64_t U = (int64_t)uniq.size();
  for (int64_t u = 0; u < U; u++) seen[uniq[(size_t)u]] = (int32_t)u;
  std::vector<uint64_t> first((size_t)U, ~0ull);
  std::vector<int32_t> uid((size_t)cn.n);
  for (int64_t c = 0; c < cn.n; c++) {
    const int32_t u = seen[cn[c]];
    uid[(size_t)c] = u;
    first[(size_t)u] = std::min<uint64_t>(first[(size_t)u], (uint64_t)c);
  }
  const int64_t dup = st_dup_column(ntab, ncol.data(), uid.data(), U);
  if (dup >= 0) {
    locate(ncol, dup, tb, at);
    return refuse(1, "Duplicated column (sequences) names in sequence table " + std::to_string(tb + 1) + ": column " + std::to_string(at) + ", " + st_show(cn[dup]));
  }
  std::vector<int32_t> partner;
  if (try_rc && U > 1) {
    uint8_t comp[256];
    st_comp_table(comp);
    uint64_t bad_first = ~0ull;
    partner.assign((size_t)U, -1);
    std::string r;
    for (int64_t u = 0; u < U; u++) {
      const std::string_view s = uniq[(size_t)u];
      r.assign(s.size(), 0);
      bool bad = false;
      for (size_t p = 0; p < s.size(); p++) { r[s.size() - 1 - p] = (char)comp[(uint8_t)s[p]]; bad |= comp[(uint8_t)s[p]] == 0; }
      if (bad) { bad_first = std::min(bad_first, first[(size_t)u]); continue; }
      auto it = seen.find(std::string_view(r));
      if (it != seen.end()) partner[(size_t)u] = it->second;
    }
    if (bad_first != ~0ull) {
      locate(ncol, (int64_t)bad_first, tb, at);
      return refuse(4, "dada2hip: mergeSequenceTables with tryRC takes the upper-case letters ACGTMRWSYKVHDBN only: table " + std::to_string(tb + 1) +
                           ", column " + std::to_string(at) + " (" + st_show(cn[(int64_t)bad_first]) + ").");
    }
  }
  // ---- the header under test: the columns ----
  StCols P;
  st_plan_columns(U, first.data(), partner.empty() ? nullptr : partner.data(), cn.n, uid.data(), P);
  const size_t NR = R.first.size(), NC = P.kept.size();
  // ---- the stand-in for k_st_accumulate, k_st_colkeys and k_st_gather ----
  std::vector<int32_t> merged(NR * NC, 0);
  int64_t r0 = 0, c0 = 0;
  for (int t = 0; t < ntab; t++) {
    for (int32_t r = 0; r < nrow[(size_t)t]; r++)
      for (int32_t c = 0; c < ncol[(size_t)t]; c++) {
        const int32_t v = cells[(size_t)t][(size_t)r * (size_t)ncol[(size_t)t] + (size_t)c];
        int32_t &cell = merged[(size_t)R.row_map[(size_t)(r0 + r)] * NC + (size_t)P.col_map[(size_t)(c0 + c)]];
        if (cell > INT32_MAX - v) return refuse(1, "dada2hip: a merged cell of the sequence tables exceeds the integer range (NA in the reference).");
        cell += v;
      }
    r0 += nrow[(size_t)t]; c0 += ncol[(size_t)t];
  }
  std::vector<uint64_t> sum(NC, 0);
  std::vector<int32_t> npos(NC, 0), order;
  for (size_t r = 0; r < NR; r++)
    for (size_t k = 0; k < NC; k++) { sum[k] += (uint64_t)merged[r * NC + k]; npos[k] += merged[r * NC + k] > 0; }
  if (order_by < 0 || order_by > 2) return refuse(1, "dada2hip: order_by must be 0 (none), 1 (abundance) or 2 (nsamples).");
  st_order((int64_t)NC, sum.data(), npos.data(), order_by, order);
  printf("%zu %zu\n", NR, NC);
  for (size_t r = 0; r < NR; r++) { const std::string_view s = rn[R.first[r]]; printf("%.*s\n", (int)s.size(), s.data()); }
  for (size_t k = 0; k < NC; k++) { const std::string_view s = cn[(int64_t)first[(size_t)P.kept[(size_t)order[k]]]]; printf("%.*s\n", (int)s.size(), s.data()); }
  for (size_t r = 0; r < NR; r++)
    for (size_t k = 0; k < NC; k++) printf("%d%c", (int)merged[r * NC + (size_t)order[k]], k + 1 < NC ? ' ' : '\n');
  std::vector<int32_t> place(NC);
  for (size_t k = 0; k < NC; k++) place[(size_t)order[k]] = (int32_t)k;
  for (int64_t c = 0; c < cn.n; c++) printf("%d%c", (int)place[(size_t)P.col_map[(size_t)c]], c + 1 < cn.n ? ' ' : '\n');
  return 0;
}
