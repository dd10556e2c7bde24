// tools/filter_ids_check.cpp — stand-alone check of dada2_amd/csrc/filter_ids_plain.h (matchIDs / id.sep / id.field of
// fastqPairedFilter, R/filter.R:940-991): plain host C++, no GPU, no library; tests/test_filter_ids_plain.py builds it with the
// address and undefined-behaviour sanitizers and runs it.
//   hand   strsplit's rules, the field detection, the key (NA, the old format's '#'), the join and the remainder, by example
//   drawn  2 000 pairs of id lists over a small alphabet with separators, against a restatement over std::set<std::string>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../dada2_amd/csrc/filter_ids_plain.h"

#define CHECK(c) do { if (!(c)) { std::printf("filter_ids_check: FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

static const auto serial = [](size_t n, size_t, auto &&f) { f((size_t)0, n); };

static std::vector<std::string> split_all(const std::string &s, const fid::Sep &sep) {
  std::vector<std::string> out;
  std::string_view f;
  for (int t = 1; fid::split_field(s, sep, t, f); t++) out.emplace_back(f);
  return out;
}

static void hand() {
  const fid::Sep ws, colon{false, ':'};
  CHECK((split_all("a  b ", ws) == std::vector<std::string>{"a", "", "b"}));
  CHECK((split_all(" a", ws) == std::vector<std::string>{"", "a"}));
  CHECK(split_all("", ws).empty());
  CHECK((split_all("a\tb\rc\vd\fe\nf", ws) == std::vector<std::string>{"a", "b", "c", "d", "e", "f"}));
  CHECK((split_all("a b:c", colon) == std::vector<std::string>{"a b", "c"}));
  bool old_format = false;
  CHECK(fid::detect_field("M01:1:A:1:2:3:4 1:N:0:1", ws, old_format) == 1 && !old_format);
  CHECK(fid::detect_field("x M01:1:A:1:2:3:4", ws, old_format) == 2 && !old_format);
  CHECK(fid::detect_field("X:1:2:3:4#0/1", ws, old_format) == 1 && old_format);
  for (const char *bad : {"plain", "", "a:b:c:d:e:f:g h:i:j:k:l:m:n", "a:b:c:d:e a:b:c:d:e", "a:b:c:d:e:f"}) CHECK(fid::detect_field(bad, ws, old_format) == 0);
  const std::string f1 = "@X:1:2:3:4#0/1", r1 = "@X:1:2:3:4#0/2", r2 = "@X:1:2:3:4", e = "@", h = "@#x y";
  CHECK(!fid::key_eq(fid::id_key(f1, ws, 1, true), fid::id_key(r1, ws, 1, false)));      // '#' leaves the forward ids only
  CHECK(fid::key_eq(fid::id_key(f1, ws, 1, true), fid::id_key(r2, ws, 1, false)));
  CHECK(fid::id_key(f1, ws, 2, false).na && fid::id_key(e, ws, 1, false).na && fid::id_key(std::string_view(), ws, 1, false).na);
  CHECK(!fid::id_key(h, ws, 1, true).na && fid::id_key(h, ws, 1, true).len == 0);         // "#x" -> "" ; an empty field -> NA
  CHECK(fid::id_key("@ y", ws, 1, true).na && !fid::id_key("@ y", ws, 1, false).na);
  // F = a b c d against R = b c e d; NA matches NA; a duplicate on one side
  const std::vector<std::string> hf = {"@a", "@b", "@c", "@d", "@"}, hr = {"@b", "@c", "@e", "@d", "@", "@b"};
  std::vector<fid::Key> kf, kr;
  for (const auto &s : hf) kf.push_back(fid::id_key(s, ws, 1, false));
  for (const auto &s : hr) kr.push_back(fid::id_key(s, ws, 1, false));
  std::vector<uint8_t> in_f, in_r;
  fid::join(kf, kr, in_f, in_r, serial);
  CHECK((in_f == std::vector<uint8_t>{0, 1, 1, 1, 1}) && (in_r == std::vector<uint8_t>{1, 1, 0, 1, 1, 1}));
  CHECK(fid::past_last(in_f) == 5 && fid::past_last({1, 0, 1, 0, 0}) == 3 && fid::past_last({0, 0}) == 0 && fid::past_last({}) == 0);
  fid::join({}, kr, in_f, in_r, serial);
  CHECK(in_f.empty() && (in_r == std::vector<uint8_t>(6, 0)));
}

static void drawn() {
  std::mt19937 rng(20);
  const char letters[] = "ab: #\t";
  for (int round = 0; round < 2000; round++) {
    const fid::Sep sep = round % 3 == 0 ? fid::Sep{false, ':'} : fid::Sep{};
    const int field = 1 + (int)(rng() % 3);
    const bool strip = rng() % 2;
    std::vector<std::string> h[2];
    for (auto &side : h)
      for (int i = (int)(rng() % 12); i > 0; i--) {
        std::string s = "@";
        for (int j = (int)(rng() % 7); j > 0; j--) s.push_back(letters[rng() % 6]);
        side.push_back(s);
      }
    // the restatement: the field as a string with a marker in front, "N" for NA
    auto restate = [&](const std::string &hdr, bool strip_hash) {
      const std::vector<std::string> f = split_all(hdr.substr(1), sep);
      if ((int)f.size() < field) return std::string("N");
      std::string v = f[(size_t)field - 1];
      if (strip_hash) {
        if (v.empty()) return std::string("N");
        v = v.substr(0, v.find('#'));
      }
      return "S" + v;
    };
    std::vector<fid::Key> k[2];
    std::set<std::string> want[2];
    for (int s = 0; s < 2; s++)
      for (const auto &x : h[s]) { k[s].push_back(fid::id_key(x, sep, field, strip && s == 0)); want[s].insert(restate(x, strip && s == 0)); }
    std::vector<uint8_t> in[2];
    fid::join(k[0], k[1], in[0], in[1], serial);
    for (int s = 0; s < 2; s++) {
      CHECK(in[s].size() == h[s].size());
      for (size_t i = 0; i < h[s].size(); i++) CHECK((in[s][i] != 0) == (want[1 - s].count(restate(h[s][i], strip && s == 0)) != 0));
    }
  }
}

int main(int argc, char **argv) {
  const std::string which = argc > 1 ? argv[1] : "hand";
  if (which == "hand") hand(); else if (which == "drawn") drawn(); else { std::printf("usage: filter_ids_check hand|drawn\n"); return 2; }
  std::printf("filter_ids_check: ok (%s)\n", which.c_str());
  return 0;
}
