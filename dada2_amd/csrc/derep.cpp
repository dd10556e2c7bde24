// derep.cpp — dereplication front-end of the hot path: FASTQ(.gz) -> uniques, abundances,
// per-unique mean qualities, read -> unique map, in the layout dada2hip_dada_uniques takes.  Host-side C++ (the
// reference does this in R on top of ShortRead: derepFastq / qtables2, /root/reference/R/sequenceIO.R:45-124,
// :150-183); no GPU work here, the result can be handed to dada2hip_sample_from_derep without another copy.
//
// Semantics kept from the reference:
//   * reads are taken in chunks of `n` records (derepFastq's n = 1e6, :57); inside a chunk the uniques are in C-locale
//     lexical order (srsort, :161) and zero-length reads are ignored with their map entry NA (:154-158,:173-177);
//     uniques first seen in a later chunk are appended after the earlier ones (:85-88);
//   * quality sums are accumulated per unique and position and divided by the abundance at the end (:95); positions past
//     a unique's length are NA;
//   * the final order is a STABLE sort by decreasing abundance (R's order(), :98), ties keep the order above.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <zlib.h>

#include "../../include/dada2hip.h"
#include "hostpar.h"

struct dada2hip_derep {
  std::unique_ptr<char[]> seq_blob;  // the uniques' sequences, NUL-terminated, in output order
  std::vector<const char *> seq_ptrs;
  std::vector<int32_t> abund, map;
  std::unique_ptr<double[]> quals;   // [nuniques][maxlen], NA past each unique's length (filled by the host pool: first touch in parallel)
  int32_t maxlen = 0;
  int64_t nreads = 0;
  // an object made by a *_resident entry (d2_derep_from_rows_resident) has no matrix: its means were rounded on the device, into
  // the sample that came with it, and never came down.  qmax is then ceiling(max(derep$quals)) as the device found it
  bool has_quals = true;
  int32_t qmax = 0;
};

// what every entry that needs the matrix says about an object without one
static const char *const NO_QUALS_MSG =
    "dada2hip: this derep object has no quality matrix (it came with its resident sample from a *_resident entry, whose qualities "
    "stay on the device); dada2hip_derep_reads / dada2hip_filter_derep_fastq keep the matrix.";

namespace {

double na_real() {
  union { double d; uint64_t u; } v;
  v.u = 0x7FF00000000007A2ULL;  // R's NA_real_
  return v.d;
}

// byte buffers that are not zero-filled when they are sized (they are about to be overwritten by a read or an inflate: the
// fill was a second pass over every byte of the file)
template <typename T>
struct NoInit {
  using value_type = T;
  NoInit() = default;
  template <typename U> NoInit(const NoInit<U> &) {}
  T *allocate(size_t n) { return static_cast<T *>(::operator new(n * sizeof(T))); }
  void deallocate(T *p, size_t) { ::operator delete(p); }
  template <typename U, typename... A> void construct(U *p, A &&...a) {
    if constexpr (sizeof...(A) == 0) ::new ((void *)p) U; else ::new ((void *)p) U(std::forward<A>(a)...);
  }
  template <typename U> bool operator==(const NoInit<U> &) const { return true; }
  template <typename U> bool operator!=(const NoInit<U> &) const { return false; }
};
using Bytes = std::vector<char, NoInit<char>>;

// Line reader: a background thread inflates the file (gzread; a plain file is read with fread - through zlib it is one more
// copy of every byte) into 8 MiB pieces while the caller parses the previous ones; lines are found with memchr.  A buffer the
// window has moved out of is RETIRED, not freed: the lines handed out stay valid until the caller says release() (the
// records of a batch are hashed in parallel before they are looked at in order).
struct LineReader {
  static constexpr size_t PIECE = 8u << 20;
  gzFile f;
  FILE *plain = nullptr;          // non-null: the file is not compressed (gzdirect) and is read directly
  std::vector<Bytes> retired;
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Bytes> ready;
  bool done = false, stop = false;
  std::string zerr;               // non-empty: the stream ended on a zlib error (corrupt / truncated .gz), not at EOF
  Bytes buf;
  size_t pos = 0, end = 0;
  bool eof = false;
  // (the whole text is in memory already: nothing to read)
  explicit LineReader(Bytes &&whole) : f(nullptr), buf(std::move(whole)) { end = buf.size(); done = true; }
  LineReader(gzFile f_, FILE *plain_) : f(f_), plain(plain_) {
    th = std::thread([this] {
      for (;;) {
        Bytes piece(PIECE);
        const int got = plain ? (int)fread(piece.data(), 1, PIECE, plain) : gzread(f, piece.data(), (unsigned)PIECE);
        std::unique_lock<std::mutex> lk(mu);
        if (got <= 0) {
          if (plain) { if (ferror(plain)) zerr = "read error"; done = true; cv.notify_all(); return; }
          // gzread returns 0 at a clean end of file AND at a stream cut short; -1 on a data / CRC error: ask gzerror
          int zrc = Z_OK;
          const char *zm = gzerror(f, &zrc);
          if (got < 0 || (zrc != Z_OK && zrc != Z_STREAM_END)) zerr = zm && *zm ? zm : "read error";
          done = true; cv.notify_all(); return;
        }
        piece.resize((size_t)got);
        ready.push_back(std::move(piece));
        cv.notify_all();
        cv.wait(lk, [this] { return ready.size() < 4 || stop; });
        if (stop) return;
      }
    });
  }
  ~LineReader() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
  bool refill() {   // append the next piece behind the unread tail
    Bytes piece;
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [this] { return !ready.empty() || done; });
      if (ready.empty()) return false;
      piece = std::move(ready.front());
      ready.pop_front();
    }
    cv.notify_all();
    if (pos == end) { buf.swap(piece); pos = 0; end = buf.size(); if (!piece.empty()) retired.push_back(std::move(piece)); return true; }
    Bytes nb(end - pos + piece.size());
    memcpy(nb.data(), &buf[pos], end - pos);
    memcpy(nb.data() + (end - pos), piece.data(), piece.size());
    buf.swap(nb); pos = 0; end = buf.size();
    retired.push_back(std::move(nb));
    return true;
  }
  void release() { retired.clear(); }   // the lines handed out before the last refill are no longer needed
  std::string error() { std::lock_guard<std::mutex> lk(mu); return zerr; }
  // next line without its terminator as [*p, *p + *n); valid until the next call; false at EOF
  bool next(const char **p, size_t *n) {
    for (;;) {
      char *nl = end > pos ? (char *)memchr(&buf[pos], '\n', end - pos) : nullptr;
      if (nl) {
        size_t len = (size_t)(nl - &buf[pos]);
        *p = &buf[pos];
        pos += len + 1;
        if (len && (*p)[len - 1] == '\r') len--;
        *n = len;
        return true;
      }
      if (eof) {
        if (end == pos) return false;
        size_t len = end - pos;
        *p = &buf[pos];
        pos = end;
        while (len && ((*p)[len - 1] == '\r')) len--;
        *n = len;
        return true;
      }
      if (!refill()) eof = true;
    }
  }
};

// A .gz file in one go through libdeflate, where the system has it (dlopen: the library is not a build dependency; zlib's
// streaming inflate - one thread, 150-300 MB/s of text - is 95 % of a dereplication's time on a compressed file, libdeflate's
// one-shot decoder is 2.4x faster on FASTQ).  Returns 0: not available / not applicable (the caller streams through zlib),
// 1: `text` holds the file's decompressed members, -1: the stream is damaged (`why`).  Concatenated members are decoded one
// after the other, as gzread does.
int inflate_whole(const char *path, Bytes &text, std::string &why) {
  struct Api {
    void *(*alloc)() = nullptr;
    int (*gunzip)(void *, const void *, size_t, void *, size_t, size_t *, size_t *) = nullptr;
    void (*release)(void *) = nullptr;
    bool ok = false;
    Api() {
      void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
      if (!h) return;
      alloc = (void *(*)())dlsym(h, "libdeflate_alloc_decompressor");
      gunzip = (int (*)(void *, const void *, size_t, void *, size_t, size_t *, size_t *))dlsym(h, "libdeflate_gzip_decompress_ex");
      release = (void (*)(void *))dlsym(h, "libdeflate_free_decompressor");
      ok = alloc && gunzip && release;
    }
  };
  static const Api api;
  if (!api.ok) return 0;
  FILE *fp = fopen(path, "rb");
  if (!fp) return 0;
  struct Closer { FILE *p; ~Closer() { fclose(p); } } closer{fp};
  if (fseek(fp, 0, SEEK_END) != 0) return 0;
  const long fsz = ftell(fp);
  if (fsz < 18 || fsz > (1l << 30)) return 0;           // (larger files: streamed, nothing of them held twice)
  rewind(fp);
  std::vector<unsigned char, NoInit<unsigned char>> gz((size_t)fsz);
  if (fread(gz.data(), 1, (size_t)fsz, fp) != (size_t)fsz) return 0;
  if (gz[0] != 0x1F || gz[1] != 0x8B) return 0;
  void *dec = api.alloc();
  if (!dec) return 0;
  struct Rel { const Api &a; void *d; ~Rel() { a.release(d); } } rel{api, dec};
  uint32_t isize;                                        // the last member's length mod 2^32: the first guess of the text's size
  memcpy(&isize, &gz[(size_t)fsz - 4], 4);
  text.resize(std::max<size_t>((size_t)isize + 64, (size_t)fsz * 3));
  size_t in_pos = 0, out_pos = 0;
  while (in_pos + 18 <= (size_t)fsz && gz[in_pos] == 0x1F && gz[in_pos + 1] == 0x8B) {
    size_t used = 0, made = 0;
    const int r = api.gunzip(dec, &gz[in_pos], (size_t)fsz - in_pos, text.data() + out_pos, text.size() - out_pos, &used, &made);
    if (r == 3) {                                              // LIBDEFLATE_INSUFFICIENT_SPACE: the member again, into more room -
      // up to a bound: a file that inflates beyond 64 x its size or 8 GiB is left to the streaming reader, which runs
      // in constant memory (a hostile or very compressible file must not end in bad_alloc or the OOM killer here)
      const size_t cap = std::min<size_t>((size_t)8 << 30, std::max<size_t>((size_t)fsz * 64, (size_t)1 << 26));
      if (text.size() >= cap) { text.clear(); text.shrink_to_fit(); return 0; }
      text.resize(std::min(cap, text.size() * 2));
      continue;
    }
    if (r != 0) { why = "damaged gzip stream (invalid or truncated deflate data, or a CRC / length mismatch)"; return -1; }
    in_pos += used; out_pos += made;
  }
  if (in_pos == 0) { why = "damaged gzip stream"; return -1; }
  // a trailing piece that starts like a member but is too short to be one: gzread reports a truncated file, so does this
  if (in_pos + 2 <= (size_t)fsz && gz[in_pos] == 0x1F && gz[in_pos + 1] == 0x8B) { why = "damaged gzip stream (truncated trailing member)"; return -1; }
  text.resize(out_pos);
  return 1;
}

// quality storage of the uniques seen ONCE (nine in ten of a deep amplicon sample): the read's quality characters as they are,
// a byte per position - the 8-byte sums below are only set up when a unique is met a second time (a 250-nt singleton then costs
// 250 bytes of memory traffic instead of 2 000)
struct ByteArena {
  static constexpr size_t BLOCK = 8u << 20;
  std::vector<std::unique_ptr<unsigned char[]>> blocks;
  size_t used = BLOCK;
  unsigned char *take(size_t n) {
    if (n > BLOCK) { blocks.emplace_back(new unsigned char[n]); used = BLOCK; return blocks.back().get(); }
    if (used + n > BLOCK) { blocks.emplace_back(new unsigned char[BLOCK]); used = 0; }
    unsigned char *r = blocks.back().get() + used;
    used += n;
    return r;
  }
};
// quality-sum storage: fixed blocks, so growing never copies what is already there
struct SumArena {
  static constexpr size_t BLOCK = 4u << 20;
  std::vector<std::unique_ptr<int64_t[]>> blocks;
  size_t used = BLOCK;
  int64_t *take(size_t n) {
    if (n > BLOCK) { blocks.emplace_back(new int64_t[n]()); used = BLOCK; return blocks.back().get(); }   // (never for reads)
    if (used + n > BLOCK) {
      blocks.emplace_back(new int64_t[BLOCK]);
      int64_t *b = blocks.back().get();
      d2::parallel_for(BLOCK, BLOCK / 16, [b](size_t i0, size_t i1) { memset(b + i0, 0, (i1 - i0) * sizeof(int64_t)); });   // first touch in parallel
      used = 0;
    }
    int64_t *r = blocks.back().get() + used;
    used += n;
    return r;
  }
};

// Sort of DISTINCT elements over the host pool (sample sort): splitters from an evenly spaced sample, every element to its
// bucket (parallel), the buckets sorted side by side.  Any correct sort of distinct elements gives the one order, so this is
// std::sort's result.  (The first form - sorted runs, then pairwise merges level by level - spent most of its time in the last
// levels, where one or two threads merge everything: 0.64 s of a 2.0 s dereplication of 1.2 M uniques.)
template <typename Cmp>
void pool_sort(int32_t *first, size_t n, Cmp cmp) {
  const size_t nt = (size_t)d2::HostPool::get().nthreads();
  if (nt <= 1 || n < ((size_t)1 << 16)) { std::sort(first, first + n, cmp); return; }
  size_t B = 16;
  while (B < 4 * nt && B < 1024 && n / (2 * B) >= 2048) B *= 2;
  const size_t OVER = 32, ns = B * OVER;
  std::vector<int32_t> sample(ns);
  for (size_t i = 0; i < ns; i++) sample[i] = first[(size_t)((double)i * (double)n / (double)ns)];
  std::sort(sample.begin(), sample.end(), cmp);
  std::vector<int32_t> split(B - 1);
  for (size_t k = 1; k < B; k++) split[k - 1] = sample[k * OVER];
  const size_t nchunk = std::min<size_t>(4 * nt, (n + 4095) / 4096);
  auto cbound = [&](size_t c) { return n * c / nchunk; };
  std::vector<uint16_t> bucket(n);
  std::vector<size_t> cnt(nchunk * B, 0);
  d2::parallel_for(nchunk, 1, [&](size_t c0, size_t c1) {
    for (size_t c = c0; c < c1; c++) {
      size_t *my = &cnt[c * B];
      for (size_t i = cbound(c); i < cbound(c + 1); i++) {
        const size_t k = (size_t)(std::upper_bound(split.begin(), split.end(), first[i], cmp) - split.begin());
        bucket[i] = (uint16_t)k;
        my[k]++;
      }
    }
  });
  std::vector<size_t> start(B + 1, 0);
  for (size_t k = 0; k < B; k++) {                       // bucket-major, chunk-minor offsets
    size_t run = start[k];
    for (size_t c = 0; c < nchunk; c++) { const size_t v = cnt[c * B + k]; cnt[c * B + k] = run; run += v; }
    start[k + 1] = run;
  }
  std::vector<int32_t> tmp(n);
  d2::parallel_for(nchunk, 1, [&](size_t c0, size_t c1) {
    for (size_t c = c0; c < c1; c++) {
      size_t *my = &cnt[c * B];
      for (size_t i = cbound(c); i < cbound(c + 1); i++) tmp[my[bucket[i]]++] = first[i];
    }
  });
  d2::parallel_for(B, 1, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; k++) {
      std::sort(tmp.begin() + (ptrdiff_t)start[k], tmp.begin() + (ptrdiff_t)start[k + 1], cmp);
      std::copy(tmp.begin() + (ptrdiff_t)start[k], tmp.begin() + (ptrdiff_t)start[k + 1], first + start[k]);
    }
  });
}

// 64-bit hash of a sequence (multiply-fold over 8-byte words; the table below compares the bytes on a tag match, so quality
// only matters for speed)
inline uint64_t fold64(uint64_t a, uint64_t b) { const __uint128_t r = (__uint128_t)a * b; return (uint64_t)r ^ (uint64_t)(r >> 64); }
inline uint64_t seq_hash(const char *p, size_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n * 0xD6E8FEB86659FD93ull;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = fold64(h ^ w, 0xA0761D6478BD642Full); }
  if (i < n) { uint64_t w = 0; memcpy(&w, p + i, n - i); h = fold64(h ^ w, 0xE7037ED1A0B428DBull); }
  return fold64(h, 0x8EBC6AF09C88C6E3ull);
}

// sequence -> provisional id: open addressing over (32-bit tag, id) pairs, the hash computed by the caller (in parallel, for a
// whole batch of records) and kept per id for the re-insertion when the table grows
struct SeqTable {
  std::vector<uint32_t> tag;
  std::vector<int32_t> id;
  size_t mask = 0, used = 0;
  SeqTable() { resize(1 << 17); }
  void resize(size_t cap) { tag.assign(cap, 0); id.assign(cap, -1); mask = cap - 1; used = 0; }
  static uint32_t tag_of(uint64_t h) { return (uint32_t)(h >> 32); }
  void put(uint64_t h, int32_t v) {                      // (the key is known to be absent)
    size_t s = (size_t)h & mask;
    while (id[s] >= 0) s = (s + 1) & mask;
    id[s] = v; tag[s] = tag_of(h); used++;
  }
  template <typename Same>
  int32_t find(uint64_t h, Same same) const {
    const uint32_t t = tag_of(h);
    for (size_t s = (size_t)h & mask;; s = (s + 1) & mask) {
      const int32_t v = id[s];
      if (v < 0) return -1;
      if (tag[s] == t && same(v)) return v;
    }
  }
  void insert(uint64_t h, int32_t v, const std::vector<uint64_t> &hashes) {
    if ((used + 1) * 2 > mask + 1) {
      resize((mask + 1) * 4);
      for (size_t k = 0; k < hashes.size(); k++) if ((int32_t)k != v) put(hashes[k], (int32_t)k);
    }
    put(h, v);
  }
};

void set_err(char *errbuf, size_t errlen, const char *m) {
  if (errbuf && errlen) snprintf(errbuf, errlen, "%s", m);
}

}  // namespace

extern "C" {

static int derep_fastq_body(const char *path, int64_t chunk_reads, int32_t qual_offset, dada2hip_derep **out, char *errbuf,
                            size_t errlen) {
  if (out) *out = nullptr;
  if (!path || !out) { set_err(errbuf, errlen, "File paths must be provided in character format."); return DADA2HIP_ERR_INPUT; }
  gzFile f = gzopen(path, "rb");
  if (!f) { set_err(errbuf, errlen, "Not all provided files exist."); return DADA2HIP_ERR_INPUT; }
  gzbuffer(f, 1 << 20);
  FILE *plain = gzdirect(f) ? fopen(path, "rb") : nullptr;           // not compressed: read it without the copy through zlib
  struct GzGuard { gzFile f; FILE *p; ~GzGuard() { gzclose(f); if (p) fclose(p); } } guard{f, plain};   // closed after the reader thread has joined
  if (chunk_reads <= 0) chunk_reads = 1000000;   // derepFastq(n = 1e6)
  // Uniques get a provisional id at first sight; at every chunk end the ids born in that chunk are put in lexical order
  // and appended to `seen` (the order derepFastq's merge produces).  Quality characters are summed raw, the encoding
  // offset is taken off once at the end (exact in integers), so nothing of a chunk has to be buffered.
  //
  // The records are taken in BATCHES: the reader's lines stay valid until the batch is done (LineReader::release), the
  // sequences of a batch are hashed over the host pool, and only the table look-ups - which assign the provisional ids in
  // read order - run one after the other.
  struct Rec { const char *seq, *qual; uint32_t len; int32_t minq; uint64_t h; };
  ByteArena seq_arena;                                  // provisional id -> sequence bytes (stable addresses)
  std::vector<const char *> sptr;                       // per provisional id
  std::vector<uint32_t> slen;
  std::vector<uint64_t> shash;
  SeqTable index;                                       // sequence -> provisional id
  std::vector<int64_t> count;                           // per provisional id
  std::vector<int64_t *> qacc;                          // per provisional id: raw quality character sums [len]; null while the unique has one read
  std::vector<const unsigned char *> qone;              // per provisional id: the quality characters of its first read
  SumArena arena;
  ByteArena barena;
  std::vector<int32_t> seen;                            // provisional ids in derepFastq's pre-sort order
  std::vector<int32_t> map;                             // per read: provisional id, -1 for zero-length reads
  d2::knobs_reload();
  const bool times = d2::knobs().derep_times;
  using dclk = std::chrono::steady_clock;
  auto t_start = dclk::now();
  double ms_sort = 0;
  auto ms_since = [](dclk::time_point t) { return std::chrono::duration<double, std::milli>(dclk::now() - t).count(); };
  Bytes whole;
  int have_whole = 0;
  if (!plain && !d2::knobs().derep_zlib) {
    std::string why;
    have_whole = inflate_whole(path, whole, why);
    if (have_whole < 0) { set_err(errbuf, errlen, ("dada2hip: error reading " + std::string(path) + ": " + why).c_str()); return DADA2HIP_ERR_INPUT; }
  }
  std::unique_ptr<LineReader> in_holder(have_whole > 0 ? new LineReader(std::move(whole)) : new LineReader(f, plain));
  LineReader &in = *in_holder;
  const char *hp, *sp, *pp, *qp;
  size_t hn, sn, pn, qn;
  int offset = qual_offset, minq = 255;
  int rc = DADA2HIP_OK;
  int64_t nreads = 0, in_chunk = 0;
  size_t chunk_first = 0;   // first provisional id born in the current chunk
  auto seq_less = [&](int32_t a, int32_t b) {            // srsort: C locale (bytes as unsigned, a prefix first)
    const size_t la = slen[a], lb = slen[b];
    const int c = memcmp(sptr[a], sptr[b], std::min(la, lb));
    return c < 0 || (c == 0 && la < lb);
  };
  auto end_chunk = [&]() {
    if (offset <= 0 && minq < 255) offset = minq < 59 ? 33 : 64;   // qualityType "Auto": below ';' only Phred+33 encodings
    const size_t n0 = seen.size();
    const auto t_sort = dclk::now();
    for (size_t id = chunk_first; id < sptr.size(); id++) seen.push_back((int32_t)id);
    pool_sort(seen.data() + n0, seen.size() - n0, seq_less);   // (10^6 string compares x 20: the largest single piece of a chunk's work)
    chunk_first = sptr.size();
    in_chunk = 0;
    ms_sort += ms_since(t_sort);
  };
  std::vector<Rec> batch;
  const size_t BATCH = 32768;
  batch.reserve(BATCH);
  auto flush = [&]() {
    const bool want_min = offset <= 0;
    d2::parallel_for(batch.size(), 512, [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++) {
        Rec &r = batch[i];
        r.h = seq_hash(r.seq, r.len);
        int m = 255;
        if (want_min) for (uint32_t p = 0; p < r.len; p++) m = std::min(m, (int)(unsigned char)r.qual[p]);
        r.minq = m;
      }
    });
    for (const Rec &r : batch) {
      nreads++;
      in_chunk++;
      if (r.len == 0) {
        map.push_back(-1);
      } else {
        const size_t n = r.len;
        int32_t id = index.find(r.h, [&](int32_t v) { return slen[v] == r.len && memcmp(sptr[v], r.seq, n) == 0; });
        if (id < 0) {
          id = (int32_t)sptr.size();
          char *b = (char *)seq_arena.take(n);
          memcpy(b, r.seq, n);
          sptr.push_back(b); slen.push_back(r.len); shash.push_back(r.h);
          index.insert(r.h, id, shash);
          count.push_back(0);
          qacc.push_back(nullptr);
          qone.push_back(nullptr);
        }
        const unsigned char *qq = (const unsigned char *)r.qual;
        if (offset <= 0 && chunk_first == 0) minq = std::min(minq, (int)r.minq);
        if (++count[id] == 1) {                           // first sight: keep the characters
          unsigned char *b = barena.take(n);
          memcpy(b, qq, n);
          qone[id] = b;
        } else {
          int64_t *acc = qacc[id];
          if (!acc) {                                     // second sight: the sums start from the first read's characters
            acc = qacc[id] = arena.take(n);
            const unsigned char *b = qone[id];
            for (size_t p = 0; p < n; p++) acc[p] = b[p];
          }
          for (size_t p = 0; p < n; p++) acc[p] += qq[p];
        }
        map.push_back(id);
      }
      if (in_chunk >= chunk_reads) end_chunk();
    }
    batch.clear();
    in.release();
  };
  while (in.next(&hp, &hn)) {
    if (hn == 0) continue;
    const bool ok = hp[0] == '@' && in.next(&sp, &sn) && in.next(&pp, &pn) && pn > 0 && pp[0] == '+' && in.next(&qp, &qn) && qn == sn;
    if (!ok) {
      const std::string ze = in.error();   // a record cut short by a damaged stream is a read error, not a format error
      if (!ze.empty()) set_err(errbuf, errlen, ("dada2hip: error reading " + std::string(path) + ": " + ze).c_str());
      else set_err(errbuf, errlen, "dada2hip: malformed FASTQ record");
      rc = DADA2HIP_ERR_INPUT;
      break;
    }
    batch.push_back(Rec{sp, qp, (uint32_t)sn, 255, 0});
    if (batch.size() >= BATCH) flush();
  }
  if (rc != DADA2HIP_OK) return rc;
  {
    const std::string ze = in.error();
    if (!ze.empty()) {   // never hand back a silently truncated object
      set_err(errbuf, errlen, ("dada2hip: error reading " + std::string(path) + ": " + ze).c_str());
      return DADA2HIP_ERR_INPUT;
    }
  }
  flush();
  end_chunk();
  const double ms_parse = ms_since(t_start) - ms_sort;
  const auto t_out = dclk::now();
  if (sptr.empty()) { set_err(errbuf, errlen, "Only zero-length sequences detected during dereplication."); return DADA2HIP_ERR_INPUT; }
  if (offset <= 0) offset = 33;
  // stable sort by decreasing abundance (sequenceIO.R:98): (abundance descending, position in `seen` ascending) is a strict
  // order without equal elements, so the pool's sort gives the stable result
  const size_t U = seen.size();
  std::vector<int32_t> pos_of(U);
  d2::parallel_for(U, 4096, [&](size_t k0, size_t k1) { for (size_t k = k0; k < k1; k++) pos_of[seen[k]] = (int32_t)k; });
  std::vector<int32_t> ord(seen);
  pool_sort(ord.data(), U, [&](int32_t a, int32_t b) { return count[a] > count[b] || (count[a] == count[b] && pos_of[a] < pos_of[b]); });
  std::vector<int32_t> rank(U);
  d2::parallel_for(U, 4096, [&](size_t k0, size_t k1) { for (size_t k = k0; k < k1; k++) rank[ord[k]] = (int32_t)k; });
  dada2hip_derep *d = new dada2hip_derep();
  std::unique_ptr<dada2hip_derep> dguard(d);
  d->nreads = nreads;
  for (size_t k = 0; k < U; k++) d->maxlen = std::max<int32_t>(d->maxlen, (int32_t)slen[k]);
  d->abund.resize(U);
  d->quals.reset(new double[U * (size_t)d->maxlen]);
  std::vector<size_t> soff(U + 1, 0);
  for (size_t k = 0; k < U; k++) soff[k + 1] = soff[k] + slen[ord[k]] + 1;
  d->seq_blob.reset(new char[soff[U]]);
  d->seq_ptrs.resize(U);
  const double na = na_real();
  const size_t ml = (size_t)d->maxlen;
  d2::parallel_for(U, 256, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; k++) {
      const int32_t id = ord[k];
      d->abund[k] = (int32_t)count[id];
      double *row = &d->quals[k * ml];
      const int64_t *acc = qacc[id];
      const size_t len = slen[id];
      if (acc) for (size_t p = 0; p < len; p++) row[p] = (double)(acc[p] - (int64_t)offset * count[id]) / (double)count[id];   // derepQuals / derepCounts (:95)
      else { const unsigned char *b = qone[id]; for (size_t p = 0; p < len; p++) row[p] = (double)((int64_t)b[p] - (int64_t)offset) / 1.0; }
      for (size_t p = len; p < ml; p++) row[p] = na;
      char *dst = d->seq_blob.get() + soff[k];
      memcpy(dst, sptr[id], len);
      dst[len] = 0;
      d->seq_ptrs[k] = dst;
    }
  });
  d->map.resize(map.size());
  d2::parallel_for(map.size(), 65536, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; i++) d->map[i] = map[i] < 0 ? DADA2HIP_NA_INTEGER : rank[map[i]];
  });
  *out = dguard.release();
  if (times) fprintf(stderr, "[derep] %lld reads, %zu uniques: read + parse + hash %.0f ms, chunk sorts %.0f ms, output (abundance order, mean qualities, map) %.0f ms\n",
                     (long long)nreads, U, ms_parse, ms_sort, ms_since(t_out));
  return DADA2HIP_OK;
}

// no exception crosses the C ABI (include/dada2hip.h): allocation failures and thread errors become error codes
int dada2hip_derep_fastq(const char *path, int64_t chunk_reads, int32_t qual_offset, dada2hip_derep **out, char *errbuf,
                         size_t errlen) {
  try {
    return derep_fastq_body(path, chunk_reads, qual_offset, out, errbuf, errlen);
  } catch (const std::bad_alloc &) {
    set_err(errbuf, errlen, "dada2hip: out of host memory during dereplication");
  } catch (const std::exception &e) {
    set_err(errbuf, errlen, (std::string("dada2hip: ") + e.what()).c_str());
  } catch (...) {
    set_err(errbuf, errlen, "dada2hip: unknown error during dereplication");
  }
  if (out) *out = nullptr;
  return DADA2HIP_ERR_RUNTIME;
}

int32_t dada2hip_derep_nuniques(const dada2hip_derep *d) { return d ? (int32_t)d->seq_ptrs.size() : 0; }
int64_t dada2hip_derep_nreads(const dada2hip_derep *d) { return d ? d->nreads : 0; }
int32_t dada2hip_derep_maxlen(const dada2hip_derep *d) { return d ? d->maxlen : 0; }
const char *const *dada2hip_derep_seqs(const dada2hip_derep *d) { return d ? d->seq_ptrs.data() : nullptr; }
const int32_t *dada2hip_derep_abundances(const dada2hip_derep *d) { return d ? d->abund.data() : nullptr; }
const double *dada2hip_derep_quals(const dada2hip_derep *d) { return d ? d->quals.get() : nullptr; }
const int32_t *dada2hip_derep_map(const dada2hip_derep *d) { return d ? d->map.data() : nullptr; }
void dada2hip_derep_free(dada2hip_derep *d) { delete d; }
int32_t dada2hip_derep_has_quals(const dada2hip_derep *d) { return d && d->has_quals ? 1 : 0; }

// ceiling(max(derep$quals, na.rm = TRUE)) (R/dada.R:290): the stored word of an object without a matrix, else from the matrix
int32_t dada2hip_derep_qmax(const dada2hip_derep *d) {
  if (!d) return 0;
  if (!d->has_quals) return d->qmax;
  const size_t n = d->seq_ptrs.size() * (size_t)d->maxlen;
  const double *q = d->quals.get();
  double mx = -1e300;
  bool any = false;
  for (size_t i = 0; i < n; i++)
    if (q[i] == q[i]) { mx = any ? std::max(mx, q[i]) : q[i]; any = true; }     // (NA past a unique's length is a NaN)
  return any ? (int32_t)std::ceil(mx) : 0;
}

int dada2hip_sample_from_derep(const dada2hip_derep *d, const uint8_t *priors, int32_t device, dada2hip_sample **out, char *errbuf,
                               size_t errlen) {
  if (out) *out = nullptr;
  if (!d) { set_err(errbuf, errlen, "dada2hip: no derep object"); return DADA2HIP_ERR_INPUT; }
  if (!d->has_quals) { set_err(errbuf, errlen, NO_QUALS_MSG); return DADA2HIP_ERR_INPUT; }
  return dada2hip_sample_create((int32_t)d->seq_ptrs.size(), d->seq_ptrs.data(), d->abund.data(), priors, d->quals.get(), d->maxlen, device,
                                out, errbuf, errlen);
}

}  // extern "C"

// ---- pooling: combineDereps2 (R/multiSample.R:165-203) ------------------------------------------------------------------------------
// The union, the order and the renumbering are pool_plain.h's (plain C++, checked alone by tools/pool_plain_check.cpp); here are the
// hashes (seq_hash over the host pool), the quality rows and the maps.  A quality is acc = acc + q * count per contributing sample
// and acc / total at the end, as sweep(..., "*"), `+` and sweep(..., "/") do it in R: the multiply and the add are two roundings.
// This translation unit is built with -ffp-contract=off (Makefile, FLAGS), so the loop below cannot become a fused multiply-add.
#include "pool_plain.h"

namespace {

int derep_combine_body(int32_t nsamples, const dada2hip_derep_view *in, dada2hip_derep **out, int32_t *unique_to_pool, char *errbuf,
                       size_t errlen) {
  if (out) *out = nullptr;
  if (!out || nsamples <= 0 || !in) { set_err(errbuf, errlen, "Requires derep-class objects."); return DADA2HIP_ERR_INPUT; }
  d2::knobs_reload();
  using dclk = std::chrono::steady_clock;
  auto t_lap = dclk::now();
  double ms_phase[5] = {0, 0, 0, 0, 0};                        // hashes, union, order, rows, maps (DADA2HIP_DEREP_TIMES=1)
  auto lap = [&](int k) { ms_phase[k] = std::chrono::duration<double, std::milli>(dclk::now() - t_lap).count(); t_lap = dclk::now(); };
  size_t nall = 0;
  int64_t nreads = 0;
  int32_t maxlen = 0;
  for (int32_t s = 0; s < nsamples; s++) {
    const dada2hip_derep_view &v = in[s];
    if (v.nuniques > 0 && v.seqs && v.abundances && !v.quals) { set_err(errbuf, errlen, NO_QUALS_MSG); return DADA2HIP_ERR_INPUT; }
    if (v.nuniques < 0 || v.maxlen < 0 || v.nreads < 0 || (v.nuniques > 0 && (!v.seqs || !v.abundances || !v.quals)) || (v.nreads > 0 && !v.map)) {
      set_err(errbuf, errlen, ("dada2hip: derep object " + std::to_string(s + 1) + " is incomplete.").c_str());
      return DADA2HIP_ERR_INPUT;
    }
    nall += (size_t)v.nuniques; nreads += v.nreads; maxlen = std::max(maxlen, v.maxlen);
  }
  if (nall > (size_t)INT32_MAX) { set_err(errbuf, errlen, "dada2hip: too many unique sequences to pool."); return DADA2HIP_ERR_INPUT; }
  // lengths and hashes of every unique of every sample, over the pool
  std::vector<size_t> first((size_t)nsamples + 1, 0);
  for (int32_t s = 0; s < nsamples; s++) first[s + 1] = first[s] + (size_t)in[s].nuniques;
  std::vector<uint32_t> len(nall);
  std::vector<uint64_t> hash(nall);
  std::vector<PoolSample> S((size_t)nsamples);
  std::atomic<int> bad{0};
  for (int32_t s = 0; s < nsamples; s++) {
    const dada2hip_derep_view &v = in[s];
    uint32_t *l = len.data() + first[s];
    uint64_t *h = hash.data() + first[s];
    d2::parallel_for((size_t)v.nuniques, 2048, [&](size_t j0, size_t j1) {
      for (size_t j = j0; j < j1; j++) {
        const size_t n = v.seqs[j] ? strlen(v.seqs[j]) : 0;
        if (n == 0 || n > (size_t)INT32_MAX || v.abundances[j] < 0) { bad.store(1, std::memory_order_relaxed); l[j] = 0; h[j] = 0; continue; }
        l[j] = (uint32_t)n;
        h[j] = seq_hash(v.seqs[j], n);
      }
    });
    S[s].n = v.nuniques; S[s].seqs = v.seqs; S[s].len = l; S[s].hash = h; S[s].abund = v.abundances;
  }
  if (bad.load()) { set_err(errbuf, errlen, "dada2hip: a derep object holds an empty sequence or a negative abundance."); return DADA2HIP_ERR_INPUT; }
  lap(0);
  PoolPlan P;
  int32_t bs = 0, bj = 0;
  const int prc = pool_group(nsamples, S.data(), P, &bs, &bj);
  lap(1);
  if (prc == POOL_DUPLICATE) {
    set_err(errbuf, errlen, ("dada2hip: derep object " + std::to_string(bs + 1) + " holds the sequence of its unique " + std::to_string(bj + 1) + " twice.").c_str());
    return DADA2HIP_ERR_INPUT;
  }
  if (prc == POOL_OVERFLOW) {
    set_err(errbuf, errlen, "dada2hip: a pooled abundance exceeds the integer range (R: NAs produced by integer overflow).");
    return DADA2HIP_ERR_INPUT;
  }
  pool_order(P, [](int32_t *f, size_t n, auto less) { pool_sort(f, n, less); });
  lap(2);
  const size_t U = (size_t)P.npool, ml = (size_t)maxlen;
  std::unique_ptr<dada2hip_derep> d(new dada2hip_derep());
  d->nreads = nreads; d->maxlen = maxlen;
  d->abund.resize(U); d->seq_ptrs.resize(U);
  std::vector<size_t> soff(U + 1, 0);
  for (size_t k = 0; k < U; k++) soff[k + 1] = soff[k] + S[P.src_sample[P.order[k]]].len[P.src_index[P.order[k]]] + 1;
  d->seq_blob.reset(new char[std::max<size_t>(soff[U], 1)]);
  d->quals.reset(new double[std::max<size_t>(U * ml, 1)]);
  const double na = na_real();
  d2::parallel_for(U, 128, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; k++) {
      const int32_t p = P.order[k];
      const PoolSample &A = S[P.src_sample[p]];
      const size_t n = A.len[P.src_index[p]];
      char *dst = d->seq_blob.get() + soff[k];
      memcpy(dst, A.seqs[P.src_index[p]], n);
      dst[n] = 0;
      d->seq_ptrs[k] = dst;
      d->abund[k] = (int32_t)P.total[p];
      double *row = &d->quals[k * ml];
      size_t lim = std::min(n, ml);                            // positions every contributing sample has a column for
      for (int64_t c = P.contrib_off[p]; c < P.contrib_off[p + 1]; c++) lim = std::min(lim, (size_t)in[P.contrib_sample[c]].maxlen);
      for (size_t x = 0; x < lim; x++) row[x] = 0.0;
      for (int64_t c = P.contrib_off[p]; c < P.contrib_off[p + 1]; c++) {
        const dada2hip_derep_view &v = in[P.contrib_sample[c]];
        const double *q = v.quals + (size_t)P.contrib_index[c] * (size_t)v.maxlen;
        const double cnt = (double)v.abundances[P.contrib_index[c]];
        for (size_t x = 0; x < lim; x++) {
          const double prod = q[x] * cnt;                       // (two roundings: see above)
          row[x] = row[x] + prod;
        }
      }
      const double tot = (double)P.total[p];
      for (size_t x = 0; x < lim; x++) row[x] = row[x] / tot;
      for (size_t x = lim; x < ml; x++) row[x] = na;
    }
  });
  lap(3);
  // the maps one after the other, through each sample's piece of to_pool
  d->map.resize((size_t)nreads);
  size_t at = 0;
  std::atomic<int> bad_map{0};
  for (int32_t s = 0; s < nsamples; s++) {
    const dada2hip_derep_view &v = in[s];
    const int32_t *tp = P.to_pool.data() + first[s];
    int32_t *o = d->map.data() + at;
    d2::parallel_for((size_t)v.nreads, 65536, [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++)
        if (!pool_map_entry(v.map[i], tp, v.nuniques, DADA2HIP_NA_INTEGER, &o[i])) bad_map.store(1, std::memory_order_relaxed);
    });
    at += (size_t)v.nreads;
  }
  if (bad_map.load()) { set_err(errbuf, errlen, "dada2hip: a derep object's map names a unique it does not hold."); return DADA2HIP_ERR_INPUT; }
  if (unique_to_pool && nall) memcpy(unique_to_pool, P.to_pool.data(), nall * sizeof(int32_t));
  lap(4);
  if (d2::knobs().derep_times)
    fprintf(stderr, "[combine] %d samples, %zu uniques -> %zu: lengths + hashes %.0f ms, union %.0f ms, order %.0f ms, sequences + quality rows %.0f ms, maps %.0f ms\n",
            (int)nsamples, nall, U, ms_phase[0], ms_phase[1], ms_phase[2], ms_phase[3], ms_phase[4]);
  *out = d.release();
  return DADA2HIP_OK;
}

}  // namespace

extern "C" int dada2hip_derep_combine(int32_t nsamples, const dada2hip_derep_view *in, dada2hip_derep **out, int32_t *unique_to_pool,
                                      char *errbuf, size_t errlen) {
  try {
    return derep_combine_body(nsamples, in, out, unique_to_pool, errbuf, errlen);
  } catch (const std::bad_alloc &) {
    set_err(errbuf, errlen, "dada2hip: out of host memory while combining derep objects");
  } catch (const std::exception &e) {
    set_err(errbuf, errlen, (std::string("dada2hip: ") + e.what()).c_str());
  } catch (...) {
    set_err(errbuf, errlen, "dada2hip: unknown error while combining derep objects");
  }
  if (out) *out = nullptr;
  return DADA2HIP_ERR_RUNTIME;
}

// ---- filterAndTrim's file level (R/filter.R:613-730 fastqFilter, :878-1140 fastqPairedFilter) -------------------------------------
// The per-read verdicts are dada2hip_filter_reads' (filter_host.h, filter.inc.hip); here are the reader, the chunks, the paired
// AND and the writer.  A chunk's records are copied out of the reader's lines into three blobs (header lines, sequences,
// qualities) and the offsets the kernels take; the kept records are laid out as ShortRead's writeFastq does (`@id`, the bases, a
// bare `+`, the qualities) by the host pool and, with compress, deflated in pieces over the pool, every piece a gzip member of
// its own (concatenated members are one valid .gz; a single deflate stream on one thread would be the whole run).
#include <sys/stat.h>

#include "filter_ids_plain.h"
#include "readqc_plain.h"
#include "stage_stats.h"

// the per-cycle quality table of a file (dada2hip_qprofile_fastq): counts[cycle * 94 + letter - '!']
struct dada2hip_qprofile {
  int32_t ncycle = 0, qual_offset = 0;
  int64_t reads = 0, profiled = 0;
  std::vector<int64_t> counts;
};

namespace {

using fclk = std::chrono::steady_clock;
inline int64_t us_since(fclk::time_point t) { return (int64_t)std::chrono::duration<double, std::micro>(fclk::now() - t).count(); }

struct FqSource {
  std::string path;
  gzFile f = nullptr;
  FILE *plain = nullptr;
  std::unique_ptr<LineReader> in;
  bool at_end = false;
  ~FqSource() {
    in.reset();                                                 // (the reader thread joins before the files close)
    if (f) gzclose(f);
    if (plain) fclose(plain);
  }
  bool open(const char *p, std::string &err) {
    path = p;
    f = gzopen(p, "rb");
    if (!f) { err = "Some input files do not exist."; return false; }
    gzbuffer(f, 1 << 20);
    plain = gzdirect(f) ? fopen(p, "rb") : nullptr;
    Bytes whole;
    int have_whole = 0;
    if (!plain && !d2::knobs().derep_zlib) {
      std::string why;
      have_whole = inflate_whole(p, whole, why);
      if (have_whole < 0) { err = "dada2hip: error reading " + path + ": " + why; return false; }
    }
    in.reset(have_whole > 0 ? new LineReader(std::move(whole)) : new LineReader(f, plain));
    return true;
  }
};

struct FqChunk {
  Bytes hdr, seq, qual;
  std::vector<int64_t> hoff, off;
  int64_t n = 0;
  void clear() { hdr.clear(); seq.clear(); qual.clear(); hoff.assign(1, 0); off.assign(1, 0); n = 0; }
};

void bytes_append(Bytes &b, const char *p, size_t n) {
  const size_t at = b.size();
  if (b.capacity() < at + n) b.reserve(std::max(at + n, b.capacity() * 2));
  b.resize(at + n);
  if (n) memcpy(b.data() + at, p, n);                          // (an empty read into an empty blob: no memcpy on a null pointer)
}

// up to `limit` records into c; false on a malformed record or a damaged stream (err)
bool fq_read_chunk(FqSource &S, int64_t limit, FqChunk &c, std::string &err) {
  c.clear();
  LineReader &in = *S.in;
  const char *hp, *sp, *pp, *qp;
  size_t hn, sn, pn, qn;
  while (c.n < limit && !S.at_end) {
    if (!in.next(&hp, &hn)) { S.at_end = true; break; }
    if (hn == 0) continue;
    const bool ok = hp[0] == '@' && in.next(&sp, &sn) && in.next(&pp, &pn) && pn > 0 && pp[0] == '+' && in.next(&qp, &qn) && qn == sn;
    if (!ok) {
      const std::string ze = in.error();
      err = !ze.empty() ? "dada2hip: error reading " + S.path + ": " + ze : std::string("dada2hip: malformed FASTQ record");
      return false;
    }
    // (a refill moves the window: each line is copied before the next one is asked for only where it has to be - the four lines
    // of a record stay valid until release())
    bytes_append(c.hdr, hp, hn); bytes_append(c.seq, sp, sn); bytes_append(c.qual, qp, qn);
    c.hoff.push_back((int64_t)c.hdr.size()); c.off.push_back((int64_t)c.seq.size());
    c.n++;
    if ((c.n & 4095) == 0) in.release();
  }
  in.release();
  if (S.at_end) {
    const std::string ze = in.error();
    if (!ze.empty()) { err = "dada2hip: error reading " + S.path + ": " + ze; return false; }
  }
  return true;
}

int fq_auto_offset(const FqChunk &c) {
  int m = 255;
  for (char ch : c.qual) m = std::min(m, (int)(unsigned char)ch);
  return m < 59 ? 33 : 64;
}

// Biostrings' complement of an IUPAC letter (A<->T C<->G M<->K R<->Y V<->B H<->D; W S N and anything else themselves)
inline char fq_complement(char c) {
  static const char from[] = "ACGTMKRYVBHD", to[] = "TGCAKMYRBVDH";
  const char *p = c ? strchr(from, c) : nullptr;
  return p ? to[p - from] : c;
}

struct FqWriter {
  std::string path;
  FILE *fp = nullptr;
  bool compress = false;
  int64_t us_deflate = 0, us_write = 0;
  ~FqWriter() { if (fp) fclose(fp); }
  // the records of c with keep[i] != 0, cut to win[2 i], win[2 i + 1]; where flip[i] != 0 (flip may be empty) the window is one of
  // the read's reverse complement: its letters complemented and its qualities, both from the read's end backwards
  bool put(const FqChunk &c, const std::vector<uint8_t> &keep, const std::vector<int32_t> &win, const std::vector<uint8_t> &flip,
           std::string &err) {
    auto t0 = fclk::now();
    std::vector<size_t> at((size_t)c.n + 1, 0);
    for (int64_t i = 0; i < c.n; i++)
      at[i + 1] = at[i] + (keep[i] ? (size_t)(c.hoff[i + 1] - c.hoff[i]) + 2 * (size_t)win[2 * i + 1] + 5 : 0);
    if (at[c.n] == 0) return true;
    Bytes text(at[c.n]);
    d2::parallel_for((size_t)c.n, 1024, [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++) {
        if (!keep[i]) continue;
        char *o = text.data() + at[i];
        const size_t hl = (size_t)(c.hoff[i + 1] - c.hoff[i]), wl = (size_t)win[2 * i + 1], wo = (size_t)win[2 * i];
        memcpy(o, c.hdr.data() + c.hoff[i], hl); o += hl; *o++ = '\n';
        if (!flip.empty() && flip[i]) {
          const char *se = c.seq.data() + c.off[i + 1] - 1 - wo, *qe = c.qual.data() + c.off[i + 1] - 1 - wo;
          for (size_t j = 0; j < wl; j++) o[j] = fq_complement(se[-(ptrdiff_t)j]);
          o += wl; *o++ = '\n'; *o++ = '+'; *o++ = '\n';
          for (size_t j = 0; j < wl; j++) o[j] = qe[-(ptrdiff_t)j];
          o += wl; *o++ = '\n';
          continue;
        }
        memcpy(o, c.seq.data() + c.off[i] + wo, wl); o += wl; *o++ = '\n'; *o++ = '+'; *o++ = '\n';
        memcpy(o, c.qual.data() + c.off[i] + wo, wl); o += wl; *o++ = '\n';
      }
    });
    if (!fp) {
      fp = fopen(path.c_str(), "wb");
      if (!fp) { err = "dada2hip: cannot write " + path; return false; }
    }
    if (!compress) {
      if (fwrite(text.data(), 1, text.size(), fp) != text.size()) { err = "dada2hip: error writing " + path; return false; }
      us_write += us_since(t0);
      return true;
    }
    const size_t PIECE = (size_t)1 << 20, np = (text.size() + PIECE - 1) / PIECE;
    std::vector<Bytes> z(np);
    std::vector<int> zrc(np, Z_OK);
    d2::parallel_for(np, 1, [&](size_t p0, size_t p1) {
      for (size_t p = p0; p < p1; p++) {
        const size_t lo = p * PIECE, len = std::min(PIECE, text.size() - lo);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) { zrc[p] = Z_MEM_ERROR; continue; }
        z[p].resize(deflateBound(&zs, (uLong)len) + 32);
        zs.next_in = (Bytef *)(text.data() + lo); zs.avail_in = (uInt)len;
        zs.next_out = (Bytef *)z[p].data(); zs.avail_out = (uInt)z[p].size();
        const int r = deflate(&zs, Z_FINISH);
        if (r != Z_STREAM_END) zrc[p] = r == Z_OK ? Z_BUF_ERROR : r;
        z[p].resize(zs.total_out);
        deflateEnd(&zs);
      }
    });
    us_deflate += us_since(t0);
    t0 = fclk::now();
    for (size_t p = 0; p < np; p++) {
      if (zrc[p] != Z_OK) { err = "dada2hip: deflate failed while writing " + path; return false; }
      if (fwrite(z[p].data(), 1, z[p].size(), fp) != z[p].size()) { err = "dada2hip: error writing " + path; return false; }
    }
    us_write += us_since(t0);
    return true;
  }
  bool finish(std::string &err) {
    if (fp) { const int r = fclose(fp); fp = nullptr; if (r != 0) { err = "dada2hip: error writing " + path; return false; } }
    return true;
  }
};

// What the file-level entries share around fq_run_chunks (which settles the chunk size and re-reads the knobs): the constructor
// starts the call's clock and resets the out-parameters, finish() sets the words every file has (reads in, reads out, the call's
// total: stage_stats.h) and hands totals and counts to the caller.
struct FqCall {
  const fclk::time_point t_call = fclk::now();
  int64_t *reads_in, *reads_out, nin = 0, nout = 0;
  FqCall(int64_t *ri, int64_t *ro) : reads_in(ri), reads_out(ro) { if (ri) *ri = 0; if (ro) *ro = 0; }
  int finish(int64_t *tot, size_t tot_bytes, int w_total, int64_t *stats) const {
    tot[FS_IN] = nin; tot[FS_KEPT] = nout; tot[w_total] = us_since(t_call);
    if (reads_in) *reads_in = nin; if (reads_out) *reads_out = nout;
    if (stats) memcpy(stats, tot, tot_bytes);
    return DADA2HIP_OK;
  }
};

// The chunk pipeline of a file-level call (filterAndTrim's and removePrimers'): the inputs are opened, existing outputs removed,
// and chunk after chunk is parsed on a thread of its own under the verdicts and the writing of the chunk before.
// verdict(ch, first_chunk, keep, win, flip) settles a chunk: keep[i] (set to 1 on entry), win[k] (offset and length per read of
// file k) and, for reads to be written as their reverse complement, flip (empty: none); it returns a DADA2HIP_* code with the
// message in errbuf.  On any failure nothing half written is left behind.  W: where the pipeline's clocks go in `tot`.
// out == nullptr is the form without writers (the read diagnostics): nothing is removed, nothing written, and W.deflate and
// W.write are not looked at; the verdict only reads the chunk.
struct FqClockWords { int parse, deflate, write, inflate; };
template <typename Verdict>
int fq_run_chunks(int nfile, const char *const *in, const char *const *out, int32_t compress, int64_t chunk_reads, int64_t *tot,
                  const FqClockWords &W, FqCall &call, Verdict &&verdict, char *errbuf, size_t errlen) {
  int64_t &nin = call.nin, &nout = call.nout;
  if (chunk_reads <= 0) chunk_reads = 100000;                   // filterAndTrim(n = 1e5)
  d2::knobs_reload();
  FqSource src[2];
  FqWriter wr[2];
  FqChunk chunks[2][2];                                         // [slot][file]: the parser fills one slot while the other is filtered and written
  std::string err;
  for (int k = 0; k < nfile; k++) {
    const auto t_open = fclk::now();                            // (a .gz that libdeflate takes is inflated HERE, in one go)
    if (!src[k].open(in[k], err)) { set_err(errbuf, errlen, err.c_str()); return DADA2HIP_ERR_INPUT; }
    tot[W.inflate] += us_since(t_open);
    if (out) { wr[k].path = out[k]; wr[k].compress = compress != 0; }
  }
  for (int k = 0; k < nfile && out; k++) (void)remove(out[k]);  // :634-640 (writeFastq does not overwrite)
  std::vector<int32_t> win[2];
  std::vector<uint8_t> keep, flip;
  int rc = DADA2HIP_OK;
  struct Parsed { bool ok; std::string err; int64_t us; };
  auto parse = [&](int slot) {
    const auto t_parse = fclk::now();
    Parsed r{true, std::string(), 0};
    for (int k = 0; k < nfile && r.ok; k++) r.ok = fq_read_chunk(src[k], chunk_reads, chunks[slot][k], r.err);
    r.us = us_since(t_parse);
    return r;
  };
  std::future<Parsed> ahead = std::async(std::launch::async, parse, 0);
  for (int slot = 0;; slot ^= 1) {
    const bool first = nin == 0;
    const Parsed got = ahead.get();
    tot[W.parse] += got.us;
    if (!got.ok) { set_err(errbuf, errlen, got.err.c_str()); rc = DADA2HIP_ERR_INPUT; break; }
    FqChunk *ch = chunks[slot];
    if (nfile == 2 && ch[0].n != ch[1].n) {                     // :966
      set_err(errbuf, errlen, ("Mismatched forward and reverse sequence files: " + std::to_string(ch[0].n) + ", " + std::to_string(ch[1].n) + ".").c_str());
      rc = DADA2HIP_ERR_INPUT;
      break;
    }
    const int64_t n = ch[0].n;
    if (n == 0) break;
    ahead = std::async(std::launch::async, parse, slot ^ 1);   // the next chunk is read and parsed under this one's kernels and deflate
    nin += n;
    keep.assign((size_t)n, 1);
    flip.clear();
    rc = verdict(ch, first, keep, win, flip);
    if (rc != DADA2HIP_OK) break;
    for (int64_t i = 0; i < n; i++) nout += keep[i];
    for (int k = 0; k < nfile && out && rc == DADA2HIP_OK; k++)
      if (!wr[k].put(ch[k], keep, win[k], flip, err)) { set_err(errbuf, errlen, err.c_str()); rc = DADA2HIP_ERR_RUNTIME; }
    if (rc != DADA2HIP_OK) break;
  }
  if (ahead.valid()) ahead.wait();                              // (a run that stops early still waits for its parser)
  for (int k = 0; k < nfile && out; k++) {
    if (!wr[k].finish(err) && rc == DADA2HIP_OK) { set_err(errbuf, errlen, err.c_str()); rc = DADA2HIP_ERR_RUNTIME; }
    tot[W.deflate] += wr[k].us_deflate; tot[W.write] += wr[k].us_write;
  }
  if (rc != DADA2HIP_OK)                                        // nothing half written is left behind
    for (int k = 0; k < nfile && out; k++) (void)remove(out[k]);
  return rc;
}

int filter_files_body(dada2hip_filter *ctx, int nfile, const char *const *in, const char *const *out,
                      const dada2hip_filter_params *const *params, int32_t compress, int64_t chunk_reads, int64_t *reads_in,
                      int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen) {
  FqCall call(reads_in, reads_out);
  for (int k = 0; k < nfile; k++)
    if (!in[k] || !out[k] || !params[k]) { set_err(errbuf, errlen, "File paths must be provided in character format."); return DADA2HIP_ERR_INPUT; }
  for (int a = 0; a < nfile; a++) {                             // :627, :887
    for (int b = 0; b < nfile; b++)
      if (strcmp(in[a], out[b]) == 0) {
        set_err(errbuf, errlen, nfile == 1 ? "The output and input files must be different." : "The output and input file names must be different.");
        return DADA2HIP_ERR_INPUT;
      }
    for (int b = 0; b < a; b++)
      if (strcmp(out[a], out[b]) == 0 || strcmp(in[a], in[b]) == 0) { set_err(errbuf, errlen, "The output and input file names must be different."); return DADA2HIP_ERR_INPUT; }
  }
  dada2hip_filter_params P[2];
  for (int k = 0; k < nfile; k++) P[k] = *params[k];
  int64_t tot[DADA2HIP_FILTER_NSTATS] = {0}, st[DADA2HIP_FILTER_NSTATS];
  std::vector<int32_t> code[2];
  const int rc = fq_run_chunks(nfile, in, out, compress, chunk_reads, tot, FqClockWords{FS_US_PARSE, FS_US_DEFLATE, FS_US_WRITE, FS_US_INFLATE}, call,
                               [&](FqChunk *ch, bool first, std::vector<uint8_t> &keep, std::vector<int32_t> *win, std::vector<uint8_t> &) -> int {
    const int64_t n = ch[0].n;
    for (int k = 0; k < nfile; k++) {
      if (first && P[k].qual_offset == 0) P[k].qual_offset = fq_auto_offset(ch[k]);
      code[k].resize((size_t)n); win[k].resize(2 * (size_t)n);
      const int r = dada2hip_filter_reads(ctx, n, ch[k].seq.data(), ch[k].qual.data(), ch[k].off.data(), &P[k], code[k].data(), win[k].data(),
                                          nullptr, nullptr, nullptr, nullptr, st, errbuf, errlen);
      if (r != DADA2HIP_OK) return r;
      // (the verdict counts are the forward reads', the clocks both files'; stage_stats.h: which words add, are taken, are the file's)
      const int w0 = k == 0 ? 0 : FS_CLOCK_FIRST, w1 = k == 0 ? FS_COUNT - 1 : FS_CLOCK_LAST;
      for (int i = w0; i <= w1; i++)
        if (i >= FS_TAKEN_FIRST && i <= FS_TAKEN_LAST) tot[i] = st[i]; else if (i != FS_US_TOTAL) tot[i] += st[i];
      for (int64_t i = 0; i < n; i++) if (code[k][i] != 0) keep[i] = 0;
    }
    return DADA2HIP_OK;
  }, errbuf, errlen);
  return rc != DADA2HIP_OK ? rc : call.finish(tot, sizeof tot, FS_US_TOTAL, stats);
}

// ---- orient.fwd, matchIDs, id.sep, id.field (R/filter.R:648-658, :940-1007) ---------------------------------------------------------
// dada2hip_filter_fastq_oriented and dada2hip_filter_fastq_paired_ex have a chunk loop of their own: a chunk's output is two runs
// of records (the reads as given, then the flipped or swapped ones), a pair's records can change files, and matchIDs carries the
// unmatched tail of each side into the next chunk.  fq_run_chunks and the entries above are not touched by any of it.
// the records idx[0 .. m) of s behind those of d: the offsets first, then the bytes over the host pool
void fq_gather(FqChunk &d, const FqChunk &s, const std::vector<int64_t> &idx) {
  const size_t m = idx.size(), n0 = (size_t)d.n;
  d.hoff.resize(n0 + m + 1); d.off.resize(n0 + m + 1);
  for (size_t j = 0; j < m; j++) {
    d.hoff[n0 + j + 1] = d.hoff[n0 + j] + (s.hoff[idx[j] + 1] - s.hoff[idx[j]]);
    d.off[n0 + j + 1] = d.off[n0 + j] + (s.off[idx[j] + 1] - s.off[idx[j]]);
  }
  d.hdr.resize((size_t)d.hoff[n0 + m]); d.seq.resize((size_t)d.off[n0 + m]); d.qual.resize((size_t)d.off[n0 + m]);
  d2::parallel_for(m, 2048, [&](size_t lo, size_t hi) {
    for (size_t j = lo; j < hi; j++) {
      const int64_t i = idx[j];
      const size_t hl = (size_t)(s.hoff[i + 1] - s.hoff[i]), sl = (size_t)(s.off[i + 1] - s.off[i]);
      if (hl) memcpy(d.hdr.data() + d.hoff[n0 + j], s.hdr.data() + s.hoff[i], hl);
      if (sl) {
        memcpy(d.seq.data() + d.off[n0 + j], s.seq.data() + s.off[i], sl);
        memcpy(d.qual.data() + d.off[n0 + j], s.qual.data() + s.off[i], sl);
      }
    }
  });
  d.n += (int64_t)m;
}
// idx = the i in [lo, hi) with pick(i)
template <typename Pick> const std::vector<int64_t> &fq_pick(std::vector<int64_t> &idx, int64_t lo, int64_t hi, Pick &&pick) {
  idx.clear();
  for (int64_t i = lo; i < hi; i++) if (pick(i)) idx.push_back(i);
  return idx;
}
std::string fq_id(const FqChunk &c, int64_t i) { return std::string(c.hdr.data() + c.hoff[i], (size_t)(c.hoff[i + 1] - c.hoff[i])); }

int filter_files_ex_body(dada2hip_filter *ctx, int nfile, const char *const *in, const char *const *out,
                         const dada2hip_filter_params *const *params, const char *orient_fwd, int32_t match_ids, const char *id_sep,
                         int32_t id_field, int32_t compress, int64_t chunk_reads, int64_t *reads_in, int64_t *reads_out, int64_t *stats,
                         char *errbuf, size_t errlen) {
  FqCall call(reads_in, reads_out);
  auto fail = [&](int code, const std::string &msg) { set_err(errbuf, errlen, msg.c_str()); return code; };
  for (int k = 0; k < nfile; k++)
    if (!in[k] || !out[k] || !params[k]) return fail(DADA2HIP_ERR_INPUT, "File paths must be provided in character format.");
  for (int a = 0; a < nfile; a++) {                             // :627, :887
    for (int b = 0; b < nfile; b++)
      if (strcmp(in[a], out[b]) == 0)
        return fail(DADA2HIP_ERR_INPUT, nfile == 1 ? "The output and input files must be different." : "The output and input file names must be different.");
    for (int b = 0; b < a; b++)
      if (strcmp(out[a], out[b]) == 0 || strcmp(in[a], in[b]) == 0) return fail(DADA2HIP_ERR_INPUT, "The output and input file names must be different.");
  }
  if (orient_fwd) {                                             // :650, :995 (the library checks again; an empty file reaches no call of it)
    if (!*orient_fwd) return fail(DADA2HIP_ERR_INPUT, "dada2hip: orient_fwd is empty.");
    for (const char *c = orient_fwd; *c; c++)
      if (!strchr("ACGT", *c)) return fail(DADA2HIP_ERR_INPUT, "Non-ACGT characters detected in orient.fwd");
  }
  const bool match = nfile == 2 && match_ids != 0;              // (single-end: matchIDs is ignored, as in the reference)
  fid::Sep sep;
  if (match) {
    if (id_sep && strcmp(id_sep, "\\s") != 0) {
      if (strlen(id_sep) != 1) return fail(DADA2HIP_ERR_UNSUPPORTED, "dada2hip: id_sep must be \"\\\\s\" or one literal character.");
      sep.space = false; sep.ch = id_sep[0];
    }
    if (id_field < 0) return fail(DADA2HIP_ERR_INPUT, "dada2hip: id_field must be at least 1 (0: detect it).");
  }
  dada2hip_filter_params P[2];
  for (int k = 0; k < nfile; k++) P[k] = *params[k];
  int64_t tot[DADA2HIP_FILTER_NSTATS] = {0}, st[DADA2HIP_FILTER_NSTATS];
  int64_t &nin = call.nin, &nout = call.nout;
  if (chunk_reads <= 0) chunk_reads = 100000;
  d2::knobs_reload();
  FqSource src[2];
  FqWriter wr[2];
  FqChunk chunks[2][2], work[2], rem[2], sel[2], comp[2], tmp;
  std::string err;
  for (int k = 0; k < nfile; k++) {
    const auto t_open = fclk::now();
    if (!src[k].open(in[k], err)) return fail(DADA2HIP_ERR_INPUT, err);
    tot[FS_US_INFLATE] += us_since(t_open);
    wr[k].path = out[k]; wr[k].compress = compress != 0;
  }
  for (int k = 0; k < nfile; k++) { (void)remove(out[k]); rem[k].clear(); }
  // a call's words into the file's (stage_stats.h): `counts` with the verdict counts (the forward reads'), else the clocks alone
  auto add_stats = [&](bool counts) {
    const int w0 = counts ? 0 : FS_CLOCK_FIRST, w1 = counts ? FS_COUNT - 1 : FS_CLOCK_LAST;
    for (int i = w0; i <= w1; i++)
      if (i >= FS_TAKEN_FIRST && i <= FS_TAKEN_LAST) tot[i] = st[i]; else if (i != FS_US_TOTAL) tot[i] += st[i];
    tot[FO_US_ORIENT] += st[FO_US_ORIENT];
  };
  // the message of a read shorter than orient_fwd names the record (ori: 3 at the read the call stopped at)
  auto name_short = [&](const FqChunk &c, const std::vector<int8_t> &ori, const char *which, int64_t first_no) {
    for (int64_t i = 0; i < c.n; i++)
      if (ori[(size_t)i] == 3) {
        const std::string no = first_no > 0 ? " " + std::to_string(first_no + i) : std::string();
        set_err(errbuf, errlen, ("dada2hip: " + std::string(which) + "read" + no + " (" + fq_id(c, i) + ") is shorter than orient_fwd.").c_str());
        return;
      }
  };
  std::vector<int32_t> code[2], win[2];
  std::vector<uint8_t> keep, keep2, flip;
  std::vector<int8_t> ori[2];
  std::vector<fid::Key> keys[2];
  std::vector<int64_t> idx;
  auto pool_for = [](size_t n, size_t grain, auto &&f) { d2::parallel_for(n, grain, f); };
  std::vector<uint8_t> inset[2];
  bool old_format = false, first = true;
  int64_t matched = 0;
  int rc = DADA2HIP_OK;
  struct Parsed { bool ok; std::string err; int64_t us; };
  auto parse = [&](int slot) {
    const auto t_parse = fclk::now();
    Parsed r{true, std::string(), 0};
    for (int k = 0; k < nfile && r.ok; k++) r.ok = fq_read_chunk(src[k], chunk_reads, chunks[slot][k], r.err);
    r.us = us_since(t_parse);
    return r;
  };
  std::future<Parsed> ahead = std::async(std::launch::async, parse, 0);
  for (int slot = 0; rc == DADA2HIP_OK; slot ^= 1, first = false) {
    const Parsed got = ahead.get();
    tot[FS_US_PARSE] += got.us;
    if (!got.ok) { rc = fail(DADA2HIP_ERR_INPUT, got.err); break; }
    FqChunk *ch = chunks[slot];
    if (nfile == 2 && !match && ch[0].n != ch[1].n) {           // :966
      rc = fail(DADA2HIP_ERR_INPUT, "Mismatched forward and reverse sequence files: " + std::to_string(ch[0].n) + ", " + std::to_string(ch[1].n) + ".");
      break;
    }
    if (ch[0].n == 0 && (nfile == 1 || ch[1].n == 0)) break;    // :645, :936
    ahead = std::async(std::launch::async, parse, slot ^ 1);
    const int64_t first_no = match ? 0 : nin + 1;               // the number of the chunk's first record, where records keep theirs
    nin += ch[0].n;                                             // :646, :938
    if (first)
      for (int k = 0; k < nfile; k++)
        if (P[k].qual_offset == 0) P[k].qual_offset = fq_auto_offset(ch[k]);
    const FqChunk *cur[2] = {&ch[0], &ch[1]};
    if (match) {                                                // :940-991
      const auto t_join = fclk::now();
      if (first) {
        if (ch[0].n == 0) { rc = fail(DADA2HIP_ERR_INPUT, "dada2hip: the forward file's first chunk is empty: no id to detect the id field from."); break; }
        if (id_field == 0) {
          const std::string id1 = fq_id(ch[0], 0);
          id_field = fid::detect_field(std::string_view(id1).substr(1), sep, old_format);
          if (id_field == 0) { rc = fail(DADA2HIP_ERR_INPUT, "Couldn't automatically detect the sequence identifier field in the fastq id string."); break; }
        }
      }
      for (int k = 0; k < 2; k++) {
        const FqChunk *w = &ch[k];
        if (rem[k].n > 0) {                                     // :962-963
          std::swap(work[k], rem[k]);
          fq_gather(work[k], ch[k], fq_pick(idx, 0, ch[k].n, [](int64_t) { return true; }));
          w = &work[k];
        }
        cur[k] = w;
        keys[k].resize((size_t)w->n);
        d2::parallel_for((size_t)w->n, 4096, [&](size_t lo, size_t hi) {
          for (size_t i = lo; i < hi; i++)
            keys[k][i] = fid::id_key(std::string_view(w->hdr.data() + w->hoff[i], (size_t)(w->hoff[i + 1] - w->hoff[i])), sep, id_field,
                                     old_format && k == 0);
        });
      }
      fid::join(keys[0], keys[1], inset[0], inset[1], pool_for);
      for (int k = 0; k < 2; k++) {
        const FqChunk &w = *cur[k];
        sel[k].clear(); tmp.clear();
        fq_gather(sel[k], w, fq_pick(idx, 0, w.n, [&](int64_t i) { return inset[k][(size_t)i] != 0; }));
        fq_gather(tmp, w, fq_pick(idx, (int64_t)fid::past_last(inset[k]), w.n, [](int64_t) { return true; }));
        std::swap(rem[k], tmp);
      }
      tot[FO_US_IDJOIN] += us_since(t_join);
      if (sel[0].n != sel[1].n) {
        rc = fail(DADA2HIP_ERR_INPUT, "dada2hip: id matching kept " + std::to_string(sel[0].n) + " forward and " + std::to_string(sel[1].n) +
                                          " reverse records of a chunk (duplicate ids?).");
        break;
      }
      cur[0] = &sel[0]; cur[1] = &sel[1];
      matched += sel[0].n;
      if (sel[0].n == 0) continue;
    }
    int64_t n = cur[0]->n;
    if (orient_fwd && nfile == 1) {                             // :648-658
      const FqChunk &c = *cur[0];
      code[0].resize((size_t)n); win[0].resize(2 * (size_t)n); ori[0].assign((size_t)n, 0);
      rc = dada2hip_filter_reads_oriented(ctx, n, c.seq.data(), c.qual.data(), c.off.data(), &P[0], orient_fwd, 0, code[0].data(), win[0].data(),
                                          nullptr, nullptr, nullptr, nullptr, ori[0].data(), st, errbuf, errlen);
      if (rc != DADA2HIP_OK) { name_short(c, ori[0], "", first_no); break; }
      add_stats(true);
      tot[FO_DROPPED_ORIENT] += st[FO_DROPPED_ORIENT]; tot[FO_FLIPPED] += st[FO_FLIPPED];
      keep.assign((size_t)n, 0); keep2.assign((size_t)n, 0); flip.assign((size_t)n, 0);
      for (int64_t i = 0; i < n; i++) {
        if (code[0][(size_t)i] != 0) continue;
        if (ori[0][(size_t)i] == 1) { keep2[(size_t)i] = 1; flip[(size_t)i] = 1; } else keep[(size_t)i] = 1;
        nout++;
      }
      // :655-657 c(fq[keepF], fq.rc[keepR])
      if (!wr[0].put(c, keep, win[0], std::vector<uint8_t>(), err) || !wr[0].put(c, keep2, win[0], flip, err)) rc = fail(DADA2HIP_ERR_RUNTIME, err);
      continue;
    }
    if (orient_fwd) {                                           // :993-1007: the forward test on both files, then the chunks rebuilt
      for (int k = 0; k < 2 && rc == DADA2HIP_OK; k++) {
        const FqChunk &c = *cur[k];
        ori[k].assign((size_t)n, 0);
        rc = dada2hip_filter_reads_oriented(ctx, n, c.seq.data(), nullptr, c.off.data(), nullptr, orient_fwd, 1, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, ori[k].data(), st, errbuf, errlen);
        if (rc != DADA2HIP_OK) { name_short(c, ori[k], k == 0 ? "forward " : "reverse ", first_no); break; }
        add_stats(false);
      }
      if (rc != DADA2HIP_OK) break;
      comp[0].clear(); comp[1].clear();
      fq_pick(idx, 0, n, [&](int64_t i) { return ori[0][(size_t)i] == 0; });                          // keepF
      fq_gather(comp[0], *cur[0], idx); fq_gather(comp[1], *cur[1], idx);
      const int64_t as_given = comp[0].n;
      fq_pick(idx, 0, n, [&](int64_t i) { return ori[0][(size_t)i] != 0 && ori[1][(size_t)i] == 0; });   // keepR
      fq_gather(comp[0], *cur[1], idx); fq_gather(comp[1], *cur[0], idx);
      tot[FO_FLIPPED] += comp[0].n - as_given; tot[FO_DROPPED_ORIENT] += n - comp[0].n;
      cur[0] = &comp[0]; cur[1] = &comp[1];
      n = comp[0].n;
      if (n == 0) continue;
    }
    keep.assign((size_t)n, 1);
    for (int k = 0; k < nfile; k++) {                           // as filter_files_body: each read by its direction's parameters, the pair's AND
      const FqChunk &c = *cur[k];
      code[k].resize((size_t)n); win[k].resize(2 * (size_t)n);
      rc = dada2hip_filter_reads(ctx, n, c.seq.data(), c.qual.data(), c.off.data(), &P[k], code[k].data(), win[k].data(), nullptr, nullptr,
                                 nullptr, nullptr, st, errbuf, errlen);
      if (rc != DADA2HIP_OK) break;
      add_stats(k == 0);
      for (int64_t i = 0; i < n; i++) if (code[k][(size_t)i] != 0) keep[(size_t)i] = 0;
    }
    if (rc != DADA2HIP_OK) break;
    for (int64_t i = 0; i < n; i++) nout += keep[(size_t)i];
    for (int k = 0; k < nfile && rc == DADA2HIP_OK; k++)
      if (!wr[k].put(*cur[k], keep, win[k], std::vector<uint8_t>(), err)) rc = fail(DADA2HIP_ERR_RUNTIME, err);
  }
  if (ahead.valid()) ahead.wait();
  for (int k = 0; k < nfile; k++) {
    if (!wr[k].finish(err) && rc == DADA2HIP_OK) rc = fail(DADA2HIP_ERR_RUNTIME, err);
    tot[FS_US_DEFLATE] += wr[k].us_deflate; tot[FS_US_WRITE] += wr[k].us_write;
  }
  if (rc != DADA2HIP_OK) {                                      // nothing half written is left behind
    for (int k = 0; k < nfile; k++) (void)remove(out[k]);
    return rc;
  }
  if (match) tot[FO_DROPPED_IDS] = nin - matched;
  return call.finish(tot, sizeof tot, FS_US_TOTAL, stats);
}

// removePrimers' file level (R/filter.R:116-225): dada2hip_primers_reads per chunk, the kept windows written in the kept
// orientation, and the whole-file rule (:157-158) at the end - it asks for the matches of the reads AS GIVEN, summed over the file
int primers_file_body(const char *in, const char *out, const dada2hip_primer_params *params, int32_t compress, int64_t chunk_reads,
                      int32_t device, int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen) {
  FqCall call(reads_in, reads_out);
  if (!in || !out || !params) { set_err(errbuf, errlen, "File paths must be provided in character format."); return DADA2HIP_ERR_INPUT; }
  if (strcmp(in, out) == 0) { set_err(errbuf, errlen, "Output files must be distinct from the input files."); return DADA2HIP_ERR_INPUT; }   // :102
  int64_t tot[DADA2HIP_PRIMERS_NSTATS] = {0}, st[DADA2HIP_PRIMERS_NSTATS];
  std::vector<int32_t> code, flip32, first, last;
  int rc = fq_run_chunks(1, &in, &out, compress, chunk_reads, tot, FqClockWords{PS_US_PARSE, PS_US_DEFLATE, PS_US_WRITE, PS_US_INFLATE}, call,
                         [&](FqChunk *ch, bool, std::vector<uint8_t> &keep, std::vector<int32_t> *win, std::vector<uint8_t> &flip) -> int {
    const int64_t n = ch[0].n;
    code.resize((size_t)n); flip32.resize((size_t)n); first.resize((size_t)n); last.resize((size_t)n);
    win[0].assign(2 * (size_t)n, 0); flip.assign((size_t)n, 0);
    const int r = dada2hip_primers_reads(n, ch[0].seq.data(), ch[0].off.data(), params, device, code.data(), flip32.data(), first.data(),
                                         last.data(), nullptr, nullptr, st, errbuf, errlen);
    if (r != DADA2HIP_OK) {
      if (r == DADA2HIP_ERR_UNSUPPORTED) {                      // a letter that is no IUPAC code: name the record, not its number in the chunk
        for (int64_t i = 0; i < n; i++)
          if (code[i] == 4) {
            const std::string id(ch[0].hdr.data() + ch[0].hoff[i], (size_t)(ch[0].hoff[i + 1] - ch[0].hoff[i]));
            set_err(errbuf, errlen, ("dada2hip: read " + std::to_string(call.nin - n + i + 1) + " (" + id +
                                     ") holds a letter outside the upper-case IUPAC codes ACGTMRWSYKVHDBN.").c_str());
            break;
          }
      }
      return r;
    }
    for (int i = 0; i <= PS_CALL_LAST; i++) tot[i] += st[i];
    for (int64_t i = 0; i < n; i++) {
      if (code[i] != 0) { keep[i] = 0; continue; }
      win[0][2 * i] = first[i] - 1; win[0][2 * i + 1] = last[i] - first[i] + 1;   // :213 narrow(fq, first, last)
      flip[i] = (uint8_t)flip32[i];
    }
    return DADA2HIP_OK;
  }, errbuf, errlen);
  if (rc != DADA2HIP_OK) return rc;
  if (tot[PS_HITS_FWD] == 0 || (params->primer_rev && tot[PS_HITS_REV] == 0)) {   // :157-158
    (void)remove(out);
    call.nout = 0;
  }
  return call.finish(tot, sizeof tot, PS_US_TOTAL, stats);
}

// ---- the read diagnostics' file level (R/plot-methods.R:163-243 on qa()'s perCycle$quality; :293-299 plotComplexity) ----------------
// fq_run_chunks without writers: a chunk's first records, while fewer than max_reads have been profiled (0: no limit), go to
// dada2hip_qprofile_reads / the complexity calls; the rest of the file is still parsed, for its count of records.
inline int64_t rq_take(const FqChunk &c, int64_t max_reads, int64_t done) { return max_reads > 0 ? std::max<int64_t>(0, std::min(c.n, max_reads - done)) : c.n; }
inline bool rq_is_dir(const char *path) { struct stat sb; return stat(path, &sb) == 0 && S_ISDIR(sb.st_mode); }
inline void rq_add_call(int64_t *tot, const int64_t *st) {
  for (int i = RQ_CALL_FIRST; i <= RQ_CALL_LAST; i++)
    if (i == RQ_CYCLES) tot[i] = std::max(tot[i], st[i]); else tot[i] += st[i];
}

int qprofile_file_body(const char *path, int64_t chunk_reads, int64_t max_reads, int32_t qual_offset, int32_t device, dada2hip_qprofile **out,
                       int64_t *stats, char *errbuf, size_t errlen) {
  FqCall call(nullptr, nullptr);
  if (out) *out = nullptr;
  if (!path || !out) { set_err(errbuf, errlen, "File paths must be provided in character format."); return DADA2HIP_ERR_INPUT; }
  if (max_reads < 0 || (qual_offset != 0 && qual_offset != 33 && qual_offset != 64)) {
    set_err(errbuf, errlen, "dada2hip: the quality offset must be 33, 64 or 0 (Auto), and the number of reads profiled not negative.");
    return DADA2HIP_ERR_INPUT;
  }
  if (rq_is_dir(path)) { set_err(errbuf, errlen, "dada2hip: a directory is not profiled; name its files."); return DADA2HIP_ERR_INPUT; }
  std::unique_ptr<dada2hip_qprofile> P(new dada2hip_qprofile());
  P->qual_offset = qual_offset;
  int64_t tot[DADA2HIP_READQC_NSTATS] = {0}, st[DADA2HIP_READQC_NSTATS];
  std::vector<int64_t> piece;
  const int rc = fq_run_chunks(1, &path, nullptr, 0, chunk_reads, tot, FqClockWords{RQ_US_PARSE, RQ_US_PARSE, RQ_US_PARSE, RQ_US_INFLATE}, call,
                               [&](FqChunk *ch, bool first, std::vector<uint8_t> &, std::vector<int32_t> *, std::vector<uint8_t> &) -> int {
    const FqChunk &c = ch[0];
    if (first && P->qual_offset == 0) P->qual_offset = fq_auto_offset(c);
    const int64_t take = rq_take(c, max_reads, P->profiled);
    if (take <= 0) return DADA2HIP_OK;
    int64_t mx = 0;
    for (int64_t i = 0; i < take; i++) mx = std::max(mx, c.off[i + 1] - c.off[i]);
    if (mx > (int64_t)1 << 18) {
      set_err(errbuf, errlen, "dada2hip: a read of more than 262144 cycles is not supported by the quality profile.");
      return DADA2HIP_ERR_UNSUPPORTED;
    }
    if (mx > P->ncycle) { P->counts.resize((size_t)mx * DADA2HIP_QPROFILE_NSCORE, 0); P->ncycle = (int32_t)mx; }   // a later chunk with a longer read
    piece.resize((size_t)mx * DADA2HIP_QPROFILE_NSCORE);
    const int r = dada2hip_qprofile_reads(take, c.qual.empty() ? "" : c.qual.data(), c.off.data(), device, (int32_t)mx, piece.data(), st, errbuf, errlen);
    if (r != DADA2HIP_OK) {
      if (r == DADA2HIP_ERR_INPUT)                              // a letter outside '!'..'~': name the record, not its number in the chunk
        for (int64_t i = 0; i < c.off[take]; i++) {
          const unsigned char q = (unsigned char)c.qual[(size_t)i];
          if (q >= 33 && q <= 126) continue;
          const int64_t rd = std::upper_bound(c.off.begin(), c.off.end(), i) - c.off.begin() - 1;
          const std::string id(c.hdr.data() + c.hoff[rd], (size_t)(c.hoff[rd + 1] - c.hoff[rd]));
          set_err(errbuf, errlen, ("dada2hip: read " + std::to_string(call.nin - c.n + rd + 1) + " (" + id + ") holds a quality letter outside '!'..'~'.").c_str());
          break;
        }
      return r;
    }
    for (size_t i = 0; i < piece.size(); i++) P->counts[i] += piece[i];
    rq_add_call(tot, st);
    P->profiled += take;
    return DADA2HIP_OK;
  }, errbuf, errlen);
  if (rc != DADA2HIP_OK) return rc;
  if (P->qual_offset == 0) P->qual_offset = 33;
  P->reads = call.nin;
  call.nout = P->profiled;
  *out = P.release();
  return call.finish(tot, sizeof tot, RQ_US_TOTAL, stats);
}

int complexity_file_body(const char *path, int64_t chunk_reads, int64_t max_reads, int32_t kmer_size, int32_t window, int32_t by, int32_t device,
                         double **out, int64_t *nout, int64_t *stats, char *errbuf, size_t errlen) {
  FqCall call(nullptr, nullptr);
  if (out) *out = nullptr;
  if (nout) *nout = 0;
  if (!path || !out || !nout) { set_err(errbuf, errlen, "File paths must be provided in character format."); return DADA2HIP_ERR_INPUT; }
  if (max_reads < 0) { set_err(errbuf, errlen, "dada2hip: the number of reads profiled must not be negative."); return DADA2HIP_ERR_INPUT; }
  if (rq_is_dir(path)) { set_err(errbuf, errlen, "dada2hip: a directory is not profiled; name its files."); return DADA2HIP_ERR_INPUT; }
  // (the refusals of the arguments, before the file is touched: a call on no reads makes them)
  int r0 = window == 0 ? dada2hip_complexity_reads(0, nullptr, nullptr, kmer_size, 0, by, device, nullptr, nullptr, errbuf, errlen)
                       : d2_complexity_pairs(0, nullptr, nullptr, kmer_size, window, by, device, nullptr, nullptr, errbuf, errlen);
  if (r0 != DADA2HIP_OK) return r0;
  const int k = kmer_size == 0 ? 2 : kmer_size;
  int64_t tot[DADA2HIP_READQC_NSTATS] = {0}, st[DADA2HIP_READQC_NSTATS];
  std::vector<double> vals;                                     // window 0: the values; otherwise the pairs of readqc_plain.h
  std::vector<int64_t> lens;
  int64_t done = 0, maxlen = 0;
  const int rc = fq_run_chunks(1, &path, nullptr, 0, chunk_reads, tot, FqClockWords{RQ_US_PARSE, RQ_US_PARSE, RQ_US_PARSE, RQ_US_INFLATE}, call,
                               [&](FqChunk *ch, bool, std::vector<uint8_t> &, std::vector<int32_t> *, std::vector<uint8_t> &) -> int {
    const FqChunk &c = ch[0];
    const int64_t take = rq_take(c, max_reads, done);
    if (take <= 0) return DADA2HIP_OK;
    const char *seq = c.seq.empty() ? "" : c.seq.data();
    const size_t per = window == 0 ? 1 : 2, at = vals.size();
    vals.resize(at + per * (size_t)take);
    const int r = window == 0 ? dada2hip_complexity_reads(take, seq, c.off.data(), kmer_size, 0, by, device, vals.data() + at, st, errbuf, errlen)
                              : d2_complexity_pairs(take, seq, c.off.data(), kmer_size, window, by, device, vals.data() + at, st, errbuf, errlen);
    if (r != DADA2HIP_OK) return r;
    for (int64_t i = 0; i < take; i++) { lens.push_back(c.off[i + 1] - c.off[i]); maxlen = std::max(maxlen, lens.back()); }
    rq_add_call(tot, st);
    done += take;
    return DADA2HIP_OK;
  }, errbuf, errlen);
  if (rc != DADA2HIP_OK) return rc;
  if (window > 0 && maxlen - window < 1) { set_err(errbuf, errlen, CW_ERR_NO_START); return DADA2HIP_ERR_INPUT; }
  double *res = (double *)malloc(std::max<size_t>(1, (size_t)done) * sizeof(double));
  if (!res) throw std::bad_alloc();
  for (int64_t i = 0; i < done; i++)
    res[i] = window == 0 ? vals[(size_t)i] : cw_finish(lens[(size_t)i], maxlen, vals[2 * (size_t)i], vals[2 * (size_t)i + 1], k);
  *out = res; *nout = done;
  call.nout = done;
  return call.finish(tot, sizeof tot, RQ_US_TOTAL, stats);
}

template <typename F> int filter_files_guarded(char *errbuf, size_t errlen, F &&f) {
  try {
    return f();
  } catch (const std::bad_alloc &) {
    set_err(errbuf, errlen, "dada2hip: out of host memory during filtering");
  } catch (const std::exception &e) {
    set_err(errbuf, errlen, (std::string("dada2hip: ") + e.what()).c_str());
  } catch (...) {
    set_err(errbuf, errlen, "dada2hip: unknown error during filtering");
  }
  return DADA2HIP_ERR_RUNTIME;
}

}  // namespace

extern "C" {

int dada2hip_filter_fastq(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params, int32_t compress,
                          int64_t chunk_reads, int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen) {
  return filter_files_guarded(errbuf, errlen, [&] {
    return filter_files_body(ctx, 1, &in, &out, &params, compress, chunk_reads, reads_in, reads_out, stats, errbuf, errlen);
  });
}

int dada2hip_filter_fastq_paired(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f, const char *out_r,
                                 const dada2hip_filter_params *params_f, const dada2hip_filter_params *params_r, int32_t compress,
                                 int64_t chunk_reads, int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen) {
  const char *in[2] = {in_f, in_r}, *out[2] = {out_f, out_r};
  const dada2hip_filter_params *params[2] = {params_f, params_r};
  return filter_files_guarded(errbuf, errlen, [&] {
    return filter_files_body(ctx, 2, in, out, params, compress, chunk_reads, reads_in, reads_out, stats, errbuf, errlen);
  });
}

int dada2hip_filter_fastq_oriented(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params,
                                   const char *orient_fwd, int32_t compress, int64_t chunk_reads, int64_t *reads_in, int64_t *reads_out,
                                   int64_t *stats, char *errbuf, size_t errlen) {
  return filter_files_guarded(errbuf, errlen, [&] {
    if (!orient_fwd) { set_err(errbuf, errlen, "dada2hip: bad arguments"); return (int)DADA2HIP_ERR_INPUT; }
    return filter_files_ex_body(ctx, 1, &in, &out, &params, orient_fwd, 0, nullptr, 0, compress, chunk_reads, reads_in, reads_out, stats, errbuf,
                                errlen);
  });
}

int dada2hip_filter_fastq_paired_ex(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f, const char *out_r,
                                    const dada2hip_filter_params *params_f, const dada2hip_filter_params *params_r, const char *orient_fwd,
                                    int32_t match_ids, const char *id_sep, int32_t id_field, int32_t compress, int64_t chunk_reads,
                                    int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen) {
  const char *in[2] = {in_f, in_r}, *out[2] = {out_f, out_r};
  const dada2hip_filter_params *params[2] = {params_f, params_r};
  return filter_files_guarded(errbuf, errlen, [&] {
    return filter_files_ex_body(ctx, 2, in, out, params, orient_fwd, match_ids, id_sep, id_field, compress, chunk_reads, reads_in, reads_out,
                                stats, errbuf, errlen);
  });
}

int dada2hip_primers_fastq(const char *in, const char *out, const dada2hip_primer_params *params, int32_t compress, int64_t chunk_reads,
                           int32_t device, int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen) {
  return filter_files_guarded(errbuf, errlen, [&] {
    return primers_file_body(in, out, params, compress, chunk_reads, device, reads_in, reads_out, stats, errbuf, errlen);
  });
}

int dada2hip_qprofile_fastq(const char *path, int64_t chunk_reads, int64_t max_reads, int32_t qual_offset, int32_t device,
                            dada2hip_qprofile **out, int64_t *stats, char *errbuf, size_t errlen) {
  return filter_files_guarded(errbuf, errlen, [&] {
    return qprofile_file_body(path, chunk_reads, max_reads, qual_offset, device, out, stats, errbuf, errlen);
  });
}
int32_t dada2hip_qprofile_ncycle(const dada2hip_qprofile *p) { return p->ncycle; }
const int64_t *dada2hip_qprofile_counts(const dada2hip_qprofile *p) { return p->counts.data(); }
int64_t dada2hip_qprofile_reads_total(const dada2hip_qprofile *p) { return p->reads; }
int64_t dada2hip_qprofile_profiled(const dada2hip_qprofile *p) { return p->profiled; }
int32_t dada2hip_qprofile_qual_offset(const dada2hip_qprofile *p) { return p->qual_offset; }
void dada2hip_qprofile_free(dada2hip_qprofile *p) { delete p; }

int dada2hip_complexity_fastq(const char *path, int64_t chunk_reads, int64_t max_reads, int32_t kmer_size, int32_t window, int32_t by,
                              int32_t device, double **out, int64_t *nout, int64_t *stats, char *errbuf, size_t errlen) {
  return filter_files_guarded(errbuf, errlen, [&] {
    return complexity_file_body(path, chunk_reads, max_reads, kmer_size, window, by, device, out, nout, stats, errbuf, errlen);
  });
}
void dada2hip_complexity_free(double *values) { free(values); }

}  // extern "C"

// ---- the device dereplicator's two ends on the host (derep_dev_host.h has the device between them) ---------------------------------
// d2_derep_from_rows: the rows of the device into a dada2hip_derep - derep_dev_plain.h's order, means and map over the host pool.
// dada2hip_filter_derep_fastq, _paired: dada2hip_filter_fastq's chunk pipeline with the kept windows dereplicated on the way -
// single-end out of the filter's own slots (d2_dd_filter_chunk), a pair's files by a second upload of the kept windows once both
// verdicts of the chunk are known (d2_dd_feed).  filter_files_body and the entries above are not touched by any of it.
#include "derep_dev_plain.h"

// sums null: the object without a quality matrix; order_out (nuniq words, or null): output row -> device unique
static int derep_from_rows_body(int64_t nuniq, const int64_t *off, const int32_t *len, const int64_t *count, const int64_t *first,
                                const uint8_t *bytes, const uint64_t *sums, int64_t nreads, const int32_t *ruid, int64_t chunk_reads,
                                int32_t qual_offset, int32_t min_char, int32_t *order_out, dada2hip_derep **out, char *errbuf, size_t errlen) {
  return filter_files_guarded(errbuf, errlen, [&]() -> int {
    if (!out) { set_err(errbuf, errlen, "dada2hip: bad arguments"); return DADA2HIP_ERR_INPUT; }
    *out = nullptr;
    DdRows R;
    R.nuniq = nuniq; R.off = off; R.len = len; R.count = count; R.first = first; R.bytes = bytes; R.sums = sums;
    DdPlan P;
    const int prc = dd_order(R, chunk_reads > 0 ? chunk_reads : 1000000, P, [](int32_t *f, size_t n, auto less) { pool_sort(f, n, less); });
    if (prc == DDP_NONE) { set_err(errbuf, errlen, "Only zero-length sequences detected during dereplication."); return DADA2HIP_ERR_INPUT; }
    if (prc == DDP_OVERFLOW) { set_err(errbuf, errlen, "dada2hip: an abundance or the number of uniques exceeds the integer range."); return DADA2HIP_ERR_INPUT; }
    const int offset = dd_offset(qual_offset, min_char);
    const size_t U = (size_t)nuniq, ml = (size_t)P.maxlen;
    std::unique_ptr<dada2hip_derep> d(new dada2hip_derep());
    d->nreads = nreads; d->maxlen = P.maxlen;
    d->abund.resize(U); d->seq_ptrs.resize(U);
    std::vector<size_t> soff(U + 1, 0);
    for (size_t k = 0; k < U; k++) soff[k + 1] = soff[k] + (size_t)len[P.order[k]] + 1;
    d->seq_blob.reset(new char[soff[U]]);
    d->has_quals = sums != nullptr;
    if (sums) d->quals.reset(new double[U * ml]);
    const double na = na_real();
    d2::parallel_for(U, 256, [&](size_t k0, size_t k1) {
      for (size_t k = k0; k < k1; k++) {
        const int32_t u = P.order[k];
        d->abund[k] = (int32_t)count[u];
        if (sums) dd_quality_row(R, u, offset, P.maxlen, na, &d->quals[k * ml]);
        char *dst = d->seq_blob.get() + soff[k];
        memcpy(dst, bytes + off[u], (size_t)len[u]);
        dst[len[u]] = 0;
        d->seq_ptrs[k] = dst;
      }
    });
    d->map.resize((size_t)nreads);
    d2::parallel_for((size_t)nreads, 65536, [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++) d->map[i] = dd_map_entry(ruid[i], P, DADA2HIP_NA_INTEGER);
    });
    if (order_out) memcpy(order_out, P.order.data(), U * sizeof(int32_t));
    *out = d.release();
    return DADA2HIP_OK;
  });
}

extern "C" int d2_derep_from_rows(int64_t nuniq, const int64_t *off, const int32_t *len, const int64_t *count, const int64_t *first,
                                  const uint8_t *bytes, const uint64_t *sums, int64_t nreads, const int32_t *ruid, int64_t chunk_reads,
                                  int32_t qual_offset, int32_t min_char, dada2hip_derep **out, char *errbuf, size_t errlen) {
  if (!sums) { set_err(errbuf, errlen, "dada2hip: bad arguments"); return DADA2HIP_ERR_INPUT; }
  return derep_from_rows_body(nuniq, off, len, count, first, bytes, sums, nreads, ruid, chunk_reads, qual_offset, min_char, nullptr, out, errbuf,
                              errlen);
}

// the object of a *_resident entry: no sums came down, so no matrix; order (nuniq words): output row -> device unique, what the
// device needs to write the sample's rows in the object's order.  The largest ceil(mean) follows by d2_derep_set_qmax.
extern "C" int d2_derep_from_rows_resident(int64_t nuniq, const int64_t *off, const int32_t *len, const int64_t *count, const int64_t *first,
                                           const uint8_t *bytes, int64_t nreads, const int32_t *ruid, int64_t chunk_reads, int32_t *order,
                                           dada2hip_derep **out, char *errbuf, size_t errlen) {
  if (!order) { set_err(errbuf, errlen, "dada2hip: bad arguments"); return DADA2HIP_ERR_INPUT; }
  return derep_from_rows_body(nuniq, off, len, count, first, bytes, nullptr, nreads, ruid, chunk_reads, 33, 255, order, out, errbuf, errlen);
}
extern "C" void d2_derep_set_qmax(dada2hip_derep *d, int32_t qmax) { if (d) d->qmax = qmax; }

namespace {

int filter_derep_files_body(dada2hip_filter *ctx, int nfile, const char *const *in, const char *const *out,
                            const dada2hip_filter_params *const *params, int32_t compress, int64_t chunk_reads, int64_t derep_chunk_reads,
                            int32_t derep_qual_offset, dada2hip_derep **const *derep, int64_t *reads_in, int64_t *reads_out, int64_t *stats,
                            char *errbuf, size_t errlen, dada2hip_sample **const *sample = nullptr, int64_t *resident_stats = nullptr) {
  FqCall call(reads_in, reads_out);
  for (int k = 0; k < nfile; k++) {
    if (!derep[k] || (sample && !sample[k])) { set_err(errbuf, errlen, "dada2hip: bad arguments"); return DADA2HIP_ERR_INPUT; }
    *derep[k] = nullptr;
    if (sample) *sample[k] = nullptr;
  }
  const bool write = out[0] != nullptr;
  for (int k = 0; k < nfile; k++)
    if (!in[k] || !params[k] || (out[k] != nullptr) != write) { set_err(errbuf, errlen, "File paths must be provided in character format."); return DADA2HIP_ERR_INPUT; }
  if (!ctx) { set_err(errbuf, errlen, "dada2hip: no filter context."); return DADA2HIP_ERR_INPUT; }
  for (int a = 0; a < nfile; a++) {                             // :627, :887
    for (int b = 0; b < nfile && write; b++)
      if (strcmp(in[a], out[b]) == 0) {
        set_err(errbuf, errlen, nfile == 1 ? "The output and input files must be different." : "The output and input file names must be different.");
        return DADA2HIP_ERR_INPUT;
      }
    for (int b = 0; b < a; b++)
      if ((write && strcmp(out[a], out[b]) == 0) || strcmp(in[a], in[b]) == 0) { set_err(errbuf, errlen, "The output and input file names must be different."); return DADA2HIP_ERR_INPUT; }
  }
  struct DdHold { void *p = nullptr; ~DdHold() { if (p) d2_dd_free(p); } } dd[2];
  // (the dereplicators live on the filter context's device: the first chunk's call says which - d2_dd_filter_chunk checks it)
  dada2hip_filter_params P[2];
  for (int k = 0; k < nfile; k++) P[k] = *params[k];
  int64_t tot[DADA2HIP_FILTER_DEREP_NSTATS] = {0}, st[DADA2HIP_FILTER_NSTATS];
  std::vector<int32_t> code[2];
  int32_t device = -1;
  const int rc = fq_run_chunks(nfile, in, write ? out : nullptr, compress, chunk_reads, tot, FqClockWords{FS_US_PARSE, FS_US_DEFLATE, FS_US_WRITE, FS_US_INFLATE}, call,
                               [&](FqChunk *ch, bool first, std::vector<uint8_t> &keep, std::vector<int32_t> *win, std::vector<uint8_t> &) -> int {
    const int64_t n = ch[0].n;
    if (device < 0) {
      device = d2_filter_device(ctx);
      for (int k = 0; k < nfile; k++) {
        const int r = d2_dd_open(device, derep_chunk_reads, derep_qual_offset, &dd[k].p, errbuf, errlen);
        if (r != DADA2HIP_OK) return r;
      }
    }
    for (int k = 0; k < nfile; k++) {
      if (first && P[k].qual_offset == 0) P[k].qual_offset = fq_auto_offset(ch[k]);
      code[k].resize((size_t)n); win[k].resize(2 * (size_t)n);
      const int r = nfile == 1 ? d2_dd_filter_chunk(ctx, dd[0].p, n, ch[k].seq.data(), ch[k].qual.data(), ch[k].off.data(), &P[k], code[k].data(),
                                                    win[k].data(), st, errbuf, errlen)
                               : dada2hip_filter_reads(ctx, n, ch[k].seq.data(), ch[k].qual.data(), ch[k].off.data(), &P[k], code[k].data(), win[k].data(),
                                                       nullptr, nullptr, nullptr, nullptr, st, errbuf, errlen);
      if (r != DADA2HIP_OK) return r;
      const int w0 = k == 0 ? 0 : FS_CLOCK_FIRST, w1 = k == 0 ? FS_COUNT - 1 : FS_CLOCK_LAST;   // (as filter_files_body)
      for (int i = w0; i <= w1; i++)
        if (i >= FS_TAKEN_FIRST && i <= FS_TAKEN_LAST) tot[i] = st[i]; else if (i != FS_US_TOTAL) tot[i] += st[i];
      for (int64_t i = 0; i < n; i++) if (code[k][i] != 0) keep[i] = 0;
    }
    for (int k = 0; k < nfile && nfile == 2; k++) {             // a pair: both objects or neither
      const int r = d2_dd_feed(dd[k].p, n, ch[k].seq.data(), ch[k].qual.data(), ch[k].off.data(), win[k].data(), keep.data(), errbuf, errlen);
      if (r != DADA2HIP_OK) return r;
    }
    return DADA2HIP_OK;
  }, errbuf, errlen);
  if (rc != DADA2HIP_OK) return rc;
  int64_t *dst = tot + DADA2HIP_FILTER_NSTATS;
  for (int k = 0; k < nfile && dd[k].p; k++) {
    int64_t ds[DADA2HIP_DEREP_NSTATS] = {0};
    // (the resident form: the sample's rows are written on the device from the dereplicator's own buffers, no sum comes down)
    const int r = sample ? d2_dd_finish_resident(dd[k].p, 1, derep[k], sample[k], ds, resident_stats ? resident_stats + k * DADA2HIP_RESIDENT_NSTATS : nullptr,
                                                 errbuf, errlen)
                         : d2_dd_finish(dd[k].p, 1, derep[k], ds, errbuf, errlen);
    if (r != DADA2HIP_OK) {
      for (int j = 0; j < nfile; j++) {
        dada2hip_derep_free(*derep[j]); *derep[j] = nullptr;
        if (sample) { dada2hip_sample_free(*sample[j]); *sample[j] = nullptr; }
        if (write) (void)remove(out[j]);
      }
      return r;
    }
    for (int i = 0; i < DD_COUNT; i++)                          // the forward object's words; of the reverse one the bytes and the clocks add
      if (k == 0) dst[i] = ds[i]; else if (i >= DD_BYTES_UP) dst[i] += ds[i];
  }
  return call.finish(tot, sizeof tot, FS_US_TOTAL, stats);
}

}  // namespace

extern "C" {

int dada2hip_filter_derep_fastq(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params, int32_t compress,
                                int64_t chunk_reads, int64_t derep_chunk_reads, int32_t derep_qual_offset, dada2hip_derep **derep,
                                int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf, size_t errlen) {
  dada2hip_derep **const dp[1] = {derep};
  return filter_files_guarded(errbuf, errlen, [&] {
    return filter_derep_files_body(ctx, 1, &in, &out, &params, compress, chunk_reads, derep_chunk_reads, derep_qual_offset, dp, reads_in, reads_out,
                                   stats, errbuf, errlen);
  });
}

int dada2hip_filter_derep_fastq_paired(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f, const char *out_r,
                                       const dada2hip_filter_params *params_f, const dada2hip_filter_params *params_r, int32_t compress,
                                       int64_t chunk_reads, int64_t derep_chunk_reads, int32_t derep_qual_offset, dada2hip_derep **derep_f,
                                       dada2hip_derep **derep_r, int64_t *reads_in, int64_t *reads_out, int64_t *stats, char *errbuf,
                                       size_t errlen) {
  const char *in[2] = {in_f, in_r}, *out[2] = {out_f, out_r};
  const dada2hip_filter_params *params[2] = {params_f, params_r};
  dada2hip_derep **const dp[2] = {derep_f, derep_r};
  return filter_files_guarded(errbuf, errlen, [&] {
    return filter_derep_files_body(ctx, 2, in, out, params, compress, chunk_reads, derep_chunk_reads, derep_qual_offset, dp, reads_in, reads_out,
                                   stats, errbuf, errlen);
  });
}

int dada2hip_filter_derep_fastq_resident(dada2hip_filter *ctx, const char *in, const char *out, const dada2hip_filter_params *params,
                                         int32_t compress, int64_t chunk_reads, int64_t derep_chunk_reads, int32_t derep_qual_offset,
                                         dada2hip_derep **derep, dada2hip_sample **sample, int64_t *reads_in, int64_t *reads_out, int64_t *stats,
                                         int64_t *resident_stats, char *errbuf, size_t errlen) {
  dada2hip_derep **const dp[1] = {derep};
  dada2hip_sample **const sp[1] = {sample};
  if (resident_stats) memset(resident_stats, 0, sizeof(int64_t) * DADA2HIP_RESIDENT_NSTATS);
  return filter_files_guarded(errbuf, errlen, [&] {
    return filter_derep_files_body(ctx, 1, &in, &out, &params, compress, chunk_reads, derep_chunk_reads, derep_qual_offset, dp, reads_in, reads_out,
                                   stats, errbuf, errlen, sp, resident_stats);
  });
}

int dada2hip_filter_derep_fastq_paired_resident(dada2hip_filter *ctx, const char *in_f, const char *in_r, const char *out_f, const char *out_r,
                                                const dada2hip_filter_params *params_f, const dada2hip_filter_params *params_r, int32_t compress,
                                                int64_t chunk_reads, int64_t derep_chunk_reads, int32_t derep_qual_offset, dada2hip_derep **derep_f,
                                                dada2hip_derep **derep_r, dada2hip_sample **sample_f, dada2hip_sample **sample_r, int64_t *reads_in,
                                                int64_t *reads_out, int64_t *stats, int64_t *resident_stats, char *errbuf, size_t errlen) {
  const char *in[2] = {in_f, in_r}, *out[2] = {out_f, out_r};
  const dada2hip_filter_params *params[2] = {params_f, params_r};
  dada2hip_derep **const dp[2] = {derep_f, derep_r};
  dada2hip_sample **const sp[2] = {sample_f, sample_r};
  if (resident_stats) memset(resident_stats, 0, sizeof(int64_t) * 2 * DADA2HIP_RESIDENT_NSTATS);
  return filter_files_guarded(errbuf, errlen, [&] {
    return filter_derep_files_body(ctx, 2, in, out, params, compress, chunk_reads, derep_chunk_reads, derep_qual_offset, dp, reads_in, reads_out,
                                   stats, errbuf, errlen, sp, resident_stats);
  });
}

}  // extern "C"
