// derep_dev_host.h — host side of the device dereplicator (derep_dev.inc.hip; derepFastq, R/sequenceIO.R:45-183); included by
// driver.cpp inside its extern "C" block, behind readqc_host.h, on top of stage_common.h and read_pieces.h.
//
// A DerepDev is one derep object in the making: the table, the arena of the uniques' bytes with the quality sums beside it, and
// the per-unique words stay on the device from the first piece to the end; per piece one word per read comes back (its unique's
// device number, for the map), at the end one row per unique.  The order, the division and the map's renumbering are
// derep_dev_plain.h's, and derep.cpp (d2_derep_from_rows) builds the dada2hip_derep - this file never sees that struct.
// Three ways in: dada2hip_derep_reads (reads in memory through read_pieces.h's two slots, DADA2HIP_DEREP_PIECE, _PIECE_BYTES);
// d2_dd_filter_chunk, the single-end fused path - dada2hip_filter_reads with a hook in its scatter, where the piece's verdicts
// are final (the complexity rule is the host's) and its reads still lie in the slot; d2_dd_feed for a pair's files, whose
// verdict needs both.  A piece is dereplicated synchronously: dd_piece returns with the stream idle, so the slot can be reused.
//
// Growth: before a piece of m reads the table is rebuilt (k_dd_rebuild into a fresh one of four times the need) if the piece
// could fill it past half; the per-unique arrays and the arena double by device copies.  Rounds: a piece takes one round plus
// one per slot a read has to move on after a true collision - at most the uniques plus one, then DADA2HIP_ERR_INTERNAL.
#pragma once

namespace {

struct DerepDev {
  int device = 0;
  int64_t chunk_reads = 1000000;
  int32_t qual_offset = 0;
  bool no_qual = false;                        // seqtab_host.h: strings without qualities - no sums beside the arena, a null `qual`
  Events<2> ev;
  DevBuf<int32_t> tab;
  size_t cap = 0, ucap = 0, acap = 0;
  DevBuf<unsigned long long> u_hash, u_count, u_first, sums;
  DevBuf<long long> u_off;
  DevBuf<int32_t> u_len;
  DevBuf<uint8_t> arena;
  DevBuf<DdCounters> ctr;
  PinBuf<DdCounters> h_ctr;
  DevBuf<DdRead> d_rec;
  PinBuf<DdRead> h_rec;
  DevBuf<unsigned long long> r_hash;
  DevBuf<int32_t> r_slot, r_uid, r_ref;
  PinBuf<int32_t> h_uid;
  int64_t nuniq = 0, used = 0, next_idx = 0;
  std::vector<int32_t> ruid;                   // per read of the call: its unique's device number, DD_SKIP for a zero-length read
  int64_t st[DADA2HIP_DEREP_NSTATS] = {0};
  std::mutex mu;
  DdState state() const {
    DdState T;
    T.tab = tab.p; T.cap = (int)cap;
    const int bits = knobs().derep_hash_bits;
    T.hmask = bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
    T.u_hash = u_hash.p; T.u_count = u_count.p; T.u_first = u_first.p; T.sums = sums.p; T.u_off = u_off.p; T.u_len = u_len.p;
    T.arena = arena.p; T.ctr = ctr.p;
    return T;
  }
};

inline size_t dd_pow2_at_least(size_t v) { size_t c = 8; while (c < v) c <<= 1; return c; }
constexpr size_t DD_CAP_MAX = (size_t)1 << 30;   // slots: the table's words are int32, its index an int

void dd_open(DerepDev &D, int32_t device, int64_t chunk_reads, int32_t qual_offset) {
  if (qual_offset != 0 && qual_offset != 33 && qual_offset != 64) throw InputError{"dada2hip: the quality offset must be 33, 64 or 0 (Auto)."};
  select_device(device);
  D.device = device; D.chunk_reads = chunk_reads > 0 ? chunk_reads : 1000000; D.qual_offset = qual_offset;
  D.ev.create();
  D.ctr.alloc(1); D.h_ctr.alloc(1);
  DdCounters c0;
  c0.arena_used = 0; c0.nuniq = 0; c0.pending = 0; c0.err = 0; c0.minq = 255;
  D2_HIP(hipMemcpy(D.ctr.p, &c0, sizeof c0, hipMemcpyHostToDevice));
}

// room for a piece of m reads and `bytes` letters, on stream st
void dd_reserve(DerepDev &D, int64_t m, int64_t bytes, hipStream_t st) {
  const size_t need_u = (size_t)(D.nuniq + m), need_a = (size_t)(D.used + bytes);
  if (need_u > (size_t)INT32_MAX) throw InputError{"dada2hip: too many unique sequences to dereplicate."};
  if (need_u > D.ucap) {                                         // the per-unique words: twice as many, the old ones copied over
    const size_t nc = std::max(need_u, 2 * D.ucap), n = (size_t)D.nuniq;
    auto grow = [&](auto &buf) {
      using B = typename std::remove_reference<decltype(buf)>::type;
      B nb;
      nb.alloc(nc);
      if (n) D2_HIP(hipMemcpyAsync(nb.p, buf.p, n * sizeof(*buf.p), hipMemcpyDeviceToDevice, st));
      D2_HIP(hipStreamSynchronize(st));                          // (the old buffer goes back to the cache behind the copy)
      std::swap(nb.p, buf.p); std::swap(nb.n, buf.n);
    };
    grow(D.u_hash); grow(D.u_count); grow(D.u_first); grow(D.u_off); grow(D.u_len);
    D.ucap = nc;
  }
  if (need_a > D.acap) {                                         // the arena and the sums beside it; fresh sums are zero
    const size_t nc = std::max({need_a, 2 * D.acap, (size_t)1 << 16}), n = (size_t)D.used;
    DevBuf<uint8_t> na;
    DevBuf<unsigned long long> ns;
    na.alloc(nc);
    if (!D.no_qual) ns.alloc(nc);
    if (n) {
      D2_HIP(hipMemcpyAsync(na.p, D.arena.p, n, hipMemcpyDeviceToDevice, st));
      if (!D.no_qual) D2_HIP(hipMemcpyAsync(ns.p, D.sums.p, n * 8, hipMemcpyDeviceToDevice, st));
    }
    if (!D.no_qual) D2_HIP(hipMemsetAsync(ns.p + n, 0, (nc - n) * 8, st));
    D2_HIP(hipStreamSynchronize(st));
    std::swap(na.p, D.arena.p); std::swap(na.n, D.arena.n); std::swap(ns.p, D.sums.p); std::swap(ns.n, D.sums.n);
    D.acap = nc;
  }
  auto fresh_table = [&](size_t nc) {
    if (nc > DD_CAP_MAX) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator's table would pass 2^30 slots."};
    DevBuf<int32_t> nt;
    nt.alloc(nc);
    D2_HIP(hipMemsetAsync(nt.p, 0xFF, nc * sizeof(int32_t), st));   // DD_EMPTY
    D2_HIP(hipStreamSynchronize(st));
    std::swap(nt.p, D.tab.p); std::swap(nt.n, D.tab.n);
    D.cap = nc;
  };
  if (D.cap == 0) fresh_table(dd_pow2_at_least((size_t)(knobs().derep_table > 0 ? knobs().derep_table : 1 << 17)));
  if (2 * need_u > D.cap) {                                      // the table: the piece could fill it past half
    fresh_table(dd_pow2_at_least(4 * need_u));
    launch_dd_rebuild(D.state(), (int)D.nuniq, st);
    D2_HIP(hipMemcpyAsync(D.h_ctr.p, D.ctr.p, sizeof(DdCounters), hipMemcpyDeviceToHost, st));
    sync_checked(st);
    if (D.h_ctr.p->err != 0) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator's rebuild found its table full."};
    D.st[DD_REBUILDS]++;
  }
}

// the m reads of D.h_rec (bytes: the sum of their lengths), lying in d_seq / d_qual, on stream st; returns with st idle
void dd_piece(DerepDev &D, int m, int64_t bytes, const uint8_t *d_seq, const uint8_t *d_qual, hipStream_t st) {
  if (m <= 0) return;
  auto t_up = clk::now();
  dd_reserve(D, m, bytes, st);
  D.d_rec.alloc((size_t)m); D.r_hash.alloc((size_t)m); D.r_slot.alloc((size_t)m); D.r_uid.alloc((size_t)m); D.r_ref.alloc((size_t)m);
  D.h_uid.alloc((size_t)m);
  D2_HIP(hipMemcpyAsync(D.d_rec.p, D.h_rec.p, (size_t)m * sizeof(DdRead), hipMemcpyHostToDevice, st));
  D.st[DD_BYTES_UP] += (int64_t)m * (int64_t)sizeof(DdRead);
  add_lap(D.st[DD_US_UP], t_up);
  const DdState T = D.state();
  DdPiece P;
  P.m = m; P.rec = D.d_rec.p; P.seq = d_seq; P.qual = d_qual; P.r_hash = D.r_hash.p; P.r_slot = D.r_slot.p; P.r_uid = D.r_uid.p;
  P.r_ref = D.r_ref.p; P.auto_reads = D.qual_offset == 0 ? D.chunk_reads : 0;
  D2_HIP(hipEventRecord(D.ev[0], st));
  launch_dd_hash(T, P, st);
  const int64_t bound = D.nuniq + m + 1;                         // a read moves one slot per round, over occupied slots only
  for (int64_t round = 0;; round++) {
    if (round >= bound)
      throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator did not settle a piece within its uniques + 1 rounds."};
    D2_HIP(hipMemsetAsync(&D.ctr.p->pending, 0, sizeof(int32_t), st));
    launch_dd_round(T, P, st);
    D2_HIP(hipMemcpyAsync(D.h_ctr.p, D.ctr.p, sizeof(DdCounters), hipMemcpyDeviceToHost, st));
    sync_checked(st);
    if (D.h_ctr.p->err != 0)
      throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator's table walk reached its bound (code " + std::to_string(D.h_ctr.p->err) + ")."};
    if (D.h_ctr.p->pending == 0) break;
    D.st[DD_ROUNDS]++;
  }
  D2_HIP(hipEventRecord(D.ev[1], st));
  D2_HIP(hipMemcpyAsync(D.h_uid.p, D.r_uid.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  sync_checked(st);
  add_elapsed(D.st[DD_US_KERNEL], D.ev[0], D.ev[1]);
  D.nuniq = D.h_ctr.p->nuniq; D.used = (int64_t)D.h_ctr.p->arena_used;
  D.ruid.insert(D.ruid.end(), D.h_uid.p, D.h_uid.p + m);
  D.st[DD_BYTES_DOWN] += (int64_t)m * 4 + (int64_t)sizeof(DdCounters);
  D.st[DD_PIECES]++;
}

// one more read for the piece being collected in D.h_rec (room for it has been made): the call's next read
inline void dd_push(DerepDev &D, int &m, int64_t &bytes, long long start, int32_t len) {
  DdRead &R = D.h_rec.p[m++];
  R.start = start; R.len = len; R.pad = 0; R.idx = D.next_idx++;
  bytes += len;
}

// reads in memory: read r is seq / qual[offsets[r] + window[2 r] .. + window[2 r + 1]) (window null: the whole read), taken if
// keep[r] (null: every read)
void dd_feed(DerepDev &D, int64_t n, const char *seq, const char *qual, const int64_t *offsets, const int32_t *window, const uint8_t *keep) {
  if (n < 0 || (n > 0 && (!seq || !offsets || (!qual) != D.no_qual))) throw InputError{"dada2hip: bad arguments"};
  for (int64_t r = 0; r < n; r++) {
    const int64_t l = offsets[r + 1] - offsets[r];
    if (l < 0 || l > (int64_t)INT32_MAX - 128) throw InputError{"dada2hip: bad read offsets."};
    if (window && keep && keep[r] && (window[2 * r] < 0 || window[2 * r + 1] < 0 || (int64_t)window[2 * r] + window[2 * r + 1] > l))
      throw InputError{"dada2hip: a kept window lies outside its read."};
  }
  if (D.next_idx + n > (int64_t)INT32_MAX) throw InputError{"dada2hip: more than 2^31 - 1 reads to dereplicate."};
  std::lock_guard<std::mutex> lock(D.mu);
  select_device(D.device);
  using Slot = PieceSlot<int32_t, 2>;
  Slot slot[2];
  for (Slot &S : slot) S.create();
  int64_t pst[4] = {0}, at = 0;                                  // at: the first read of the piece being launched (pieces come in order)
  auto launch = [&](Slot &S, int c) {
    D.h_rec.alloc((size_t)c);
    int m = 0;
    int64_t bytes = 0;
    const int64_t r0 = at;
    at += c;
    for (int i = 0; i < c; i++) {
      const int64_t r = r0 + i;
      if (keep && !keep[r]) continue;
      const long long b = S.h_off.p[i];
      if (window) dd_push(D, m, bytes, b + window[2 * r], window[2 * r + 1]);
      else dd_push(D, m, bytes, b, (int32_t)(S.h_off.p[i + 1] - b));
    }
    dd_piece(D, m, bytes, S.d_seq.p, S.d_qual.p, S.st);
  };
  auto scatter = [&](Slot &) {};
  run_pieces(slot, n, seq, qual, offsets, knobs().derep_piece, knobs().derep_piece_bytes, 0, pst, 0, 1, 2, launch, scatter);
  D.st[DD_BYTES_UP] += pst[0]; D.st[DD_US_UP] += pst[1];
}

}  // namespace

// ---- what derep.cpp's file level takes from here, and what this file takes from derep.cpp (derep_dev_plain.h declares both) ----

int d2_dd_open(int32_t device, int64_t chunk_reads, int32_t qual_offset, void **dd, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (!dd) throw InputError{"dada2hip: bad arguments"};
    *dd = nullptr;
    std::unique_ptr<DerepDev> D(new DerepDev());
    dd_open(*D, device, chunk_reads, qual_offset);
    *dd = D.release();
  });
}

void d2_dd_free(void *dd) { delete (DerepDev *)dd; }
int32_t d2_filter_device(const dada2hip_filter *ctx) { return ctx ? ctx->device : 0; }

int d2_dd_feed(void *dd, int64_t n, const char *seq, const char *qual, const int64_t *offsets, const int32_t *window, const uint8_t *keep,
               char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (!dd) throw InputError{"dada2hip: bad arguments"};
    dd_feed(*(DerepDev *)dd, n, seq, qual, offsets, window, keep);
  });
}

// dada2hip_filter_reads with code and window asked for, and every kept window of a piece into the dereplicator while the piece
// still lies in its slot
int d2_dd_filter_chunk(dada2hip_filter *ctx, void *dd, int64_t n, const char *seq, const char *qual, const int64_t *offsets,
                       const dada2hip_filter_params *params, int32_t *code, int32_t *window, int64_t *stats, char *errbuf, size_t errlen) {
  return guarded(errbuf, errlen, [&] {
    if (!dd || !ctx || !code || !window) throw InputError{"dada2hip: bad arguments"};
    DerepDev &D = *(DerepDev *)dd;
    if (D.device != ctx->device) throw InputError{"dada2hip: the dereplicator and the filter context are on different devices."};
    if (D.next_idx + n > (int64_t)INT32_MAX) throw InputError{"dada2hip: more than 2^31 - 1 reads to dereplicate."};
    std::lock_guard<std::mutex> lock(D.mu);
    int64_t expect = 0;                                          // the read the next piece in file order starts with
    FtSlot *early = nullptr;
    auto take = [&](FtSlot &S) {
      const int64_t f = S.first, c = S.count;
      D.h_rec.alloc((size_t)c);
      int m = 0;
      int64_t bytes = 0;
      for (int64_t i = 0; i < c; i++)
        if (code[f + i] == 0) dd_push(D, m, bytes, S.h_off.p[i] + window[2 * (f + i)], window[2 * (f + i) + 1]);
      dd_piece(D, m, bytes, S.d_seq.p, S.d_qual.p, S.st);
      expect = f + c;
    };
    // The pieces are harvested in file order, but for the call's last two when their number is odd: run_pieces drains slot 0
    // and then slot 1.  The later piece waits in its slot, which nothing reuses any more, until the earlier one is in.
    FilterPieceHook hook = [&](FtSlot &S) {
      if (S.first != expect) { early = &S; return; }
      take(S);
      if (early && early->first == expect) { FtSlot &E = *early; early = nullptr; take(E); }
    };
    filter_reads_body(ctx, n, seq, qual, offsets, params, code, window, nullptr, nullptr, nullptr, nullptr, stats, nullptr, 0, nullptr, &hook);
    if (early || expect != n) throw RuntimeErr{DADA2HIP_ERR_INTERNAL, "dada2hip: the dereplicator did not see every piece of the filter's call."};
  });
}

// the rows back, and the object: *out null with DADA2HIP_OK when no read at all went in (a filter that kept nothing)
int d2_dd_finish(void *dd, int32_t allow_none, dada2hip_derep **out, int64_t *stats, char *errbuf, size_t errlen) {
  const auto t_call = clk::now();
  std::vector<int64_t> off, cnt, fst;
  std::vector<int32_t> len;
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> sums;
  DerepDev *D = (DerepDev *)dd;
  int rc = guarded(errbuf, errlen, [&] {
    if (!D || !out) throw InputError{"dada2hip: bad arguments"};
    *out = nullptr;
    if (allow_none && D->next_idx == 0) return;
    if (D->nuniq == 0) throw InputError{"Only zero-length sequences detected during dereplication."};
    std::lock_guard<std::mutex> lock(D->mu);
    select_device(D->device);
    const size_t U = (size_t)D->nuniq, A = (size_t)D->used;
    off.resize(U); cnt.resize(U); fst.resize(U); len.resize(U); bytes.resize(A); sums.resize(A);
    D2_HIP(hipMemcpy(off.data(), D->u_off.p, U * 8, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(cnt.data(), D->u_count.p, U * 8, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(fst.data(), D->u_first.p, U * 8, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(len.data(), D->u_len.p, U * 4, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(bytes.data(), D->arena.p, A, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(sums.data(), D->sums.p, A * 8, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(D->h_ctr.p, D->ctr.p, sizeof(DdCounters), hipMemcpyDeviceToHost));
    D->st[DD_BYTES_DOWN] += (int64_t)(U * 28 + A * 9);
    add_lap(D->st[DD_US_DOWN], t_call);
  });
  if (rc != DADA2HIP_OK || !D || (allow_none && D->next_idx == 0)) {
    if (rc == DADA2HIP_OK && D && stats) memcpy(stats, D->st, sizeof D->st);
    return rc;
  }
  const auto t_final = clk::now();
  rc = d2_derep_from_rows((int64_t)off.size(), off.data(), len.data(), cnt.data(), fst.data(), bytes.data(), sums.data(), (int64_t)D->ruid.size(),
                          D->ruid.data(), D->chunk_reads, D->qual_offset, D->h_ctr.p->minq, out, errbuf, errlen);
  add_lap(D->st[DD_US_FINAL], t_final);
  D->st[DD_IN] = D->next_idx; D->st[DD_UNIQUES] = D->nuniq; D->st[DD_CAPACITY] = (int64_t)D->cap;
  if (stats) memcpy(stats, D->st, sizeof D->st);
  return rc;
}

// ---- the resident form: the uniques become a resident sample where they lie ---------------------------------------------------------
// What d2_dd_finish brings down at 9 bytes per base only so that d2_derep_from_rows can divide it into doubles and
// dada2hip_sample_from_derep can round them into bytes and send them up again, stays on the device here: the small rows come
// down (28 bytes per unique and the arena's letters, for the order, the strings and the map), the order goes up at 4 bytes per
// unique, and k_dd_to_sample (derep_resident.inc.hip) writes the sample's rows - packed letters, rounded qualities, length,
// count - from the arena and the sums, in that order, on the sample's stream; the k-mer records are built behind it and the
// packed rows come down once into the sample's pinned mirror (result strings are decoded from it).  The derep object has no
// quality matrix (derep.cpp).  The sample's input errors are raised behind the kernel, in sample_create's order and with its
// texts; the k-mer build is launched only if every length fits, as there.  On such an error the call returns NEITHER object -
// the host route would have made the derep object and failed at dada2hip_sample_from_derep.
namespace {

void dd_to_sample(DerepDev &D, dada2hip_sample *s, const std::vector<int32_t> &len, const std::vector<int64_t> &cnt, const std::vector<int32_t> &order,
                  int64_t *rs, int32_t *ceil_max) {
  const auto t0 = clk::now();
  std::lock_guard<std::mutex> lock(D.mu);
  const size_t U = order.size();
  int maxlen = 0, minlen = INT32_MAX;
  uint64_t total = 0;
  for (size_t u = 0; u < U; u++) {
    maxlen = std::max(maxlen, len[u]); minlen = std::min(minlen, len[u]);
    total += (uint32_t)cnt[u];
  }
  sample_shell(s, (int32_t)U, maxlen, D.device);
  SampleDev &S = s->D;
  DevBuf<int32_t> d_order;
  DevBuf<DrRecord> d_rec;
  PinBuf<DrRecord> h_rec;
  d_order.alloc(U); d_rec.alloc(1); h_rec.alloc(1);
  const auto t_up = clk::now();
  const DrRecord r0 = {0, 0, 0, INT32_MIN};
  D2_HIP(hipMemcpy(d_order.p, order.data(), U * sizeof(int32_t), hipMemcpyHostToDevice));
  D2_HIP(hipMemcpy(d_rec.p, &r0, sizeof r0, hipMemcpyHostToDevice));
  rs[DR_BYTES_UP] += (int64_t)(U * sizeof(int32_t) + sizeof r0);
  add_lap(rs[DR_US_ORDER], t_up);
  Events<4> ev;
  ev.create();
  D2_HIP(hipMemsetAsync(S.prior, 0, U, s->stream));
  D2_HIP(hipEventRecord(ev[0], s->stream));
  const int blocks = knobs().dd_sample_blocks > 0 ? knobs().dd_sample_blocks : 4096;
  rs[DR_BLOCKS] = launch_dd_to_sample(D.state(), d_order.p, (int)U, dd_offset(D.qual_offset, D.h_ctr.p->minq), S, d_rec.p, blocks, s->stream);
  D2_HIP(hipEventRecord(ev[1], s->stream));
  // (the k-mer kernel trusts a row's length: only for rows that fit, as in sample_create; the call is going to fail otherwise)
  const bool fits = maxlen < SEQLEN && minlen > KMER_SIZE;
  if (fits) launch_build_kmers_rows(S, 0, (int)U, s->stream);
  D2_HIP(hipEventRecord(ev[2], s->stream));
  D2_HIP(hipMemcpyAsync(s->h_seq2.p, S.seq2, U * (size_t)S.W2 * 4, hipMemcpyDeviceToHost, s->stream));
  D2_HIP(hipMemcpyAsync(h_rec.p, d_rec.p, sizeof(DrRecord), hipMemcpyDeviceToHost, s->stream));
  D2_HIP(hipEventRecord(ev[3], s->stream));
  sync_checked(s->stream);
  rs[DR_BYTES_DOWN] += (int64_t)(U * (size_t)S.W2 * 4 + sizeof(DrRecord));
  add_elapsed(rs[DR_US_KERNEL], ev[0], ev[1]);
  add_elapsed(rs[DR_US_KMERS], ev[1], ev[2]);
  add_elapsed(rs[DR_US_MIRROR], ev[2], ev[3]);
  const DrRecord R = *h_rec.p;
  if (maxlen >= SEQLEN) throw InputError{"Input sequences exceed the maximum allowed string length."};
  if (minlen <= KMER_SIZE) throw InputError{"Input sequences must all be longer than the kmer-size (5)."};
  if (R.bad_base) throw InputError{"Invalid derep$uniques vector. Sequences must be made up only of A/C/G/T."};
  if (R.bad_qual) throw InputError{"Invalid derep$quals matrix. Quality values must be positive integers."};
  for (size_t r = 0; r < U; r++) {
    s->h_len[r] = len[(size_t)order[r]];
    s->h_reads[r] = (uint32_t)cnt[(size_t)order[r]];
  }
  S.minlen = minlen;
  s->total_reads = total;
  s->qmax = R.qmax;
  s->ms_upload = ms_since(t0);
  *ceil_max = R.ceil_max;
}

}  // namespace

int d2_dd_finish_resident(void *dd, int32_t allow_none, dada2hip_derep **out, dada2hip_sample **sample, int64_t *stats, int64_t *resident_stats,
                          char *errbuf, size_t errlen) {
  const auto t_call = clk::now();
  std::vector<int64_t> off, cnt, fst;
  std::vector<int32_t> len, order;
  std::vector<uint8_t> bytes;
  int64_t rs[DADA2HIP_RESIDENT_NSTATS] = {0};
  DerepDev *D = (DerepDev *)dd;
  int rc = guarded(errbuf, errlen, [&] {
    if (!D || !out || !sample || D->no_qual) throw InputError{"dada2hip: bad arguments"};
    *out = nullptr; *sample = nullptr;
    if (allow_none && D->next_idx == 0) return;
    if (D->nuniq == 0) throw InputError{"Only zero-length sequences detected during dereplication."};
    std::lock_guard<std::mutex> lock(D->mu);
    select_device(D->device);
    const size_t U = (size_t)D->nuniq, A = (size_t)D->used;
    off.resize(U); cnt.resize(U); fst.resize(U); len.resize(U); bytes.resize(A);
    D2_HIP(hipMemcpy(off.data(), D->u_off.p, U * 8, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(cnt.data(), D->u_count.p, U * 8, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(fst.data(), D->u_first.p, U * 8, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(len.data(), D->u_len.p, U * 4, hipMemcpyDeviceToHost));
    D2_HIP(hipMemcpy(bytes.data(), D->arena.p, A, hipMemcpyDeviceToHost));          // (the letters; the sums stay where they are)
    D2_HIP(hipMemcpy(D->h_ctr.p, D->ctr.p, sizeof(DdCounters), hipMemcpyDeviceToHost));
    rs[DR_BYTES_DOWN] += (int64_t)(U * 28 + A + sizeof(DdCounters));
    add_lap(rs[DR_US_ROWS], t_call);
  });
  if (rc != DADA2HIP_OK || !D || (allow_none && D->next_idx == 0)) {
    if (rc == DADA2HIP_OK && D && stats) memcpy(stats, D->st, sizeof D->st);
    return rc;
  }
  const auto t_final = clk::now();
  order.resize(off.size());
  dada2hip_derep *d = nullptr;
  rc = d2_derep_from_rows_resident((int64_t)off.size(), off.data(), len.data(), cnt.data(), fst.data(), bytes.data(), (int64_t)D->ruid.size(),
                                   D->ruid.data(), D->chunk_reads, order.data(), &d, errbuf, errlen);
  add_lap(rs[DR_US_ORDER], t_final);
  if (rc != DADA2HIP_OK) return rc;
  dada2hip_sample *s = new dada2hip_sample();
  int32_t ceil_max = 0;
  rc = guarded(errbuf, errlen, [&] { dd_to_sample(*D, s, len, cnt, order, rs, &ceil_max); });
  if (rc != DADA2HIP_OK) { dada2hip_sample_free(s); dada2hip_derep_free(d); return rc; }
  d2_derep_set_qmax(d, ceil_max);
  *out = d; *sample = s;
  add_lap(D->st[DD_US_FINAL], t_final);
  rs[DR_UNIQUES] = D->nuniq;
  D->st[DD_BYTES_UP] += rs[DR_BYTES_UP]; D->st[DD_BYTES_DOWN] += rs[DR_BYTES_DOWN]; D->st[DD_US_DOWN] += rs[DR_US_ROWS];
  D->st[DD_IN] = D->next_idx; D->st[DD_UNIQUES] = D->nuniq; D->st[DD_CAPACITY] = (int64_t)D->cap;
  if (stats) memcpy(stats, D->st, sizeof D->st);
  if (resident_stats) memcpy(resident_stats, rs, sizeof rs);
  return rc;
}

int dada2hip_derep_reads_resident(int64_t n, const char *seq, const char *qual, const int64_t *offsets, int64_t chunk_reads, int32_t qual_offset,
                                  int32_t device, dada2hip_derep **out, dada2hip_sample **sample, int64_t *stats, int64_t *resident_stats,
                                  char *errbuf, size_t errlen) {
  const auto t_call = clk::now();
  if (out) *out = nullptr;
  if (sample) *sample = nullptr;
  if (resident_stats) memset(resident_stats, 0, sizeof(int64_t) * DADA2HIP_RESIDENT_NSTATS);
  void *dd = nullptr;
  int rc = d2_dd_open(device, chunk_reads, qual_offset, &dd, errbuf, errlen);
  std::unique_ptr<DerepDev> hold((DerepDev *)dd);                // (the table, the arena and the sums are freed when the call returns)
  if (rc == DADA2HIP_OK) rc = d2_dd_feed(dd, n, seq, qual, offsets, nullptr, nullptr, errbuf, errlen);
  int64_t st[DADA2HIP_DEREP_NSTATS] = {0};
  if (rc == DADA2HIP_OK) rc = d2_dd_finish_resident(dd, 0, out, sample, st, resident_stats, errbuf, errlen);
  if (rc == DADA2HIP_OK && stats) {
    st[DD_US_TOTAL] = (int64_t)(ms_since(t_call) * 1e3);
    memcpy(stats, st, sizeof st);
  }
  return rc;
}

int dada2hip_derep_reads(int64_t n, const char *seq, const char *qual, const int64_t *offsets, int64_t chunk_reads, int32_t qual_offset,
                         int32_t device, dada2hip_derep **out, int64_t *stats, char *errbuf, size_t errlen) {
  const auto t_call = clk::now();
  if (out) *out = nullptr;
  void *dd = nullptr;
  int rc = d2_dd_open(device, chunk_reads, qual_offset, &dd, errbuf, errlen);
  std::unique_ptr<DerepDev> hold((DerepDev *)dd);
  if (rc == DADA2HIP_OK) rc = d2_dd_feed(dd, n, seq, qual, offsets, nullptr, nullptr, errbuf, errlen);
  int64_t st[DADA2HIP_DEREP_NSTATS] = {0};
  if (rc == DADA2HIP_OK) rc = d2_dd_finish(dd, 0, out, st, errbuf, errlen);
  if (rc == DADA2HIP_OK && stats) {
    st[DD_US_TOTAL] = (int64_t)(ms_since(t_call) * 1e3);
    memcpy(stats, st, sizeof st);
  }
  return rc;
}
