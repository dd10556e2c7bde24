// read_pieces.h — the two-slot pipeline that takes a call's reads to the device, for filterAndTrim and removePrimers; included by
// driver.cpp behind stage_common.h.  A call is cut into pieces (next_piece, stage_plain.h) that alternate between two slots, each
// with pinned staging, device buffers and a stream of its own: while the kernels of one piece run, the host copies the next piece
// into the other slot's pinned buffers and queues its upload, so the copy of piece k + 1 runs under the kernels of piece k.
//
// Draining.  A slot is `busy` from the moment its piece is queued until a synchronise of its stream has RETURNED: harvest clears
// the flag right behind hipStreamSynchronize and asks hipGetLastError afterwards, so an error a kernel left behind throws from a
// slot that is idle with nothing in flight, and a synchronise that itself fails leaves the slot busy for the drain.  Whoever lets
// go of a busy slot drains it: run_pieces on the way out of a call that threw (a filter context's slots outlive the call and stay
// usable), and the slot's destructor, before any of its buffers goes back to the allocation cache.
#pragma once

namespace {

constexpr int64_t PIECE_READS = 1 << 16, PIECE_BYTES = 32 << 20;   // a piece: at most these, or what the stage's knob says if less
inline int64_t piece_limit(long long knob, int64_t most) { return knob > 0 ? std::min<int64_t>(knob, most) : most; }

// Out: the stage's record per read; aux: int32 words per read that only some calls ask for
template <typename Out, int NEV> struct PieceSlot {
  PinBuf<uint8_t> h_seq, h_qual;
  DevBuf<uint8_t> d_seq, d_qual;
  PinBuf<long long> h_off; DevBuf<long long> d_off;
  PinBuf<Out> h_out;       DevBuf<Out> d_out;
  PinBuf<int32_t> h_aux;   DevBuf<int32_t> d_aux;
  hipStream_t st = nullptr;
  Events<NEV> ev;                      // [0] in front of the stage's kernels, [NEV - 1] behind them; those between are the stage's
  int64_t first = 0, count = 0;        // the reads in flight
  bool busy = false;
  void create() { D2_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); ev.create(); }
  void drain() { if (busy) { (void)hipStreamSynchronize(st); busy = false; } }
  ~PieceSlot() { drain(); if (st) (void)hipStreamDestroy(st); }
};

// Reads [0, n) of seq (and qual, unless null) through slot[0] and slot[1], with `aux` words per read (0: none).  The stage's
// hooks: launch(S, c) queues the kernels of c reads on S.st; scatter(S), with S.st synchronised, takes the events' times and the
// results of reads S.first .. S.first + S.count to the caller's arrays.  knob_reads, knob_bytes: the stage's piece knobs.
// st[w_bytes], [w_up], [w_down]: bytes copied up, host microseconds of the upload and of the harvest.
template <typename Out, int NEV, typename Launch, typename Scatter>
void run_pieces(PieceSlot<Out, NEV> (&slot)[2], int64_t n, const char *seq, const char *qual, const int64_t *offsets, long long knob_reads,
                long long knob_bytes, size_t aux, int64_t *st, int w_bytes, int w_up, int w_down, Launch &&launch, Scatter &&scatter) {
  const int64_t piece_reads = piece_limit(knob_reads, PIECE_READS), piece_bytes = piece_limit(knob_bytes, PIECE_BYTES);
  auto harvest = [&](PieceSlot<Out, NEV> &S) {
    if (!S.busy) return;
    auto t0 = clk::now();
    D2_HIP(hipStreamSynchronize(S.st));
    S.busy = false;
    D2_HIP(hipGetLastError());
    scatter(S);
    add_lap(st[w_down], t0);
  };
  struct Drain { PieceSlot<Out, NEV> *s; ~Drain() { s[0].drain(); s[1].drain(); } } drain{slot};
  int64_t r0 = 0;
  for (int piece = 0; r0 < n; piece++) {
    const int64_t r1 = next_piece(offsets, n, r0, piece_reads, piece_bytes);
    PieceSlot<Out, NEV> &S = slot[piece & 1];
    harvest(S);
    auto t_up = clk::now();
    const int64_t c = r1 - r0, base = offsets[r0], bytes = offsets[r1] - base;
    S.h_seq.alloc((size_t)bytes); S.h_off.alloc((size_t)c + 1); S.d_seq.alloc((size_t)bytes); S.d_off.alloc((size_t)c + 1);
    if (qual) { S.h_qual.alloc((size_t)bytes); S.d_qual.alloc((size_t)bytes); }
    S.h_out.alloc((size_t)c); S.d_out.alloc((size_t)c);
    if (aux) { S.h_aux.alloc((size_t)c * aux); S.d_aux.alloc((size_t)c * aux); }
    parallel_for((size_t)bytes, (size_t)1 << 20, [&](size_t lo, size_t hi) {
      memcpy(S.h_seq.p + lo, seq + base + lo, hi - lo);
      if (qual) memcpy(S.h_qual.p + lo, qual + base + lo, hi - lo);
    });
    for (int64_t i = 0; i <= c; i++) S.h_off.p[i] = (long long)(offsets[r0 + i] - base);
    if (bytes > 0) {
      D2_HIP(hipMemcpyAsync(S.d_seq.p, S.h_seq.p, (size_t)bytes, hipMemcpyHostToDevice, S.st));
      if (qual) D2_HIP(hipMemcpyAsync(S.d_qual.p, S.h_qual.p, (size_t)bytes, hipMemcpyHostToDevice, S.st));
    }
    D2_HIP(hipMemcpyAsync(S.d_off.p, S.h_off.p, (size_t)(c + 1) * 8, hipMemcpyHostToDevice, S.st));
    D2_HIP(hipEventRecord(S.ev[0], S.st));
    launch(S, (int)c);
    D2_HIP(hipEventRecord(S.ev[NEV - 1], S.st));
    D2_HIP(hipMemcpyAsync(S.h_out.p, S.d_out.p, (size_t)c * sizeof(Out), hipMemcpyDeviceToHost, S.st));
    if (aux) D2_HIP(hipMemcpyAsync(S.h_aux.p, S.d_aux.p, (size_t)c * aux * 4, hipMemcpyDeviceToHost, S.st));
    S.first = r0; S.count = c; S.busy = true;
    st[w_bytes] += (qual ? 2 : 1) * bytes + (c + 1) * 8;
    add_lap(st[w_up], t_up);
    r0 = r1;
  }
  harvest(slot[0]); harvest(slot[1]);
}

}  // namespace
