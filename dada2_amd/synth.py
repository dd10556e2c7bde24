"""Seeded synthetic amplicon samples for the parity tests and bench.py.

The reference ships no benchmark inputs; BASELINE.json's configs are defined on synthetic
uniques.  The generator follows the survey's recipe: families of true variants derived
from one ancestor, Zipf abundances, a linear quality ramp with Gaussian jitter, and
substitution errors drawn from the error matrix itself (so the data are self-consistent
with the model), then dereplication exactly as ``derepFastq`` would do it
(dada2_amd/io.py).  Everything is numpy-vectorised, and each chunk's element-wise work runs on a few
threads while the next chunk is drawn: 10^6 uniques take 10-15 s.  The random stream is consumed in a
fixed order, so a seed gives the same sample bit for bit however the work is scheduled.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .io import Derep

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def true_variants(rng, G: int, L: int, Lmin: int = None, Lmin5: int = None):
    """G/8 roots at divergence U(0.03,0.25) from one ancestor; each root + 7 variants at
    Hamming 1..7 from it.  Returns uint8 codes 0..3, shape [G, L] and lengths [G].
    ``Lmin``: 3'-ragged variants (lengths U{Lmin..L}, the tail cut off).  ``Lmin5``: 5'-ragged variants (a variant is
    the SUFFIX of its full-length sequence, start offset U{0..L-Lmin5}) — primer-trim variation, ordinary for long
    amplicons: the alignment of such a read to a full-length centre runs |i - j| = offset cells off the main diagonal."""
    nroot = max(1, G // 8)
    anc = rng.integers(0, 4, size=L, dtype=np.uint8)
    out = np.empty((nroot * 8, L), dtype=np.uint8)
    for r in range(nroot):
        root = anc.copy()
        div = rng.uniform(0.03, 0.25)
        pos = rng.choice(L, size=max(1, int(round(div * L))), replace=False)
        root[pos] = (root[pos] + rng.integers(1, 4, size=pos.size, dtype=np.uint8)) & 3
        out[r * 8] = root
        for h in range(1, 8):
            v = root.copy()
            p = rng.choice(L, size=h, replace=False)
            v[p] = (v[p] + rng.integers(1, 4, size=h, dtype=np.uint8)) & 3
            out[r * 8 + h] = v
    lens = np.full(nroot * 8, L, dtype=np.int32)
    if Lmin is not None and Lmin < L:
        lens = rng.integers(Lmin, L + 1, size=nroot * 8).astype(np.int32)
    if Lmin5 is not None and Lmin5 < L:
        off = rng.integers(0, L - Lmin5 + 1, size=nroot * 8)
        off[::8] = 0                                  # the roots stay full length at the 5' end
        for g in range(nroot * 8):
            o = int(min(off[g], max(0, lens[g] - max(8, Lmin5 // 4))))
            if o > 0:
                out[g, : L - o] = out[g, o:].copy()
                lens[g] -= o
    return out[:G], lens[:G]


def _derep_codes(codes: np.ndarray, lens: np.ndarray, quals: np.ndarray) -> Derep:
    """Dereplicate reads given as code rows (0..3, padded with 255 past each read's end)."""
    n, L = codes.shape
    key = np.ascontiguousarray(codes).view(np.dtype((np.void, L))).ravel()
    uniq, first, inv, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    # np.unique sorts the void rows bytewise; with codes 0..3 == A<C<G<T and 255 padding a shorter
    # read sorts AFTER its extensions, whereas C-locale strings sort a prefix first.  Re-rank by
    # the actual strings only when lengths vary.
    U = uniq.size
    ulen = lens[first]
    # per-unique quality sums: singletons are their own row; the rest via sort + reduceat
    mean = quals[first].astype(np.float64)
    multi = counts > 1
    if multi.any():
        sel = np.nonzero(multi[inv])[0]
        o = sel[np.argsort(inv[sel], kind="stable")]
        starts = np.concatenate([[0], np.cumsum(counts[multi])[:-1]])
        qs = np.add.reduceat(quals[o].astype(np.int32), starts, axis=0)
        mean[multi] = qs.astype(np.float64) / counts[multi][:, None]
    ucodes = codes[first]
    lut = np.full(256, ord("-"), dtype=np.uint8)
    lut[:4] = _ACGT
    asc = lut[ucodes]
    seqs = [asc[u, : ulen[u]].tobytes().decode("ascii") for u in range(U)]
    if (ulen != L).any():
        lex = np.array(sorted(range(U), key=lambda u: seqs[u]), dtype=np.int64)
    else:
        lex = np.arange(U)
    order = lex[np.argsort(-counts[lex], kind="stable")]   # (-abundance, sequence): stable R order()
    mean = mean[order]
    short = ulen[order] < L
    if short.any():
        rows = np.flatnonzero(short)
        mean[rows] = np.where(np.arange(L)[None, :] >= ulen[order][rows][:, None], np.nan, mean[rows])
    rank = np.empty(U, dtype=np.int64)
    rank[order] = np.arange(U)
    return Derep([seqs[u] for u in order], counts[order].astype(np.int32), mean, rank[inv].astype(np.int32))


def make_sample(err: np.ndarray, n_uniques: int, L: int = 250, G: int = 256, seed: int = 0, Lmin: int = None,
                q_hi: float = 38.0, q_lo: float = 22.0, q_sd: float = 4.0, q_max: int = 40, indel_rate: float = 0.0,
                zipf: float = 1.1, variants=None, chunk: int = 200_000, Lmin5: int = None, ins_rate: float = 0.0) -> Derep:
    """Draw reads until the dereplicated unique count reaches ``n_uniques`` (then trim the
    rarest uniques so N is exact), and dereplicate.  ``err`` is the 16 x Q matrix errors are
    drawn from.  ``variants`` (codes, lens) may be passed to share truth across samples."""
    rng = np.random.default_rng(seed)
    tv, tl = variants if variants is not None else true_variants(rng, G, L, Lmin, Lmin5)
    G = tv.shape[0]
    w = (np.arange(1, G + 1, dtype=np.float64)) ** (-zipf)
    w /= w.sum()
    err = np.asarray(err, dtype=np.float64)
    Q = err.shape[1]
    ramp = np.linspace(q_hi, q_lo, L)
    qcap = min(q_max, Q - 1)
    # substitution errors: P(b -> b') = err[4b+b', q].  A base b read at quality q becomes (b + k) & 3 for the first k in 1..3
    # whose running sum err[4b + (b+1)&3, q] + ... + err[4b + (b+k)&3, q] exceeds its uniform draw; the sums are tabulated
    # once per (b, q), added in that same order
    cut = np.zeros((3, 4 * Q))
    for b in range(4):
        c = np.zeros(Q)
        for k in range(1, 4):
            c = c + err[4 * b + ((b + k) & 3)]
            cut[k - 1, b * Q:(b + 1) * Q] = c
    nthreads = max(1, min(8, os.cpu_count() or 1))

    def draw():
        """One chunk's random draws, in stream order: truth, quality noise, substitution draws, then the per-read indel draws
        (their positions depend on the read lengths only, so they are drawn here and applied by build())."""
        g = rng.choice(G, size=chunk, p=w)
        lens = tl[g].copy()
        noise = rng.normal(0.0, q_sd, size=(chunk, L))
        u = rng.random(size=(chunk, L))
        dels, ins = [], []
        if indel_rate > 0:
            # rare single-base deletions (exercise the band); applied per read, at most one
            has = rng.random(chunk) < indel_rate * lens
            for r in np.nonzero(has)[0]:
                dels.append((r, int(rng.integers(1, lens[r] - 1))))
                lens[r] -= 1
        if ins_rate > 0:
            # rare single-base insertions (a read at full length keeps its length: its last base falls off)
            has = rng.random(chunk) < ins_rate * lens
            for r in np.nonzero(has)[0]:
                ins.append((r, int(rng.integers(1, lens[r] - 1)), rng.integers(0, 4)))
                lens[r] = min(L, lens[r] + 1)
        return g, lens, noise, u, dels, ins

    def build(g, lens, noise, u, dels, ins):
        """The reads of one drawn chunk, and the distinct reads among them."""
        codes = tv[g].copy()
        q = np.empty((chunk, L), dtype=np.uint8)

        def rows(r0, r1):   # element-wise on a block of reads (numpy releases the GIL: the blocks run side by side)
            qb = np.clip(np.rint(ramp[None, :] + noise[r0:r1]), 2, qcap).astype(np.uint8)
            q[r0:r1] = qb
            cb = codes[r0:r1]
            idx = cb.astype(np.intp) * Q + qb
            ub = u[r0:r1]
            out = np.where(ub < cut[2].take(idx), (cb + 3) & 3, cb)
            out = np.where(ub < cut[1].take(idx), (cb + 2) & 3, out)
            codes[r0:r1] = np.where(ub < cut[0].take(idx), (cb + 1) & 3, out)

        edges = np.linspace(0, chunk, min(nthreads, chunk) + 1).astype(int)
        with ThreadPoolExecutor(len(edges) - 1) as ex:
            list(ex.map(rows, edges[:-1], edges[1:]))
        for r, p in dels:
            codes[r, p:-1] = codes[r, p + 1:]
            q[r, p:-1] = q[r, p + 1:]
        for r, p, base in ins:
            codes[r, p + 1:] = codes[r, p:-1].copy()
            q[r, p + 1:] = q[r, p:-1].copy()
            codes[r, p] = base
        pad = np.arange(L)[None, :] >= lens[:, None]
        codes[pad] = 255
        q[pad] = 0
        keys = np.ascontiguousarray(codes).view(np.dtype((np.void, L))).ravel()
        return codes, lens, q, np.unique(keys).tolist()

    all_codes, all_lens, all_q = [], [], []
    seen_keys = set()
    with ThreadPoolExecutor(1) as builder:
        pending = builder.submit(build, *draw())
        while True:
            ahead = draw()   # the next chunk of the stream, drawn while the last one is built (unused if that one was enough)
            codes, lens, q, keys = pending.result()
            all_codes.append(codes); all_lens.append(lens); all_q.append(q)
            seen_keys.update(keys)
            if len(seen_keys) >= n_uniques:
                break
            pending = builder.submit(build, *ahead)
        del ahead
    codes = np.concatenate(all_codes); lens = np.concatenate(all_lens); q = np.concatenate(all_q)
    d = _derep_codes(codes, lens, q)
    if d.nraw > n_uniques:  # drop the rarest (last) uniques and the reads that map to them
        keep = n_uniques
        d = Derep(d.seqs[:keep], d.abundances[:keep], d.quals[:keep], np.where(d.map < keep, d.map, -1).astype(np.int32))
    maxlen = max(len(s) for s in d.seqs)   # quals has exactly maxlen columns (Rmain.cpp:69-72)
    if d.quals.shape[1] != maxlen:
        d = Derep(d.seqs, d.abundances, np.ascontiguousarray(d.quals[:, :maxlen]), d.map)
    return d


def make_shared_truth_samples(err: np.ndarray, n_uniques: int = 250_000, nsamples: int = 8, L: int = 250, G: int = 512,
                              seed: int = 20260929, **kw) -> list:
    """``nsamples`` samples that share half of their true variants (BASELINE.json configs[3]: 8 x 250 000 uniques x 250 nt, G = 512;
    the defaults, seed included, draw the samples bench.py's config 4 draws).  The other half of a sample's variants are its own,
    and the abundance ranks of the variants differ per sample."""
    shared = true_variants(np.random.default_rng(seed), G // 2, L)
    out = []
    for i in range(nsamples):
        own = true_variants(np.random.default_rng(seed + 17 * (i + 1)), G - G // 2, L)
        tv, tl = np.concatenate([shared[0], own[0]]), np.concatenate([shared[1], own[1]])
        perm = np.random.default_rng(99 + i).permutation(tv.shape[0])
        out.append(make_sample(err, n_uniques, L=L, G=G, seed=seed + 1000 * (i + 1), variants=(tv[perm], tl[perm]), **kw))
    return out
