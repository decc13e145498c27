#!/usr/bin/env python3
"""Runs the resumable beam search (beam_kernel<..., RESUME = true>) on the CPU SIMT emulation (tools/emu/beam_stream_emu.cpp):
one utterance cut into chunks, the carried search advanced one launch per chunk, and after every chunk its hypotheses held to
the whole-utterance kernel over the same prefix (emulated in the same process: tokens, timesteps, lengths and the double
totals bit for bit) and to oracle/beam.py over that prefix (tokens, timesteps, lengths).

    python tools/emu/run_beam_stream_emu.py [--threads 1024|192]
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import beam as ob  # noqa: E402

EXE = os.path.join(ROOT, "tools", "emu", "beam_stream_emu")


def build():
    src = os.path.join(ROOT, "tools", "emu", "beam_stream_emu.cpp")
    deps = [src, os.path.join(ROOT, "tools", "emu", "simt.h"), os.path.join(ROOT, "danspeech_amd", "csrc", "beam_kernel.inc")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-DSIMT_EMU", "-O1", "-g", "-std=c++20", "-pthread", "-I", os.path.join(ROOT, "danspeech_amd", "csrc"),
                               "-I", os.path.join(ROOT, "tools", "emu"), src, "-o", EXE])


def run(probs, chunks, labels, beam, lm_path=None, alpha=0.0, beta=0.0, top_n=40, cutoff_prob=1.0, threads=1024, timeout=900):
    """probs [T, C] -> per chunk ((tok, step, len, n, score) of the carried search, the same of the whole kernel over the prefix)"""
    T, C = probs.shape
    assert sum(chunks) == T
    with tempfile.TemporaryDirectory() as d:
        pin, pout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(pin, "wb") as f:
            f.write(struct.pack("<8i", 1, T, C, beam, 0, top_n, 1 if lm_path else 0, len(labels)))
            f.write(struct.pack("<3d", cutoff_prob, alpha, beta))
            f.write(np.ascontiguousarray(probs, dtype=np.float32).tobytes())
            for c in labels:
                e = c.encode("utf-8")
                f.write(struct.pack("<i", len(e)) + e)
            e = (lm_path or "").encode()
            f.write(struct.pack("<i", len(e)) + e)
            f.write(struct.pack("<i", len(chunks)) + np.asarray(chunks, dtype=np.int32).tobytes())
        subprocess.run([EXE, pin, pout, str(threads)], check=True, timeout=timeout)
        raw = open(pout, "rb").read()
    Tw = max(T, 1)
    n = beam * Tw
    blk = 8 * n + 4 * beam + 4 + 8 * beam
    assert len(raw) == 2 * blk * len(chunks)

    def block(off):
        tok = np.frombuffer(raw, dtype=np.int32, count=n, offset=off).reshape(beam, Tw)
        step = np.frombuffer(raw, dtype=np.int32, count=n, offset=off + 4 * n).reshape(beam, Tw)
        ln = np.frombuffer(raw, dtype=np.int32, count=beam, offset=off + 8 * n)
        nb = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=off + 8 * n + 4 * beam)[0])
        sc = np.frombuffer(raw, dtype=np.float64, count=beam, offset=off + 8 * n + 4 * beam + 4)
        return tok, step, ln, nb, sc

    return [(block(2 * k * blk), block((2 * k + 1) * blk)) for k in range(len(chunks))]


def compare(probs, chunks, labels, beam, threads, **kw):
    """True when, after every chunk, the carried search equals the whole kernel over the prefix (bit for bit) and the oracle
    (tokens, timesteps, lengths)."""
    res = run(probs, chunks, labels, beam, threads=threads, **kw)
    scorer = ob.Scorer(kw.get("alpha", 0.0), kw.get("beta", 0.0), kw["lm_path"], labels) if kw.get("lm_path") else None
    bad = 0
    t = 0
    for k, (s, w) in enumerate(res):
        t += chunks[k]
        stok, sstep, sln, snb, ssc = s
        wtok, wstep, wln, wnb, wsc = w
        why = []
        if snb != wnb:
            why.append("beam count %d vs %d" % (snb, wnb))
        else:
            for p in range(snb):
                L = int(sln[p])
                if L != int(wln[p]) or not np.array_equal(stok[p, :L], wtok[p, :L]) or not np.array_equal(sstep[p, :L], wstep[p, :L]):
                    why.append("beam %d differs from the whole kernel" % p)
                elif ssc[p].tobytes() != wsc[p].tobytes():
                    why.append("beam %d score %r vs %r" % (p, ssc[p], wsc[p]))
            ref = ob.ctc_beam_search(probs[:t].astype(np.float64), labels, beam, kw.get("cutoff_prob", 1.0), kw.get("top_n", 40), 0, scorer)
            if len(ref) != snb:
                why.append("oracle has %d beams, the carried search %d" % (len(ref), snb))
            else:
                for p, (_, rt, ro) in enumerate(ref):
                    L = int(sln[p])
                    if list(stok[p, :L]) != list(rt) or list(sstep[p, :L]) != list(ro):
                        why.append("beam %d differs from the oracle" % p)
        if why:
            bad += 1
            print("chunk %d (frames %d): %s" % (k, t, "; ".join(why[:4])))
    print("%d frames in %d chunks, beam %d, %d threads: %s" % (probs.shape[0], len(chunks), beam, threads,
                                                                 "OK" if not bad else "%d MISMATCHES" % bad))
    return bad == 0


def random_chunks(rng, T, n_zero=2, n_one=2):
    """a ragged cut of T frames with some 0- and 1-frame chunks mixed in"""
    cuts = []
    left = T
    while left > 0:
        c = int(min(left, rng.integers(1, 9)))
        cuts.append(c)
        left -= c
    for _ in range(n_zero):
        cuts.insert(int(rng.integers(0, len(cuts) + 1)), 0)
    for _ in range(n_one):
        k = int(rng.integers(0, len(cuts)))
        if cuts[k] > 1:
            cuts[k] -= 1
            cuts.insert(k + 1, 1)
    return cuts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=1024)
    a = ap.parse_args()
    build()
    rng = np.random.default_rng(0)
    probs = rng.dirichlet(np.ones(4), size=12).astype(np.float32)
    ok = compare(probs, random_chunks(rng, 12), "_ab ", 5, a.threads)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
