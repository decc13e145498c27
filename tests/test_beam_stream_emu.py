"""The resumable beam search (beam_kernel<..., RESUME = true> in danspeech_amd/csrc/beam_kernel.inc) compiled for the CPU on
the SIMT emulation (tools/emu/beam_stream_emu.cpp): an utterance cut into ragged chunks, 0- and 1-frame chunks among them, is
advanced one launch per chunk, and after every chunk the carried search's hypotheses must equal the whole-utterance kernel's
over that prefix -- tokens, timesteps, lengths, and the double totals bit for bit -- and oracle/beam.py's over that prefix
(tokens, timesteps, lengths; the oracle's scores are its own formulation's rounding, which is why the existing emulation test
compares no scores either).  Test infrastructure, not a CPU path of the product."""
import os
import shutil
import sys

import numpy as np
import pytest

from danspeech_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))


@pytest.fixture(scope="module")
def emu():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    import run_beam_stream_emu
    import run_beam_emu
    try:
        run_beam_stream_emu.build()
    except Exception as e:            # an older g++ without <barrier>
        pytest.skip("cannot build the emulation: %s" % e)
    run_beam_stream_emu.peaky = run_beam_emu.peaky
    return run_beam_stream_emu


def test_resumed_search_small_alphabet(emu):
    rng = np.random.default_rng(0)
    probs = rng.dirichlet(np.ones(4), size=14).astype(np.float32)
    assert emu.compare(probs, emu.random_chunks(rng, 14), "_ab ", 64, 192)
    assert emu.compare(probs, [0, 1, 1, 5, 0, 7], "_ab ", 5, 192)


def test_resumed_search_revivals_across_chunk_boundaries(emu):
    """the walk seeds of test_beam_emu.py: dormant prefixes re-enter the beam, some of them in a chunk after the one in which
    they left it (the child table and the node pool carry them)"""
    for seed, beam in ((61, 3), (119, 3)):
        probs = np.random.default_rng(seed).dirichlet(np.ones(4) * 0.5, size=40).astype(np.float32)
        chunks = emu.random_chunks(np.random.default_rng(seed + 1), 40)
        assert emu.compare(probs, chunks, "_abc", beam, 192)
        assert emu.compare(probs, [1] * 40, "_abc", beam, 192)


def test_resumed_search_vocabulary_pruning(emu):
    probs = emu.peaky(np.random.default_rng(4), 1, 16, 33, 3.0)[0]
    chunks = emu.random_chunks(np.random.default_rng(5), 16)
    assert emu.compare(probs, chunks, syn.DANSPEECH_LABELS, 10, 192, top_n=10, cutoff_prob=0.98)


def test_resumed_search_with_a_trigram_scorer(emu, tmp_path):
    """the trailing-word term is added to the hypotheses written after each chunk and must not reach the carried scores:
    a leak would show up as a difference in the next chunk's beams or totals"""
    path = str(tmp_path / "emu_stream3.arpa")
    syn.make_arpa(path, order=3, n_words=120, seed=5, ngrams_per_order=300)
    probs = emu.peaky(np.random.default_rng(2), 1, 24, 33, 2.0)[0]
    chunks = emu.random_chunks(np.random.default_rng(3), 24)
    assert emu.compare(probs, chunks, syn.DANSPEECH_LABELS, 12, 192, lm_path=path, alpha=1.3, beta=0.2)
