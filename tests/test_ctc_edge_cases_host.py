"""The edge table of the CTC tools' shared feeder (tests/_ctc_edge_cases.py) on the CPU: no case is infeasible, so the three GPU
tests that use it never skip one -- every numpy reference gives a finite result for every row and every phrase fits."""
import numpy as np
import pytest

import _align_ref as aref
import _ctc_edge_cases as edge
import _score_ref as sref
import _spot_ref as pref


@pytest.mark.parametrize("shape", edge.SHAPES + edge.LONG, ids=edge.name)
def test_every_row_is_feasible_for_the_references(shape):
    T, C, L = shape
    probs, rows = edge.case(T, C, L)
    assert [len(p) for p in probs] == [T, T - 1 - T // 4] and len(probs[1]) < T
    for p, rs in zip(probs, rows):
        for r in rs:
            assert len(r) <= len(p) // 2 and all(1 <= t < C for t in r)
            v = aref.viterbi(p, r)
            assert v is not None and np.isfinite(v["path_logp"])
            f = sref.forward(p, r)
            assert f is not None and np.isfinite(f)
    if L is None:
        for ph in edge.phrases(T, C):
            assert 1 <= len(ph) and aref.min_frames(ph) <= T
            E, ST = pref.tracks(probs[0], ph)
            assert np.isfinite(E[-1]) and 0 <= ST[-1] < T
    else:
        assert 2 * len(rows[0][0]) + 1 in (255, 257)
