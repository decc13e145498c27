"""GPU: ``Recognizer.adjust_for_speech`` / ``adjust_for_ambient_noise`` (reference Recognizer.py:717-797) over arrays, against
their formulas over ``audioop.rms``; the gate parameters and ``update_stream_parameters`` (:42-62, :800-818)."""
import audioop

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _rms(x, chunk, duration, rate):
    spb, t, out = (chunk + 0.0) / rate, 0, []
    for k in range(len(x) // chunk):
        t += spb
        if t > duration:
            break
        out.append(audioop.rms(x[k * chunk:(k + 1) * chunk].tobytes(), 2))
    return out, spb


def test_adjust_methods_follow_their_formulas():
    from danspeech_amd import Recognizer
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    r = Recognizer()
    assert (r.energy_threshold, r.pause_threshold, r.phrase_threshold, r.non_speaking_duration) == (1000, 0.8, 0.3, 0.35)
    r.update_stream_parameters(pause_threshold=0.5, non_speaing_duration=0.2)
    assert (r.energy_threshold, r.pause_threshold, r.phrase_threshold, r.non_speaking_duration) == (1000, 0.5, 0.3, 0.2)
    rng = np.random.RandomState(7)
    x = (rng.randint(-2000, 2001, size=5 * 16000) * np.linspace(0.2, 1.0, 5 * 16000)).astype(np.int16)
    for chunk, rate, duration in ((1024, None, 4), (4096, None, 4), (1000, 44100, 1)):
        e, _ = _rms(x, chunk, duration, rate or 16000)
        assert len(e) > 3
        r.adjust_for_speech(x, duration=duration, chunk=chunk, sample_rate=rate)
        assert r.energy_threshold == sum(e) / len(e) - 80
    r.adjust_for_speech(np.full(4096, 30, dtype=np.int16), chunk=1024)
    assert r.energy_threshold == 30                                         # at most 80: taken as it is
    r.energy_threshold = 1000
    e, spb = _rms(x, 1024, 2, 16000)
    want = 1000
    for v in e:
        damping = 0.15 ** spb
        want = want * damping + v * 1.5 * (1 - damping)
    r.adjust_for_ambient_noise(x, chunk=1024)
    assert r.energy_threshold == want and len(e) == 31
    # a gate made now carries the tuned parameters
    ep = r.new_endpointer(chunk=1024)
    segs = ep.push(torch.from_numpy(x[:32000]).cuda(), end_of_stream=True)
    assert segs and segs[-1][1]
    ep.close()
