#!/usr/bin/env python3
"""Generate tests/golden/g13_ratecv.npz by running the REFERENCE's own rate conversion (needs the reference tree and a
Python that still has ``audioop``).

For a dozen seeded cases the file holds the input bytes, (sample width, channels, frame rate) and what the reference
returns for them: mono cases call ``AudioData(frames, rate, width).get_array_data(convert_rate=16000)``; stereo cases are
written as WAV files and read back through ``SpeechFile``'s stream (the saturating fold of ``audioop.tomono``) first.
The reference is imported at run time with the stub recipe of tools/gen_golden.py; only data is written.

    python tools/gen_golden_resample.py [path/to/reference]      # default: $DANSPEECH_REFERENCE
"""
import os
import sys
import tempfile
import types
import warnings
import wave

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DANSPEECH_REFERENCE", "")
if not os.path.isdir(os.path.join(REFERENCE, "danspeech")):
    raise SystemExit("pass the reference tree (the directory that holds danspeech/) as the argument or in DANSPEECH_REFERENCE")
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)
for _n in ("Levenshtein", "librosa", "wget"):
    sys.modules[_n] = types.ModuleType(_n)
import scipy.signal  # noqa: E402
import scipy.signal.windows as _W  # noqa: E402
for _w in ("hamming", "hann", "blackman", "bartlett"):
    setattr(scipy.signal, _w, getattr(_W, _w))

import numpy as np  # noqa: E402

from danspeech.audio.resources import AudioData, SpeechFile  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_ratecv.npz")

# (sample width, channels, frame rate, frames, kind of samples)
CASES = [
    (2, 1, 44100, 3000, "uniform"),
    (2, 1, 8000, 2000, "uniform"),
    (2, 1, 16001, 3000, "uniform"),          # coprime to 16000
    (1, 1, 11025, 2500, "uniform"),
    (3, 1, 48000, 3000, "uniform"),
    (4, 1, 22050, 2000, "uniform"),
    (1, 1, 96000, 2400, "uniform"),
    (2, 2, 44100, 3000, "fullscale"),        # L + R saturates
    (3, 2, 8000, 1500, "uniform"),
    (4, 2, 48000, 2000, "fullscale"),
    (2, 1, 44100, 1, "uniform"),
    (2, 1, 8000, 2, "uniform"),
    (2, 2, 32000, 1, "fullscale"),
    (3, 1, 11025, 2, "uniform"),
]


def frames_of(x, width):
    x = np.asarray(x, dtype=np.int64)
    if width == 1:
        return (x + 128).astype(np.uint8).tobytes()
    if width == 3:
        u = (x & 0xFFFFFF).astype(np.uint32)
        return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], axis=1).astype(np.uint8).tobytes()
    return x.astype({2: "<i2", 4: "<i4"}[width]).tobytes()


def main():
    out = {"n_cases": np.array(len(CASES))}
    with tempfile.TemporaryDirectory() as tmp:
        for c, (width, nch, rate, n, kind) in enumerate(CASES):
            rng = np.random.default_rng(1300 + c)
            lim = 1 << (8 * width - 1)
            x = rng.integers(-lim, lim, size=n * nch)
            if kind == "fullscale":                       # every third frame has both channels at one rail
                rail = np.where(rng.integers(0, 2, size=n) == 0, -lim, lim - 1)
                pick = np.arange(n) % 3 == 0
                x = x.reshape(n, nch)
                x[pick] = rail[pick, None]
                x = x.reshape(-1)
            raw = frames_of(x, width)
            mono = raw
            if nch == 2:
                path = os.path.join(tmp, "c%d.wav" % c)
                with wave.open(path, "wb") as w:
                    w.setnchannels(2); w.setsampwidth(width); w.setframerate(rate); w.writeframes(raw)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    with SpeechFile(path) as src:
                        mono = src.stream.read()
            y = np.atleast_1d(AudioData(mono, rate, width).get_array_data(convert_rate=16000)).astype(np.float64)
            out["raw_%d" % c] = np.frombuffer(raw, dtype=np.uint8)
            out["fmt_%d" % c] = np.array([width, nch, rate], dtype=np.int64)
            out["out_%d" % c] = y
            print("case %2d: width %d, %d ch, %6d Hz, %5d frames -> %5d samples" % (c, width, nch, rate, n, len(y)))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.1f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
