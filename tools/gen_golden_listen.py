#!/usr/bin/env python3
"""G14: what the reference's ``Recognizer.listen_stream`` yields over seeded streams (build container only; data-only fixture).

The reference ``Recognizer`` is imported with the stand-ins of tools/gen_golden_surface.py for its absent third parties (none
of them is touched by the listener) and ``listen_stream`` (/root/reference/danspeech/Recognizer.py:218-324) is driven the way
``threaded_listen`` (:356-377) drives it: a new generator after every ``is_last``, stopping at the first end-of-stream close.
The sources are the reference's own ``SpeechFile`` over seeded WAV files (chunk 4096, one and two channels) and a minimal
``SpeechSource`` subclass over bytes (chunk 1024 and 256).  For every yield the fixture records ``is_last``, the first sample
and the sample count, taken from the source's read position.  tests/golden/g14_listen.json holds the streams' seeded recipes
(tests/_listen_ref.py make_stream) and those yields: no audio, no program text.

    python tools/gen_golden_listen.py            # rewrites tests/golden/g14_listen.json
"""
import json
import os
import sys
import tempfile
import types
import wave

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy.signal  # noqa: E402
import scipy.signal.windows as _W  # noqa: E402
for _w in ("hamming", "hann", "blackman", "bartlett"):
    setattr(scipy.signal, _w, getattr(_W, _w))

for _n in ("librosa", "Levenshtein", "wget", "ctcdecode"):
    sys.modules[_n] = types.ModuleType(_n)
sys.modules["ctcdecode"].CTCBeamDecoder = object

from danspeech import Recognizer  # noqa: E402
from danspeech.audio.resources import SpeechFile, SpeechSource  # noqa: E402

from _listen_ref import make_stream, buffer_counts  # noqa: E402

RATE = 16000


class BytesSource(SpeechSource):
    """The least a listener needs of a source: chunk, sampling_rate, sampling_width and a stream with read(frames)."""

    class _Stream(object):
        def __init__(self, data):
            self.data, self.pos = data, 0

        def read(self, size):
            out = self.data[2 * self.pos:2 * (self.pos + size)]
            self.pos += len(out) // 2
            return out

    def __init__(self, samples, chunk):
        self.sampling_rate, self.sampling_width, self.chunk = RATE, 2, chunk
        self.stream = BytesSource._Stream(samples.astype("<i2").tobytes())

    def position(self):
        return self.stream.pos


def drive(recognizer, source, position):
    """threaded_listen's loop; -> [[is_last, start, count], ...]"""
    recognizer.stream = True
    yields = []
    while True:
        generator = recognizer.listen_stream(source)
        while True:
            is_last, temp = next(generator)
            nbytes = sum(len(t) for t in temp) if isinstance(temp, list) else len(temp)
            count = nbytes // source.sampling_width
            yields.append([int(bool(is_last)), position() - count, count])
            if is_last:
                break
        if count == 0:
            return yields


def cases():
    L, S = 3000, 60          # noise amplitudes: rms about 1730 and 35 against the threshold 1000 (and 500)

    def plan(chunk, *runs):
        return [[int(round(n * chunk)), amp, kind] for n, amp, kind in runs]

    out = []
    for chunk, src in ((4096, "file"), (1024, "bytes"), (256, "bytes")):
        pn, hn, kn = buffer_counts(chunk, RATE)
        t = lambda name: "%s_c%d" % (name, chunk)
        out += [
            dict(name=t("silence_only"), plan=plan(chunk, (9.4, S, "noise"))),
            dict(name=t("speech_in_first_buffer"), plan=plan(chunk, (hn + 2, L, "noise"), (pn + 3, S, "noise"))),
            dict(name=t("too_short_then_real"), plan=plan(chunk, (2, S, "noise"), (1, L, "noise"), (pn + 2, S, "noise"), (hn + 2, L, "noise"),
                                                          (pn + 2, S, "noise"))),
            dict(name=t("pause_of_pause_n"), plan=plan(chunk, (1, S, "noise"), (hn + 1, L, "noise"), (pn, S, "noise"), (2, L, "noise"),
                                                       (pn + 2.5, S, "noise"))),
            dict(name=t("pause_of_pause_n_plus_1"), plan=plan(chunk, (1, S, "noise"), (hn + 1, L, "noise"), (pn + 1, S, "noise"), (hn + 1, L, "noise"),
                                                              (pn + 2.5, S, "noise"))),
            dict(name=t("rms_equals_threshold"), plan=plan(chunk, (5.5, 1000, "const"))),
            dict(name=t("rms_threshold_plus_1"), plan=plan(chunk, (5.5, 1001, "const"))),
            dict(name=t("ends_mid_phrase_short_buffer"), plan=plan(chunk, (2, S, "noise"), (hn + 1.4, L, "noise"))),
        ]
        for c in out[-8:]:
            c.update(chunk=chunk, source=src, channels=1, params=None)
    pn, hn, kn = buffer_counts(256, RATE)
    three = []
    for _ in range(3):
        three += [(kn + 3, S, "noise"), (hn + 4, L, "noise"), (pn + 1, S, "noise")]
    out.append(dict(name="three_utterances_c256", chunk=256, source="bytes", channels=1, params=None, plan=plan(256, *three, (0.5, S, "noise"))))
    pn, hn, kn = buffer_counts(4096, RATE)
    out.append(dict(name="stereo_fold_saturates_c4096", chunk=4096, source="file", channels=2, params=None,
                    plan=plan(4096, (2, S, "noise"), (hn + 2, 30000, "noise"), (pn + 1, S, "noise"), (1.3, 30000, "noise"))))
    second = dict(energy_threshold=500, pause_threshold=0.5, phrase_threshold=0.2, non_speaking_duration=0.2)
    pn, hn, kn = buffer_counts(1024, RATE, **second)
    out.append(dict(name="second_parameters_c1024", chunk=1024, source="bytes", channels=1, params=second,
                    plan=plan(1024, (kn + 2, S, "noise"), (hn + 1, 600, "const"), (pn, S, "noise"), (1, 600, "const"), (pn + 1, S, "noise"),
                              (2, 500, "const"), (hn, 501, "const"), (0.7, S, "noise"))))
    for i, c in enumerate(out):
        c["seed"] = 1400 + i
    return out


def main():
    records = []
    for c in cases():
        recipe = {"seed": c["seed"], "plan": c["plan"]}
        x = make_stream(recipe, c["channels"])
        assert len(x) <= 6 * RATE, c["name"]
        r = Recognizer()
        if c["params"]:
            p = c["params"]
            r.update_stream_parameters(energy_threshold=p["energy_threshold"], pause_threshold=p["pause_threshold"],
                                       phrase_threshold=p["phrase_threshold"], non_speaing_duration=p["non_speaking_duration"])
        if c["source"] == "file":
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "s.wav")
                with wave.open(path, "wb") as w:
                    w.setnchannels(c["channels"]); w.setsampwidth(2); w.setframerate(RATE)
                    w.writeframes(x.astype("<i2").tobytes())
                with SpeechFile(path) as s:
                    assert s.chunk == c["chunk"]
                    yields = drive(r, s, s.audio_reader.tell)
        else:
            s = BytesSource(x, c["chunk"])
            yields = drive(r, s, s.position)
        records.append(dict(name=c["name"], source=c["source"], chunk=c["chunk"], channels=c["channels"], rate=RATE, params=c["params"],
                            recipe=recipe, n_samples=len(x), n_last=sum(y[0] for y in yields), yields=yields))
        print("%-40s %6d samples  %3d yields  %d last" % (c["name"], len(x), len(yields), records[-1]["n_last"]))
    path = os.path.join(ROOT, "tests", "golden", "g14_listen.json")
    with open(path, "w") as f:
        json.dump({"reference": "danspeech/Recognizer.py:218-324 listen_stream, driven as :356-377 threaded_listen",
                   "yield": ["is_last", "start_sample", "n_samples"], "cases": records}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
