"""The live gate in plain Python: ``Recognizer.listen_stream`` (reference Recognizer.py:218-324) driven as ``threaded_listen``
drives it (:356-377: a new generator after every ``is_last``), restated over an array of int16 samples with the energies from
``audioop.rms``.  tests/golden/g14_listen.json (tools/gen_golden_listen.py ran the reference itself) pins this restatement;
the host gate and the kernels are held to it.  Also the seeded streams the golden cases are made of."""
import audioop
import math

import numpy as np

DEFAULTS = dict(energy_threshold=1000, pause_threshold=0.8, phrase_threshold=0.3, non_speaking_duration=0.35)


def make_stream(recipe, channels=1):
    """int16 [n] (or [n, 2]) from a recipe {"seed", "plan": [[n_samples, amplitude, kind], ...]}: kind "noise" draws integers
    uniformly from [-amplitude, amplitude], "const" is the amplitude itself (rms exactly the amplitude)."""
    rng = np.random.RandomState(recipe["seed"])
    parts = []
    for n, amp, kind in recipe["plan"]:
        shape = (n,) if channels == 1 else (n, channels)
        if kind == "const":
            parts.append(np.full(shape, amp, dtype=np.int16))
        else:
            parts.append(rng.randint(-amp, amp + 1, size=shape).astype(np.int16))
    return np.concatenate(parts) if parts else np.zeros((0,) if channels == 1 else (0, channels), dtype=np.int16)


def fold_stereo(x):
    """audioop.tomono(buf, 2, 1, 1): the saturating sum of the two channels."""
    if x.ndim == 1:
        return x
    return np.frombuffer(audioop.tomono(np.ascontiguousarray(x).tobytes(), 2, 1, 1), dtype=np.int16)


def buffer_counts(chunk, rate, pause_threshold=0.8, phrase_threshold=0.3, non_speaking_duration=0.35, **_):
    spb = float(chunk) / rate
    return (int(math.ceil(pause_threshold / spb)), int(math.ceil(phrase_threshold / spb)), int(math.ceil(non_speaking_duration / spb)))


def energies(mono, chunk):
    """audioop.rms of every buffer of the stream, the short final one included."""
    return [audioop.rms(mono[k:k + chunk].tobytes(), 2) for k in range(0, len(mono), chunk)]


class Gate:
    """The generators' state between reads: ``buffer(energy, n)`` is one read of ``n`` samples, ``end()`` the empty read.
    Both return the yields they cause, [(is_last, start_sample, n_samples), ...]."""

    def __init__(self, chunk, rate=16000, **params):
        self.p = dict(DEFAULTS, **params)
        self.pause_n, self.phrase_n, self.keep_n = buffer_counts(chunk, rate, **self.p)
        self.pos, self.kept, self.in_phrase = 0, [], False
        self.pause_count = self.phrase_count = 0

    def buffer(self, energy, n):
        self.pos += n
        loud = energy > self.p["energy_threshold"]
        if not self.in_phrase:                      # waiting (:254-272)
            self.kept.append(n)
            if len(self.kept) > self.keep_n:
                self.kept.pop(0)
            if not loud:
                return []
            out = [(False, self.pos - sum(self.kept), sum(self.kept))]
            self.in_phrase, self.kept, self.pause_count, self.phrase_count = True, [], 0, 0
            return out
        self.phrase_count += 1                      # phrase (:284-309)
        self.pause_count = 0 if loud else self.pause_count + 1
        if self.pause_count <= self.pause_n:
            return [(False, self.pos - n, n)]
        self.in_phrase = False                      # :311-320: long enough closes the utterance, too short waits again
        if self.phrase_count - self.pause_count >= self.phrase_n:
            return [(True, self.pos - n, n)]
        return []

    def end(self):
        out = [] if self.in_phrase else [(False, self.pos - sum(self.kept), sum(self.kept))]
        self.in_phrase, self.kept = False, []
        return out + [(True, self.pos, 0)]


def listen(mono, chunk, rate=16000, energy=None, **params):
    """Every yield of the listen generators over the whole stream, up to the first end-of-stream close:
    [(is_last, start_sample, n_samples), ...].  ``energy``: the buffers' energies when they are given rather than measured
    (``mono`` then only says how long the stream is)."""
    e = energies(mono, chunk) if energy is None else list(energy)
    g = Gate(chunk, rate, **params)
    out = []
    for k, v in enumerate(e):
        out += g.buffer(v, min(chunk, len(mono) - k * chunk))
    return out + g.end()


def utterances(yields):
    """What a consumer sees whatever the segmentation: the sample indices of every closed utterance, and of the open rest."""
    done, cur = [], []
    for is_last, start, count in yields:
        cur.extend(range(start, start + count))
        if is_last:
            done.append(cur)
            cur = []
    return done, cur


# ---- real_time_streaming's pass rule (:602-611, :664-715) without its sleeps, transcribed directly.  `rounds` are the
# (is_last, samples) pairs the listener has queued each time the consumer looks: the inner loop (:627-662) drains the queue up
# to an is_last, then the rule runs once; a round that still holds data goes round again.
def pass_requirements(context, rate):
    required_spec_frames = (context - 1) * 2
    samples_pr_10ms = int(rate / 100)
    general = samples_pr_10ms * 2 + (samples_pr_10ms * (required_spec_frames - 1))
    return general + samples_pr_10ms * 15, general


def passes(rounds, first_req, general_req):
    """-> per round, [(samples, is_first, is_last), ...]: the streaming_transcribe calls real_time_streaming makes."""
    result = []
    data_array = []
    is_first_data = True
    is_first_pass = True
    is_last = False
    for arrivals in rounds:
        out = []
        queue = list(arrivals)
        while queue:
            while queue and not is_last:
                if is_first_data:
                    is_last, data_array = queue.pop(0)
                    data_array = np.asarray(data_array)
                    is_first_data = False
                else:
                    is_last, temp = queue.pop(0)
                    data_array = np.concatenate((data_array, np.asarray(temp)))
            if is_first_pass:
                if is_last:
                    pass            # :668-669: no pass.  data_array and is_first_data stay: these samples precede the next utterance's
                elif len(data_array) >= first_req:
                    out.append((data_array, True, False))
                    is_first_pass = False
                    data_array = []
                    is_first_data = True
            else:
                if is_last:
                    out.append((data_array, False, True))
                    data_array = []
                    is_first_data = True
                elif len(data_array) >= general_req:
                    out.append((data_array, False, False))
                    data_array = []
                    is_first_data = True
            if is_last:
                is_first_pass = True
                is_last = False
        result.append(out)
    return result
