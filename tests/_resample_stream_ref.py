"""The chunked sample-rate conversion (dsmi_resampler_*, csrc/resample_stream.hip) restated in numpy: an utterance arrives in
chunks, every push returns the outputs that are final now, and what the next outputs still need of the past input waits in a
tail.  Each output is computed exactly as tests/_resample_ref.py computes it for the whole signal (the same products, summed by
the same numpy call), so that the two can be compared with ``array_equal``.  A helper module of the tests (not collected)."""
import numpy as np

import _resample_ref as R


def k_hi(j, up, down, half):
    return (j * down + half) // up


def ready(method, rate_in, rate_out, n_in):
    """Outputs final after ``n_in`` samples, from the definitions (closed forms; brute force below)."""
    up, down = R.ratio(rate_in, rate_out)
    if n_in <= 0:
        return 0
    if up == down:
        return n_in
    if method == R.RATECV:
        return R.count(R.RATECV, rate_in, rate_out, n_in)
    half = 10 * max(up, down)
    return min(R.count(R.POLYPHASE, rate_in, rate_out, n_in), max(0, -((half - n_in * up) // down)))


def ready_brute(method, rate_in, rate_out, n_in):
    """The number of outputs j < count(n_in) whose every input is among the first n_in samples, counted one by one."""
    up, down = R.ratio(rate_in, rate_out)
    half = 10 * max(up, down)
    total = R.count(method, rate_in, rate_out, n_in) if up != down else n_in
    j = 0
    while j < total:
        last = j if up == down else (-((-j * down) // up) if method == R.RATECV else k_hi(j, up, down, half))
        if last > n_in - 1:
            break
        j += 1
    return j


def kmax(rate_in, rate_out):
    up, down = R.ratio(rate_in, rate_out)
    return -((-(20 * max(up, down) + 1)) // up)


class Chunked(object):
    """One utterance in flight.  ``push(chunk, is_last)`` -> the outputs that are final now (int64 for ratecv, float64 else)."""

    def __init__(self, method, rate_in, rate_out=16000, width=2):
        self.method, self.rate_in, self.rate_out, self.width = method, rate_in, rate_out, width
        self.up, self.down = R.ratio(rate_in, rate_out)
        self.same = self.up == self.down
        self.half = 10 * max(self.up, self.down)
        self.kmax = kmax(rate_in, rate_out)
        self.h = None if self.same or method == R.RATECV else R.taps(rate_in, rate_out)[0]
        self.longest_tail = 0
        self.reset()

    def reset(self):
        self.total, self.emitted, self.tail_start = 0, 0, 0
        self.tail = np.zeros(0, dtype=np.float64 if self.method == R.POLYPHASE else np.int64)

    def _tail_start(self, emitted, total):
        if self.same:
            return total
        if self.method == R.RATECV:
            return max(total - 1, 0)
        return min(max(k_hi(emitted, self.up, self.down, self.half) - (self.kmax - 1), 0), total)

    def push(self, chunk, is_last=False):
        chunk = np.asarray(chunk, dtype=self.tail.dtype)
        assert self.tail_start + len(self.tail) == self.total
        known = np.concatenate((self.tail, chunk))           # samples [tail_start, total + len(chunk))
        base, total = self.tail_start, self.total + len(chunk)
        if self.same:
            end = total
        elif is_last:
            end = R.count(self.method, self.rate_in, self.rate_out, total)
        else:
            end = ready(self.method, self.rate_in, self.rate_out, total)
        js = np.arange(self.emitted, end, dtype=np.int64)
        if self.same:
            out = chunk.copy()
        elif self.method == R.RATECV:
            out = self._ratecv(js, known, base)
        else:
            out = self._polyphase(js, known, base, total)
        if is_last:
            self.reset()
            return out
        self.emitted, self.total = end, total
        self.tail_start = self._tail_start(end, total)
        self.tail = known[self.tail_start - base:].copy()
        self.longest_tail = max(self.longest_tail, len(self.tail))
        return out

    def _ratecv(self, j, known, base):
        """_resample_ref.ratecv's lines with X[c - 1] looked up in tail + chunk."""
        o, i = self.up, self.down
        sh = 32 - 8 * self.width
        if len(j) == 0:
            return np.zeros(0, dtype=np.int64)
        X = known << sh
        c = -((-j * i) // o)
        d = c * o - j * i
        assert (c - base < len(X)).all() and (np.where(c > 0, c - 1 - base, 0) >= 0).all()
        prev = np.where(c > 0, X[np.maximum(c - 1 - base, 0)], 0)
        v = prev.astype(np.float64) * d.astype(np.float64) + X[c - base].astype(np.float64) * (o - d).astype(np.float64)
        return np.trunc(v / np.float64(o)).astype(np.int64) >> sh

    def _polyphase(self, js, known, base, total):
        """_resample_ref.polyphase's loop body with x[k] looked up in tail + chunk; x is zero outside [0, total)."""
        y = np.zeros(len(js))
        for m, j in enumerate(js):
            hi = k_hi(j, self.up, self.down, self.half)
            lo = -((self.half - j * self.down) // self.up)
            k = np.arange(max(lo, 0), min(hi, total - 1) + 1)
            assert len(k) == 0 or k[0] >= base, "the tail has dropped a sample an output still needs"
            y[m] = (known[k - base] * self.h[j * self.down - k * self.up + self.half]).sum()
        return y


def chunkings(n, rng, tail):
    """Ways of cutting ``n`` samples: random, all of one sample (the flush comes with the last sample), with zero-sample chunks,
    one chunk shorter than the tail in the middle, one chunk holding everything.  -> {name: [chunk lengths]}"""
    def cut(sizes):
        out, left = [], n
        for s in sizes:
            s = min(int(s), left)
            out.append(s)
            left -= s
        if left:
            out.append(left)
        return out
    return {
        "random": cut(rng.integers(1, max(2, n // 3), size=64)),
        "ones": [1] * n,
        "zeros": cut([0, 5, 0, 0, max(1, n // 4), 0, 1, 0, max(1, n // 3), 0]),
        "short": cut([max(1, n // 2), max(1, tail // 3), 1, 2]),
        "whole": [n],
    }
