"""Reference of the streaming phrase watch (dsmi_spot_stream_advance_many, csrc/spot_stream.hip) in numpy: dsmi_spot's trellis
cut into chunks with the row of the last frame carried from one to the next, and the online picking rule of include/dsmi.h
written out plainly.  A helper module of the tests (not collected)."""
import numpy as np

import _spot_ref
from _align_ref import log_probs


class Trellis:
    """One phrase's carried search: ``advance(probs_chunk)`` -> (E, ST) of the chunk's frames, starts counted from the
    utterance's first frame.  The arithmetic is ``_spot_ref.tracks``'s, line by line."""

    def __init__(self, phrase, blank=0, dtype=np.float32):
        self.dtype = dtype
        S = 2 * len(phrase) - 1
        self.lab = _spot_ref.state_labels(phrase, blank)
        self.skip = np.array([s % 2 == 0 and s >= 2 and self.lab[s] != self.lab[s - 2] for s in range(S)])
        self.a = np.full(S, dtype(-np.inf), dtype=dtype)
        self.b = np.full(S, -1, dtype=np.int32)
        self.t0 = 0

    def advance(self, probs):
        probs = np.asarray(probs, dtype=np.float32)
        T, dtype, ninf = probs.shape[0], self.dtype, self.dtype(-np.inf)
        lp = log_probs(probs, dtype) if T else None
        E, ST = np.full(T, ninf, dtype=dtype), np.full(T, -1, dtype=np.int32)
        a, b, S = self.a, self.b, len(self.lab)
        for f in range(T):
            a1, b1 = _spot_ref._shift(a, 1, ninf), _spot_ref._shift(b, 1, -1)
            a2, b2 = _spot_ref._shift(a, 2, ninf), _spot_ref._shift(b, 2, -1)
            a2[~self.skip] = ninf
            best, start = a.copy(), b.copy()
            m = a1 > best
            best[m], start[m] = a1[m], b1[m]
            m = a2 > best
            best[m], start[m] = a2[m], b2[m]
            best[0], start[0] = 0, self.t0 + f
            a, b = (best + lp[f, self.lab]).astype(dtype), start
            E[f], ST[f] = a[S - 1], b[S - 1]
        self.a, self.b, self.t0 = a, b, self.t0 + T
        return E, ST


def chunked_tracks(probs, phrase, cuts, blank=0, dtype=np.float32):
    """(E, ST) of ``probs`` [T, C] fed in chunks of ``cuts`` frames (they sum to T), laid end to end."""
    tr, at, Es, Ss = Trellis(phrase, blank, dtype), 0, [], []
    for c in cuts:
        E, ST = tr.advance(probs[at:at + c])
        Es.append(E), Ss.append(ST)
        at += c
    assert at == len(probs)
    return np.concatenate(Es + [np.zeros(0, dtype)]), np.concatenate(Ss + [np.zeros(0, np.int32)])


class Picker:
    """The online picking rule of one (stream, phrase), the three steps of include/dsmi.h in their order."""

    def __init__(self, min_mean_logp, settle_frames):
        self.floor, self.settle = np.float32(min_mean_logp), int(settle_frames)
        self.pending, self.last_end, self.frames = None, -1, 0         # pending: (pv, ps, pe)

    def feed(self, E, ST, flush=False):
        """The next ``len(E)`` frames -> the events fired: [(start, end, score, fired), ...], frames [start, end)."""
        out = []
        for e, st in zip(np.asarray(E, dtype=np.float32), np.asarray(ST, dtype=np.int64)):
            f = self.frames
            if self.pending is not None and f - self.pending[2] >= self.settle:                       # 1
                out.append(self._fire(f))
            with np.errstate(invalid="ignore"):
                cand = e > -np.inf and e >= self.floor * np.float32(f - st + 1) and st > self.last_end    # 2
            if cand:                                                                                  # 3
                if self.pending is None:
                    self.pending = (e, int(st), f)
                elif st <= self.pending[2]:
                    if e > self.pending[0]:
                        self.pending = (e, int(st), f)
                else:
                    out.append(self._fire(f))
                    self.pending = (e, int(st), f)
            self.frames += 1
        if flush and self.pending is not None:
            out.append(self._fire(self.frames))
        return out

    def _fire(self, at):
        pv, ps, pe = self.pending
        self.pending, self.last_end = None, pe
        return (ps, pe + 1, float(pv), int(at))


def online_pick(E, ST, min_mean_logp, settle_frames, cuts=None, flush=True):
    """Every event of the whole tracks, fed in ``cuts`` (default: at once) and flushed at the end."""
    p, at, out = Picker(min_mean_logp, settle_frames), 0, []
    cuts = [len(E)] if cuts is None else list(cuts)
    for i, c in enumerate(cuts):
        out += p.feed(E[at:at + c], ST[at:at + c], flush and i == len(cuts) - 1)
        at += c
    assert at == len(E)
    return out


def disjoint_in_time_order(events):
    return all(a[0] < a[1] for a in events) and all(a[1] <= b[0] and a[3] <= b[3] for a, b in zip(events, events[1:]))


def cuts_of(rng, T, kind):
    """The five chunkings of the tests: 'random' (lengths from 0, 1, 15, 16, 17, 33), 'single' (every frame alone), 'one',
    'empties' (random with empty calls between) and 'aligned' (16 frames each, the rest last)."""
    if kind == "single":
        return [1] * T
    if kind == "one":
        return [T]
    if kind == "aligned":
        return [16] * (T // 16) + ([T % 16] if T % 16 else [])
    cuts, left = [], T
    while left:
        c = min(left, int(rng.choice([1, 15, 16, 17, 33] if kind == "random" else [0, 0, 1, 15, 16, 17, 33])))
        cuts.append(c)
        left -= c
    if kind == "empties":
        cuts = [0] + cuts + [0]
    return cuts


def planted(rng, T_noise, C, phrases, copies, hold=2, p=0.9, sharp=4.0):
    """Probabilities with well-separated occurrences planted: ``_spot_ref.peaky`` noise and, ``copies`` times per phrase in a
    shuffled order, the phrase's tokens held ``hold`` frames each at probability ``p`` (a blank frame at ``p`` between two equal
    tokens), with gaps of at least 3 phrase lengths (in frames) of noise on either side.  -> probs [T, C]."""
    order = [k for k in range(len(phrases)) for _ in range(copies)]
    rng.shuffle(order)
    longest = max(len(ph) for ph in phrases) * hold
    rows = [_spot_ref.peaky(rng, 3 * longest + int(rng.integers(0, 5)), C, sharp)]
    for k in order:
        path = []
        for j, t in enumerate(phrases[k]):
            if j and phrases[k][j - 1] == t:
                path.append(0)
            path += [int(t)] * hold
        blk = np.full((len(path), C), (1.0 - p) / (C - 1), dtype=np.float32)
        blk[np.arange(len(path)), path] = p
        rows += [blk, _spot_ref.peaky(rng, 3 * longest + int(rng.integers(0, 5)), C, sharp)]
    rows.append(_spot_ref.peaky(rng, T_noise, C, sharp))
    return np.concatenate(rows).astype(np.float32)
