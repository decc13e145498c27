"""The host-side schedule of real-time streaming: how ``Recognizer.stream_recording`` cuts one utterance into passes and
how ``Recognizer.stream_recordings`` deals the passes of many utterances into batched rounds.  Pure Python (no GPU)."""
def stream_cut_plan(n_samples, chunk_samples, lookahead_context, samples_pr_10ms):
    """How ``real_time_streaming`` (reference Recognizer.py:560-710) cuts an utterance of ``n_samples`` that arrives in parts
    of ``chunk_samples`` (1024 when not given): the passes of ``streaming_transcribe`` as ``(lo, hi, is_first, is_last)``
    sample ranges.  The first pass waits for ``general + 15 * samples_pr_10ms`` samples, later ones for ``general``
    (:598-612); the last part always makes a pass, except that an utterance that ends before its first pass is discarded
    (:666-667)."""
    required_spec_frames = (lookahead_context - 1) * 2
    general = samples_pr_10ms * 2 + (samples_pr_10ms * (required_spec_frames - 1))
    first = general + (samples_pr_10ms * 15)
    step = int(chunk_samples) if chunk_samples else 1024
    plan = []
    pos, lo, is_first_pass = 0, 0, True
    while pos < n_samples:
        pos = min(pos + step, n_samples)
        is_last = pos >= n_samples
        if is_first_pass:
            if is_last:
                break                                  # too short for a first pass: discarded
            if pos - lo >= first:
                plan.append((lo, pos, True, False))
                is_first_pass, lo = False, pos
        elif is_last or pos - lo >= general:
            plan.append((lo, pos, False, is_last))
            lo = pos
    return plan


def stream_rounds(plans):
    """The rounds of ``Recognizer.stream_recordings``: round r holds ``(index, plans[index][r])`` for every plan that has an
    r-th pass, in index order -- each session advances once per round, in its own order, until all plans are done."""
    rounds = []
    for r in range(max([len(p) for p in plans] + [0])):
        rounds.append([(k, p[r]) for k, p in enumerate(plans) if r < len(p)])
    return rounds


# ---- streaming from a source of another rate: the arithmetic of dsmi_resample_count / dsmi_resample_ready, restated here so that
# the schedule needs neither the library nor a GPU
def _ratio(rate_in, rate_out):
    from math import gcd
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in <= 0 or rate_out <= 0:
        raise ValueError("rates must be positive")
    g = gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g          # up, down


def _method(method):
    if method not in ("polyphase", "ratecv"):
        raise ValueError("resample method must be 'polyphase' or 'ratecv'")
    return method


def resample_count(n_in, rate_in, rate_out=16000, method="polyphase"):
    """Length ``n_in`` samples at ``rate_in`` have at ``rate_out`` (``dsmi_resample_count``)."""
    up, down = _ratio(rate_in, rate_out)
    if n_in <= 0:
        return 0
    return (n_in - 1) * up // down + 1 if _method(method) == "ratecv" else -((-n_in * up) // down)


def resample_ready(n_in, rate_in, rate_out=16000, method="polyphase"):
    """Outputs that are final once the first ``n_in`` source samples are known (``dsmi_resample_ready``): the polyphase filter
    looks ``half / up`` samples ahead, ``ratecv`` and equal rates do not."""
    up, down = _ratio(rate_in, rate_out)
    if _method(method) == "ratecv" or up == down or n_in <= 0:
        return resample_count(n_in, rate_in, rate_out, method)
    half = 10 * max(up, down)
    return min(resample_count(n_in, rate_in, rate_out, method), max(0, -((half - n_in * up) // down)))


def resample_need(n_out, rate_in, rate_out=16000, method="polyphase"):
    """The fewest source samples after which ``n_out`` outputs are final -- ``k_hi(n_out - 1) + 1`` for the polyphase filter.  It
    may exceed the source's length: the last outputs need the zeros behind the source's end, i.e. the flush."""
    up, down = _ratio(rate_in, rate_out)
    if n_out <= 0:
        return 0
    if up == down:
        return n_out
    if _method(method) == "ratecv":
        return -((-(n_out - 1) * down) // up) + 1
    return ((n_out - 1) * down + 10 * max(up, down)) // up + 1


def resample_feed_plan(plan, n_source, rate_in, rate_out=16000, method="polyphase"):
    """How a source of ``n_source`` samples at ``rate_in`` is fed to a session whose passes ``plan`` (``stream_cut_plan`` over the
    converted length) are counted in ``rate_out`` samples: one ``(src_lo, src_hi, flush)`` per pass.  Before pass ``(lo, hi)``
    the source is pushed up to ``resample_need(hi)`` samples, just enough for the pass's last sample to be final; the pass that
    reaches the source's end also flushes (its last outputs need the end), and later passes push nothing.  Nothing is pushed
    twice; outputs beyond ``hi`` wait in the session."""
    feed, pos, flushed = [], 0, False
    for lo, hi, _, is_last in plan:
        upto = n_source if is_last else min(n_source, resample_need(hi, rate_in, rate_out, method))
        upto = max(upto, pos)
        flush = upto >= n_source and not flushed
        feed.append((pos, upto, flush))
        flushed = flushed or flush
        pos = upto
    return feed


# ---- live audio: the pass rule of real_time_streaming (reference Recognizer.py:602-611, :664-715) without its sleeps
def live_requirements(lookahead_context, sample_rate):
    """(first_sample_requirement, general_sample_requirement) of :602-611."""
    required_spec_frames = (lookahead_context - 1) * 2
    samples_pr_10ms = int(sample_rate / 100)
    general = samples_pr_10ms * 2 + (samples_pr_10ms * (required_spec_frames - 1))
    return general + samples_pr_10ms * 15, general


class LivePasses:
    """One live session's side of ``real_time_streaming``: the segments the gate emits accumulate, and ``feed`` says which
    ``streaming_transcribe`` passes are due.  A round's segments are taken up to a ``last`` mark (the reference drains its queue
    the same way, :627-662), then the rule runs once: the first pass of an utterance as soon as ``first`` samples are there,
    later ones at ``general``, a ``last`` mark passes whatever has accumulated with ``is_last``.  A ``last`` mark that arrives
    before the first pass makes no pass (:668-669) -- and, as in the reference, what had accumulated is not cleared: those
    samples stand in front of the next utterance's.  Segments are anything with a ``len``; they are handed back, not joined."""

    def __init__(self, lookahead_context, sample_rate):
        self.first, self.general = live_requirements(lookahead_context, sample_rate)
        self.parts, self.n, self.is_first_pass = [], 0, True

    def feed(self, segments):
        """``segments``: [(samples, last), ...] in order -> [(parts, is_first, is_last), ...], the passes to make now, each a
        list of segments to lay end to end."""
        out = []
        queue = list(segments)
        while queue:
            is_last = False
            while queue and not is_last:
                samples, is_last = queue.pop(0)
                self.parts.append(samples)
                self.n += len(samples)
            if self.is_first_pass:
                if not is_last and self.n >= self.first:
                    out.append((self._take(), True, False))
                    self.is_first_pass = False
            elif is_last or self.n >= self.general:
                out.append((self._take(), False, bool(is_last)))
            if is_last:
                self.is_first_pass = True
        return out

    def _take(self):
        parts, self.parts, self.n = self.parts, [], 0
        return parts
