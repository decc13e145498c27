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
