"""Public facade of the drop-in surface (reference danspeech/Recognizer.py:13-130).

``Recognizer(model=None, lm=None, with_gpu=False, **kwargs)``, ``recognize``, ``update_model``,
``update_decoder`` with the reference's signatures, prints and exceptions, plus
``recognize_batch`` / ``recognize_files`` / ``recognize_long``.  Of the streaming half of the reference
class (Recognizer.py:133-818) the real-time path is provided array-driven
(``enable_real_time_streaming`` + ``stream_recording``); the microphone threads are live-audio control
flow outside the hot path.
"""
import numpy as np

from .errors.recognizer_errors import ModelNotInitialized
from .DanSpeechRecognizer import DanSpeechRecognizer
from .stream_plan import stream_cut_plan, stream_rounds, resample_count, resample_feed_plan


class Recognizer(object):

    def __init__(self, model=None, lm=None, with_gpu=False, **kwargs):
        # the live gate's parameters (reference Recognizer.py:42-62): read when a gate is made (``new_endpointer``)
        self.energy_threshold = 1000
        self.pause_threshold = 0.8
        self.phrase_threshold = 0.3
        self.non_speaking_duration = 0.35
        self.dynamic_energy_adjustment_damping = 0.15
        self.dynamic_energy_ratio = 1.5
        self.danspeech_recognizer = DanSpeechRecognizer(with_gpu=with_gpu, **kwargs)
        self.stream = False
        self.stream_thread_stopper = None
        if model:
            self.update_model(model)
        if lm:
            if not model:
                raise ModelNotInitialized("Trying to initialize language model without also choosing a DanSpeech "
                                          "acoustic model.")
            else:
                self.update_decoder(lm=lm)
        self.microphone = None

    def recognize(self, audio_data, show_all=False):
        """Most likely transcription of ``audio_data`` (numpy array as returned by ``load_audio``);
        all beams when ``show_all`` and a language model is set."""
        return self.danspeech_recognizer.transcribe(audio_data, show_all=show_all)

    def recognize_batch(self, audio_list, show_all=False, sample_rate=None, resample="polyphase"):
        """``recognize`` for a list of clips in one batched pass over the GPU.  ``sample_rate``: the clips' rate when it is not
        the model's 16 kHz; they are converted on the GPU first (``resample``: "polyphase", or "ratecv" for the reference's
        ``audioop.ratecv``)."""
        return self.danspeech_recognizer.transcribe_batch(audio_list, show_all=show_all, sample_rate=sample_rate, resample=resample)

    def align(self, audio_data, transcript):
        """Word timings of a transcript the caller already has (an edited subtitle, a correction, or ``recognize(audio_data)``)
        in ``audio_data``: ``[(word, start_s, end_s, confidence), ...]``, or ``None`` when the transcript cannot fit the
        audio (``DanSpeechRecognizer.align_batch``)."""
        return self.danspeech_recognizer.align(audio_data, transcript)

    def align_batch(self, audio_list, transcripts):
        """``align`` for a list of clips in one batched pass over the GPU; results in the caller's order."""
        return self.danspeech_recognizer.align_batch(audio_list, transcripts)

    def recognize_grammar(self, audio_list, grammar):
        """What was said in each clip, given that it is a sentence of ``grammar`` (``danspeech_amd.grammar``: commands, digits,
        a closed vocabulary, a transcript with alternatives): per clip ``(text, [(word, start_s, end_s, confidence), ...],
        path_logp, logp)``, or ``None`` when no sentence of the grammar fits the audio; one batched pass over the GPU, results
        in the caller's order (``DanSpeechRecognizer.transcribe_grammar_batch``)."""
        return self.danspeech_recognizer.transcribe_grammar_batch(audio_list, grammar)

    def grammar_confidence_batch(self, audio_list, grammar):
        """Was a sentence of ``grammar`` said in each clip, and how sure is the decoded one?  Per clip ``None`` when no sentence
        fits the audio, else ``dict(text, chars, path_logp, grammar_logp, sentence_posterior)``: ``recognize_grammar``'s best
        sentence, the natural log of the summed probability of every path the grammar accepts (the rejection score) and the
        posterior of ``text`` given that a sentence of the grammar was said (``DanSpeechRecognizer.grammar_confidence_batch``)."""
        return self.danspeech_recognizer.grammar_confidence_batch(audio_list, grammar)

    def grammar_confidence(self, audio_data, grammar):
        """``grammar_confidence_batch`` of one clip."""
        return self.danspeech_recognizer.grammar_confidence(audio_data, grammar)

    def align_flexible(self, audio_data, grammar_text):
        """``align`` for a transcript that is almost right: ``grammar_text`` is the transcript with alternatives ``(2 | to |
        toogtyve)`` and optional words ``[øh]`` (``danspeech_amd.grammar``).  ``(text, [(word, start_s, end_s, confidence),
        ...], path_logp, logp)`` with the variant that was spoken and its word timings, or ``None`` when no variant fits."""
        return self.danspeech_recognizer.transcribe_grammar(audio_data, grammar_text)

    def find_phrases(self, audio_data, phrases, max_hits=5, min_confidence=0.0):
        """Where in the clip each of ``phrases`` is spoken: per phrase a list of ``(start_s, end_s, confidence, logp)``, best
        first (``DanSpeechRecognizer.find_phrases_batch``)."""
        return self.danspeech_recognizer.find_phrases(audio_data, phrases, max_hits, min_confidence)

    def find_phrases_batch(self, audio_list, phrases, max_hits=5, min_confidence=0.0):
        """``find_phrases`` for a list of clips in one batched pass over the GPU; ``result[i][k]`` for clip i and phrase k."""
        return self.danspeech_recognizer.find_phrases_batch(audio_list, phrases, max_hits, min_confidence)

    def score(self, audio_data, candidates):
        """How probable is each of ``candidates`` as the transcript of ``audio_data``: per candidate ``(text, logp, confidence,
        share)``, or ``None`` when it cannot fit the audio (``DanSpeechRecognizer.score_batch``)."""
        return self.danspeech_recognizer.score(audio_data, candidates)

    def score_batch(self, audio_list, candidates):
        """``score`` for a list of clips in one batched pass over the GPU; ``result[i][k]`` for clip i and ``candidates[i][k]``."""
        return self.danspeech_recognizer.score_batch(audio_list, candidates)

    def recognize_scored(self, audio_list, n_best=1):
        """``recognize_batch`` with the exact likelihood of each recognised text: per clip ``[(text, logp), ...]``, the
        decoder's first ``n_best`` hypotheses (``DanSpeechRecognizer.transcribe_scored_batch``)."""
        return self.danspeech_recognizer.transcribe_scored_batch(audio_list, n_best=n_best)

    def recognize_min_risk(self, audio_list, n_best=8, unit="word"):
        """``recognize_scored`` in minimum-Bayes-risk order: per clip ``[(text, risk, logp), ...]``, the decoder's first
        ``n_best`` hypotheses by ascending expected ``unit`` ("word" or "char") errors under the acoustic posteriors of the
        list (``DanSpeechRecognizer.transcribe_min_risk_batch``)."""
        return self.danspeech_recognizer.transcribe_min_risk_batch(audio_list, n_best=n_best, unit=unit)

    def recognize_rescored(self, audio_list, n_best=8, alpha=None, beta=None):
        """``recognize_scored`` rescored with the language model: per clip ``[(text, total, logp), ...]``, the decoder's first
        ``n_best`` hypotheses by descending ``total = logp + alpha * lm + beta * n_words`` (``alpha`` / ``beta`` None: the
        decoder's own; ``DanSpeechRecognizer.transcribe_rescored_batch``)."""
        return self.danspeech_recognizer.transcribe_rescored_batch(audio_list, n_best=n_best, alpha=alpha, beta=beta)

    def tune_lm(self, audio_list, transcripts, alphas, betas, n_best=8, unit="word"):
        """Tune the language-model weights on clips with known transcripts: the errors of every (alpha, beta) of the grid when
        the n-best lists of ONE search are rescored with it, and the best pair (``BeamCTCDecoder.tune_lm_weights``)."""
        return self.danspeech_recognizer.tune_lm_batch(audio_list, transcripts, alphas, betas, n_best=n_best, unit=unit)

    def evaluate(self, audio_list, transcripts):
        """Recognise the clips and compare with their known transcripts: a dict of ``texts``, the corpus ``wer`` and ``cer``,
        ``word_counts`` / ``char_counts`` (per clip: distance, substitutions, deletions, insertions) and ``word_ref_lens`` /
        ``char_ref_lens`` (``DanSpeechRecognizer.evaluate_batch``)."""
        return self.danspeech_recognizer.evaluate_batch(audio_list, transcripts)

    def confidence(self, audio_data, transcript):
        """How sure the model is of each word and character of a transcript of ``audio_data``: ``(words, chars)`` with
        ``words = [(word, confidence), ...]`` and ``chars = [(char, confidence, alternative, alternative_confidence), ...]``,
        or ``None`` when the transcript cannot fit the audio (``DanSpeechRecognizer.confidence_batch``)."""
        return self.danspeech_recognizer.confidence(audio_data, transcript)

    def confidence_batch(self, audio_list, transcripts):
        """``confidence`` for a list of clips in one batched pass over the GPU; results in the caller's order."""
        return self.danspeech_recognizer.confidence_batch(audio_list, transcripts)

    def recognize_confident(self, audio_list):
        """``recognize_batch`` with the confidence of each recognised text: per clip ``(text, words, chars)``
        (``DanSpeechRecognizer.transcribe_confident_batch``)."""
        return self.danspeech_recognizer.transcribe_confident_batch(audio_list)

    def soft_align(self, audio_data, transcript):
        """Soft timings of a transcript of ``audio_data``, over every alignment: ``(words, chars)`` with ``chars = [(char,
        centre_s, spread_s, dwell_s), ...]`` and ``words = [(word, first_centre_s, last_centre_s), ...]``, or ``None`` when
        the transcript cannot fit the audio (``DanSpeechRecognizer.soft_align_batch``)."""
        return self.danspeech_recognizer.soft_align(audio_data, transcript)

    def soft_align_batch(self, audio_list, transcripts):
        """``soft_align`` for a list of clips in one batched pass over the GPU; results in the caller's order."""
        return self.danspeech_recognizer.soft_align_batch(audio_list, transcripts)

    def recognize_batches(self, batches, show_all=False):
        """Generator: ``recognize_batch`` over a sequence of batches, with the upload of the next batch and the
        decoding of the previous one overlapped with the GPU's work on the current one."""
        return self.danspeech_recognizer.transcribe_batches(batches, show_all=show_all)

    def recognize_batch_distributed(self, audio_list):
        """``recognize_batch`` sharded over the ranks of an initialised ``torch.distributed`` job (one process per
        GPU, backend "nccl" = RCCL): rank 0 passes the clips and receives the transcriptions in its order, the
        other ranks pass ``None`` and receive ``None``.  Clips are dealt longest-first round-robin
        (``parallel.plan_shards``), int16/float32/float64 PCM travels in its own sample type."""
        import torch
        import torch.distributed as dist
        from . import parallel
        eng = self.danspeech_recognizer
        dev = torch.device("cuda", eng._device_index())
        return parallel.recognize_sharded(eng, audio_list, dist.get_rank(), dist.get_world_size(), dev)

    # ---- real-time streaming (Recognizer.py:499-720) without the microphone -----------------------------
    def enable_real_time_streaming(self, streaming_model, secondary_model=None, string_parts=True, lm_partials=False, watch=None,
                                   watch_confidence=0.5, watch_settle_s=0.5, grammar=None, grammar_partials=False, grammar_max_s=30.0):
        """Recognizer.py:499-533: switch to a unidirectional streaming model (e.g.
        ``pretrained_models.GPUStreamingRNN``), optionally with a secondary model for the final text.  ``lm_partials``
        (needs a language model): every middle output is the language-model decoder's best text of the whole utterance so
        far, from a beam search carried from part to part (``DanSpeechRecognizer.enable_streaming``).  ``watch``: phrases to
        listen for in every stream -- a name, a command, a wake word; ``stream_recording``, ``stream_recordings`` and
        ``stream_live`` then report each occurrence to their ``on_detection`` callback ``watch_settle_s`` seconds after it was
        said, when its per-frame confidence is at least ``watch_confidence`` (``DanSpeechRecognizer.enable_streaming``).
        ``grammar``: a ``Grammar`` or its text -- commands, digits, a closed vocabulary: every utterance of every stream is then
        also decoded live as a sentence of the grammar and reported to the ``on_command`` callback of the three calls; with
        ``grammar_partials`` the best sentence prefix so far after every part, too.  ``grammar_max_s``: the longest utterance
        the search holds (a longer one gets a warning and ``None``).  ``ValueError`` for a faulty grammar, before any GPU work."""
        self.update_model(streaming_model)
        self.danspeech_recognizer.enable_streaming(secondary_model, string_parts, lm_partials, watch=watch, watch_confidence=watch_confidence,
                                                   watch_settle_s=watch_settle_s, grammar=grammar, grammar_partials=grammar_partials,
                                                   grammar_max_s=grammar_max_s)
        self.stream = True

    def disable_real_time_streaming(self, keep_secondary_model_loaded=False):
        """Recognizer.py:535-558 (no microphone thread to stop here)."""
        if getattr(self, "stream", False):
            self.stream = False
            self.danspeech_recognizer.disable_streaming(keep_secondary_model=keep_secondary_model_loaded)
        else:
            print("No stream is running for the Recognizer")

    @staticmethod
    def _report(on_detection, index, session, on_command=None):
        """Hand the detections and the grammar's results that wait on ``session`` to the callbacks (without one they are dropped)."""
        for ordinal, phrase, start_s, end_s, confidence, logp in session.take_detections():
            if on_detection is not None:
                on_detection(index, ordinal, phrase, start_s, end_s, confidence, logp)
        for item in session.take_commands():
            if on_command is not None:
                on_command(index, *item)

    def stream_recording(self, audio_data, chunk_samples=None, sample_rate=None, resample="polyphase", on_detection=None, on_command=None):
        """The body of ``real_time_streaming`` (Recognizer.py:560-710) driven by an array instead of the
        microphone thread: the utterance is cut with the reference's sample requirements (first pass
        ``general + 15 * samples_pr_10ms``, later passes ``general``, :598-612; ``chunk_samples`` is the size
        of the parts the source would deliver), every part goes through
        ``DanSpeechRecognizer.streaming_transcribe`` and ``(is_last, text)`` is yielded for every non-empty
        output.  Requires ``enable_real_time_streaming``.
        ``sample_rate``: the recording's rate when it is not the model's.  It is converted on the GPU as it streams
        (``resample``: "polyphase" or "ratecv"): the passes are cut over the converted length (``chunk_samples`` counts
        model-rate samples) and the source is fed just far enough for each pass (``stream_plan.resample_feed_plan``), so that
        the yields equal ``stream_recording(audio.resample(audio_data, sample_rate, method=resample), chunk_samples)``.
        ``on_detection``: with a phrase watch (``enable_real_time_streaming(watch=...)``), called as ``on_detection(index,
        utterance_ordinal, phrase, start_s, end_s, confidence, logp)`` for every occurrence, before the part's text is yielded
        (``index`` is 0 here); what is yielded is the same with and without it.
        ``on_command``: with a grammar (``enable_real_time_streaming(grammar=...)``), called as ``on_command(index,
        utterance_ordinal, is_final, result)`` with what ``take_commands()`` holds, before the part's text is yielded."""
        if not getattr(self, "stream", False):
            raise RuntimeError("call enable_real_time_streaming(streaming_model) first")
        rec = self.danspeech_recognizer
        if not self._other_rate(sample_rate):
            audio_data = np.asarray(audio_data, dtype=np.float64)
            for lo, hi, is_first, is_last in self._cut_plan(len(audio_data), chunk_samples):
                output = rec.streaming_transcribe(audio_data[lo:hi], is_last=is_last, is_first=is_first)
                self._report(on_detection, 0, rec, on_command)
                if output:
                    yield is_last, output
            return
        audio_data = np.asarray(audio_data).reshape(-1)
        plan, feed = self._feed_plan(len(audio_data), chunk_samples, sample_rate, resample)
        before = rec._session.source
        rec.set_streaming_source(sample_rate, resample)
        try:
            for (lo, hi, is_first, is_last), (a, b, flush) in zip(plan, feed):
                output = rec.streaming_transcribe(audio_data[a:b], is_last=is_last, is_first=is_first, take=hi - lo, flush=flush)
                self._report(on_detection, 0, rec, on_command)
                if output:
                    yield is_last, output
        finally:
            rec.set_streaming_source(*(before or (None, "polyphase")))

    def stream_recordings(self, audio_list, chunk_samples=None, sample_rate=None, resample="polyphase", on_detection=None, on_command=None):
        """``stream_recording`` for many recordings at once, one streaming session each: every recording is cut as
        ``stream_recording`` cuts it, and in each round every session that has a part due advances in ONE batched pass
        (``DanSpeechRecognizer.streaming_transcribe_many``).  Yields ``(index, is_last, text)``; for every index the
        subsequence it yields equals ``list(stream_recording(audio_list[index], chunk_samples))`` as the first recording
        after ``enable_real_time_streaming`` (every session starts with a fresh parser).  Requires
        ``enable_real_time_streaming``.
        ``sample_rate``: the recordings' rate, or a list with one rate per recording (None among them: the model's); the
        sessions of other rates are converted together, one launch per round and method (``stream_recording``).
        ``on_detection`` and ``on_command``: as ``stream_recording``'s, ``index`` the recording's; a round's detections and
        commands are reported before the round's texts are yielded."""
        if not getattr(self, "stream", False):
            raise RuntimeError("call enable_real_time_streaming(streaming_model) first")
        rec = self.danspeech_recognizer
        rates = list(sample_rate) if isinstance(sample_rate, (list, tuple)) else [sample_rate] * len(audio_list)
        if len(rates) != len(audio_list):
            raise ValueError("sample_rate must be one rate or one rate per recording")
        rates = [r if self._other_rate(r) else None for r in rates]
        audio = [np.asarray(a, dtype=np.float64) if r is None else np.asarray(a).reshape(-1) for a, r in zip(audio_list, rates)]
        plans, feeds = [], []
        for a, r in zip(audio, rates):
            if r is None:
                plans.append(self._cut_plan(len(a), chunk_samples))
                feeds.append([(lo, hi, is_last) for lo, hi, _, is_last in plans[-1]])
            else:
                plan, feed = self._feed_plan(len(a), chunk_samples, r, resample)
                plans.append(plan)
                feeds.append(feed)
        sessions = {}
        try:
            for r, due in enumerate(stream_rounds(plans)):
                for k, _ in due:
                    if k not in sessions:
                        sessions[k] = rec.new_streaming_session(sample_rate=rates[k], resample=resample)
                texts = rec.streaming_transcribe_many([sessions[k] for k, _ in due], [audio[k][feeds[k][r][0]:feeds[k][r][1]] for k, _ in due],
                                                      [c[3] for _, c in due], [c[2] for _, c in due],
                                                      take=[c[1] - c[0] for _, c in due], flush=[feeds[k][r][2] for k, _ in due])
                for k, _ in due:
                    self._report(on_detection, k, sessions[k], on_command)
                for (k, c), text in zip(due, texts):
                    if text:
                        yield k, c[3], text
        finally:
            for ses in sessions.values():
                ses.close()

    def stream_live(self, sources, chunk=1024, sample_rate=None, resample="polyphase", on_detection=None, on_command=None):
        """Continuous audio from many sources -> per-utterance texts: ``real_time_streaming`` (Recognizer.py:560-715) for every
        source at once, with the listener's gate (``listen_stream``, :218-324), the conversion to the model's rate and the
        model passes all on the GPU.  ``sources``: a list of iterables of sample arrays of any lengths (int16 -- ``[n, 2]``
        for two channels --, float32 or float64; a source's first array fixes its type).  Each round takes the next array of
        every source that still has one; a source that is exhausted ends its stream.  Yields ``(index, is_last, text)`` until
        every source is exhausted.  ``chunk``: the gate's buffer; ``sample_rate``: the sources' rate, or one per source, when it
        is not the model's (``resample`` must be "polyphase").  The gate's parameters are this recognizer's
        ``energy_threshold``, ``pause_threshold``, ``phrase_threshold`` and ``non_speaking_duration`` as they are when a source
        delivers its first array.  Requires ``enable_real_time_streaming``.  ``on_detection``: as ``stream_recording``'s, ``index``
        the source's and ``utterance_ordinal`` counting the utterances the gate has found in it; a round's detections are
        reported before the round's texts are yielded.  ``on_command``: as ``stream_recording``'s, in the same place."""
        if not getattr(self, "stream", False):
            raise RuntimeError("call enable_real_time_streaming(streaming_model) first")
        if resample != "polyphase":
            raise ValueError("resample='%s' cannot follow the gate (it hands on float64 samples): use 'polyphase'" % (resample,))
        rec = self.danspeech_recognizer
        rates = list(sample_rate) if isinstance(sample_rate, (list, tuple)) else [sample_rate] * len(sources)
        if len(rates) != len(sources):
            raise ValueError("sample_rate must be one rate or one rate per source")
        its = [iter(s) for s in sources]
        live, sessions = set(range(len(its))), {}
        try:
            while live:
                ks, parts, eos = [], [], []
                for k in sorted(live):
                    try:
                        part = np.asarray(next(its[k]))
                    except StopIteration:
                        live.discard(k)
                        if k in sessions:
                            ks.append(k); parts.append(None); eos.append(True)
                        continue
                    if k not in sessions:
                        if part.dtype not in (np.int16, np.float32, np.float64):
                            part = part.astype(np.float64)
                        sessions[k] = rec.new_live_session(chunk, rates[k], resample, self.energy_threshold, self.pause_threshold,
                                                           self.phrase_threshold, self.non_speaking_duration, dtype=part.dtype,
                                                           channels=2 if part.ndim == 2 else 1)
                    ks.append(k); parts.append(part); eos.append(False)
                if not ks:
                    continue
                heard = rec.streaming_listen_many([sessions[k] for k in ks], parts, eos)
                for k in ks:
                    self._report(on_detection, k, sessions[k], on_command)
                for k, said in zip(ks, heard):
                    for is_last, text in said:
                        yield k, is_last, text
        finally:
            for ses in sessions.values():
                ses.close()

    # ---- the live gate (Recognizer.py:218-324, :717-818): its parameters, and the two ways the reference tunes the threshold
    def update_stream_parameters(self, energy_threshold=None, pause_threshold=None, phrase_threshold=None, non_speaing_duration=None):
        """Recognizer.py:800-818, its misspelt keyword included."""
        if energy_threshold:
            self.energy_threshold = energy_threshold
        if pause_threshold:
            self.pause_threshold = pause_threshold
        if phrase_threshold:
            self.phrase_threshold = phrase_threshold
        if non_speaing_duration:
            self.non_speaking_duration = non_speaing_duration

    def new_endpointer(self, chunk=1024, sample_rate=None, dtype=np.int16, channels=1):
        """A ``NativeEndpointer`` (``dsmi_endpointer``: the gate of ``listen_stream`` over one live stream, on the GPU) with this
        recognizer's gate parameters as they are now, on the frontend of the engine's parser (``sample_rate``: the stream's
        rate when it is not the model's)."""
        from . import _native
        if not self.pause_threshold >= self.non_speaking_duration >= 0:
            raise ValueError("the gate needs pause_threshold >= non_speaking_duration >= 0 (Recognizer.py:237)")
        parser = self.danspeech_recognizer.audio_parser
        if parser is not None:
            frontend, model_rate = parser._frontend(), parser.sampling_rate
        else:                               # no model yet: the gate needs none (the reference tunes its threshold before loading one)
            if getattr(self, "_gate_frontend", None) is None:
                self._gate_frontend = _native.NativeFrontend()
            frontend, model_rate = self._gate_frontend, 16000
        rate = int(model_rate if sample_rate is None else sample_rate)
        return _native.NativeEndpointer(frontend, chunk, rate, self.energy_threshold, self.pause_threshold, self.phrase_threshold,
                                        self.non_speaking_duration, dtype=dtype, channels=channels)

    def _buffer_energies(self, audio, duration, chunk, sample_rate):
        """``audioop.rms`` of the buffers of ``chunk`` samples the reference would read within ``duration`` seconds
        (:742-749: while the time elapsed, this buffer included, does not exceed it) -- the ``energies_host`` of one push."""
        import torch
        audio = np.asarray(audio)
        if audio.dtype not in (np.int16, np.float32, np.float64):
            audio = audio.astype(np.float64)
        if not torch.cuda.is_available():
            raise RuntimeError("the gate runs on the GPU")
        if audio.ndim == 2 and audio.dtype != np.int16:
            raise ValueError("two channels ([n, 2]) are taken as int16 frames only; fold float audio to one channel first")
        if audio.ndim > 2 or (audio.ndim == 2 and audio.shape[1] != 2):
            raise ValueError("audio must be [n] samples or [n, 2] int16 frames")
        ep = self.new_endpointer(chunk, sample_rate, dtype=audio.dtype, channels=2 if audio.ndim == 2 else 1)
        try:
            seconds_per_buffer = (chunk + 0.0) / ep.rate
            elapsed_time, n = 0, 0
            while True:
                elapsed_time += seconds_per_buffer
                if elapsed_time > duration or (n + 1) * chunk > len(audio):
                    break
                n += 1
            if n == 0:
                raise ValueError("audio holds less than one whole buffer of %d samples within %r s" % (chunk, duration))
            pcm = torch.from_numpy(np.ascontiguousarray(audio[:n * chunk])).to("cuda:%d" % ep.frontend.device)
            return [int(e) for e in ep.push(pcm, return_energies=True)[1]], seconds_per_buffer
        finally:
            ep.close()

    def adjust_for_speech(self, audio, duration=4, chunk=1024, sample_rate=None):
        """Recognizer.py:717-757 over an array holding speech: the threshold becomes the mean buffer energy, less 80 when it is
        above 80.  Only whole buffers of ``audio`` count."""
        energy_levels, _ = self._buffer_energies(audio, duration, chunk, sample_rate)
        energy_average = sum(energy_levels) / len(energy_levels)
        self.energy_threshold = energy_average - 80 if energy_average > 80 else energy_average

    def adjust_for_ambient_noise(self, audio, duration=2, chunk=1024, sample_rate=None):
        """Recognizer.py:759-797 over an array holding background noise: the damped average towards
        ``dynamic_energy_ratio`` times each buffer's energy."""
        energy_levels, seconds_per_buffer = self._buffer_energies(audio, duration, chunk, sample_rate)
        for energy in energy_levels:
            damping = self.dynamic_energy_adjustment_damping ** seconds_per_buffer
            target_energy = energy * self.dynamic_energy_ratio
            self.energy_threshold = self.energy_threshold * damping + target_energy * (1 - damping)

    def _other_rate(self, sample_rate):
        return sample_rate is not None and int(sample_rate) != int(self.danspeech_recognizer.audio_parser.sampling_rate)

    def _feed_plan(self, n_source, chunk_samples, sample_rate, resample):
        """The passes over the converted length and what of the source each of them is fed."""
        rate_out = int(self.danspeech_recognizer.audio_parser.sampling_rate)
        plan = self._cut_plan(resample_count(n_source, sample_rate, rate_out, resample), chunk_samples)
        return plan, resample_feed_plan(plan, n_source, sample_rate, rate_out, resample)

    def _cut_plan(self, n_samples, chunk_samples=None):
        rec = self.danspeech_recognizer
        return stream_cut_plan(n_samples, chunk_samples, rec.model.context, int(rec.audio_parser.sampling_rate / 100))

    def recognize_long(self, audio_data, energy_threshold=600, step=1024, pause_threshold=0.55, phrase_threshold=0.2,
                       max_batch=32, show_all=False, sample_rate=None, resample="polyphase"):
        """Segment a long recording with the reference example's energy gate
        (example_scripts/video_transcribe_simulation.py:68-143) and transcribe the phrases in batches:
        ``[(start_sample, end_sample, transcription), ...]`` in time order.  ``sample_rate``: the recording's rate when it is
        not the model's 16 kHz (a video sound track); it is converted once on the GPU (``resample``), the gate runs on the
        converted signal, and ``start_sample`` / ``end_sample`` count 16 kHz samples."""
        return self.danspeech_recognizer.transcribe_long(audio_data, energy_threshold=energy_threshold, step=step,
                                                         pause_threshold=pause_threshold, phrase_threshold=phrase_threshold,
                                                         max_batch=max_batch, show_all=show_all, sample_rate=sample_rate,
                                                         resample=resample)

    def align_long(self, audio_data, sentences, energy_threshold=600, step=1024, pause_threshold=0.55, phrase_threshold=0.2,
                   max_batch=32, sample_rate=None, resample="polyphase", window=30):
        """Sentence and word timings of a long recording with its transcript, cut into phrases as ``recognize_long`` cuts it:
        per sentence ``(start_s, end_s, confidence, [(word, start_s, end_s, confidence), ...])``, or ``None`` when the transcript
        cannot fit the recording (``DanSpeechRecognizer.align_long``)."""
        return self.danspeech_recognizer.align_long(audio_data, sentences, energy_threshold=energy_threshold, step=step,
                                                    pause_threshold=pause_threshold, phrase_threshold=phrase_threshold,
                                                    max_batch=max_batch, sample_rate=sample_rate, resample=resample, window=window)

    def recognize_files(self, paths, show_all=False, resample=None):
        """``[recognize(load_audio(p)) for p in paths]`` in batched passes, WAV decoding on the GPU.  ``resample``: None takes
        every file as 16 kHz audio (``load_audio``'s contract); "polyphase" or "ratecv" reads each file's frame rate and
        converts the files of another rate to 16 kHz on the GPU."""
        return self.danspeech_recognizer.transcribe_files(paths, show_all=show_all, resample=resample)

    def update_model(self, model):
        self.danspeech_recognizer.update_model(model)
        print("DanSpeech model updated to: {0}".format(model.model_name))

    def update_decoder(self, lm=None, alpha=None, beta=None, beam_width=None):
        self.danspeech_recognizer.update_decoder(lm=lm, alpha=alpha, beta=beta, beam_width=beam_width)
        print("DanSpeech decoder updated ")  # ToDO: Include model name

