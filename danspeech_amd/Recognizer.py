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
    def enable_real_time_streaming(self, streaming_model, secondary_model=None, string_parts=True, lm_partials=False):
        """Recognizer.py:499-533: switch to a unidirectional streaming model (e.g.
        ``pretrained_models.GPUStreamingRNN``), optionally with a secondary model for the final text.  ``lm_partials``
        (needs a language model): every middle output is the language-model decoder's best text of the whole utterance so
        far, from a beam search carried from part to part (``DanSpeechRecognizer.enable_streaming``)."""
        self.update_model(streaming_model)
        self.danspeech_recognizer.enable_streaming(secondary_model, string_parts, lm_partials)
        self.stream = True

    def disable_real_time_streaming(self, keep_secondary_model_loaded=False):
        """Recognizer.py:535-558 (no microphone thread to stop here)."""
        if getattr(self, "stream", False):
            self.stream = False
            self.danspeech_recognizer.disable_streaming(keep_secondary_model=keep_secondary_model_loaded)
        else:
            print("No stream is running for the Recognizer")

    def stream_recording(self, audio_data, chunk_samples=None, sample_rate=None, resample="polyphase"):
        """The body of ``real_time_streaming`` (Recognizer.py:560-710) driven by an array instead of the
        microphone thread: the utterance is cut with the reference's sample requirements (first pass
        ``general + 15 * samples_pr_10ms``, later passes ``general``, :598-612; ``chunk_samples`` is the size
        of the parts the source would deliver), every part goes through
        ``DanSpeechRecognizer.streaming_transcribe`` and ``(is_last, text)`` is yielded for every non-empty
        output.  Requires ``enable_real_time_streaming``.
        ``sample_rate``: the recording's rate when it is not the model's.  It is converted on the GPU as it streams
        (``resample``: "polyphase" or "ratecv"): the passes are cut over the converted length (``chunk_samples`` counts
        model-rate samples) and the source is fed just far enough for each pass (``stream_plan.resample_feed_plan``), so that
        the yields equal ``stream_recording(audio.resample(audio_data, sample_rate, method=resample), chunk_samples)``."""
        if not getattr(self, "stream", False):
            raise RuntimeError("call enable_real_time_streaming(streaming_model) first")
        rec = self.danspeech_recognizer
        if not self._other_rate(sample_rate):
            audio_data = np.asarray(audio_data, dtype=np.float64)
            for lo, hi, is_first, is_last in self._cut_plan(len(audio_data), chunk_samples):
                output = rec.streaming_transcribe(audio_data[lo:hi], is_last=is_last, is_first=is_first)
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
                if output:
                    yield is_last, output
        finally:
            rec.set_streaming_source(*(before or (None, "polyphase")))

    def stream_recordings(self, audio_list, chunk_samples=None, sample_rate=None, resample="polyphase"):
        """``stream_recording`` for many recordings at once, one streaming session each: every recording is cut as
        ``stream_recording`` cuts it, and in each round every session that has a part due advances in ONE batched pass
        (``DanSpeechRecognizer.streaming_transcribe_many``).  Yields ``(index, is_last, text)``; for every index the
        subsequence it yields equals ``list(stream_recording(audio_list[index], chunk_samples))`` as the first recording
        after ``enable_real_time_streaming`` (every session starts with a fresh parser).  Requires
        ``enable_real_time_streaming``.
        ``sample_rate``: the recordings' rate, or a list with one rate per recording (None among them: the model's); the
        sessions of other rates are converted together, one launch per round and method (``stream_recording``)."""
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
                for (k, c), text in zip(due, texts):
                    if text:
                        yield k, c[3], text
        finally:
            for ses in sessions.values():
                ses.close()

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

