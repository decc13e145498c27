"""The engine behind ``Recognizer`` (the role of reference danspeech/DanSpeechRecognizer.py): it owns the
device, the acoustic model, the audio parser and the CTC decoder, and turns recordings into text.

Behaviour kept from the reference, because callers and the parity tests rely on it:

* constructor arguments and defaults (``alpha=1.3, beta=0.2, beam_width=64``, DanSpeechRecognizer.py:16-17), the
  ``Using device:`` line, ``ModelNotInitialized`` when a language model is given without a model (:36-38);
* ``update_decoder``: only truthy arguments that differ from the current setting count as a change, the decoder object
  is rebuilt only on a change, the very first call selects greedy decoding (:58-95); the beam decoder is created with
  ``num_processes=6, cutoff_prob=1.0, cutoff_top_n=40`` and the blank at ``labels.index('_')`` (:89-94);
* ``transcribe``: one recording -> best transcription, or every beam with ``show_all`` (with a
  ``NoLmInstantiatedWarning`` when there is no language model, :218-231);
* the chunked real-time protocol ``enable_streaming`` / ``streaming_transcribe`` / ``disable_streaming`` (:97-216).

What is new is batching: ``transcribe_batch`` runs many recordings as ONE padded batch, and ``transcribe_batches``
keeps one batch in flight on the GPU while the next one is staged and uploaded and the previous one is decoded.
Everything numeric runs in libdsmi.so on the MI355X; ``with_gpu`` is accepted for signature compatibility only.
"""
import warnings

import os
import numpy as np

from .deepspeech.decoder import GreedyDecoder, BeamCTCDecoder
from .errors.recognizer_errors import ModelNotInitialized
from .audio.parsers import SpectrogramAudioParser, InferenceSpectrogramAudioParser, DeviceClips, StagedClips
from . import batch_plan


class NoLmInstantiatedWarning(Warning):
    pass


# decoder settings update_decoder can change, in the order the reference examines them
_DECODER_SETTINGS = ("lm", "alpha", "beta", "labels", "beam_width")


class _StreamingSession(object):
    """Running state of one utterance that arrives in parts (reference DanSpeechRecognizer.py:97-216): the text so
    far, the model outputs of every part (for a final pass of the language-model decoder) and, when a secondary
    model gives the final text, the spectrograms of every part.  With ``lm_partials`` also the utterance's beam search,
    carried from part to part (a ``NativeBeamStream`` of ``beam_decoder``), and its best text after the last part.  A session
    whose source has another rate than the model's owns a ``NativeResampler`` (``resampler``; ``source`` = (rate, method)); the
    converted samples that a pass did not take wait in ``pending`` (a float64 CUDA tensor).  With ``watching`` (a phrase watch,
    ``enable_streaming(watch=...)``) also the utterance's phrase search, carried from part to part (``spot``, a
    ``NativeSpotStream``), the detections nobody has taken yet and the ordinal of the utterance under way.  With ``commanding`` (a
    grammar, ``enable_streaming(grammar=...)``) the utterance's graph search, carried from part to part (``command``, a
    ``NativeGrammarStream``), the commands nobody has taken yet, the ordinal of the utterance it is on and whether that utterance
    has outgrown the search's frames."""

    def __init__(self, secondary_model, string_parts, lm_partials=False, watching=False, commanding=False):
        self.secondary_model = secondary_model
        self.string_parts = string_parts
        self.lm_partials = lm_partials
        self.watching = watching
        self.spot = None
        self.detections = []
        self.utterance = 0
        self.commanding = commanding
        self.command = None
        self.commands = []
        self.command_utterance = 0
        self.command_overrun = False
        self.beam = None
        self.beam_decoder = None
        self.resampler = None
        self.source = None
        self.clear()

    def clear(self):
        self.text = ""
        self.outputs = []
        self.spectrograms = []
        self.beam_text = None
        self.pending = None
        if self.beam is not None:
            self.beam.reset()
        if self.spot is not None:
            self.spot.reset()
        if self.command is not None:
            self.command.reset()
        self.command_overrun = False
        if self.resampler is not None:
            self.resampler.reset()

    def take_detections(self):
        """The phrase watch's detections since the last call, in firing order: ``(utterance_ordinal, phrase, start_s, end_s,
        confidence, logp)``, seconds from the utterance's first output frame."""
        found, self.detections = self.detections, []
        return found

    def take_commands(self):
        """The grammar's results since the last call, in order: partials ``(utterance_ordinal, False, (text, complete))`` --
        the best sentence prefix so far and whether the grammar accepts it as it stands -- and per utterance one final
        ``(utterance_ordinal, True, None | (text, [(word, start_s, end_s, confidence), ...], path_logp))``, ``None`` when no
        sentence of the grammar fits the utterance (or it outgrew ``grammar_max_s``)."""
        found, self.commands = self.commands, []
        return found

    def set_source(self, parser, sample_rate, resample):
        """The rate of the parts to come (None, or the model's own rate: they are taken as they are) and how to convert;
        ``parser``: the streaming parser whose frontend the resampler belongs to."""
        from . import _native
        if resample not in _native.RESAMPLE_METHODS:
            raise ValueError("resample method must be one of %s" % sorted(_native.RESAMPLE_METHODS))
        source = None if sample_rate is None or int(sample_rate) == int(parser.sampling_rate) else (int(sample_rate), resample)
        if source == self.source:
            return
        if self.resampler is not None:
            self.resampler.close()
        self.resampler, self.source, self.pending = None, source, None
        if source is not None:
            # ratecv works on integers of a sample width: int16, as everywhere in the package; the polyphase filter takes float64,
            # which holds int16 / float32 sources exactly
            self.resampler = _native.NativeResampler(parser._frontend(), source[0], resample, dtype=np.int16 if resample == "ratecv" else np.float64)

    def close(self):
        if self.beam is not None:
            self.beam.close()
            self.beam = None
        if self.spot is not None:
            self.spot.close()
            self.spot = None
        if self.command is not None:
            self.command.close()
            self.command = None
        if self.resampler is not None:
            self.resampler.close()
            self.resampler = None

    def extend_text(self, piece):
        """Append a part's greedy text; a part that starts with the character the text ends with continues that
        character (CTC collapse across the part boundary).  Returns what this part contributed."""
        if self.text and piece and self.text[-1] == piece[0]:
            piece = piece[1:]
        self.text += piece
        return piece


class LiveSessionHandle:
    """One live source of ``streaming_listen_many``: its gate (``NativeEndpointer``), the polyphase resampler behind the gate when
    the source's rate is not the model's, the pass rule (``stream_plan.LivePasses``) and a streaming session of its own."""

    def __init__(self, endpointer, resampler, passes, session, dtype):
        self.endpointer, self.resampler, self.passes, self.session, self.dtype = endpointer, resampler, passes, session, dtype

    def take_detections(self):
        return self.session.take_detections()

    def take_commands(self):
        return self.session.take_commands()

    def close(self):
        self.endpointer.close()
        if self.resampler is not None:
            self.resampler.close()
        self.session.close()


class StreamingSessionHandle(object):
    """One utterance of ``DanSpeechRecognizer.streaming_transcribe_many``: its streaming parser, its ``dsmi_stream`` handle
    (conv contexts, recurrent state, lookahead buffer on the GPU) and its running text / outputs / spectrograms."""

    def __init__(self, parser, stream, state):
        self.parser = parser
        self.stream = stream
        self.state = state

    text = property(lambda self: self.state.text)

    def take_detections(self):
        return self.state.take_detections()

    def take_commands(self):
        return self.state.take_commands()

    def close(self):
        self.stream.close()
        self.state.close()


class _UnmergedDeviceClips(object):
    """Device-resident batches on their way into one forward: merged on the stream that runs it."""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return sum(len(b) for b in self.batches)


class _BatchJob(object):
    """One batch between enqueue and decode."""
    __slots__ = ("order", "probs", "sizes", "count", "model", "ticket", "slot", "collected", "recomputed")

    def __init__(self, order, probs, sizes, count, model):
        self.order, self.probs, self.sizes, self.count, self.model = order, probs, sizes, count, model
        self.ticket = None                       # a beam search launched behind the forward (transcribe_batches)
        self.slot = 0                            # the decoder handle that search occupies
        self.collected = self.recomputed = False # the forward has been waited for (model.collect) / had to be redone

    def collect_forward(self):
        if not self.collected:
            self.recomputed = self.model.collect()
            self.collected = True
        return self.recomputed


def _words(text, spans, token_probs, frame_s):
    """Characters of ``text`` with their frame spans and mean probabilities -> ``[(word, start_s, end_s, confidence)]``, a
    word being a maximal run of non-space characters."""
    words, k = [], 0
    while k < len(text):
        if text[k] == " ":
            k += 1
            continue
        j = k
        while j < len(text) and text[j] != " ":
            j += 1
        words.append((text[k:j], int(spans[k][0]) * frame_s, int(spans[j - 1][1]) * frame_s, float(np.mean(token_probs[k:j]))))
        k = j
    return words


def _confidences(chars, ids, post, labels, blank):
    """Characters ``chars`` with label ids ``ids`` and their slot posteriors ``post`` [L, C] (``Decoder.confidence_ids``) ->
    ``(words, char_rows)``: ``char_rows[k] = (char, confidence, alternative, alternative_confidence)``, the alternative being
    the most probable other label of the slot ('' for no character there), and ``words = [(word, confidence)]``, a word
    being a maximal run of non-space characters and its confidence the least of its characters'."""
    rows = []
    for k, ch in enumerate(chars):
        others = post[k].copy()
        others[int(ids[k])] = -1.0
        c = int(np.argmax(others))
        rows.append((ch, float(post[k, int(ids[k])]), "" if c == blank else labels[c], float(post[k, c])))
    words, k = [], 0
    while k < len(chars):
        if chars[k] == " ":
            k += 1
            continue
        j = k
        while j < len(chars) and chars[j] != " ":
            j += 1
        words.append(("".join(chars[k:j]), min(r[1] for r in rows[k:j])))
        k = j
    return words, rows


def _packed_upload(chunks, device):
    """uint8 arrays -> (one uint8 tensor on ``device`` that holds them all, where each starts): one host buffer of at least 8
    bytes in which every chunk starts on 8 bytes, one copy to the device."""
    import torch
    offs, size = [], 0
    for a in chunks:
        offs.append(size)
        size += (len(a) + 7) & ~7
    host = np.zeros(max(size, 8), dtype=np.uint8)
    for a, o in zip(chunks, offs):
        host[o:o + len(a)] = a
    return torch.from_numpy(host).to(device), offs


_SIDE_STREAMS = {}        # (name, device index) -> torch.cuda.Stream, shared by every engine of the process: see _side_stream


class DanSpeechRecognizer(object):

    def __init__(self, model_name=None, lm_name=None, alpha=1.3, beta=0.2, with_gpu=False, beam_width=64):
        import torch
        from . import _native
        _native.want_hw_queues(8)          # one hardware queue per stream of the batch pipeline, if the runtime can still be told
        self.device = torch.device("cuda")
        print("Using device: {0}".format(self.device))
        self.lm = None
        self.decoder = None
        self.alpha, self.beta, self.beam_width = alpha, beta, beam_width
        self.model = self.model_name = self.labels = self.audio_config = self.audio_parser = None
        self._session = None
        self._grammar_spec = self._grammar_net = None      # enable_streaming(grammar=...): (Grammar, partials, max frames), its NativeGrammarNet
        self._watch_spec = self._watch = None      # enable_streaming(watch=...): (phrases, ids, confidence, settle frames), its NativeSpotWatch
        self._side_streams = {}
        self._replicas = []
        if model_name:
            self.update_model(model_name)
        if lm_name:
            if not self.model:
                raise ModelNotInitialized("Trying to initialize LM without also choosing a DanSpeech model.")
            self.update_decoder(lm_name)

    # ---- model / decoder lifecycle ----------------------------------------------------------------------------------
    def _device_index(self):
        name = str(self.model.device)
        return int(name.split(":")[1]) if ":" in name else 0

    def update_model(self, model):
        self.audio_config = model.audio_conf
        self.model = model.to(self.device)
        self.model.eval()
        self._replicas = []
        self.audio_parser = SpectrogramAudioParser(self.audio_config, device=self._device_index())
        # a new model may bring a new alphabet: the decoder follows
        self.update_decoder(labels=self.model.labels)

    def _build_decoder(self):
        blank = self.labels.index("_")
        if self.lm == "greedy":
            return GreedyDecoder(labels=self.labels, blank_index=blank)
        return BeamCTCDecoder(labels=self.labels, lm_path=self.lm, alpha=self.alpha, beta=self.beta,
                              beam_width=self.beam_width, num_processes=6, cutoff_prob=1.0, cutoff_top_n=40,
                              blank_index=blank)

    def update_decoder(self, lm=None, alpha=None, beta=None, labels=None, beam_width=None):
        requested = dict(lm=lm, alpha=alpha, beta=beta, labels=labels, beam_width=beam_width)
        stale = not self.lm and not self.decoder
        if stale:
            self.lm = "greedy"
        for name in _DECODER_SETTINGS:
            value = requested[name]
            if value and value != getattr(self, name):
                setattr(self, name, value)
                stale = True
        if stale:
            self.decoder = self._build_decoder()

    # ---- batches ----------------------------------------------------------------------------------------------------
    def _side_stream(self, name):
        """A HIP stream beside the compute stream ("lane k": the k-th forward in flight; "decode": the decoder of batch i runs
        while batch i + 1 computes).  ONE set per device for every engine of the process: the ROCm runtime deals each stream a
        process creates onto GPU_MAX_HW_QUEUES hardware queues in turn, so a second engine with streams of its own would find
        two of them on one queue as often as not, and those run one after the other (measured: config 5's share 113 ms per
        batch as the fourth engine of a process, 100 ms alone).  Engines are used one at a time; two used at once share the lanes."""
        import torch
        key = (name, self._device_index())
        if key not in _SIDE_STREAMS:
            _SIDE_STREAMS[key] = torch.cuda.Stream(device=key[1])
        self._side_streams[key] = _SIDE_STREAMS[key]
        return _SIDE_STREAMS[key]

    def _stage_batch(self, recordings, parser=None):
        """Host clips, longest first (pack_padded_sequence's order, reference model.py:117), copied to pinned memory and on
        their way to the device: (order, StagedClips).  Needs no model handle, so a pipeline calls it before it waits for one."""
        order = batch_plan.longest_first([len(r) for r in recordings])
        return order, (parser or self.audio_parser).stage([recordings[i] for i in order])

    def _enqueue_batch(self, recordings, model=None, parser=None, decode_slot=None, staged=None):
        """Stage + upload + spectrograms + forward of one batch, all asynchronous.  Clips run longest first
        (pack_padded_sequence's order, reference model.py:117)."""
        import torch
        model = model or self.model
        if isinstance(recordings, DeviceClips):             # already on the device, longest first
            order = getattr(recordings, "order", None)
            order = np.arange(len(recordings)) if order is None else order      # (a merged batch remembers where its clips came from)
            # the clips were produced on whatever stream was current when the batch was handed over (an RCCL scatter, a widening
            # copy, a slicing kernel): the stream this batch runs on waits for that point, and the allocator learns of the use
            here = torch.cuda.current_stream(self._device_index())
            if isinstance(staged, torch.cuda.Event):
                here.wait_event(staged)
            recordings.pcm.record_stream(here)
            feats, frames = (parser or self.audio_parser).parse_batch(recordings)
        else:
            if staged is not None:
                order, clips = staged
            else:
                order = batch_plan.longest_first([len(r) for r in recordings])
                clips = [recordings[i] for i in order]
            feats, frames = (parser or self.audio_parser).parse_batch(clips)
        probs, sizes = model.enqueue(feats, torch.from_numpy(frames.astype(np.int32)))
        job = _BatchJob(order, probs, sizes, len(recordings), model)
        if decode_slot is not None and hasattr(self.decoder, "decode_enqueue"):
            job.slot = decode_slot
            if getattr(self.decoder, "on_lane", False):
                # greedy decoding: a short kernel and three small copies, queued right behind the forward on its own stream -- the
                # host never stands in a busy device's copy queue while the stream it should be feeding runs dry
                job.ticket = self.decoder.decode_enqueue(probs, sizes, slot=decode_slot)
            else:
                # the beam search is a kernel: launched now, behind this forward, on a stream of its own, so that the host
                # never waits for it while it could be feeding the next batch
                side = self._side_stream("decode")           # one decode stream for all slots: see audio/parsers.py on hardware queues
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(self._device_index()))
                side.wait_event(done)
                probs.record_stream(side)
                with torch.cuda.stream(side):
                    job.ticket = self.decoder.decode_enqueue(probs, sizes, slot=decode_slot)
        return job

    def _finish_batch(self, job, show_all, warn=True):
        import torch
        recomputed = job.collect_forward()       # waits for the forward; a timed-out batch has been recomputed by now
        side = self._side_stream("decode")
        job.probs.record_stream(side)
        decoded = None
        if getattr(job, "ticket", None) is not None:
            decoded, _ = self.decoder.decode_collect(job.ticket)      # the search launched behind the forward ...
            if recomputed:
                decoded = None                                         # ... read the probabilities of a forward that had to be redone
        if decoded is None:
            with torch.cuda.stream(side):
                if hasattr(self.decoder, "decode_enqueue"):
                    # on the job's OWN decoder handle: it is free again after the collect above, while handle 0 may hold the
                    # search of the batch enqueued after this one
                    decoded, _ = self.decoder.decode_collect(self.decoder.decode_enqueue(job.probs, job.sizes, slot=job.slot))
                else:
                    decoded, _ = self.decoder.decode(job.probs, job.sizes)
        if warn and show_all and self.lm == "greedy":
            warnings.warn("You are trying to get all beams but no LM has been instantiated.", NoLmInstantiatedWarning)
        if getattr(self, "keep_last_output", False):
            self.last_output = (job.probs, job.sizes)        # bench.py checks the timed batch's probabilities against the oracle
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            results[i] = decoded[pos] if show_all else decoded[pos][0]
        return results

    def transcribe_batch(self, recordings, show_all=False, sample_rate=None, resample="polyphase"):
        """``[transcribe(r) for r in recordings]`` as one batch; results in the caller's order.  ``sample_rate``: the rate of the
        recordings when it is not the model's; they are then converted on the device first (``dsmi_resample``, method
        ``resample``: "polyphase" or "ratecv") and never come back to the host in between."""
        if len(recordings) == 0:
            return []
        if sample_rate is not None and int(sample_rate) != int(self.audio_parser.sampling_rate) and not isinstance(recordings, DeviceClips):
            order = batch_plan.longest_first([len(r) for r in recordings])
            clips = self.audio_parser.resample_batch([recordings[i] for i in order], int(sample_rate), resample)
            clips.order = order
            return self._finish_batch(self._enqueue_batch(clips), show_all)
        return self._finish_batch(self._enqueue_batch(recordings), show_all)

    # how `transcribe_batches` fills the GPU: forwards in flight (each on a model handle, stream and persistent-kernel gate slot of
    # its own) and clips per forward (consecutive batches are merged up to this many: the recurrent kernel walks up to four
    # 16-clip tiles per workgroup, and its cost per clip falls with the tiles it walks)
    pipeline_lanes = 4
    pipeline_merge_clips = 64
    pipeline_balance_tail = True         # a sized source's last round of forwards is dealt evenly over the lanes (batch_plan.ForwardGrouper)

    def _lanes(self, count):
        """The model handles, parsers and streams of the pipeline's forwards in flight: the engine's own and `count - 1` replicas."""
        import torch
        while len(self._replicas) < count - 1 and hasattr(self.model, "replica"):
            # every forward in flight has its own model handle AND its own parser (frontend scratch, staging buffers)
            self._replicas.append((self.model.replica(), SpectrogramAudioParser(self.audio_config, device=self._device_index())))
        handles = [self.model] + [r[0] for r in self._replicas[:count - 1]]
        parsers = [self.audio_parser] + [r[1] for r in self._replicas[:count - 1]]
        streams = [torch.cuda.current_stream(self._device_index())] + [self._side_stream("lane %d" % k) for k in range(1, len(handles))]
        return handles, parsers, streams

    def _set_up_lanes(self, count, searching):
        """``_lanes(count)``, configured for a pipelined call; ``_tear_down_lanes`` is the other half."""
        handles, parsers, streams = self._lanes(count)
        for h in handles:
            if hasattr(h, "set_inflight"):
                h.set_inflight(max(2, len(handles)) if len(handles) > 1 else 1)     # (re-stated per forward: batch_plan.chip_forms)
        for p, st in zip(parsers, streams):
            p.share_copy_stream = searching      # a search kernel on the decode stream: fewer streams
            p.upload_on_compute_stream = True    # no copy stream in the pipeline: see SpectrogramAudioParser.stage
            # ... and the upload is ISSUED where the clips are staged, on the helper thread, into the lane's own stream: the first
            # copy a process hands a DMA engine holds its caller for 6-12 ms (hipMemcpyAsync creating the engine's queue; which
            # engine a copy gets depends on which are busy, so new ones are met well into a process's second call:
            # profiles/r06_second_call_stall.txt) -- the thread that feeds the other lanes must not be the one held
            p.upload_stream = st
        return handles, parsers, streams

    def _tear_down_lanes(self, handles, parsers):
        """The end of a pipelined call: the handles take a lone batch's kernel forms again, and no parser keeps the call's stream --
        a later ``transcribe_batch`` uploads on whatever stream runs its features (``parse_batch``), which may be another one.
        ``share_copy_stream`` and ``upload_on_compute_stream`` stay as the call left them: that later batch keeps uploading by
        kernel rather than by hipMemcpyAsync on a copy stream."""
        for h in handles:
            if hasattr(h, "set_inflight"):
                h.set_inflight(1)
            if hasattr(h, "set_ring_windows"):
                h.set_ring_windows(0)
        for p in parsers:
            p.upload_stream = None

    def _lanes_that_pay(self, most, clips):
        """Forwards in flight when the caller did not say: ``batch_plan.lanes_that_pay`` for this engine's model."""
        return batch_plan.lanes_that_pay(getattr(self.model, "rnn_hidden_size", 0), getattr(self.model, "rnn_type", "gru"), most, clips)

    def transcribe_batches(self, batches, show_all=False, lanes=None, merge_clips=None):
        """Generator over ``transcribe_batch(b)`` for every ``b`` of ``batches`` through the pipeline of ``_transcribe_forwards``
        (read its docstring for ``lanes`` / ``merge_clips``, the read-ahead and the helper thread).  What this layer adds: a
        caller's batch of MORE than ``merge_clips`` clips is cut into forwards of at most that many -- longest clips first, so
        that a forward's clips are of a kind -- and its results are put back in the caller's order: the recurrent kernel's cost
        per clip is lowest at four 16-clip tiles per window, and four forwards of 64 clips side by side fill the chip where two
        of 128 leave it to one recurrent window at a time (config 5's share, 128 x 30 s: DESIGN.md 6)."""
        import collections
        merge = self.pipeline_merge_clips if merge_clips is None else int(merge_clips)
        shapes = collections.deque()          # per caller batch: None (handed through) or its cuts, [caller positions of piece k]

        def pieces():
            for b in batches:
                on_device = isinstance(b, DeviceClips)      # longest first already: consecutive parts
                cuts = batch_plan.cut_batch(len(b), None if on_device else [len(r) for r in b], merge)
                shapes.append(cuts)
                if cuts is None:
                    yield b
                    continue
                for c in cuts:
                    yield b.part(c[0], c[-1] + 1) if on_device else [b[i] for i in c]

        total = batch_plan.count_pieces(batches, merge)
        inner = self._transcribe_forwards(pieces(), show_all=show_all, lanes=lanes, merge_clips=merge_clips, total=total)
        try:
            for res in inner:
                cuts = shapes.popleft()
                if cuts is None:
                    yield res
                    continue
                whole = [None] * sum(len(c) for c in cuts)
                for k, cut in enumerate(cuts):
                    part = res if k == 0 else next(inner)
                    for pos, i in enumerate(cut):
                        whole[i] = part[pos]
                yield whole
        finally:
            inner.close()

    def _stage_group(self, parts, parser, caller_stream):
        """The batches of one forward (``batch_plan.ForwardGrouper.next_group``) on their way to the device: -> (merged recordings,
        what ``_enqueue_batch`` needs of the staging).  Runs where the group was formed: on the pipeline's helper thread."""
        import torch
        live = [b for b in parts if len(b)]
        if not live:
            return [], None
        if isinstance(live[0], DeviceClips):
            # device-resident clips: ordered behind whatever produced them on the caller's stream (the lanes' streams are
            # ordered behind nothing else); merged into one longest-first buffer on the LANE's stream, behind that point
            ahead = torch.cuda.Event()
            ahead.record(caller_stream)
            return (live[0] if len(live) == 1 else _UnmergedDeviceClips(live)), ahead
        merged = live[0] if len(live) == 1 else [clip for b in live for clip in b]
        return merged, (self._stage_batch(merged, parser) if hasattr(parser, "stage") else None)

    def _transcribe_forwards(self, batches, show_all=False, lanes=None, merge_clips=None, total=None):
        """Generator over ``transcribe_batch(b)`` for every ``b`` of ``batches``, software-pipelined: consecutive batches are
        merged into forwards of up to ``merge_clips`` clips (per-clip results do not depend on the batch they run in), and up to
        ``lanes`` forwards are in flight (default: ``pipeline_lanes``, or two where more do not pay: ``_lanes_that_pay``), each
        on a model handle, stream and workspaces of its own -- the latency-bound recurrent layers of several forwards run side by side on disjoint compute units while the dense kernels of the others
        fill the rest of the chip; the decoder of a finished forward runs on a side stream.  Results come out in order, one
        list per batch.  ``batches`` is read AHEAD of the results: up to ``merge_clips`` clips for the forward being put
        together, plus one forward more (host clips are copied to pinned memory and uploaded before the loop waits for the
        GPU) -- a source that produces a batch only after it has seen an earlier batch's result must pass ``lanes=1,
        merge_clips=0``: then batch k + 1 is read only after result k has been yielded, on the caller's own thread.  In every
        other mode ``batches`` is advanced on a HELPER THREAD (one, the same for the whole call), concurrently with the
        consumer's loop body: a source with thread-affine state (a GUI toolkit's objects, a thread-local CUDA stream of its own)
        must be wrapped accordingly or use the sequential mode.  Latency: with the defaults (four forwards of up to 64 clips in
        flight and one staged) a result comes out eight to ten batches of 32 clips after its batch was read.

        The schedule -- which batches share a forward, a sized source's last round, the kernel forms of a forward -- is decided in
        ``batch_plan``; this method runs it: set up the lanes, then get a group, enqueue it, drain, repeat, then tear down."""
        import torch
        import collections
        auto_lanes = lanes is None
        lanes = self.pipeline_lanes if auto_lanes else max(1, int(lanes))
        merge_clips = self.pipeline_merge_clips if merge_clips is None else int(merge_clips)
        searching = hasattr(self.decoder, "decode_enqueue") and not getattr(self.decoder, "on_lane", False)
        grouper = batch_plan.ForwardGrouper(batches, merge_clips, lanes, total, self.pipeline_balance_tail,
                                            kind=lambda b: b.pcm.dtype if isinstance(b, DeviceClips) else None)     # (one sample type per device-resident forward)
        # (the lanes are set up once the first forward has been put together: how many pay depends on its size)
        handles, parsers, streams = self._lanes(1)
        caller_stream, device_index = streams[0], self._device_index()
        pending, turn, count, job, done = collections.deque(), 0, 0, None, None

        def drain(keep):
            """Results of the oldest forwards, one list per batch, until `keep` forwards are pending."""
            nonlocal done
            while len(pending) > keep:
                done = pending.popleft()
                parts, finished = done
                res = self._finish_batch(finished, show_all) if finished is not None else []
                done = finished = None
                for r in batch_plan.split_results([len(b) for b in parts], res):
                    yield r

        def next_forward(parser):
            """-> (batches, merged recordings, staging) of the next forward, or None at the end of the source."""
            parts = grouper.next_group()
            return None if parts is None else (parts,) + self._stage_group(parts, parser, caller_stream)

        # The next forward is put together by a helper thread (reading the source, the copy into pinned memory, the upload's start)
        # while this thread waits for the GPU, makes strings and runs the caller's loop body: on a busy host the staging of 80 MB
        # is milliseconds during which a lane that has just finished would otherwise stand empty.  (One forward in flight without
        # merging = the caller asked for strictly sequential reads: inline.)
        helper = None
        if lanes > 1 or merge_clips > 0:
            from concurrent.futures import ThreadPoolExecutor
            helper = ThreadPoolExecutor(max_workers=1)

        def fetch_ahead(parser):
            if helper is None:
                return next_forward(parser)

            def work():
                torch.cuda.set_device(device_index)
                torch.cuda.set_stream(caller_stream)     # a source that launches GPU work does so on the caller's stream, as inline
                return next_forward(parser)
            return helper.submit(work)

        try:
            handles, parsers, streams = self._set_up_lanes(1, searching)
            ahead = fetch_ahead(parsers[0])
            group = ahead.result() if helper is not None else ahead
            if auto_lanes and group is not None:
                lanes = self._lanes_that_pay(lanes, sum(len(b) for b in group[0]))
            handles, parsers, streams = self._set_up_lanes(lanes, searching)
            grouper.lanes = lanes = len(handles)     # (the first group was formed with the count the call started with: batch_plan)
            # Depth of the pipeline in forwards.  Greedy decoding is a short host-synchronous step.  A beam search is a kernel of its
            # own that starts when its forward ends: one more job in flight (the oldest forward's search) keeps every lane's forward
            # running while the host waits for that search.
            depth = lanes + 1 if searching else lanes
            while group is not None:
                parts, merged, staged = group
                if len(merged):
                    for older in pending:            # this forward's model handle gives back its previous forward first
                        if older[1] is not None and older[1].model is handles[turn]:
                            older[1].collect_forward()
                    if lanes > 1 and hasattr(handles[turn], "set_ring_windows"):
                        busy = sum(1 for _p, j in pending if j is not None and not j.collected and not j.model.ready())
                        inflight, ring_windows = batch_plan.chip_forms(busy, grouper.forwards_to_come(len(parts)), lanes)
                        handles[turn].set_inflight(inflight)
                        handles[turn].set_ring_windows(ring_windows)
                    with torch.cuda.stream(streams[turn]):
                        if isinstance(merged, _UnmergedDeviceClips):
                            streams[turn].wait_event(staged)
                            merged = DeviceClips.merge(merged.batches)
                        job = self._enqueue_batch(merged, handles[turn], parsers[turn], decode_slot=count % (depth + 1), staged=staged)
                    turn = (turn + 1) % lanes
                    count += 1
                pending.append((parts, job))
                job = None
                if helper is None:
                    # strictly sequential (lanes=1, merge_clips=0): every result is out before the source is asked for its next
                    # batch -- a source may wait for result k before it produces batch k + 1
                    yield from drain(0)
                ahead = fetch_ahead(parsers[turn])   # the next forward: staged now, beside the waits below
                # (one more than `depth` may be pending for a moment: the oldest forward has been waited for above -- it ran on the
                # lane that was just refilled -- and only its strings are still to be made, while every lane is busy again)
                yield from drain(depth)
                group = ahead.result() if helper is not None else ahead
            yield from drain(0)
        finally:
            if helper is not None:
                helper.shutdown(wait=True)       # (a staging in progress finishes: its pinned slot must not be refilled under it)
            # the caller stopped early, or a batch raised: whatever is still enqueued gives its forward and its beam-search
            # ticket back, otherwise the decoder handle stays "not collected" and every later call on this engine fails
            for left in [done[1] if done else None, job] + [pj[1] for pj in pending]:
                if isinstance(left, _BatchJob):
                    self._abandon(left)
            self._tear_down_lanes(handles, parsers)

    def _abandon(self, job):
        """Wait for an enqueued batch and drop its results."""
        for release in (job.collect_forward, (lambda: self.decoder.decode_collect(job.ticket)) if job.ticket is not None else None):
            if release is not None:
                try:
                    release()
                except Exception:      # the batch is being discarded: its own failure must not mask the caller's
                    pass

    def transcribe_device(self, pcm, n_samples, show_all=False, max_batch=None):
        """Clips that already sit back to back in GPU memory (int16 / float32 / float64, longest first), e.g. a
        shard received over RCCL (``parallel.recognize_sharded``): no host staging at all.  With ``max_batch`` the shard
        runs as a pipelined sequence of batches of at most that many clips (``transcribe_batches``)."""
        clips = DeviceClips(pcm, n_samples)
        if not max_batch or len(clips) <= max_batch:
            return self.transcribe_batch(clips, show_all=show_all) if len(clips) else []
        parts = [clips.part(lo, min(lo + max_batch, len(clips))) for lo in range(0, len(clips), max_batch)]
        return [r for res in self.transcribe_batches(parts, show_all=show_all) for r in res]

    def transcribe(self, recording, show_all=False):
        beams = self._finish_batch(self._enqueue_batch([recording]), True, warn=show_all)[0]
        return beams if show_all else beams[0]

    # ---- word timings of known transcripts (CTC forced alignment) ----------------------------------------------------
    def frame_seconds(self):
        """Seconds per output frame: the parser's hop times the time strides of the model's convolutions."""
        from .synthetic import CONV_SPECS
        stride = 1
        for spec in CONV_SPECS[:self.model.conv_layers]:
            stride *= spec[5]
        return float(self.audio_config["window_stride"]) * stride

    def align_batch(self, recordings, transcripts):
        """Word timings of ``transcripts[i]`` in ``recordings[i]``, as one batch: per recording ``None`` when the transcript
        cannot fit the recording's frames, else ``[(word, start_s, end_s, confidence), ...]`` for the words of the normalised
        transcript (``Decoder.normalise_transcript``).  A word's start is its first character's first frame, its end the end
        of its last character's last frame, its confidence the mean of its characters' mean probabilities.  Every transcript
        is checked before any GPU work (``ValueError`` for characters that are not labels)."""
        if self.model is None:
            raise ModelNotInitialized("Trying to align without a DanSpeech model.")
        if len(recordings) != len(transcripts):
            raise ValueError("align_batch: %d recordings and %d transcripts" % (len(recordings), len(transcripts)))
        texts = [self.decoder.normalise_transcript(t) for t in transcripts]
        ids = [self.decoder.transcript_ids(t) for t in texts]
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        aligned = self.decoder.align_ids(job.probs, [ids[i] for i in job.order], job.sizes)
        frame_s = self.frame_seconds()
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            if aligned[pos] is not None:
                results[i] = _words(texts[i], aligned[pos][0], aligned[pos][1], frame_s)
        return results

    def align(self, recording, transcript):
        """``align_batch`` of one recording."""
        return self.align_batch([recording], [transcript])[0]

    # ---- the best sentence of a grammar (CTC grammar decoding) --------------------------------------------------------
    def transcribe_grammar_batch(self, recordings, grammar):
        """What was said in ``recordings[i]``, given that it is a sentence of ``grammar`` (a ``danspeech_amd.grammar.Grammar``,
        its text, or a list with one of either per recording)?  Per recording ``None`` when no sentence of the grammar fits the
        recording's frames, else ``(text, [(word, start_s, end_s, confidence), ...], path_logp, logp)``: the sentence of the
        most probable path through the grammar (``dsmi_grammar``), its words timed as ``align_batch`` times them, the path's
        natural-log probability with the grammar's weights, and the natural log of the probability that the model emits
        exactly ``text``, summed over every alignment (``dsmi_score``: one more call for the batch).  The grammar is compiled
        before any GPU work (``ValueError`` for its faults)."""
        if self.model is None:
            raise ModelNotInitialized("Trying to decode with a grammar without a DanSpeech model.")
        per_clip = isinstance(grammar, (list, tuple))
        if per_clip and len(grammar) != len(recordings):
            raise ValueError("transcribe_grammar_batch: %d recordings and %d grammars" % (len(recordings), len(grammar)))
        graphs = [self.decoder.grammar(g) for g in grammar] if per_clip else self.decoder.grammar(grammar)
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        decoded = self.decoder.decode_grammar(job.probs, [graphs[i] for i in job.order] if per_clip else graphs, job.sizes)
        ids = [[] if d is None else [self.decoder.transcript_ids(d[0])] for d in decoded]
        scored = self.decoder.score_ids(job.probs, ids, job.sizes)
        frame_s = self.frame_seconds()
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            if decoded[pos] is not None:
                text, chars, path_logp = decoded[pos]
                words = _words(text, [(a, e) for _, a, e, _ in chars], [p for *_, p in chars], frame_s)
                results[i] = (text, words, path_logp, scored[pos][0])
        return results

    def transcribe_grammar(self, recording, grammar):
        """``transcribe_grammar_batch`` of one recording."""
        return self.transcribe_grammar_batch([recording], grammar if not isinstance(grammar, (list, tuple)) else list(grammar))[0]

    # ---- was a sentence of the grammar said, and how sure is the decoded one (CTC grammar posterior) ---------------------
    def grammar_confidence_batch(self, recordings, grammar):
        """Was a sentence of ``grammar`` (as for ``transcribe_grammar_batch``) said in ``recordings[i]``, and how sure is the
        decoded one?  Per recording ``None`` when no sentence of the grammar fits the recording's frames, else a dict:
        ``text``, ``chars`` and ``path_logp``, the best sentence, its characters ``[(char, start_frame, end_frame, prob), ...]``
        and its path's natural-log probability as ``transcribe_grammar_batch`` finds them; ``grammar_logp``, the natural log
        of the summed probability of every path the grammar accepts (``dsmi_grammar_posterior``) -- the posterior that a
        sentence of the grammar was said at all, the rejection score; ``sentence_posterior``, exp(the likelihood of ``text``
        summed over every alignment + its weight in the grammar - grammar_logp): how sure ``text`` is, given that a sentence
        of the grammar was said.  One forward and three decoder calls for the batch."""
        if self.model is None:
            raise ModelNotInitialized("Trying to decode with a grammar without a DanSpeech model.")
        per_clip = isinstance(grammar, (list, tuple))
        if per_clip and len(grammar) != len(recordings):
            raise ValueError("grammar_confidence_batch: %d recordings and %d grammars" % (len(recordings), len(grammar)))
        graphs = [self.decoder.grammar(g) for g in grammar] if per_clip else self.decoder.grammar(grammar)
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        ordered = [graphs[i] for i in job.order] if per_clip else graphs
        decoded = self.decoder.decode_grammar(job.probs, ordered, job.sizes)
        summed = self.decoder.grammar_posterior(job.probs, ordered, job.sizes)
        ids = [[] if d is None else [self.decoder.transcript_ids(d[0])] for d in decoded]
        scored = self.decoder.score_ids(job.probs, ids, job.sizes)
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            if decoded[pos] is not None and summed[pos] is not None:
                text, chars, path_logp = decoded[pos]
                g = ordered[pos] if per_clip else graphs
                total = summed[pos]["logp"]
                results[i] = dict(text=text, chars=chars, path_logp=path_logp, grammar_logp=total,
                                  sentence_posterior=float(np.exp(scored[pos][0] + g.weight_of(text) - total)))
        return results

    def grammar_confidence(self, recording, grammar):
        """``grammar_confidence_batch`` of one recording."""
        return self.grammar_confidence_batch([recording], grammar if not isinstance(grammar, (list, tuple)) else list(grammar))[0]

    # ---- where given phrases are spoken (CTC phrase search) -----------------------------------------------------------
    def find_phrases_batch(self, recordings, phrases, max_hits=5, min_confidence=0.0):
        """Where in ``recordings[i]`` is ``phrases[k]`` spoken?  ``result[i][k]`` is a list of ``(start_s, end_s, confidence,
        logp)``, best first and pairwise disjoint, at most ``max_hits``.  ``logp`` is the natural-log probability of the best
        path that emits exactly the phrase (normalised with ``Decoder.normalise_transcript``) over the span, ``confidence`` its
        per-frame geometric mean ``exp(logp / frames)``; ``min_confidence > 0`` keeps only the hits at or above it.  A hit
        starts inside the phrase's first character and ends inside its last one (``dsmi_spot``).  Every phrase is checked before
        any GPU work (``ValueError`` for characters that are not labels, an empty phrase, one longer than 128 labels)."""
        if self.model is None:
            raise ModelNotInitialized("Trying to find phrases without a DanSpeech model.")
        ids = [self.decoder.phrase_ids(p) for p in phrases]
        if len(recordings) == 0:
            return []
        if len(ids) == 0:
            return [[] for _ in recordings]
        floor = float(np.log(min_confidence)) if min_confidence > 0 else -np.inf
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        found = self.decoder.spot_ids(job.probs, ids, job.sizes, max_hits, floor)
        frame_s = self.frame_seconds()
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            results[i] = [[(a * frame_s, e * frame_s, float(np.exp(lp / (e - a))), lp) for a, e, lp in hits] for hits in found[pos]]
        return results

    def find_phrases(self, recording, phrases, max_hits=5, min_confidence=0.0):
        """``find_phrases_batch`` of one recording: ``result[k]`` for ``phrases[k]``."""
        return self.find_phrases_batch([recording], phrases, max_hits, min_confidence)[0]

    # ---- how probable are given transcripts (CTC transcript scoring) --------------------------------------------------
    def score_batch(self, recordings, candidates):
        """How probable is each of ``candidates[i]`` (a list of transcripts) as the transcript of ``recordings[i]``?
        ``result[i][k]`` is ``None`` when the transcript cannot fit the recording's frames, else ``(text, logp, confidence,
        share)``: the normalised transcript (``Decoder.normalise_transcript``), the natural log of the probability that the
        model emits exactly it, summed over every alignment (``dsmi_score``, float64), its per-frame geometric mean
        ``exp(logp / frames)``, and ``exp(logp)`` as a share of the sum over recording i's feasible candidates (the posterior
        among them).  Every transcript is checked before any GPU work (``ValueError`` for characters that are not labels)."""
        if self.model is None:
            raise ModelNotInitialized("Trying to score without a DanSpeech model.")
        if len(recordings) != len(candidates):
            raise ValueError("score_batch: %d recordings and %d candidate lists" % (len(recordings), len(candidates)))
        texts = [[self.decoder.normalise_transcript(t) for t in cands] for cands in candidates]
        ids = [[self.decoder.transcript_ids(t) for t in cands] for cands in texts]
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        scored = self.decoder.score_ids(job.probs, [ids[i] for i in job.order], job.sizes)
        frames = np.asarray(job.sizes).astype(np.int64)
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            lps = [lp for lp in scored[pos] if lp is not None]
            total = float(np.logaddexp.reduce(lps)) if lps else 0.0
            results[i] = [None if lp is None else (texts[i][k], lp, float(np.exp(lp / max(int(frames[pos]), 1))), float(np.exp(lp - total)))
                          for k, lp in enumerate(scored[pos])]
        return results

    def score(self, recording, candidates):
        """``score_batch`` of one recording: ``result[k]`` for ``candidates[k]``."""
        return self.score_batch([recording], [candidates])[0]

    def transcribe_scored_batch(self, recordings, n_best=1):
        """``transcribe_batch`` with the exact likelihood of what was recognised: per recording ``[(text, logp), ...]``, the
        decoder's first ``n_best`` hypotheses in its own order (a greedy decoder has one), ``logp`` the natural log of the
        probability of the hypothesis' label sequence summed over every alignment (``dsmi_score``), or ``None`` if infeasible."""
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        strings, _, logps = self.decoder.decode_scored(job.probs, job.sizes, n_best)
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            results[i] = list(zip(strings[pos], logps[pos]))
        return results

    # ---- the least expected error among the hypotheses, and the errors against known transcripts (batched edit distance) ----
    def transcribe_min_risk_batch(self, recordings, n_best=8, unit="word"):
        """``transcribe_scored_batch`` in minimum-Bayes-risk order: per recording ``[(text, risk, logp), ...]``, the decoder's
        first ``n_best`` hypotheses by ascending ``risk``, the expected number of ``unit`` ("word" or "char") errors of the
        hypothesis under the acoustic posteriors ``exp(logp)`` of the list (``Decoder.min_risk``; the language model has no
        part in the weights).  The first text is the one to take when the error rate matters more than the exact text."""
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        strings, _, risks, logps = self.decoder.decode_min_risk(job.probs, job.sizes, n_best, unit)
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            results[i] = list(zip(strings[pos], risks[pos], logps[pos]))
        return results

    # ---- the language model over finished n-best lists (LM sentence scoring): rescoring, and tuning alpha / beta --------------
    def _lm_decoder(self, what):
        if not hasattr(self.decoder, "rescore") or not getattr(self.decoder, "lm_path", None):
            raise ValueError("%s needs a beam-search decoder with a language model" % what)
        return self.decoder

    def transcribe_rescored_batch(self, recordings, n_best=8, alpha=None, beta=None):
        """``transcribe_scored_batch`` rescored with the language model: per recording ``[(text, total, logp), ...]``, the
        decoder's first ``n_best`` hypotheses by descending ``total = logp + alpha * lm + beta * n_words`` (``logp`` the exact
        acoustic ``dsmi_score`` likelihood, ``lm`` the ``dsmi_lm_score`` sentence score; ``alpha`` / ``beta`` None: the
        decoder's own).  ``ValueError`` without a beam-search decoder that has a language model."""
        dec = self._lm_decoder("transcribe_rescored_batch")
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        strings, _, totals, logps = dec.decode_rescored(job.probs, job.sizes, n_best, alpha, beta)
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            results[i] = list(zip(strings[pos], totals[pos], logps[pos]))
        return results

    def tune_lm_batch(self, recordings, transcripts, alphas, betas, n_best=8, unit="word"):
        """``BeamCTCDecoder.tune_lm_weights`` on ``recordings`` with their known ``transcripts``: one forward, one n-best
        search at the decoder's current weights, one ``dsmi_lm_score`` and one ``dsmi_edit_distance`` call, then the whole
        alpha x beta grid on the host.  It tunes a rescoring of that search's n-best lists, not the search's own pruning."""
        dec = self._lm_decoder("tune_lm_batch")
        if len(recordings) != len(transcripts):
            raise ValueError("tune_lm_batch: %d recordings and %d transcripts" % (len(recordings), len(transcripts)))
        if len(recordings) == 0:
            raise ValueError("tune_lm_batch: no recording")
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        return dec.tune_lm_weights(job.probs, job.sizes, [transcripts[i] for i in job.order], alphas, betas, n_best, unit)

    def evaluate_batch(self, recordings, transcripts):
        """Recognise ``recordings`` and compare with their known ``transcripts`` (normalised with
        ``Decoder.normalise_transcript``): a dict of ``texts``, the corpus rates ``wer`` and ``cer`` (summed distances over
        summed reference lengths; ``None`` where the transcripts hold no token), ``word_counts`` / ``char_counts`` (int32
        [N, 4]: distance, substitutions, deletions, insertions per recording) and ``word_ref_lens`` / ``char_ref_lens``.  One
        recognition and two ``dsmi_edit_distance`` calls."""
        if len(recordings) != len(transcripts):
            raise ValueError("evaluate_batch: %d recordings and %d transcripts" % (len(recordings), len(transcripts)))
        refs = [self.decoder.normalise_transcript(t) for t in transcripts]
        texts = list(self.transcribe_batch(recordings)) if len(recordings) else []
        out = {"texts": texts}
        for unit, name in (("word", "wer"), ("char", "cer")):
            counts, ref_lens = self.decoder.error_counts(refs, texts, unit)
            total = int(ref_lens.sum())
            out[name] = int(counts[:, 0].sum()) / total if total else None
            out[unit + "_counts"], out[unit + "_ref_lens"] = counts, ref_lens
        return out

    # ---- how sure is the model of each character and word (CTC token confidence) --------------------------------------
    def confidence_batch(self, recordings, transcripts):
        """How sure is the model of each character and word of ``transcripts[i]`` as the transcript of ``recordings[i]``, and
        what else might it have heard there?  Per recording ``None`` when the transcript cannot fit the recording's frames,
        else ``(words, chars)``: ``chars = [(char, confidence, alternative, alternative_confidence), ...]`` for every
        character of the normalised transcript (``Decoder.normalise_transcript``), spaces included -- ``confidence`` the
        posterior of the character against every other label and against no character in its place, given the rest of the
        transcript and summed over every alignment (``dsmi_alternatives``, float64), ``alternative`` the most probable other
        label ('' for no character) -- and ``words = [(word, confidence), ...]``, a word's confidence the least of its
        characters'.  Every transcript is checked before any GPU work (``ValueError`` for characters that are not labels)."""
        if self.model is None:
            raise ModelNotInitialized("Trying to compute confidences without a DanSpeech model.")
        if len(recordings) != len(transcripts):
            raise ValueError("confidence_batch: %d recordings and %d transcripts" % (len(recordings), len(transcripts)))
        texts = [self.decoder.normalise_transcript(t) for t in transcripts]
        ids = [self.decoder.transcript_ids(t) for t in texts]
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        conf = self.decoder.confidence_ids(job.probs, [ids[i] for i in job.order], job.sizes)
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            if conf[pos] is not None:
                results[i] = _confidences(list(texts[i]), ids[i], conf[pos][1], self.decoder.labels, self.decoder.blank_index)
        return results

    def confidence(self, recording, transcript):
        """``confidence_batch`` of one recording."""
        return self.confidence_batch([recording], [transcript])[0]

    def transcribe_confident_batch(self, recordings):
        """``transcribe_batch`` with the confidence of what was recognised, from one forward: per recording ``(text, words,
        chars)``, the decoder's first hypothesis and, for its label sequence as it is, ``words`` and ``chars`` as
        ``confidence_batch`` returns them."""
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        strings, ids, conf = self.decoder.decode_confident(job.probs, job.sizes)
        labels, blank = self.decoder.labels, self.decoder.blank_index
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            words, chars = _confidences([labels[int(c)] for c in ids[pos]], ids[pos], conf[pos][1], labels, blank)      # (what was decoded from the frames fits them)
            results[i] = (strings[pos], words, chars)
        return results

    # ---- soft timings of known transcripts (CTC occupancy) -------------------------------------------------------------
    def soft_align_batch(self, recordings, transcripts):
        """When is each character and word of ``transcripts[i]`` spoken in ``recordings[i]``, over EVERY alignment rather
        than the one best path of ``align_batch``?  Per recording ``None`` when the transcript cannot fit the recording's
        frames, else ``(words, chars)``: ``chars = [(char, centre_s, spread_s, dwell_s), ...]`` for every character of the
        normalised transcript (``Decoder.normalise_transcript``), spaces included -- the moments over the frames t of the
        posterior ``tok[t, k]`` that frame t is emitted by character k (``dsmi_occupancy``, float64): ``centre`` its mean
        frame ``sum t tok / sum tok``, ``spread`` its standard deviation, ``dwell`` the expected frames ``sum tok`` (at least
        one), all in seconds (``frame_seconds``) -- and ``words = [(word, first character's centre_s, last character's
        centre_s), ...]``.  A boundary the model cannot place shows as a wide spread.  Every transcript is checked before any
        GPU work (``ValueError`` for characters that are not labels)."""
        import torch
        if self.model is None:
            raise ModelNotInitialized("Trying to align without a DanSpeech model.")
        if len(recordings) != len(transcripts):
            raise ValueError("soft_align_batch: %d recordings and %d transcripts" % (len(recordings), len(transcripts)))
        texts = [self.decoder.normalise_transcript(t) for t in transcripts]
        ids = [self.decoder.transcript_ids(t) for t in texts]
        if len(recordings) == 0:
            return []
        job = self._enqueue_batch(recordings)
        job.collect_forward()                    # waits for the forward; a timed-out batch has been recomputed by now
        occupied = self.decoder.occupancy_ids(job.probs, [ids[i] for i in job.order], job.sizes)
        frame_s = self.frame_seconds()
        results = [None] * job.count
        for pos, i in enumerate(job.order):
            if occupied[pos] is None:
                continue
            tok = occupied[pos][2]                                                   # [frames, L] on the device
            t = torch.arange(tok.shape[0], dtype=tok.dtype, device=tok.device)[:, None]
            dwell = tok.sum(0)
            centre = (t * tok).sum(0) / dwell
            spread = (((t - centre[None, :]) ** 2 * tok).sum(0) / dwell).sqrt()
            m = (torch.stack((centre, spread, dwell), 1) * frame_s).cpu().numpy()    # [L, 3] seconds
            chars = [(ch, float(m[k, 0]), float(m[k, 1]), float(m[k, 2])) for k, ch in enumerate(texts[i])]
            words, k = [], 0
            for word in texts[i].split():
                k = texts[i].index(word, k)
                words.append((word, chars[k][1], chars[k + len(word) - 1][1]))
                k += len(word)
            results[i] = (words, chars)
        return results

    def soft_align(self, recording, transcript):
        """``soft_align_batch`` of one recording."""
        return self.soft_align_batch([recording], [transcript])[0]

    # ---- long recordings and files ----------------------------------------------------------------------------------
    def _cut_long(self, recording, energy_threshold, step, pause_threshold, phrase_threshold, sample_rate, resample):
        """The recording on the device at the model's rate and its phrases ``[(start_sample, end_sample), ...]`` in time order:
        the front of ``transcribe_long`` and ``align_long``."""
        import torch
        parser = self.audio_parser
        if sample_rate is not None and int(sample_rate) != int(parser.sampling_rate):
            pcm = parser.resample_batch([recording], int(sample_rate), resample).pcm
        else:
            pcm = torch.from_numpy(np.ascontiguousarray(recording, dtype=np.float64)).to("cuda:%d" % parser.device)
        hop_seconds = step / float(parser.sampling_rate)
        segs = parser._frontend().segment(pcm, energy_threshold=energy_threshold, step=step,
                                          pause_hops=int(np.ceil(pause_threshold / hop_seconds)),
                                          phrase_hops=int(np.ceil(phrase_threshold / hop_seconds)))
        return pcm, segs

    def transcribe_long(self, recording, energy_threshold=600, step=1024, pause_threshold=0.55, phrase_threshold=0.2,
                        max_batch=32, show_all=False, sample_rate=None, resample="polyphase"):
        """Long-form transcription: the energy gate of the reference's
        example_scripts/video_transcribe_simulation.py:68-143 cuts the recording into phrases (``dsmi_segment``: hop
        energies on the GPU), the phrases are transcribed in batches of at most ``max_batch`` (longest first), and
        ``[(start_sample, end_sample, transcription), ...]`` comes back in time order.  The recording is uploaded
        once; phrases are sliced on the device.  ``sample_rate``: the recording's rate when it is not the model's (a video
        sound track): the whole recording is then converted once on the device (``resample``: "polyphase" or "ratecv"), the
        energy gate and the slicing run on the converted signal, and the returned sample ranges count samples at the MODEL's
        rate (16 kHz), not the recording's."""
        import torch
        parser = self.audio_parser
        pcm, segs = self._cut_long(recording, energy_threshold, step, pause_threshold, phrase_threshold, sample_rate, resample)
        res = [None] * len(segs)
        order = sorted(range(len(segs)), key=lambda i: -(int(segs[i][1]) - int(segs[i][0])))
        for k in range(0, len(order), max_batch):
            idxs = order[k:k + max_batch]
            n = np.array([int(segs[i][1] - segs[i][0]) for i in idxs], dtype=np.int64)
            cat = torch.cat([pcm[int(segs[i][0]):int(segs[i][1])] for i in idxs])
            feats, frames = parser._frontend().features(cat, n)
            out, output_sizes = self.model(feats, torch.from_numpy(frames.astype(np.int32)))
            decoded_output, _ = self.decoder.decode(out, output_sizes)
            for pos, i in enumerate(idxs):
                res[i] = (int(segs[i][0]), int(segs[i][1]), decoded_output[pos] if show_all else decoded_output[pos][0])
        return res

    def align_long(self, recording, sentences, energy_threshold=600, step=1024, pause_threshold=0.55, phrase_threshold=0.2,
                   max_batch=32, sample_rate=None, resample="polyphase", window=30):
        """Sentence and word timings of a whole recording with its transcript (a sitting, a lecture, a film with subtitles):
        which phrase holds which sentence is what the alignment finds.  The recording is cut into phrases and forwarded exactly
        as ``transcribe_long`` does it (the same gate, batching and optional rate conversion); the phrases' valid probability
        rows are concatenated on the device in time order and ``" ".join`` of the normalised sentences is aligned to them with
        both ends free (``Decoder.align_long_ids``: audio before the first and after the last sentence costs nothing).
        Returns per sentence ``(start_s, end_s, confidence, words)``, or ``None`` for the whole call when the transcript cannot
        fit the frames.  ``words`` are ``[(word, start_s, end_s, confidence), ...]`` as ``align`` gives them.  ``confidence``
        is the least mean of the characters' mean probabilities over any ``window`` consecutive characters of the sentence (the
        whole sentence when it is shorter): the worst stretch gives away a sentence that is not in the audio.  Times are
        seconds at the model's rate, counted on the recording (the pauses between phrases included): a frame of phrase i lies
        at the phrase's start plus its index times ``frame_seconds()``; an exclusive end is its last frame's time plus one frame.
        Every sentence is checked before any GPU work: ``ValueError`` for a character that is not a label and for a sentence
        that is empty after normalising."""
        import torch
        if self.model is None:
            raise ModelNotInitialized("Trying to align without a DanSpeech model.")
        texts = [self.decoder.normalise_transcript(t) for t in sentences]
        for i, t in enumerate(texts):
            self.decoder.transcript_ids(t)
            if not t:
                raise ValueError("sentence %d is empty after normalisation: %r" % (i, sentences[i]))
        if int(window) < 1:
            raise ValueError("window must be at least 1")
        if not texts:
            return []
        whole = " ".join(texts)
        ids = self.decoder.transcript_ids(whole)
        parser = self.audio_parser
        pcm, segs = self._cut_long(recording, energy_threshold, step, pause_threshold, phrase_threshold, sample_rate, resample)
        if len(segs) == 0:
            return None
        rows = [None] * len(segs)
        order = sorted(range(len(segs)), key=lambda i: -(int(segs[i][1]) - int(segs[i][0])))
        for k in range(0, len(order), max_batch):
            idxs = order[k:k + max_batch]
            n = np.array([int(segs[i][1] - segs[i][0]) for i in idxs], dtype=np.int64)
            cat = torch.cat([pcm[int(segs[i][0]):int(segs[i][1])] for i in idxs])
            feats, frames = parser._frontend().features(cat, n)
            out, output_sizes = self.model(feats, torch.from_numpy(frames.astype(np.int32)))
            sizes = np.asarray(torch.as_tensor(output_sizes).cpu()).astype(np.int64)
            for pos, i in enumerate(idxs):
                rows[i] = out[pos, :int(sizes[pos])]
        counts = np.array([r.shape[0] for r in rows], dtype=np.int64)
        aligned = self.decoder.align_long_ids(torch.cat(rows).float().contiguous(), ids, True, True)
        if aligned is None:
            return None
        spans, token_probs, _ = aligned
        # the time of every concatenated frame: its phrase's start on the recording plus its index in the phrase
        frame_s, rate = self.frame_seconds(), float(parser.sampling_rate)
        first = np.concatenate(([0], np.cumsum(counts)[:-1]))
        starts = np.array([int(sg[0]) for sg in segs], dtype=np.float64) / rate
        frame_t = np.repeat(starts, counts) + (np.arange(int(counts.sum())) - np.repeat(first, counts)) * frame_s
        begin = lambda f: float(frame_t[int(f)])
        end = lambda f: float(frame_t[int(f) - 1] + frame_s)
        results, at, w = [], 0, int(window)
        for t in texts:
            sp, tp = spans[at:at + len(t)], token_probs[at:at + len(t)]
            at += len(t) + 1
            sums = np.concatenate(([0.0], np.cumsum(tp.astype(np.float64))))
            conf = float(sums[-1] / len(t)) if len(t) <= w else float(np.min(sums[w:] - sums[:-w]) / w)
            words = [(wd, begin(a), end(b), c) for wd, a, b, c in _words(t, sp, tp, 1)]
            results.append((begin(sp[0][0]), end(sp[-1][1]), conf, words))
        return results

    def transcribe_files(self, paths, show_all=False, resample=None):
        """``transcribe_batch([load_audio(p) for p in paths])`` without decoding the files on the host:
        the WAV frames go to the GPU as bytes and ``dsmi_features`` applies ``load_audio``'s sample-width
        conversion and saturating stereo fold (resources.py:302-303).  Files are grouped by
        (sample width, channels); every group is one batch.
        ``resample=None`` takes every file's samples as 16 kHz whatever its header says, as ``load_audio`` does.  With
        "polyphase" or "ratecv" the header's frame rate counts: files are grouped by (sample width, channels, rate) and the
        groups whose rate is not the model's are converted on the device (``dsmi_resample``) in front of the spectrograms."""
        import torch
        from .audio.resources import read_wav_frames, read_wav_frames_rate
        if len(paths) == 0:
            return []
        if resample is None:
            loaded = [read_wav_frames(p) + (None,) for p in paths]
        else:
            if resample not in ("polyphase", "ratecv"):
                raise ValueError("resample must be None, 'polyphase' or 'ratecv'")
            loaded = [read_wav_frames_rate(p) for p in paths]
            loaded = [(raw, width, nch, None if rate == int(self.audio_parser.sampling_rate) else rate) for raw, width, nch, rate in loaded]
        groups = {}
        for i, (raw, width, nch, rate) in enumerate(loaded):
            groups.setdefault((width, nch, rate), []).append(i)
        res = [None] * len(paths)
        for (width, nch, rate), idxs in groups.items():
            idxs = sorted(idxs, key=lambda i: -len(loaded[i][0]))       # stable: longest first
            feats, frames = self.audio_parser.parse_wav_frames([loaded[i][0] for i in idxs], width, nch, rate=rate,
                                                               resample=resample or "polyphase")
            out, output_sizes = self.model(feats, torch.from_numpy(frames.astype(np.int32)))
            decoded_output, _ = self.decoder.decode(out, output_sizes)
            for pos, i in enumerate(idxs):
                res[i] = decoded_output[pos] if show_all else decoded_output[pos][0]
        if show_all and self.lm == 'greedy':
            warnings.warn("You are trying to get all beams but no LM has been instantiated.", NoLmInstantiatedWarning)
        return res

    # ---- utterances that arrive in parts ----------------------------------------------------------------------------
    def enable_streaming(self, secondary_model=None, return_string_parts=True, lm_partials=False, sample_rate=None, resample="polyphase",
                         watch=None, watch_confidence=0.5, watch_settle_s=0.5, grammar=None, grammar_partials=False, grammar_max_s=30.0):
        """Streaming mode.  ``sample_rate``: the rate of the parts ``streaming_transcribe`` will be given when it is not the
        model's (telephony's 8 kHz, a sound card's 44.1 or 48 kHz): each part is then converted on the GPU as it arrives
        (``resample``: "polyphase" or "ratecv"), with the state carried from part to part, so that the converted parts are bit
        for bit the conversion of the whole utterance.  ``lm_partials=True`` (needs a language-model decoder, else ``ValueError``) carries the beam search
        from part to part: every middle part then returns the best beam's text of the WHOLE utterance so far -- language-model
        hypotheses revise earlier words, so ``return_string_parts`` does not apply to them -- and the final text, when no
        secondary model gives it, comes from the carried search (equal to the full decode it replaces).  The running greedy
        text and the final-text rules are those of ``lm_partials=False``, which is the reference's behaviour.
        ``watch``: a list of phrases to listen for in every session (``Decoder.watch``: normalised and checked as
        ``find_phrases`` does it, ``ValueError`` before any GPU work).  Every session then carries a phrase search of its own on
        the one shared watch; all due sessions' searches advance in one launch after the model pass, over exactly the rows the
        pass produced.  A window counts when its per-frame geometric mean probability is at least ``watch_confidence`` and is
        reported ``watch_settle_s`` seconds after its end (unless a better window that meets it has come up by then, or the
        utterance ends first).  Detections wait on the session for ``take_detections()``: ``(utterance_ordinal, phrase, start_s,
        end_s, confidence, logp)`` in seconds from the utterance's first output frame, ``confidence = exp(logp / frames)`` as
        ``find_phrases`` reports it.  What the streaming calls return is the same with and without a watch.
        ``grammar``: a ``Grammar`` or its text (compiled before any GPU work, ``ValueError`` for its faults): every utterance is
        then also decoded as a sentence of the grammar, live.  Every session carries a graph search of its own on the one shared
        net (``Decoder.grammar_net``); all due sessions' searches advance in one launch after the model pass, over exactly the
        rows the pass produced, and the last part reports the final result: ``transcribe_grammar``'s text, word timings and
        ``path_logp`` of the utterance's rows, bit for bit.  With ``grammar_partials`` every middle part also reports the best
        sentence prefix so far.  Results wait on the session for ``take_commands()``.  A search holds ``grammar_max_s`` seconds
        of frames; a longer utterance gets one warning and ``None`` for its final, and no call is refused because of it.  What
        the streaming calls return is the same with and without a grammar; ``watch`` and ``grammar`` may both be set."""
        if lm_partials and not isinstance(self.decoder, BeamCTCDecoder):
            raise ValueError("lm_partials needs a language-model decoder (update_decoder(lm=...)); this recogniser decodes greedily")
        spec = None
        if watch is not None:
            phrases = [self.decoder.normalise_transcript(p) for p in watch]
            ids = [self.decoder.phrase_ids(p) for p in watch]
            if not ids:
                raise ValueError("watch: at least one phrase")
            if not watch_settle_s > 0:
                raise ValueError("watch_settle_s must be positive")
            spec = (phrases, ids, float(watch_confidence), max(1, int(round(watch_settle_s / self.frame_seconds()))))
        self._watch_spec, self._watch = spec, None
        gspec = None
        if grammar is not None:
            if not grammar_max_s > 0:
                raise ValueError("grammar_max_s must be positive")
            gspec = (self.decoder.grammar(grammar), bool(grammar_partials), max(1, int(round(grammar_max_s / self.frame_seconds()))))
        self._grammar_spec, self._grammar_net = gspec, None
        if secondary_model:
            secondary_model = secondary_model.to(self.device)
            secondary_model.eval()
        if self._session:
            self._session.close()
        self._session = _StreamingSession(secondary_model or None, bool(return_string_parts), bool(lm_partials), spec is not None, gspec is not None)
        self.greedy_decoder = GreedyDecoder(labels=self.labels, blank_index=self.labels.index('_'))
        self.audio_parser = InferenceSpectrogramAudioParser(audio_config=self.audio_config, device=self._device_index())
        self.set_streaming_source(sample_rate, resample)

    def set_streaming_source(self, sample_rate=None, resample="polyphase"):
        """The rate of the parts ``streaming_transcribe`` is given from now on (see ``enable_streaming``); None: the model's."""
        self._session.set_source(self.audio_parser, sample_rate, resample)

    def disable_streaming(self, keep_secondary_model=False):
        self.audio_parser = SpectrogramAudioParser(self.audio_config, device=self._device_index())
        self.greedy_decoder = None
        kept = self._session.secondary_model if (self._session and keep_secondary_model) else None
        if self._session:
            self._session.close()
        self._session = _StreamingSession(kept, False)
        self._watch_spec = self._watch = None
        self._grammar_spec = self._grammar_net = None

    def reset_streaming_params(self):
        if self._session:
            self._session.clear()

    # attribute names of the reference object, for code that peeks at them
    secondary_model = property(lambda self: self._session.secondary_model if self._session else None)
    string_parts = property(lambda self: self._session.string_parts if self._session else False)
    iterating_transcript = property(lambda self: self._session.text if self._session else "")
    full_output = property(lambda self: self._session.outputs if self._session else [])
    spectrograms = property(lambda self: self._session.spectrograms if self._session else [])

    def _final_text(self, ses):
        """The utterance is over: the secondary model on all spectrograms, else the language-model decoder on all
        outputs, else the running greedy text."""
        import torch
        if ses.secondary_model:
            spect = torch.cat(ses.spectrograms, dim=1)
            spect = spect.view(1, 1, spect.size(0), spect.size(1)).to(self.device)
            probs, _ = ses.secondary_model(spect, torch.IntTensor([spect.size(3)]).int())
            text = self.decoder.decode(probs)[0][0][0]
        elif self.lm != "greedy":
            if ses.beam_text is not None and ses.beam_decoder is self.decoder:
                text = ses.beam_text          # the carried search, advanced by the last part
            else:
                text = self.decoder.decode(torch.cat(ses.outputs, dim=1))[0][0][0]
        else:
            text = ses.text
        ses.clear()
        return text

    def new_streaming_session(self, sample_rate=None, resample="polyphase"):
        """A session of its own for ``streaming_transcribe_many``: its parser, its ``dsmi_stream`` handle on the streaming
        model and its running text, outputs and spectrograms; the secondary model and string-parts setting are those of
        ``enable_streaming``.  ``sample_rate`` / ``resample``: the rate of THIS session's source when it is not the model's
        (sessions of different rates advance together)."""
        from . import _native
        if self._session is None or not isinstance(self.audio_parser, InferenceSpectrogramAudioParser):
            raise RuntimeError("call enable_streaming first")
        native = getattr(self.model, "_native", None)
        if native is None:
            raise RuntimeError("the streaming model runs only on an MI355X: call model.to('cuda') first (no CPU path)")
        state = _StreamingSession(self._session.secondary_model, self._session.string_parts, self._session.lm_partials, self._session.watching,
                                  self._session.commanding)
        # the resamplers of all sessions belong to ONE frontend (the engine's streaming parser's): one push_many serves them all
        state.set_source(self.audio_parser, sample_rate, resample)
        return StreamingSessionHandle(InferenceSpectrogramAudioParser(audio_config=self.audio_config, device=self._device_index()),
                                      _native.NativeStream(native), state)

    def new_live_session(self, chunk=1024, sample_rate=None, resample="polyphase", energy_threshold=1000, pause_threshold=0.8,
                         phrase_threshold=0.3, non_speaking_duration=0.35, dtype=np.int16, channels=1):
        """A live source for ``streaming_listen_many``: continuous audio that nobody has cut into utterances.  ``chunk`` and the
        four gate parameters are ``listen_stream``'s (reference Recognizer.py:218-324); ``sample_rate`` is the source's rate when
        it is not the model's -- the gate then runs at the source's rate and what it emits goes through a polyphase
        ``dsmi_resampler``.  ``resample="ratecv"`` is refused: the gate hands on float64 samples, ``audioop.ratecv`` is defined on
        integers.  ``dtype`` / ``channels``: the sample type of the parts (int16, two channels allowed; float32; float64)."""
        from . import _native
        from .stream_plan import LivePasses
        if resample == "ratecv":
            raise ValueError("resample='ratecv' cannot follow the gate (it hands on float64 samples): use 'polyphase'")
        if resample != "polyphase":
            raise ValueError("resample method must be 'polyphase'")
        if not pause_threshold >= non_speaking_duration >= 0:
            raise ValueError("the gate needs pause_threshold >= non_speaking_duration >= 0")
        session = self.new_streaming_session()
        model_rate = int(self.audio_parser.sampling_rate)
        rate = model_rate if sample_rate is None else int(sample_rate)
        fe = self.audio_parser._frontend()          # every gate and resampler on ONE frontend: one push_many serves them all
        ep = rs = None
        try:
            ep = _native.NativeEndpointer(fe, chunk, rate, energy_threshold, pause_threshold, phrase_threshold, non_speaking_duration,
                                          dtype=dtype, channels=channels)
            if rate != model_rate:
                rs = _native.NativeResampler(fe, rate, "polyphase", dtype=np.float64)
        except Exception:
            if ep is not None:
                ep.close()
            session.close()
            raise
        return LiveSessionHandle(ep, rs, LivePasses(self.model.context, model_rate), session, np.dtype(dtype))

    def streaming_listen_many(self, sessions, parts, end_of_stream):
        """One round of live audio for several sources (``new_live_session``): ``parts[k]`` holds session k's new samples, of any
        length (None or empty for none), ``end_of_stream[k]`` ends its stream after them.  The gate runs for all sessions in one
        ``dsmi_endpointer_push_many``; what it emits is converted for the sessions of another rate (one ``push_many`` per
        segment rank), accumulates under ``real_time_streaming``'s pass rule, and the sessions that have a pass due advance in
        one ``streaming_transcribe_many`` (a session whose round closes an utterance and opens the next has several passes:
        they run in as many batched calls).  Samples stay on the device from the upload on.
        -> per session, the ``(is_last, text)`` pairs ``real_time_streaming`` would yield, empty texts left out."""
        import torch
        from . import _native
        n = len(sessions)
        if not (len(parts) == len(end_of_stream) == n):
            raise ValueError("sessions, parts and end_of_stream must have one entry per session")
        if len(set(id(s) for s in sessions)) != n:
            raise ValueError("a session appears twice in one call")
        dev = "cuda:%d" % self._device_index()
        # ---- one upload of all the parts, each in its session's sample type, every part on 8 bytes
        chunks = []
        for k, ses in enumerate(sessions):
            a = np.zeros(0, dtype=ses.dtype) if parts[k] is None else np.ascontiguousarray(np.asarray(parts[k], dtype=ses.dtype))
            a = a.reshape(-1).view(np.uint8)
            if len(a) % ses.endpointer.frame_bytes:
                raise ValueError("session %d: the part is not a whole number of frames" % k)
            chunks.append(a)
        pcm, offs = _packed_upload(chunks, dev)
        segs = _native.NativeEndpointer.push_many([s.endpointer for s in sessions], [pcm[o:o + len(a)] if len(a) else None for a, o in zip(chunks, offs)],
                                                  [bool(v) for v in end_of_stream])
        # ---- the sessions of another rate: segment j of each of them in one resampler push; a last mark flushes the utterance
        conv = [k for k in range(n) if sessions[k].resampler is not None]
        for j in range(max([len(segs[k]) for k in conv] + [0])):
            due = [k for k in conv if j < len(segs[k])]
            outs = _native.NativeResampler.push_many([sessions[k].resampler for k in due], [segs[k][j][0] if segs[k][j][0].numel() else None for k in due],
                                                     [segs[k][j][1] for k in due])
            for k, out in zip(due, outs):
                segs[k][j] = (out, segs[k][j][1])
        # ---- the passes that are due, rank by rank over the sessions
        due = [s.passes.feed(segs[k]) for k, s in enumerate(sessions)]
        said = [[] for _ in sessions]
        for r in range(max([len(d) for d in due] + [0])):
            ks = [k for k in range(n) if r < len(due[k])]
            recs = []
            for k in ks:
                tensors = [t for t in due[k][r][0] if t.numel()]
                recs.append(torch.cat(tensors) if len(tensors) > 1 else (tensors[0] if tensors else torch.empty(0, dtype=torch.float64, device=dev)))
            texts = self.streaming_transcribe_many([sessions[k].session for k in ks], recs, [due[k][r][2] for k in ks], [due[k][r][1] for k in ks])
            for k, text in zip(ks, texts):
                if text:
                    said[k].append((due[k][r][2], text))
        return said

    def _convert_parts(self, states, parts, flush, take):
        """The parts of the sessions whose source has another rate, converted: one upload of all of them, one
        ``NativeResampler.push_many``, nothing synchronised.  -> ``parts`` with those entries replaced by float64 CUDA tensors
        at the model's rate.  ``flush[k]``: session k's source ends with this part; ``take[k]``: how many converted samples
        the session hands on now (None: all it has) -- the rest waits in the session for its next part.  Everything that can
        refuse the call (a ratecv part that is not int16, a ``take`` beyond what is final) does so before any session moves; for
        a session that does not convert, ``take`` can only be the part's own length."""
        import torch
        from . import _native
        for k, ses in enumerate(states):
            if ses.resampler is None and take[k] is not None and int(take[k]) != len(parts[k]):
                raise ValueError("session %d takes its parts as they are: take must be the part's length (%d), not %d"
                                 % (k, len(parts[k]), int(take[k])))
        due = [k for k, ses in enumerate(states) if ses.resampler is not None]
        if not due:
            return parts
        chunks = []
        for k in due:
            a = np.asarray(parts[k]).reshape(-1)
            if states[k].source[1] == "ratecv" and a.dtype != np.int16:
                if not np.array_equal(a, np.clip(np.round(a), -32768, 32767)):
                    raise ValueError("resample='ratecv' needs int16 samples (or float arrays holding int16 integers, as load_audio "
                                     "returns them for 16-bit files)")
                a = a.astype(np.int16)
            elif states[k].source[1] != "ratecv":
                a = a.astype(np.float64, copy=False)
            have = (0 if states[k].pending is None else states[k].pending.numel()) + states[k].resampler._due(len(a), bool(flush[k]))
            if take[k] is not None and int(take[k]) > have:
                raise ValueError("session %d: %d converted samples asked for, %d are final" % (k, int(take[k]), have))
            chunks.append(np.ascontiguousarray(a).view(np.uint8))
        pcm, offs = _packed_upload(chunks, "cuda:%d" % self._device_index())
        outs = _native.NativeResampler.push_many([states[k].resampler for k in due], [pcm[o:o + len(a)] for a, o in zip(chunks, offs)],
                                                 [bool(flush[k]) for k in due])
        parts = list(parts)
        for k, out in zip(due, outs):
            ses = states[k]
            if ses.pending is not None:
                out = torch.cat((ses.pending, out))
            n = out.numel() if take[k] is None else int(take[k])          # (<= out.numel(): checked before the push)
            ses.pending = out[n:] if n < out.numel() else None
            parts[k] = out[:n]
        return parts

    def _advance_lm_partials(self, items):
        """lm_partials: advance the carried beam searches of several sessions in ONE launch, [(session state, this part's
        probabilities or None)], and keep each one's best text in ``beam_text``.  A session without a search yet, or whose
        search belongs to a decoder that ``update_decoder`` has since replaced, gets a fresh one that replays all its kept
        outputs in this same launch."""
        import torch
        dec = self.decoder
        if not items or not isinstance(dec, BeamCTCDecoder):
            for ses, _ in items:
                ses.beam_text = None
            return
        streams, chunks = [], []
        for ses, probs in items:
            if ses.beam is None or ses.beam_decoder is not dec:
                if ses.beam is not None:
                    ses.beam.close()
                ses.beam, ses.beam_decoder = dec.new_stream(self._device_index()), dec
                kept = [o for o in ses.outputs if o is not None]
                probs = torch.cat(kept, dim=1) if kept else None
            streams.append(ses.beam)
            chunks.append(probs)
        strings, _ = dec.advance_streams(streams, chunks, 1)
        for (ses, _), s in zip(items, strings):
            ses.beam_text = s[0]

    def take_detections(self):
        """The phrase watch's detections of ``streaming_transcribe``'s own session since the last call (``enable_streaming``)."""
        return self._session.take_detections() if self._session else []

    def take_commands(self):
        """The grammar's results of ``streaming_transcribe``'s own session since the last call (``enable_streaming``)."""
        return self._session.take_commands() if self._session else []

    def _advance_grammar(self, items):
        """The grammar: advance the carried graph searches of several sessions in ONE launch, [(session state, the rows the pass
        appended to its outputs or None, is_last)], and queue the results on each session.  The last part takes the final
        result and resets the search for the session's next utterance."""
        from . import _native
        items = [it for it in items if it[0].commanding]
        if not items:
            return
        g, partials, max_frames = self._grammar_spec
        if self._grammar_net is None:
            self._grammar_net = self.greedy_decoder.grammar_net(g, self._device_index())
        streams, rows, modes, due = [], [], [], []
        for ses, probs, last in items:
            if ses.command is None or ses.command.net is not self._grammar_net:
                if ses.command is not None:
                    ses.command.close()
                ses.command = _native.NativeGrammarStream(self._grammar_net, 0, max_frames)
            new = 0 if probs is None else int(probs.shape[-2])
            if not ses.command_overrun and ses.command.frames() + new > max_frames:
                ses.command_overrun = True
                warnings.warn("grammar: an utterance is longer than grammar_max_s (%d frames); it gets no command" % max_frames)
            if ses.command_overrun:
                if last:
                    ses.commands.append((ses.command_utterance, True, None))
                    ses.command.reset()
                    ses.command_overrun = False
                    ses.command_utterance += 1
                continue
            if not (new or last or partials):
                continue
            streams.append(ses.command); rows.append(probs); modes.append(2 if last else 1 if partials else 0)
            due.append(ses)
        if not streams:
            return
        frame_s = self.frame_seconds()
        for ses, mode, res in zip(due, modes, _native.NativeGrammarStream.advance_many(streams, rows, modes)):
            if mode == 0:
                continue
            M, nodes, spans, tp, logp, status, complete = res
            text = g.text_of(nodes[:M])
            if mode == 1:
                ses.commands.append((ses.command_utterance, False, (text, bool(complete))))
                continue
            ses.commands.append((ses.command_utterance, True, None if status else (text, _words(text, spans[:M], tp[:M], frame_s), logp)))
            ses.command.reset()
            ses.command_utterance += 1

    def _advance_watch(self, items):
        """The phrase watch: advance the carried searches of several sessions in ONE launch, [(session state, the rows the pass
        appended to its outputs or None, is_last)], and queue what fired on each session.  The last part flushes the search and
        resets it for the session's next utterance."""
        from . import _native
        items = [it for it in items if it[0].watching]
        if not items:
            return
        phrases, ids, confidence, settle = self._watch_spec
        if self._watch is None:
            self._watch = self.greedy_decoder.watch_ids(ids, confidence, settle, self._device_index())
        for ses, _, _ in items:
            if ses.spot is None or ses.spot.watch is not self._watch:
                if ses.spot is not None:
                    ses.spot.close()
                ses.spot = _native.NativeSpotStream(self._watch)
        found, counts = _native.NativeSpotStream.advance_many_counts([ses.spot for ses, _, _ in items], [rows for _, rows, _ in items],
                                                                     [last for _, _, last in items], _native.SPOT_MAX_HITS)
        frame_s = self.frame_seconds()
        for (ses, _, last), events, count in zip(items, found, counts):
            for k, a, e, lp, _ in events:
                ses.detections.append((ses.utterance, phrases[k], a * frame_s, e * frame_s, float(np.exp(lp / (e - a))), lp))
            if int(count.max()) > _native.SPOT_MAX_HITS:
                warnings.warn("phrase watch: more than %d detections of one phrase in one part; the later ones were dropped" % _native.SPOT_MAX_HITS)
            if last:
                ses.spot.reset()
                ses.utterance += 1

    def streaming_transcribe_many(self, sessions, recordings, is_last, is_first, take=None, flush=None):
        """``streaming_transcribe`` for several sessions (``new_streaming_session``) at once, each on its next part of its own
        utterance; the parts' spectrograms and the model pass run batched over all sessions.  -> one string per session, each
        what ``streaming_transcribe`` returns for that session alone.
        The parts of sessions with a ``sample_rate`` are at that rate: they are uploaded once and converted in ONE
        ``push_many``; the session then goes on with what the conversion has final.  A caller that schedules passes in
        model-rate samples (``Recognizer.stream_recordings``) says with ``take[k]`` how many converted samples pass k consists of
        (the rest waits in the session) and with ``flush[k]`` that session k's SOURCE ends with this part (default: ``is_last``)."""
        from . import _native
        n = len(sessions)
        if not (len(recordings) == len(is_last) == len(is_first) == n):
            raise ValueError("sessions, recordings, is_last and is_first must have one entry per session")
        if len(set(id(s) for s in sessions)) != n:
            raise ValueError("a session appears twice in one call")
        recordings = self._convert_parts([s.state for s in sessions], recordings, is_last if flush is None else flush,
                                         [None] * n if take is None else take)
        spects = InferenceSpectrogramAudioParser.parse_audio_many([s.parser for s in sessions], recordings, is_last)
        run = [k for k in range(n) if len(spects[k]) != 0]
        for k in run:
            if sessions[k].state.secondary_model:
                sessions[k].state.spectrograms.append(spects[k])
        probs = _native.NativeStream.forward_many([sessions[k].stream for k in run], [spects[k] for k in run],
                                                  [is_first[k] for k in run], [is_last[k] for k in run])
        probs = dict(zip(run, probs))
        pieces, lm_items = [None] * n, []
        for k in range(n):
            ses = sessions[k].state
            piece = ""
            if k in probs:
                if is_first[k]:
                    continue
                ses.outputs.append(probs[k])
                piece = ses.extend_text(self.greedy_decoder.decode(probs[k])[0][0][0])
                piece = piece if ses.string_parts else ses.text
            pieces[k] = piece
            if ses.lm_partials and (k in probs or is_last[k]):
                lm_items.append((ses, probs.get(k)))
        self._advance_lm_partials(lm_items)          # every due session's search in one launch, last parts included
        due = [(sessions[k].state, probs[k] if k in probs and not is_first[k] else None, is_last[k]) for k in range(n)
               if (k in probs and not is_first[k]) or is_last[k]]
        self._advance_watch(due)
        self._advance_grammar(due)
        said = []
        for k in range(n):
            ses = sessions[k].state
            if pieces[k] is None:
                said.append("")
            elif not is_last[k]:
                said.append(ses.beam_text if ses.lm_partials and k in probs and ses.beam_text is not None else pieces[k])
            else:
                said.append(self._final_text(ses) if len(ses.text) > 1 else "")
        return said

    def streaming_transcribe(self, recording, is_last, is_first, take=None, flush=None):
        """One part of an utterance through the streaming model.  Returns this part's text (or the whole text so far
        when string parts are off); on the first part nothing (the lookahead is filling); on the last part the final
        text of the utterance, provided more than one character was recognised.  With a ``sample_rate``
        (``enable_streaming``) the part is at that rate and is converted first; ``take`` / ``flush`` as in
        ``streaming_transcribe_many``."""
        ses = self._session
        recording = self._convert_parts([ses], [recording], [is_last if flush is None else flush], [take])[0]
        spect = self.audio_parser.parse_audio(recording, is_last)
        said = ""
        probs = None
        if len(spect) != 0:
            if ses.secondary_model:
                ses.spectrograms.append(spect)
            spect = spect.view(1, 1, spect.size(0), spect.size(1)).to(self.device)
            probs = self.model(spect, is_first, is_last)
            if is_first:
                if is_last:
                    self._advance_watch([(ses, None, True)])
                    self._advance_grammar([(ses, None, True)])
                return ""
            ses.outputs.append(probs)
            piece = ses.extend_text(self.greedy_decoder.decode(probs)[0][0][0])
            said = piece if ses.string_parts else ses.text
        if ses.lm_partials and (len(spect) != 0 or is_last):
            self._advance_lm_partials([(ses, probs)])
            if len(spect) != 0 and ses.beam_text is not None:
                said = ses.beam_text
        if probs is not None or is_last:
            self._advance_watch([(ses, probs, is_last)])
            self._advance_grammar([(ses, probs, is_last)])
        if not is_last:
            return said
        return self._final_text(ses) if len(ses.text) > 1 else ""
