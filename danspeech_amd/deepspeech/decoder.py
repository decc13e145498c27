"""Decoders of the drop-in surface (reference danspeech/deepspeech/decoder.py).

``GreedyDecoder`` and ``BeamCTCDecoder`` keep the reference's constructor arguments and the
``decode(probs, sizes=None) -> (strings[B][K], offsets[B][K])`` contract; the work is done by
the HIP kernels behind ``dsmi_greedy`` / ``dsmi_beam`` (danspeech_amd/csrc/decoder.hip).
"""
import numpy as np


def _edit_distance(a, b):
    """Levenshtein distance (the reference imports the ``Levenshtein`` package for this)."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


class Decoder(object):
    """decoder.py:24-88."""

    def __init__(self, labels, blank_index=0):
        self.labels = labels
        self.int_to_char = dict([(i, c) for (i, c) in enumerate(labels)])
        self.blank_index = blank_index
        space_index = len(labels)          # out-of-range marker when there is no space label
        if ' ' in labels:
            space_index = labels.index(' ')
        self.space_index = space_index
        self._native = None
        # id -> code point table for the common case of one-character labels
        self._code_points = (np.array([ord(c) for c in labels], dtype="<u4")
                             if all(len(c) == 1 for c in labels) else None)

    def _to_string(self, ids):
        """Label ids (int array) -> text."""
        if self._code_points is not None:
            return self._code_points[ids].tobytes().decode("utf-32-le")
        return "".join(self.int_to_char[int(i)] for i in ids)

    def _dec(self, device_index, slot=0):
        """The native handle; ``slot`` > 0: a further handle with its own workspaces, for a caller that keeps several
        decodes in flight (one search per handle at a time)."""
        from .. import _native
        if self._native is None or self._native_device != device_index:
            if self._native is not None:
                self._native.close()
            for extra in getattr(self, "_native_slots", {}).values():
                extra.close()
            self._native_slots = {}
            self._native = _native.NativeDecoder(self.labels, blank_index=self.blank_index, device=device_index)
            self._native_device = device_index
            self._configure(self._native)
        if slot == 0:
            return self._native
        slots = self.__dict__.setdefault("_native_slots", {})
        if slot not in slots:
            slots[slot] = _native.NativeDecoder(self.labels, blank_index=self.blank_index, device=device_index)
            self._configure(slots[slot])
        return slots[slot]

    def _configure(self, native):
        pass

    @staticmethod
    def _on_gpu(probs):
        import torch
        probs = torch.as_tensor(probs, dtype=torch.float32)
        if not probs.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("decoding runs on the MI355X only (no CPU path) and no GPU is visible")
            probs = probs.cuda()
        return probs.contiguous()

    def wer(self, s1, s2):
        b = set(s1.split() + s2.split())
        word2char = dict(zip(b, range(len(b))))
        return _edit_distance([word2char[w] for w in s1.split()], [word2char[w] for w in s2.split()])

    def cer(self, s1, s2):
        return _edit_distance(s1.replace(' ', ''), s2.replace(' ', ''))

    def decode(self, probs, sizes=None):
        raise NotImplementedError

    # ---- CTC forced alignment of known transcripts (dsmi_align); the same on every decoder, a language model plays no part
    @staticmethod
    def normalise_transcript(text):
        """What ``align`` aligns: lower case, runs of whitespace collapsed to one space, stripped."""
        return " ".join(str(text).lower().split())

    def transcript_ids(self, text):
        """Label ids of an already normalised transcript; ``ValueError`` naming every character that is not a label (the
        blank's character included): nothing is dropped."""
        table = getattr(self, "_char_ids", None)
        if table is None:
            table = {c: i for i, c in enumerate(self.labels) if i != self.blank_index and len(c) == 1}
            self._char_ids = table
        bad = sorted(set(c for c in text if c not in table))
        if bad:
            raise ValueError("transcript holds characters that are not labels of this model: %s" % ", ".join(repr(c) for c in bad))
        return np.array([table[c] for c in text], dtype=np.int32)

    def align(self, probs, transcripts, sizes=None):
        """Forced alignment of ``transcripts[b]`` (normalised with ``normalise_transcript``) to the probabilities of clip b
        (``probs`` [B,T,C], ``sizes`` frames per clip).  Per clip ``None`` when the transcript cannot fit the clip's frames,
        else ``(spans int32 [L,2], token_probs float32 [L], path_logp)``: the frames [start, end) of each character of the
        normalised transcript, the mean probability of the character over them, and the path's natural-log probability."""
        ids = [self.transcript_ids(self.normalise_transcript(t)) for t in transcripts]      # every check before any GPU work
        return self.align_ids(probs, ids, sizes)

    def align_ids(self, probs, ids, sizes=None):
        """``align`` for label-id sequences as they are (no normalisation)."""
        import torch
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        spans, tp, lp, status = dec.align(probs, sz, ids)
        out = []
        for b, t in enumerate(ids):
            L = len(t)
            out.append(None if status[b] else (spans[b, :L].copy(), tp[b, :L].copy(), float(lp[b])))
        return out

    # ---- CTC grammar decoding (dsmi_grammar): the best sentence of a word graph; a language model plays no part
    def grammar(self, text):
        """``text`` compiled for this decoder's labels (``danspeech_amd.grammar.Grammar``); a Grammar passes through."""
        from ..grammar import Grammar
        return text if isinstance(text, Grammar) else Grammar(text, self.labels, self.blank_index)

    def decode_grammar(self, probs, grammar_or_list, sizes=None):
        """The most probable CTC path of any sentence a grammar accepts (``probs`` [B,T,C], ``sizes`` frames per clip).
        ``grammar_or_list``: one grammar (a ``Grammar`` or its text) for every clip, or a list with one per clip.  Per clip
        ``None`` when no accepted sentence fits the clip's frames, else ``(text, chars, path_logp)``: the labels of the path,
        ``chars = [(char, start_frame, end_frame, prob), ...]`` with the frames [start, end) of each character and the mean
        probability of the character over them, and the path's natural-log probability, the grammar's weights included."""
        import torch
        probs = self._on_gpu(probs)
        B = probs.shape[0]
        if isinstance(grammar_or_list, (list, tuple)):
            if len(grammar_or_list) != B:
                raise ValueError("decode_grammar: %d grammars for a batch of %d" % (len(grammar_or_list), B))
            graphs, clip_graph = [self.grammar(g) for g in grammar_or_list], np.arange(B, dtype=np.int32)
        else:
            graphs, clip_graph = [self.grammar(grammar_or_list)], None
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        lens, nodes, spans, tp, lp, status = dec.grammar(probs, sz, graphs, clip_graph)
        out = []
        for b in range(B):
            if status[b]:
                out.append(None)
                continue
            g, M = graphs[0 if clip_graph is None else b], int(lens[b])
            text = g.text_of(nodes[b, :M])
            out.append((text, [(text[k], int(spans[b, k, 0]), int(spans[b, k, 1]), float(tp[b, k])) for k in range(M)], float(lp[b])))
        return out

    # ---- CTC grammar posterior (dsmi_grammar_posterior): the summed probability of every path of a word graph
    def grammar_posterior(self, probs, grammar_or_list, sizes=None, candidates=None):
        """Was a sentence of the grammar said, and which?  ``probs`` [B,T,C], ``sizes`` frames per clip, ``grammar_or_list`` as
        for ``decode_grammar``.  Per clip ``None`` when no accepted sentence fits the clip's frames, else a dict: ``logp``, the
        natural log (float64) of the summed probability of every path the grammar accepts, its weights included (the
        posterior that a sentence of the grammar was said, for an unambiguous grammar without weights); ``visits`` float64
        [nodes], the expected number of entries into each node of the clip's graph; ``occ`` a CUDA float64 [T, C] view, the
        posterior of each label at each frame given the grammar.  With ``candidates`` (sentences, normalised like
        transcripts; the same for every clip) also ``posteriors``: per candidate exp(its ``score`` + its weight in the
        graph, ``Grammar.weight_of`` - logp), 0.0 for a sentence the grammar does not accept or that cannot fit -- one
        ``dsmi_score`` call for the whole batch."""
        import torch
        probs = self._on_gpu(probs)
        B = probs.shape[0]
        if isinstance(grammar_or_list, (list, tuple)):
            if len(grammar_or_list) != B:
                raise ValueError("grammar_posterior: %d grammars for a batch of %d" % (len(grammar_or_list), B))
            graphs, clip_graph = [self.grammar(g) for g in grammar_or_list], np.arange(B, dtype=np.int32)
        else:
            graphs, clip_graph = [self.grammar(grammar_or_list)], None
        texts = None if candidates is None else [self.normalise_transcript(t) for t in candidates]
        cand_ids = None if texts is None else [self.transcript_ids(t) for t in texts]       # every check before any GPU work
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        logp, visits, occ, status = dec.grammar_posterior(probs, sz, graphs, clip_graph)
        scored = None
        if texts is not None:
            weights = [[g.weight_of(t) for t in texts] for g in graphs]
            live = [[k for k in range(len(texts)) if not status[b] and weights[0 if clip_graph is None else b][k] is not None] for b in range(B)]
            scored = self.score_ids(probs, [[cand_ids[k] for k in ks] for ks in live], sz)
        out = []
        for b in range(B):
            if status[b]:
                out.append(None)
                continue
            gi = 0 if clip_graph is None else b
            res = dict(logp=float(logp[b]), visits=visits[b, :graphs[gi].n_nodes].copy(), occ=occ[b])
            if texts is not None:
                post = np.zeros(len(texts), dtype=np.float64)
                for k, s in zip(live[b], scored[b]):
                    if s is not None:
                        post[k] = np.exp(s + weights[gi][k] - res["logp"])
                res["posteriors"] = post
            out.append(res)
        return out

    def grammar_net(self, grammar_or_list, device_index=0):
        """Streaming grammar decoding (``dsmi_grammar_net_*``): one grammar or a list of them (``Grammar`` or text), compiled,
        checked, packed and uploaded once -> a ``NativeGrammarNet`` whose ``NativeGrammarStream``s carry one live utterance's
        search each; ``NativeGrammarStream.advance_many`` advances any number of them in one launch, and its final result is
        ``decode_grammar``'s of the rows laid end to end, bit for bit."""
        from .. import _native
        many = isinstance(grammar_or_list, (list, tuple))
        graphs = [self.grammar(g) for g in grammar_or_list] if many else [self.grammar(grammar_or_list)]
        net = _native.NativeGrammarNet(self._dec(device_index), graphs)
        net.graphs = graphs
        return net

    # ---- long-form CTC forced alignment (dsmi_align_long): one recording, its whole transcript, no limit from LDS
    def align_long(self, probs, transcript, lead_free=True, tail_free=True):
        """Forced alignment of ``transcript`` (normalised with ``normalise_transcript``) to the probabilities ``probs`` [T,C] of
        one long recording: the softmax rows of its phrases, concatenated in time order.  ``lead_free`` / ``tail_free``: the
        frames before the first and after the last character cost nothing.  ``None`` when the transcript cannot fit the
        frames, else ``(spans int32 [L,2], token_probs float32 [L], path_logp)`` as ``align`` gives them for one clip."""
        ids = self.transcript_ids(self.normalise_transcript(transcript))                     # every check before any GPU work
        return self.align_long_ids(probs, ids, lead_free, tail_free)

    def align_long_ids(self, probs, ids, lead_free=True, tail_free=True):
        """``align_long`` for a label-id sequence as it is (no normalisation)."""
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        spans, tp, lp, status = dec.align_long(probs, ids, lead_free, tail_free)
        return None if status else (spans, tp, lp)

    # ---- CTC phrase search (dsmi_spot): where are given phrases spoken; the same on every decoder, no language model
    def spot(self, probs, phrases, sizes=None, max_hits=5, min_mean_logp=-np.inf):
        """Occurrences of ``phrases[k]`` (normalised with ``normalise_transcript``) in the probabilities of every clip
        (``probs`` [B,T,C], ``sizes`` frames per clip): ``result[b][k]`` is a list of ``(start_frame, end_frame, logp)``, best
        first and pairwise disjoint, at most ``max_hits``, each with ``logp >= min_mean_logp * frames``.  ``logp`` is the
        natural-log probability of the best path that emits exactly the phrase over frames [start, end)."""
        ids = [self.phrase_ids(p) for p in phrases]                                          # every check before any GPU work
        return self.spot_ids(probs, ids, sizes, max_hits, min_mean_logp)

    def phrase_ids(self, phrase):
        """Label ids of a search phrase; ``ValueError`` for characters that are not labels, a phrase that is empty after
        normalisation, or one longer than ``SPOT_MAX_TOKENS`` labels."""
        from .. import _native
        ids = self.transcript_ids(self.normalise_transcript(phrase))
        if len(ids) == 0:
            raise ValueError("phrase %r is empty after normalisation" % (phrase,))
        if len(ids) > _native.SPOT_MAX_TOKENS:
            raise ValueError("phrase of %d labels is longer than %d: %r" % (len(ids), _native.SPOT_MAX_TOKENS, phrase))
        return ids

    def spot_ids(self, probs, ids, sizes=None, max_hits=5, min_mean_logp=-np.inf):
        """``spot`` for label-id sequences as they are (no normalisation)."""
        import torch
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        hits, scores, counts = dec.spot(probs, sz, ids, max_hits, min_mean_logp)
        return [[[(int(hits[b, k, n, 0]), int(hits[b, k, n, 1]), float(scores[b, k, n])) for n in range(counts[b, k])]
                 for k in range(len(ids))] for b in range(hits.shape[0])]

    # ---- streaming phrase watch (dsmi_spot_watch / dsmi_spot_stream): the same phrases, searched in live sessions chunk by chunk
    def watch(self, phrases, min_confidence=0.5, settle_frames=25, device_index=0):
        """A phrase list for live sessions (``NativeSpotWatch``): ``phrases`` normalised and checked exactly as ``spot`` does it
        (the same ``ValueError``s, before any GPU work).  A window counts as an occurrence when its per-frame geometric mean
        probability is at least ``min_confidence`` (0: every window), and is reported ``settle_frames`` frames after its last
        frame unless a better window that meets it has come up by then (``dsmi_spot_stream_advance_many``).  One
        ``NativeSpotStream(watch)`` per live utterance carries the search; ``NativeSpotStream.advance_many`` advances many."""
        ids = [self.phrase_ids(p) for p in phrases]                                          # every check before any GPU work
        return self.watch_ids(ids, min_confidence, settle_frames, device_index)

    def watch_ids(self, ids, min_confidence=0.5, settle_frames=25, device_index=0):
        """``watch`` for label-id sequences as they are (no normalisation)."""
        from .. import _native
        if len(ids) == 0:
            raise ValueError("watch: at least one phrase")
        if int(settle_frames) < 1:
            raise ValueError("watch: settle_frames must be at least 1")
        floor = float(np.log(min_confidence)) if min_confidence > 0 else -np.inf
        return _native.NativeSpotWatch(self._dec(device_index), ids, floor, int(settle_frames))

    # ---- CTC transcript scoring (dsmi_score): how probable is a transcript, over every alignment; no language model
    def score(self, probs, candidates, sizes=None):
        """The exact likelihood of candidate transcripts: ``candidates[b]`` is a list of transcripts for clip b (``probs``
        [B,T,C], ``sizes`` frames per clip), each normalised with ``normalise_transcript``.  ``result[b][k]`` is ``None`` when
        the transcript cannot fit the clip's frames, else the natural log (float64) of the probability that the model emits
        exactly its label sequence, summed over every CTC alignment."""
        ids = [[self.transcript_ids(self.normalise_transcript(t)) for t in cands] for cands in candidates]   # every check before any GPU work
        return self.score_ids(probs, ids, sizes)

    def score_ids(self, probs, ids, sizes=None):
        """``score`` for label-id sequences as they are (no normalisation): ``ids[b]`` a list of id sequences for clip b."""
        import torch
        from .. import _native
        if len(ids) != len(probs):
            raise ValueError("score: candidate lists for %d clips and a batch of %d" % (len(ids), len(probs)))
        flat = [t for cands in ids for t in cands]
        longest = max([len(t) for t in flat] + [0])
        if longest > _native.SCORE_MAX_TOKENS:
            raise ValueError("candidate of %d labels is longer than %d" % (longest, _native.SCORE_MAX_TOKENS))
        if not flat:
            return [[] for _ in ids]
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        clip = [b for b, cands in enumerate(ids) for _ in cands]
        lp, status = dec.score(probs, sz, clip, flat)
        out, n = [], 0
        for cands in ids:
            out.append([None if status[n + k] else float(lp[n + k]) for k in range(len(cands))])
            n += len(cands)
        return out

    # ---- CTC token confidence (dsmi_alternatives): how sure is the model of each token, and what else might it have heard
    def confidence(self, probs, transcripts, sizes=None):
        """The posterior of every token of ``transcripts[b]`` (normalised with ``normalise_transcript``) against its
        alternatives, over the probabilities of clip b (``probs`` [B,T,C], ``sizes`` frames per clip).  Per clip ``None`` when
        the transcript cannot fit the clip's frames, else ``(logp, post)``: the natural log of the transcript's likelihood
        summed over every alignment, and float64 [L, C] with ``post[k, c]`` the probability of label c in place of character
        k given the rest of the transcript -- the blank's column is "no character here", ``post[k, ids[k]]`` the confidence
        of the character itself, each row sums to 1."""
        ids = [self.transcript_ids(self.normalise_transcript(t)) for t in transcripts]      # every check before any GPU work
        return self.confidence_ids(probs, ids, sizes)

    def confidence_ids(self, probs, ids, sizes=None):
        """``confidence`` for label-id sequences as they are (no normalisation): ``ids[b]`` one id sequence for clip b."""
        import torch
        from .. import _native
        if len(ids) != len(probs):
            raise ValueError("confidence: transcripts for %d clips and a batch of %d" % (len(ids), len(probs)))
        longest = max([len(t) for t in ids] + [0])
        if longest > _native.ALT_MAX_TOKENS:
            raise ValueError("transcript of %d labels is longer than %d" % (longest, _native.ALT_MAX_TOKENS))
        if not len(ids):
            return []
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        lp, alt, status = dec.alternatives(probs, sz, np.arange(len(ids)), ids)
        out = []
        for b, t in enumerate(ids):
            if status[b]:
                out.append(None)
                continue
            rows = alt[b, :len(t)]
            out.append((float(lp[b]), np.exp(rows - np.logaddexp.reduce(rows, axis=1, keepdims=True))))
        return out

    def decode_confident(self, probs, sizes=None):
        """``decode`` and the token confidences of each clip's first hypothesis over the same (still resident) probabilities:
        ``(strings [B], ids [B], confidences [B])``, ``confidences[b]`` as ``confidence_ids`` returns it."""
        strings, _, ids = self._decode_best_ids(probs, sizes)
        return strings, ids, self.confidence_ids(probs, ids, sizes)

    # ---- CTC occupancy (dsmi_occupancy): which frames each token occupies and which label each frame carries, given the transcript
    def occupancy(self, probs, transcripts, sizes=None):
        """The per-frame posteriors of ``transcripts[b]`` (normalised with ``normalise_transcript``) over the probabilities of
        clip b (``probs`` [B,T,C], ``sizes`` frames per clip).  Per clip ``None`` when the transcript cannot fit the clip's
        frames, else ``(logp, occ, tok)``: the natural log of the transcript's likelihood summed over every alignment, and
        two CUDA float64 tensors over the clip's own frames -- ``occ`` [frames, C], the probability that frame t carries
        label c given the transcript (each row sums to 1), and ``tok`` [frames, L], the probability that frame t is emitted
        by character k (``sum_t tok[t, k]`` is the expected number of frames character k lasts)."""
        ids = [self.transcript_ids(self.normalise_transcript(t)) for t in transcripts]      # every check before any GPU work
        return self.occupancy_ids(probs, ids, sizes)

    def occupancy_ids(self, probs, ids, sizes=None):
        """``occupancy`` for label-id sequences as they are (no normalisation): ``ids[b]`` one id sequence for clip b."""
        import torch
        from .. import _native
        if len(ids) != len(probs):
            raise ValueError("occupancy: transcripts for %d clips and a batch of %d" % (len(ids), len(probs)))
        longest = max([len(t) for t in ids] + [0])
        if longest > _native.OCC_MAX_TOKENS:
            raise ValueError("transcript of %d labels is longer than %d" % (longest, _native.OCC_MAX_TOKENS))
        if not len(ids):
            return []
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        lp, occ, tok, status = dec.occupancy(probs, sz, np.arange(len(ids)), ids)
        out = []
        for b, t in enumerate(ids):
            frames = probs.shape[1] if sz is None else int(sz[b])
            out.append(None if status[b] else (float(lp[b]), occ[b, :frames], tok[b, :frames, :len(t)]))
        return out

    # ---- batched edit distance (dsmi_edit_distance): WER / CER with their error counts, and minimum-risk choice among the
    # hypotheses of an n-best list; the same on every decoder, a language model plays no part
    def _edit_device(self):
        """The native handle of the current CUDA device (no ``probs`` names one here)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("the edit distance runs on the MI355X only (no CPU path) and no GPU is visible")
        return self._dec(torch.cuda.current_device())

    @staticmethod
    def _edit_tokens(texts, unit, table):
        """Id sequences of ``texts``: words (``s.split()``, as ``wer``) through the dictionary ``table``, which grows, or
        characters without spaces (as ``cer``) by code point."""
        if unit == "word":
            return [np.array([table.setdefault(w, len(table)) for w in s.split()], dtype=np.int32) for s in texts]
        if unit == "char":
            return [np.array([ord(c) for c in s.replace(' ', '')], dtype=np.int32) for s in texts]
        raise ValueError("unit must be 'word' or 'char', not %r" % (unit,))

    @staticmethod
    def _edit_limit(seqs):
        from .. import _native
        longest = max([len(t) for t in seqs] + [0])
        if longest > _native.EDIT_MAX_TOKENS:
            raise ValueError("sequence of %d tokens is longer than %d" % (longest, _native.EDIT_MAX_TOKENS))

    def error_counts(self, references, hypotheses, unit="word"):
        """The errors of ``hypotheses[n]`` against ``references[n]`` for N pairs of strings in one call: ``(counts, ref_lens)``
        with ``counts`` int32 [N, 4] = distance, substitutions, deletions, insertions (of the minimum-distance alignment with
        the fewest substitutions) and ``ref_lens`` int32 [N] the tokens of each reference.  ``unit="word"``: tokens are
        ``s.split()`` words (``wer``'s tokenisation); ``"char"``: the characters without spaces (``cer``'s)."""
        references, hypotheses = list(references), list(hypotheses)
        if len(references) != len(hypotheses):
            raise ValueError("error_counts: %d references and %d hypotheses" % (len(references), len(hypotheses)))
        table = {}
        seqs = self._edit_tokens(references, unit, table) + self._edit_tokens(hypotheses, unit, table)
        self._edit_limit(seqs)                                                                # every check before any GPU work
        N = len(references)
        ref_lens = np.array([len(t) for t in seqs[:N]], dtype=np.int32)
        if N == 0:
            return np.zeros((0, 4), dtype=np.int32), ref_lens
        pairs = np.stack([np.arange(N), np.arange(N, 2 * N)], axis=1)
        return self._edit_device().edit_distance(seqs, pairs), ref_lens

    def wer_batch(self, references, hypotheses):
        """``[self.wer(r, h) for r, h in zip(references, hypotheses)]`` in one call, as a list of ints."""
        return self.error_counts(references, hypotheses, "word")[0][:, 0].tolist()

    def cer_batch(self, references, hypotheses):
        """``[self.cer(r, h) for r, h in zip(references, hypotheses)]`` in one call, as a list of ints."""
        return self.error_counts(references, hypotheses, "char")[0][:, 0].tolist()

    def error_rate(self, references, hypotheses, unit="word"):
        """The corpus error rate: the summed distances over the summed reference lengths (WER for ``"word"``, CER for
        ``"char"``).  ``ValueError`` when the references hold no token."""
        counts, ref_lens = self.error_counts(references, hypotheses, unit)
        total = int(ref_lens.sum())
        if total == 0:
            raise ValueError("error_rate: the references hold no token")
        return int(counts[:, 0].sum()) / total

    def _risk_tokens(self, ids, unit, table):
        """One hypothesis (label ids) as the tokens its risk is counted in: the words between space labels (empty words
        dropped) through the dictionary ``table``, or the labels without the space label."""
        ids = np.asarray(ids, dtype=np.int32).reshape(-1)
        if unit == "char":
            return ids[ids != self.space_index]
        if unit != "word":
            raise ValueError("unit must be 'word' or 'char', not %r" % (unit,))
        words, out = np.split(ids, np.flatnonzero(ids == self.space_index)), []
        for k, w in enumerate(words):
            w = w[1:] if k else w                     # (every later piece begins with the space it was cut at)
            if len(w):
                out.append(table.setdefault(w.tobytes(), len(table)))
        return np.array(out, dtype=np.int32)

    def min_risk(self, ids, logps, unit="word"):
        """Minimum-Bayes-risk order of n-best lists.  ``ids[b]``: clip b's K_b hypotheses as label-id sequences; ``logps[b]``:
        their natural-log posteriors (``None`` = infeasible), as ``decode_scored`` returns them -- ``dsmi_score``'s, acoustic
        only: the language model has no part in the weights (``BeamCTCDecoder.rescore``'s totals are valid ``logps`` too, and
        bring it in).  Per clip ``(order, risks)``: ``risks[i]`` (float64) is the
        expected number of word (``unit="word"``: the words between space labels) or character (``"char"``: the labels
        without the space label) errors of hypothesis i, sum_j w_j * distance(i, j), under the weights w = softmax(logps[b])
        (``None`` or -inf: 0; all ``None``: uniform); ``order`` is the stable ascending order of the risks, so ties keep
        the decoder's order.  The pairs i < j of every clip go in ONE ``dsmi_edit_distance`` call."""
        if len(ids) != len(logps):
            raise ValueError("min_risk: hypotheses for %d clips and posteriors for %d" % (len(ids), len(logps)))
        table, pool, base, pairs = {}, [], [], []
        for hyps, lps in zip(ids, logps):
            if len(hyps) != len(lps):
                raise ValueError("min_risk: %d hypotheses and %d posteriors of one clip" % (len(hyps), len(lps)))
            base.append(len(pool))
            pool.extend(self._risk_tokens(t, unit, table) for t in hyps)
            iu = np.triu_indices(len(hyps), 1)
            pairs.append(np.stack([iu[0] + base[-1], iu[1] + base[-1]], axis=1))
        self._edit_limit(pool)                                                                # every check before any GPU work
        pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), dtype=np.int64)
        dist = self._edit_device().edit_distance(pool, pairs)[:, 0] if len(pairs) else np.zeros(0, dtype=np.int32)
        out, at = [], 0
        for hyps, lps in zip(ids, logps):
            K = len(hyps)
            lp = np.array([-np.inf if v is None else float(v) for v in lps], dtype=np.float64)
            if K and np.isfinite(lp.max()):
                w = np.exp(lp - lp.max())
                w /= w.sum()
            else:
                w = np.full(K, 1.0 / K if K else 0.0)
            D = np.zeros((K, K), dtype=np.int32)
            iu = np.triu_indices(K, 1)
            D[iu] = dist[at:at + len(iu[0])]
            at += len(iu[0])
            D = D + D.T
            risks = (D.astype(np.float64) * w[None, :]).sum(axis=1)
            out.append((np.argsort(risks, kind="stable"), risks))
        return out

    def decode_min_risk(self, probs, sizes=None, n_best=None, unit="word"):
        """``decode_scored``'s hypotheses in minimum-Bayes-risk order (``min_risk``): ``(strings, offsets, risks, logps)``,
        each clip's lists reordered by ascending risk.  The first hypothesis is the one with the least expected ``unit``
        errors under the acoustic posteriors, which need not be the most probable one."""
        strings, offsets, logps, ids = self._decode_scored_ids(probs, sizes, n_best)
        out_s, out_o, out_r, out_l = [], [], [], []
        for b, (order, risks) in enumerate(self.min_risk(ids, logps, unit)):
            out_s.append([strings[b][i] for i in order])
            out_o.append([offsets[b][i] for i in order])
            out_r.append([float(risks[i]) for i in order])
            out_l.append([logps[b][i] for i in order])
        return out_s, out_o, out_r, out_l


class GreedyDecoder(Decoder):
    """decoder.py:147-198: argmax per frame, collapse repeats, drop blanks; one path per utterance."""

    def __init__(self, labels, blank_index=0):
        super(GreedyDecoder, self).__init__(labels, blank_index)

    def decode(self, probs, sizes=None):
        import torch
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        res = dec.greedy(probs, sz)
        strings = [[self._to_string(ids)] for ids, _ in res]
        offsets = [[torch.from_numpy(off.astype(np.int32))] for _, off in res]
        return strings, offsets

    def decode_scored(self, probs, sizes=None, n_best=None):
        """``decode`` and, for each clip's one hypothesis, the exact likelihood of its label sequence over the same (still
        resident) probabilities (``dsmi_score``): ``(strings, offsets, logps)`` with ``logps[b][0]`` the natural log."""
        import torch
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        res = dec.greedy(probs, sz)
        strings = [[self._to_string(ids)] for ids, _ in res]
        offsets = [[torch.from_numpy(off.astype(np.int32))] for _, off in res]
        return strings, offsets, self.score_ids(probs, [[ids] for ids, _ in res], sizes)

    def decode_min_risk(self, probs, sizes=None, n_best=None, unit="word"):
        """``decode_scored`` with the risk of each clip's one hypothesis, which is 0 (nothing to choose among):
        ``(strings, offsets, risks, logps)``."""
        strings, offsets, logps = self.decode_scored(probs, sizes, n_best)
        return strings, offsets, [[0.0] for _ in strings], logps

    def _decode_best_ids(self, probs, sizes=None):
        """(the text of each clip, None, its label ids)"""
        import torch
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        res = dec.greedy(probs, sz)
        return [self._to_string(ids) for ids, _ in res], None, [np.asarray(ids, dtype=np.int32) for ids, _ in res]

    # the same in two halves for the batch pipeline (DanSpeechRecognizer.transcribe_batches): the kernel and the copies of its
    # results are queued right behind the forward, on the forward's own stream (on_lane: no side stream), `slot` = one native
    # handle per forward in flight
    on_lane = True

    def decode_enqueue(self, probs, sizes=None, slot=0):
        import torch
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0, slot)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        if not hasattr(dec, "greedy_enqueue"):           # (a native handle without the split entry points: decode now)
            return ("decoded", dec.greedy(probs, sz))
        dec.greedy_enqueue(probs, sz)
        return dec

    def decode_collect(self, ticket):
        import torch
        res = ticket[1] if isinstance(ticket, tuple) else ticket.greedy_collect()
        strings = [[self._to_string(ids)] for ids, _ in res]
        offsets = [[torch.from_numpy(off.astype(np.int32))] for _, off in res]
        return strings, offsets


class BeamCTCDecoder(Decoder):
    """decoder.py:91-144.  ``lm_path`` may be an ARPA text model; ``num_processes`` is accepted for
    signature compatibility (the batch is decoded in parallel on the GPU, one workgroup per utterance)."""

    def __init__(self, labels, lm_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0, beam_width=100,
                 num_processes=4, blank_index=0):
        super(BeamCTCDecoder, self).__init__(labels, blank_index)
        self.lm_path = lm_path
        self.alpha = alpha
        self.beta = beta
        self.cutoff_top_n = cutoff_top_n
        self.cutoff_prob = cutoff_prob
        self.beam_width = beam_width
        self.num_processes = num_processes
        self.last_scores = None

    def _configure(self, native):
        native.set_lm(self.lm_path, self.alpha, self.beta)

    def decode(self, probs, sizes=None):
        return self.decode_collect(self.decode_enqueue(probs, sizes))

    def decode_enqueue(self, probs, sizes=None, slot=0):
        """Launch the search on the current stream and return a ticket at once (the search is a kernel; ctcdecode's
        thread pool has no counterpart).  ``decode_collect(ticket)`` waits and builds the strings."""
        import torch
        probs = self._on_gpu(probs)
        dec = self._dec(probs.device.index or 0, slot)
        sz = None if sizes is None else np.asarray(torch.as_tensor(sizes).cpu()).astype(np.int32)
        dec.beam_enqueue(probs, sz, beam_width=self.beam_width, cutoff_top_n=self.cutoff_top_n, cutoff_prob=self.cutoff_prob)
        return dec

    def new_stream(self, device_index=0):
        """A resumable search of one utterance (``NativeBeamStream``) on the native decoder ``decode`` uses on that device:
        the same language-model tables, alpha and beta, and this decoder's beam_width / cutoff_top_n / cutoff_prob.  It is
        tied to this decoder's settings: a decoder with other settings needs streams of its own."""
        from .. import _native
        return _native.NativeBeamStream(self._dec(device_index), self.beam_width, self.cutoff_top_n, self.cutoff_prob)

    def advance_streams(self, streams, probs_list, n_best=1):
        """Advance streams of ``new_stream`` by one chunk of probabilities each (CUDA [1,T,C] / [T,C], or None) in one launch
        and return ``(strings[N][n_best], offsets[N][n_best])`` over each stream's whole utterance so far: what ``decode``
        returns first for the concatenated chunks."""
        import torch
        from .. import _native
        res = _native.NativeBeamStream.advance_many(streams, probs_list, n_best)
        strings = [[self._to_string(tok[p, :ln[p]]) for p in range(n_best)] for tok, _, ln, _ in res]
        offsets = [[torch.from_numpy(ts[p, :ln[p]].astype(np.int32)) for p in range(n_best)] for _, ts, ln, _ in res]
        return strings, offsets

    def decode_collect(self, ticket):
        tok, ts, ln, sc = ticket.beam_collect()
        self.last_scores = sc      # the reference drops ctcdecode's scores (decoder.py:140); kept for inspection
        return self._beam_strings(tok, ts, ln)

    def decode_scored(self, probs, sizes=None, n_best=None):
        """``decode`` cut to the first ``n_best`` beams (None: all of them) and, for every hypothesis, the exact likelihood of
        its label sequence over the same (still resident) probabilities, all of a clip's hypotheses in one ``dsmi_score``
        call: ``(strings, offsets, logps)`` with ``logps[b][p]`` the natural log.  Unlike the search's own scores
        (``last_scores``) these sum over every alignment, carry no language-model term and are not pruned."""
        return self._decode_scored_ids(probs, sizes, n_best)[:3]

    def _decode_scored_ids(self, probs, sizes=None, n_best=None):
        """``decode_scored`` and the label ids of every hypothesis: (strings, offsets, logps, ids)."""
        probs = self._on_gpu(probs)
        tok, ts, ln, sc = self.decode_enqueue(probs, sizes).beam_collect()
        self.last_scores = sc
        W = tok.shape[1] if n_best is None else max(1, min(int(n_best), tok.shape[1]))
        tok, ts, ln = tok[:, :W], ts[:, :W], ln[:, :W]
        strings, offsets = self._beam_strings(tok, ts, ln)
        ids = [[tok[b, p, :ln[b, p]] for p in range(W)] for b in range(tok.shape[0])]
        return strings, offsets, self.score_ids(probs, ids, sizes), ids

    # ---- LM sentence scoring (dsmi_lm_score): the language model's score of known sentences, n-best rescoring, weight tuning
    def lm_score_ids(self, ids, terms=False):
        """The language model's score of sentences given as label-id sequences (no normalisation), all in ONE
        ``dsmi_lm_score`` call: numpy arrays ``(lm_ln, n_words, n_oov)`` -- the natural-log sentence score as ctcdecode's
        ``Scorer.get_sent_log_prob`` gives it (``</s>`` included, -1000 for every window that holds an out-of-vocabulary word),
        the words between space labels, and how many of them the dictionary does not know -- and, with ``terms``, a list of
        float64 arrays: each sentence's n_words + 1 window terms (2 for no words), which sum to its lm_ln.  ``DsmiError`` when
        the decoder has no language model."""
        from .. import _native
        ids = [np.asarray(t, dtype=np.int32).reshape(-1) for t in ids]
        longest = max([len(t) for t in ids] + [0])
        if longest > _native.LM_SCORE_MAX_TOKENS:
            raise ValueError("sentence of %d labels is longer than %d" % (longest, _native.LM_SCORE_MAX_TOKENS))
        if not ids:
            empty = (np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
            return empty + ([],) if terms else empty
        return self._edit_device().lm_score(ids, want_terms=terms)

    def lm_score(self, texts, terms=False):
        """``lm_score_ids`` of texts, each normalised with ``normalise_transcript``; ``ValueError`` for characters that are
        not labels.  ``-lm_ln.sum() / (n_words.sum() + len(texts))`` is the natural log of the model's perplexity on them."""
        return self.lm_score_ids([self.transcript_ids(self.normalise_transcript(t)) for t in texts], terms)     # every check before any GPU work

    def rescore(self, ids, logps, alpha=None, beta=None, eos=True):
        """Rescore n-best lists with the language model.  ``ids[b]``: clip b's K_b hypotheses as label-id sequences;
        ``logps[b]``: their natural-log acoustic scores (``None`` = infeasible: -inf), as ``decode_scored`` returns them.
        Per clip ``(order, totals)`` with ``totals[i] = logp + alpha * lm + beta * n_words`` in float64, in that order of
        operations -- ``lm`` the hypothesis' ``lm_score_ids`` score, or, with ``eos=False``, that score less its last window's
        term (the ``</s>`` one): the sum the beam search itself accumulates, which never sees ``</s>`` -- and ``order`` the
        stable descending order of the totals, so ties keep the incoming order.  ``alpha`` and ``beta`` default to the
        decoder's own; the language model may be scored for a greedy decoder's list, or with other weights than the search
        ran with.  All hypotheses of all clips go in ONE ``dsmi_lm_score`` call.  The totals are natural-log scores of the
        hypotheses and therefore valid ``logps`` for ``min_risk``: its weights then include the language model."""
        if len(ids) != len(logps):
            raise ValueError("rescore: hypotheses for %d clips and scores for %d" % (len(ids), len(logps)))
        for hyps, lps in zip(ids, logps):
            if len(hyps) != len(lps):
                raise ValueError("rescore: %d hypotheses and %d scores of one clip" % (len(hyps), len(lps)))
        alpha = float(self.alpha if alpha is None else alpha)
        beta = float(self.beta if beta is None else beta)
        lm, n_words = self._lm_terms([t for hyps in ids for t in hyps], eos)
        out, at = [], 0
        for hyps, lps in zip(ids, logps):
            K = len(hyps)
            lp = np.array([-np.inf if v is None else float(v) for v in lps], dtype=np.float64)
            totals = lp + alpha * lm[at:at + K] + beta * n_words[at:at + K].astype(np.float64)
            out.append((np.argsort(-totals, kind="stable"), totals))
            at += K
        return out

    def _lm_terms(self, flat, eos):
        """(lm float64 [N], n_words int32 [N]) of N hypotheses: ``rescore``'s ``lm``."""
        if eos:
            lm, n_words, _ = self.lm_score_ids(flat)
            return lm, n_words
        lm, n_words, _, terms = self.lm_score_ids(flat, terms=True)
        return lm - np.array([t[-1] for t in terms], dtype=np.float64).reshape(len(flat)), n_words

    def decode_rescored(self, probs, sizes=None, n_best=None, alpha=None, beta=None):
        """``decode_scored``'s hypotheses (exact acoustic ``dsmi_score`` likelihoods) in the order of ``rescore``:
        ``(strings, offsets, totals, logps)``, each clip's lists by descending ``logp + alpha * lm + beta * n_words``."""
        strings, offsets, logps, ids = self._decode_scored_ids(probs, sizes, n_best)
        out_s, out_o, out_t, out_l = [], [], [], []
        for b, (order, totals) in enumerate(self.rescore(ids, logps, alpha, beta)):
            out_s.append([strings[b][i] for i in order])
            out_o.append([offsets[b][i] for i in order])
            out_t.append([float(totals[i]) for i in order])
            out_l.append([logps[b][i] for i in order])
        return out_s, out_o, out_t, out_l

    def tune_lm_weights(self, probs, sizes, references, alphas, betas, n_best=8, unit="word", eos=True):
        """Tune alpha and beta on clips with known transcripts.  ONE n-best search at the decoder's current weights
        (``decode_scored``: exact acoustic scores), ONE ``dsmi_lm_score`` call over every hypothesis, ONE
        ``dsmi_edit_distance`` call of every hypothesis against its clip's reference (normalised with
        ``normalise_transcript``; ``unit`` "word" or "char"), then the grid in numpy: at each (alpha, beta) every clip takes
        the hypothesis of the largest ``rescore`` total (the first of equals) and its errors are summed.  Returns a dict:
        ``errors`` and ``ref_tokens`` int64 [len(alphas), len(betas)], ``best_index`` (i, j) -- the fewest errors, then the
        lowest alpha index, then the lowest beta index -- ``best`` (alphas[i], betas[j]) and ``error_rate`` there (None when
        the references hold no token).  It tunes a RESCORING of the current search's n-best lists, not the search's own
        pruning: a hypothesis the search at its current weights dropped cannot win at any grid point."""
        references = [self.normalise_transcript(t) for t in references]
        if len(references) != len(probs):
            raise ValueError("tune_lm_weights: %d references and a batch of %d" % (len(references), len(probs)))
        alphas = np.asarray(alphas, dtype=np.float64).reshape(-1)
        betas = np.asarray(betas, dtype=np.float64).reshape(-1)
        strings, _, logps, ids = self._decode_scored_ids(probs, sizes, n_best)
        flat = [t for hyps in ids for t in hyps]
        clip = np.array([b for b, hyps in enumerate(ids) for _ in hyps], dtype=np.int64)
        lm, n_words = self._lm_terms(flat, eos)
        counts, ref_lens = self.error_counts([references[b] for b in clip], [s for row in strings for s in row], unit)
        dist = counts[:, 0].astype(np.int64)
        lp = np.array([-np.inf if v is None else float(v) for row in logps for v in row], dtype=np.float64)
        starts = np.concatenate(([0], np.cumsum([len(hyps) for hyps in ids])))
        errors = np.zeros((len(alphas), len(betas)), dtype=np.int64)
        nw = n_words.astype(np.float64)
        for i, a in enumerate(alphas):
            for j, bt in enumerate(betas):
                totals = lp + a * lm + bt * nw
                errors[i, j] = sum(int(dist[s + int(np.argmax(totals[s:e]))]) for s, e in zip(starts[:-1], starts[1:]) if e > s)
        total_ref = int(sum(int(ref_lens[s]) for s, e in zip(starts[:-1], starts[1:]) if e > s))
        best = np.unravel_index(int(np.argmin(errors)), errors.shape) if errors.size else (0, 0)
        i, j = int(best[0]), int(best[1])
        return {"errors": errors, "ref_tokens": np.full(errors.shape, total_ref, dtype=np.int64), "best_index": (i, j),
                "best": (float(alphas[i]), float(betas[j])) if errors.size else None,
                "error_rate": int(errors[i, j]) / total_ref if errors.size and total_ref else None}

    def _decode_best_ids(self, probs, sizes=None):
        """(the first beam's text of each clip, None, its label ids)"""
        probs = self._on_gpu(probs)
        tok, ts, ln, sc = self.decode_enqueue(probs, sizes).beam_collect()
        self.last_scores = sc
        strings, _ = self._beam_strings(tok[:, :1], ts[:, :1], ln[:, :1])
        return [s[0] for s in strings], None, [np.asarray(tok[b, 0, :ln[b, 0]], dtype=np.int32) for b in range(tok.shape[0])]

    def _beam_strings(self, tok, ts, ln):
        import torch
        # label strings and emission offsets of every beam, built in bulk: the valid prefixes of all beams are gathered
        # once (a few hundred thousand ids instead of B x beam x T), turned into ONE string, and cut by length
        B, W = tok.shape[0], tok.shape[1]
        lmax = int(ln.max()) if ln.size else 0
        valid = np.arange(lmax, dtype=np.int32)[None, None, :] < ln[:, :, None]
        flat_len = ln.reshape(-1).tolist()
        flat_ts = torch.split(torch.from_numpy(ts[:, :, :lmax][valid]), flat_len)
        ids = tok[:, :, :lmax][valid]
        cuts = np.concatenate(([0], np.cumsum(ln.reshape(-1), dtype=np.int64))).tolist()
        if self._code_points is not None:
            big = self._code_points[ids].tobytes().decode("utf-32-le")
            flat_str = [big[cuts[k]:cuts[k + 1]] for k in range(B * W)]
        else:
            flat_str = ["".join(self.int_to_char[int(i)] for i in ids[cuts[k]:cuts[k + 1]]) for k in range(B * W)]
        strings = [flat_str[b * W:(b + 1) * W] for b in range(B)]
        offsets = [list(flat_ts[b * W:(b + 1) * W]) for b in range(B)]
        return strings, offsets
