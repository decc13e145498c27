"""The host-side schedule of the batch pipeline (``DanSpeechRecognizer.transcribe_batches``): how a caller's batches are cut, which
consecutive batches share a forward, how a sized source's last round is dealt over the lanes, how many forwards are still to come
and which kernel forms a forward gets for it, how many lanes pay, and how a forward's results go back to its batches.  The engine
runs what is decided here.  Pure Python: no torch, no numpy, no library handle (tests/test_batch_plan_host.py runs on the CPU)."""


def longest_first(lengths):
    """Positions of ``lengths`` by descending length, equal lengths in their own order (a stable sort): the order a batch's
    clips run in (pack_padded_sequence's, reference model.py:117)."""
    return sorted(range(len(lengths)), key=lambda i: -lengths[i])


def cut_batch(n, lengths, merge):
    """A caller's batch of ``n`` clips as forwards of at most ``merge``: ``None`` when it is handed through whole (``merge <= 0``,
    or it fits), otherwise the caller positions of every piece -- longest clips first, so that a forward's clips are of a kind.
    ``lengths=None``: a device-resident batch, longest first already, cut into consecutive ranges."""
    if merge <= 0 or n <= merge:
        return None
    order = list(range(n)) if lengths is None else longest_first(lengths)
    return [order[lo:lo + merge] for lo in range(0, n, merge)]


def count_pieces(batches, merge):
    """How many pieces ``cut_batch`` will make of a SIZED source (a list of lists), or None: the pipeline then knows when it is
    enqueueing its last forwards and gives a forward that has the chip to itself the kernels of a lone batch (``chip_forms``)."""
    if not hasattr(batches, "__len__"):
        return None
    try:
        # (every sized source is walked once here, before its first forward -- for a list that is nothing; a Dataset-like source
        # pays a whole extra pass, and one that can be iterated only once is empty afterwards.  Known, and kept as it is.)
        return sum(1 if (merge <= 0 or len(b) <= merge) else -(-len(b) // merge) for b in batches)
    except TypeError:
        return None


_NOTHING = object()


class ForwardGrouper(object):
    """Which consecutive batches of ``source`` become one forward: batches of one ``kind(batch)`` (anything hashable; the engine
    says host clips or device-resident ones and, for those, their sample type) up to ``merge_clips`` clips.  ``total``: the number
    of batches ``source`` will give, where that is known; ``lanes``: the forwards in flight, settable once the first group has
    been formed (how many lanes pay depends on that group's size).  The source is read at most one batch past the group being
    returned; that batch waits in ``held``.

    Threading: ``next_group`` runs on the pipeline's helper thread; ``forwards_to_come`` (and setting ``lanes``) on the consumer's,
    and only between one ``next_group`` having returned and the next being submitted -- nothing here is locked."""

    def __init__(self, source, merge_clips, lanes, total=None, balance_tail=True, kind=None):
        self.source = iter(source)
        self.merge_clips, self.lanes, self.total, self.balance_tail = merge_clips, lanes, total, balance_tail
        self.kind = kind or (lambda batch: None)
        self.held = _NOTHING             # a batch read from the source that did not fit the group being put together
        self.taken = 0                   # batches read from the source so far
        self.ended = False               # the source has ended
        self.formed = 0                  # forwards put together so far
        self.tail = None                 # the call's last round, once it is known: batches per forward still to be formed

    def _next_batch(self):
        if self.held is not _NOTHING:
            batch, self.held = self.held, _NOTHING
            return batch
        batch = next(self.source, _NOTHING)
        if batch is _NOTHING:
            self.ended = True
        else:
            self.taken += 1
        return batch

    def _left(self):
        """Batches of a sized source that are in no forward yet."""
        return self.total - self.taken + (0 if self.held is _NOTHING else 1)

    def _tail_plan(self, first_len):
        """A sized source's LAST ROUND of forwards is dealt evenly over the lanes: 20 batches of 32 clips on four lanes are
        eight forwards of 64 clips and then four of 32 -- not ten of 64, whose last two run on two lanes while the other two
        stand empty (a 20-batch call: 115.25 -> 112.22 ms, profiles/r06_short_calls.txt, AFTER -> FINAL; FINAL also holds the
        dense-kernel token and the uploads by kernel, so the figure is not this plan's alone).  -> batches this forward may
        merge, or None."""
        index, self.formed = self.formed, self.formed + 1
        if self.total is None or self.merge_clips <= 0 or self.lanes < 2 or not self.balance_tail:
            return None
        if self.tail is None:
            # (the FIRST forward is planned with the lane count the call started with, before the engine has reduced it to the
            # lanes that pay: a wide model on two lanes has a short call's only round dealt over four.  Known, and kept as it is.)
            if index % self.lanes:                # rounds start on the first lane
                return None
            full = max(1, self.merge_clips // max(first_len, 1))
            rem = self._left() + 1                # batches not yet in a forward, this one's first included
            if rem > self.lanes * full:
                return None
            k = min(self.lanes, rem)
            self.tail = [rem // k + (1 if i < rem % k else 0) for i in range(k)]
        return self.tail.pop(0) if self.tail else None

    def next_group(self):
        """The batches of the next forward, or None at the end of the source."""
        first = self._next_batch()
        if first is _NOTHING:
            return None
        group, nclips, kind = [first], len(first), self.kind(first)
        most = self._tail_plan(len(first))
        while nclips and nclips < self.merge_clips and (most is None or len(group) < most):
            batch = self._next_batch()
            if batch is _NOTHING:
                break
            if self.kind(batch) != kind or nclips + len(batch) > self.merge_clips:
                self.held = batch
                break
            group.append(batch)
            nclips += len(batch)
        return group

    def forwards_to_come(self, per_forward):
        """Forwards that will follow the one being enqueued (which merged ``per_forward`` batches), as far as this call can know
        WITHOUT asking the source for anything (a live source must not be waited for here): from the batch count of a sized
        source (``total``), otherwise none once the source has ended and 'plenty' before."""
        if self.ended:
            return 0 if self.held is _NOTHING else 1
        if self.total is not None:
            return min(-(-self._left() // max(per_forward, 1)), self.lanes)
        return self.lanes


def chip_forms(busy, to_come, lanes):
    """The kernel forms of a forward, ``(inflight, ring_windows)`` for its model handle, from what will BE on the chip (``busy``
    forwards running, this one, ``to_come`` behind it) and not from what the call was set up for: a forward that is enqueued with
    nothing else running and nothing to come (a call of one or two batches) takes the forms of a lone batch (the whole-device
    recurrent kernel, or two ring windows side by side); two forwards that will share the chip between them (a call of three or
    four batches, the last forwards of a sized source) take two ring windows each; anything more, one window each.
    profiles/r06_short_calls.txt"""
    expect = busy + 1 + to_come
    return (1 if expect <= 1 else max(2, lanes)), (2 if expect == 2 else 0)


def lanes_that_pay(hidden, kind, most, clips):
    """Forwards in flight when the caller did not say.  Several forwards side by side pay where the recurrent kernel of
    each holds a fifth of the chip (the ring form: GRU / RNN up to 896 units, LSTM up to 512, one window of up to 64
    clips -- ``transcribe_batches`` cuts larger batches to that) and the dense kernels of the others fill the rest.  A model
    whose recurrent kernel takes the whole device runs two: their recurrent launches take turns (csrc/api.hip, the turn
    lock) and each forward's GEMM runs beside the other's launch; a third forward only slows those launches down (config 4:
    33.7 ms per batch with two, 35.0 with three, 37.1 with four; profiles/r06_config4.txt)."""
    ring = hidden % 16 == 0 and hidden <= (512 if kind == "lstm" else 896)
    return most if ring and clips <= 64 else min(most, 2)


def split_results(part_lengths, results):
    """A forward's results -> one list per batch it was merged from (``part_lengths``: the clips of each, empty ones included)."""
    out, lo = [], 0
    for n in part_lengths:
        out.append(results[lo:lo + n])
        lo += n
    return out
