"""The batch pipeline's schedule (danspeech_amd/batch_plan.py), checked on the CPU without torch: every row of
tests/batch_plan_table.json -- written by the planning closures of ``DanSpeechRecognizer._transcribe_forwards`` and
``transcribe_batches`` as they stood at commit 5ad27dd, BEFORE batch_plan.py existed (see the file's header) -- the answers the
short-call measurements rely on, stated here by name, and what must hold for every source."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from danspeech_amd import batch_plan as bp


class _Batch(object):
    """A caller's batch as far as the schedule looks at it: its size, its kind and (for the tests) its place in the source."""

    def __init__(self, index, n, kind):
        self.index, self.n, self.kind = index, n, kind

    def __len__(self):
        return self.n


class _Counted(object):
    """An iterator that says how many items it has handed out."""

    def __init__(self, items):
        self.items, self.given = iter(items), 0

    def __iter__(self):
        return self

    def __next__(self):
        item = next(self.items)
        self.given += 1
        return item


def _run(sizes, kinds=None, lanes=4, merge=64, total=None, balance=True, lanes_after=None):
    """The engine's loop without the engine -> per forward: batch indices, forwards_to_come, batches read so far."""
    batches = [_Batch(i, n, k) for i, (n, k) in enumerate(zip(sizes, kinds or ["host"] * len(sizes)))]
    source = _Counted(batches)
    grouper = bp.ForwardGrouper(source, merge, lanes, total, balance, kind=lambda b: b.kind)
    groups, to_come, reads = [], [], []
    group = grouper.next_group()
    if lanes_after is not None:
        grouper.lanes = lanes_after
    while group is not None:
        groups.append([b.index for b in group])
        reads.append(source.given)
        to_come.append(grouper.forwards_to_come(len(group)))
        group = grouper.next_group()
    assert grouper.next_group() is None            # the end of the source stays the end
    return groups, to_come, reads


@pytest.fixture(scope="module")
def table():
    doc = json.load(open(os.path.join(ROOT, "tests", "batch_plan_table.json")))
    assert "PARENT" in doc["header"]["generated_by"] and "5ad27dd" in doc["header"]["generated_by"]
    return doc


def _cases(table):
    sources = {s["name"]: s for s in table["sources"]}
    for row in table["forwards"]:
        src = sources[row["source"]]
        yield row, src["sizes"], src["kinds"]


def test_the_grid_of_the_table(table):
    """What the table has to contain, so that a regenerated one cannot quietly shrink."""
    sources = {s["name"]: s for s in table["sources"]}
    for n in (1, 2, 3, 4, 5, 8, 9, 20):
        assert sources["32x%d" % n]["sizes"] == [32] * n
    assert sources["16x13"]["sizes"] == [16] * 13 and sources["mixed"]["sizes"] == [40, 40, 10, 0, 64, 30]
    assert set(sources["empties"]["sizes"]) == {0} and 150 in sources["oversized"]["sizes"]
    assert set(sources["host_device"]["kinds"]) == {"host", "int16"} and set(sources["two_dtypes"]["kinds"]) == {"int16", "float32"}
    rows = table["forwards"]
    assert 300 < len(rows) < 800
    for name in sources:
        mine = [r for r in rows if r["source"] == name]
        assert {(r["lanes"], r["lanes_after"]) for r in mine} == {(1, 1), (2, 2), (3, 3), (4, 4), (4, 2)}
        assert {r["merge"] for r in mine} == {0, 64, 128} and {r["total"] is None for r in mine} == {True, False}
        assert {r["balance"] for r in mine} == {True, False}
    assert len(table["forms"]) == sum((lanes + 1) ** 2 for lanes in (1, 2, 3, 4))
    assert any(c["n"] == 150 and c["merge"] == 64 and c["lengths"] for c in table["cuts"])
    assert any(c["n"] == 150 and c["merge"] == 64 and c["lengths"] is None for c in table["cuts"])


def test_forwards_row_by_row(table):
    wrong = []
    for row, sizes, kinds in _cases(table):
        got = _run(sizes, kinds, row["lanes"], row["merge"], row["total"], row["balance"], row["lanes_after"])
        if list(got) != [row["groups"], row["to_come"], row["reads"]]:
            wrong.append((row, got))
    assert not wrong, "%d rows differ, the first: %s\n  plan %s" % ((len(wrong),) + wrong[0])


def test_chip_forms_row_by_row(table):
    for busy, to_come, lanes, inflight, ring_windows in table["forms"]:
        assert bp.chip_forms(busy, to_come, lanes) == (inflight, ring_windows), (busy, to_come, lanes)


def test_cuts_and_totals_row_by_row(table):
    for c in table["cuts"]:
        assert bp.cut_batch(c["n"], c["lengths"], c["merge"]) == c["cuts"], (c["n"], c["merge"])
    for t in table["totals"]:
        if t["sizes"] is None:
            batches = [iter([1, 2])]                            # a sized source of things without a length: not known
        else:
            batches = [[0] * n for n in t["sizes"]]
            batches = {"list": batches, "tuple": tuple(batches), "iterator": iter(batches)}[t["source"]]
        assert bp.count_pieces(batches, t["merge"]) == t["total"], t


@pytest.mark.parametrize("sizes, total, lanes, per_forward, to_come", [
    # 20 batches of 32 on four lanes: eight forwards of 64 and a last round of four of 32 -- not ten of 64
    ([32] * 20, 20, 4, [2] * 8 + [1] * 4, [4, 4, 4, 4, 4, 4, 3, 2, 3, 2, 1, 0]),
    ([32] * 20, None, 4, [2] * 10, [4] * 10),                   # ... which an unsized source cannot know
    ([32] * 3, 3, 4, [1, 1, 1], [2, 1, 0]),
    ([32] * 5, 5, 4, [2, 1, 1, 1], [2, 2, 1, 0]),
    ([32] * 9, 9, 4, [2, 2, 2, 2, 1], [4, 3, 2, 1, 0]),
    ([16] * 13, 13, 4, [4, 3, 3, 3], None),
    ([40, 40, 10, 0, 64, 30], 6, 4, [1, 3, 1, 1], None),
    ([32] * 6, 6, 2, [2, 2, 1, 1], None),
])
def test_named_cases(sizes, total, lanes, per_forward, to_come):
    groups, got, _ = _run(sizes, lanes=lanes, merge=64, total=total)
    assert [len(g) for g in groups] == per_forward
    assert to_come is None or got == to_come


def test_short_calls_get_a_lone_batch_s_kernels():
    """What profiles/r06_short_calls.txt measured: one batch alone on the chip runs as a lone batch, two forwards that share it take
    two ring windows each, more take one window each and the call's lane count."""
    assert bp.chip_forms(0, 0, 4) == (1, 0)
    assert bp.chip_forms(0, 1, 4) == (4, 2) and bp.chip_forms(1, 0, 4) == (4, 2) and bp.chip_forms(1, 0, 2) == (2, 2)
    assert bp.chip_forms(1, 1, 4) == (4, 0) and bp.chip_forms(4, 4, 4) == (4, 0) and bp.chip_forms(0, 2, 2) == (2, 0)


def test_lanes_that_pay():
    for kind, widest in (("gru", 896), ("rnn", 896), ("lstm", 512)):
        assert bp.lanes_that_pay(widest, kind, 4, 64) == 4 and bp.lanes_that_pay(widest, kind, 4, 65) == 2
        assert bp.lanes_that_pay(widest + 16, kind, 4, 32) == 2 and bp.lanes_that_pay(widest - 8, kind, 4, 32) == 2
        assert bp.lanes_that_pay(widest + 16, kind, 1, 32) == 1 and bp.lanes_that_pay(widest, kind, 3, 1) == 3


def test_invariants_over_the_grid(table):
    for row, sizes, kinds in _cases(table):
        groups, _, reads = _run(sizes, kinds, row["lanes"], row["merge"], row["total"], row["balance"], row["lanes_after"])
        # every batch in exactly one forward, in source order
        assert [i for g in groups for i in g] == list(range(len(sizes))), row
        for g, read in zip(groups, reads):
            assert len(g) == 1 or sum(sizes[i] for i in g) <= row["merge"], row           # no forward beyond merge_clips but a single batch
            assert len({kinds[i] for i in g}) == 1, row                                      # no forward mixes kinds
            assert read <= g[-1] + 2, row                                                    # at most one batch read past the forward
        if row["lanes"] == 1 and row["merge"] == 0:
            assert reads == list(range(1, len(sizes) + 1)) and all(len(g) == 1 for g in groups), row       # strictly one batch per call


def test_split_results_inverts_the_grouping(table):
    for row, sizes, kinds in _cases(table):
        for g in row["groups"]:
            lengths = [sizes[i] for i in g]
            merged = [(i, k) for i in g for k in range(sizes[i])]          # what the forward ran: the clips of its non-empty batches
            parts = bp.split_results(lengths, merged)
            assert len(parts) == len(g)
            for i, part in zip(g, parts):
                assert part == [(i, k) for k in range(sizes[i])]
    assert bp.split_results([0, 0], []) == [[], []] and bp.split_results([], []) == []


def test_longest_first_is_the_stable_descending_order():
    import numpy as np
    rng = np.random.default_rng(2)
    for n in (0, 1, 2, 33, 64, 200):
        lengths = [int(x) for x in rng.integers(1, 12, n)]                 # (few distinct values: the ties are the test)
        assert bp.longest_first(lengths) == np.argsort([-l for l in lengths], kind="stable").tolist()
    assert bp.longest_first([5, 9, 5, 9, 1]) == [1, 3, 0, 2, 4]


def test_cut_batch_150_by_64():
    lengths = [(7 * i) % 31 for i in range(150)]
    cuts = bp.cut_batch(150, lengths, 64)
    assert [len(c) for c in cuts] == [64, 64, 22] and sorted(i for c in cuts for i in c) == list(range(150))
    flat = [lengths[i] for c in cuts for i in c]
    assert flat == sorted(flat, reverse=True)
    assert bp.cut_batch(150, None, 64) == [list(range(0, 64)), list(range(64, 128)), list(range(128, 150))]
    assert bp.cut_batch(64, lengths[:64], 64) is None and bp.cut_batch(150, lengths, 0) is None


def test_the_module_needs_neither_torch_nor_numpy():
    import subprocess
    code = "import sys; sys.path.insert(0, %r); from danspeech_amd import batch_plan; assert 'torch' not in sys.modules and 'numpy' not in sys.modules" % ROOT
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
