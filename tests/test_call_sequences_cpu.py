"""The call order of the handle-state tests (tests/call_sequences.py) is what their coverage claim rests on: every ordered pair of every
catalogue's kinds, (a, a) included, is executed as two consecutive calls exactly once."""
import pytest
import torch

from call_sequences import CATALOGUES, euler_sequence, pair_counts, pick_eos

KIND_LISTS = [list(range(n)) for n in (1, 2, 3, 8)] + [[k.name for k in make()] for make in CATALOGUES.values()]
IDS = ["n1", "n2", "n3", "n8"] + [f"catalogue_{c}" for c in CATALOGUES]


@pytest.mark.parametrize("kinds", KIND_LISTS, ids=IDS)
def test_every_ordered_pair_is_met_exactly_once(kinds):
    n = len(kinds)
    seq = euler_sequence(kinds)
    assert len(seq) == n * n + 1
    counts = pair_counts(seq)
    assert counts == {(a, b): 1 for a in kinds for b in kinds}
    assert seq[0] == seq[-1] == kinds[0]
    assert seq == euler_sequence(kinds)                      # no randomness


def test_the_empty_catalogue_has_the_empty_sequence():
    assert euler_sequence([]) == []


@pytest.mark.parametrize("name", list(CATALOGUES))
def test_kind_names_are_unique_and_kinds_are_closures(name):
    kinds = CATALOGUES[name]()
    names = [k.name for k in kinds]
    assert len(set(names)) == len(names), names
    assert all(callable(k.run) and callable(k.make) for k in kinds)
    assert [k.name for k in CATALOGUES[name]()] == names    # a catalogue is a function of nothing


def test_pick_eos_splits_every_required_kind():
    streams = {"a": torch.tensor([[5, 7, 9, 9], [5, 8, 7, 9], [5, 6, 6, 6]]), "b": torch.tensor([[5, 8, 8], [5, 7, 8]]),
               "c": torch.tensor([[5, 9, 9]])}
    # 5: every row; 9: no row of b; 7 splits a (first steps 1, 2) and b; 8 splits a and b too, with fewer distinct first steps
    assert pick_eos(streams, ["a", "b"], pad_id=0) == 7
    with pytest.raises(AssertionError):
        pick_eos(streams, ["a", "b", "c"], pad_id=0)       # one row cannot be split
