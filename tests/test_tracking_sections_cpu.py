"""The tracking chain with the section tracker's parts, without a GPU (yourmt3_amd/tracking.py): layout, pack and unpack for every set of
switches and every number of beats that takes another path; the result of no records is the specifications'; the sections'
frames_per_second refusal fires before anything is compiled."""
import itertools

import numpy as np
import pytest
import torch

from yourmt3_amd import sections as S
from yourmt3_amd import tracking as Tk

N_WINDOWS, CAP = 7, 11                                                      # the beat and metre buffers are longer than any n_beats below


def _parts(bars, chords, sections, n_beats, n_notes):
    """CPU tensors at the sizes the device pass gives them, every word distinct (the 64-bit parts' high words too), n_beats where it is read"""
    sizes = [("ticks", (n_notes, 2), torch.int32), ("beat_result", (4,), torch.int64), ("tempo", (N_WINDOWS,), torch.int32), ("beats", (CAP,), torch.int32)]
    sizes += [("novelty", (CAP + 1,), torch.int64), ("section", (CAP + 1,), torch.int32), ("section_result", (8,), torch.int64)] if sections else []
    sizes += [("metre", (CAP,), torch.int32), ("bar_result", (8,), torch.int64)] if bars else []          # (not in layout order: layout orders)
    sizes += [("chord", (CAP + 2,), torch.int32), ("chord_result", (8,), torch.int64)] if chords else []
    parts, at = {}, 1000
    for name, shape, dtype in sizes:
        n = int(np.prod(shape))
        v = torch.arange(at, at + n, dtype=dtype) * (3 + (1 << 33) if dtype == torch.int64 else 1)
        parts[name], at = v.reshape(shape), at + n
    parts["beat_result"][0] = n_beats
    return parts


def test_the_order_ends_in_the_sections_parts():
    assert Tk.ORDER == ("ticks", "beat_result", "tempo", "beats", "bar_result", "metre", "chord_result", "chord", "section_result", "section", "novelty")


@pytest.mark.parametrize("bars,chords,sections,n_beats,n_notes", list(itertools.product((False, True), (False, True), (False, True), (0, 1, 2, 5), (0, 3))))
def test_what_is_packed_is_what_is_unpacked(bars, chords, sections, n_beats, n_notes):
    parts = _parts(bars, chords, sections, n_beats, n_notes)
    lay = Tk.layout(parts)
    names = ["ticks", "beat_result", "tempo", "beats"] + (["bar_result", "metre"] if bars else []) + (["chord_result", "chord"] if chords else []) + \
        (["section_result", "section", "novelty"] if sections else [])
    assert [name for name, _ in lay] == names
    assert dict(lay) == {name: parts[name].numel() * (2 if parts[name].dtype == torch.int64 else 1) for name in names}
    riders = torch.arange(5, dtype=torch.uint8)
    both = torch.cat([riders] + Tk.pack(parts)).numpy()
    tracked = Tk.unpack(both[5:].view(np.int32), lay)
    per_beat = n_beats if n_beats >= 2 else 0
    want = {"beats": parts["beats"][:n_beats], "tempo": parts["tempo"], "ticks": parts["ticks"]}
    if bars:
        want.update(metre=parts["metre"][:per_beat], bar_result=parts["bar_result"])
    if chords:
        want.update(chord=parts["chord"][:per_beat], chord_result=parts["chord_result"])
    if sections:
        want.update(section=parts["section"][:per_beat], novelty=parts["novelty"][:per_beat], section_result=parts["section_result"])
    assert set(tracked) == set(want)
    for name, v in want.items():
        assert tracked[name].dtype == (np.int64 if name.endswith("result") or name == "novelty" else np.int32), name
        assert tracked[name].shape == tuple(v.shape) and tracked[name].tolist() == v.tolist(), name


@pytest.mark.parametrize("bars,chords", list(itertools.product((False, True), repeat=2)))
def test_the_empty_result_is_the_specifications(bars, chords):
    none = Tk.empty(bars, chords, sections=True)
    without = Tk.empty(bars, chords)
    assert set(none) == set(without) | {"section", "novelty", "section_result"} and set(Tk.empty(bars, chords, False)) == set(without)
    for name in without:
        assert none[name].dtype == without[name].dtype and none[name].tolist() == without[name].tolist(), name
    for name, want in zip(("section", "novelty", "section_result"), S.track_sections([], [], 1)):
        assert none[name].dtype == want.dtype and none[name].shape == want.shape and none[name].tolist() == want.tolist(), name
    assert none["section"].shape == none["novelty"].shape == (0,) and not none["section_result"].any()


def test_the_frames_per_second_must_agree_before_anything_is_compiled():
    class NoModel:                                                          # any use of the model would raise AttributeError
        pass

    with pytest.raises(ValueError, match="^the sections' frames_per_second must be the beats'$"):
        Tk.Chain(NoModel(), 100, 8, {}, None, None, {"frames_per_second": 50.0})
    with pytest.raises(ValueError, match="^the sections' frames_per_second must be the beats'$"):
        Tk.Chain(NoModel(), 100, 8, {"frames_per_second": 50.0}, {"frames_per_second": 50.0}, {"frames_per_second": 50.0}, section_params={"frames_per_second": 100.0})
    with pytest.raises(ValueError, match="^the chords' frames_per_second must be the beats'$"):             # the earlier trackers' refusals come first
        Tk.Chain(NoModel(), 100, 8, None, None, {"frames_per_second": 100.5}, {"frames_per_second": 100.5})
    with pytest.raises(AttributeError):                                     # equal ones pass the check and reach the model
        Tk.Chain(NoModel(), 100, 8, {"frames_per_second": 50.0}, None, None, {"frames_per_second": 50})
