"""The tracking chain without a GPU (yourmt3_amd/tracking.py): what rides back is taken apart where it was put together, for every set of
switches and every number of beats that takes another path; the result of no records is the specifications'; the frames_per_second
refusal fires before anything is compiled."""
import itertools

import numpy as np
import pytest
import torch

from yourmt3_amd import bars as B
from yourmt3_amd import beats as T
from yourmt3_amd import chords as Ch
from yourmt3_amd import tracking as Tk

N_WINDOWS, CAP = 7, 11                                                      # the beat and metre buffers are longer than any n_beats below


def _parts(bars, chords, n_beats, n_notes):
    """CPU tensors at the sizes the device pass gives them, every word distinct (the results' high words too), n_beats where it is read"""
    sizes = [("ticks", (n_notes, 2), torch.int32), ("beat_result", (4,), torch.int64), ("tempo", (N_WINDOWS,), torch.int32), ("beats", (CAP,), torch.int32)]
    sizes += [("metre", (CAP,), torch.int32), ("bar_result", (8,), torch.int64)] if bars else []          # (not in layout order: layout orders)
    sizes += [("chord", (CAP + 2,), torch.int32), ("chord_result", (8,), torch.int64)] if chords else []   # (an object made for more beats)
    parts, at = {}, 1000
    for name, shape, dtype in sizes:
        n = int(np.prod(shape))
        v = torch.arange(at, at + n, dtype=dtype) * (3 + (1 << 33) if dtype == torch.int64 else 1)
        parts[name], at = v.reshape(shape), at + n
    parts["beat_result"][0] = n_beats
    return parts


@pytest.mark.parametrize("bars,chords,n_beats,n_notes", list(itertools.product((False, True), (False, True), (0, 1, 2, 5), (0, 3))))
def test_what_is_packed_is_what_is_unpacked(bars, chords, n_beats, n_notes):
    parts = _parts(bars, chords, n_beats, n_notes)
    lay = Tk.layout(parts)
    names = ["ticks", "beat_result", "tempo", "beats"] + (["bar_result", "metre"] if bars else []) + (["chord_result", "chord"] if chords else [])
    assert [name for name, _ in lay] == names
    assert dict(lay) == {name: parts[name].numel() * (2 if parts[name].dtype == torch.int64 else 1) for name in names}
    riders = torch.arange(5, dtype=torch.uint8)                             # a caller's records and velocities come first, of any length
    both = torch.cat([riders] + Tk.pack(parts)).numpy()
    tracked = Tk.unpack(both[5:].view(np.int32), lay)
    per_beat = n_beats if n_beats >= 2 else 0
    want = {"beats": parts["beats"][:n_beats], "tempo": parts["tempo"], "ticks": parts["ticks"]}
    if bars:
        want.update(metre=parts["metre"][:per_beat], bar_result=parts["bar_result"])
    if chords:
        want.update(chord=parts["chord"][:per_beat], chord_result=parts["chord_result"])
    assert set(tracked) == set(want)
    for name, v in want.items():
        assert tracked[name].dtype == (np.int64 if name.endswith("result") else np.int32), name
        assert tracked[name].shape == tuple(v.shape) and tracked[name].tolist() == v.tolist(), name
    assert tracked["ticks"].shape == (n_notes, 2) and tracked["beats"].shape == (n_beats,) and tracked["tempo"].shape == (N_WINDOWS,)


@pytest.mark.parametrize("bars,chords", list(itertools.product((False, True), repeat=2)))
def test_the_empty_result_is_the_specifications(bars, chords):
    none = Tk.empty(bars, chords)
    assert set(none) == {"beats", "tempo", "ticks"} | ({"metre", "bar_result"} if bars else set()) | ({"chord", "chord_result"} if chords else set())
    beats, _, beat_result = T.track_beats([], 1)
    assert none["beats"].tolist() == beats.tolist() == [] and none["beats"].dtype == beats.dtype and beat_result[0] == 0
    assert none["tempo"].shape == (0,) and none["tempo"].dtype == np.int32 and none["ticks"].shape == (0, 2) and none["ticks"].dtype == np.int32
    assert none["ticks"].tolist() == T.beat_positions([], beats).tolist()
    for on, names, spec in ((bars, ("metre", "bar_result"), B.track_bars), (chords, ("chord", "chord_result"), Ch.track_chords)):
        if on:
            for name, want in zip(names, spec([], beats, 1)):
                assert none[name].dtype == want.dtype and none[name].tolist() == want.tolist(), name
    if bars:
        assert none["bar_result"][3] == -1 == B.track_bars([], [], 1)[1][3]
    if chords:
        assert not none["chord_result"].any() and not Ch.track_chords([], [], 1)[1].any()


def test_the_frames_per_second_must_agree_before_anything_is_compiled():
    class NoModel:                                                          # any use of the model would raise AttributeError
        pass

    with pytest.raises(ValueError, match="^the bars' frames_per_second must be the beats'$"):
        Tk.Chain(NoModel(), 100, 8, {}, {"frames_per_second": 50.0}, None)
    with pytest.raises(ValueError, match="^the chords' frames_per_second must be the beats'$"):
        Tk.Chain(NoModel(), 100, 8, {"frames_per_second": 50.0}, {"frames_per_second": 50.0}, {"frames_per_second": 100.0})
    with pytest.raises(ValueError, match="^the chords' frames_per_second must be the beats'$"):
        Tk.Chain(NoModel(), 100, 8, None, None, {"frames_per_second": 100.5})
    with pytest.raises(AttributeError):                                     # equal ones pass the check and reach the model
        Tk.Chain(NoModel(), 100, 8, {"frames_per_second": 50.0}, {"frames_per_second": 50.0}, {"frames_per_second": 50})
