"""The tracking chain on the device (yourmt3_amd/tracking.py) against the host specifications, for every set of switches: the chain object
on device records (known music, the same under a device count, fewer than two beats, no records), and the in-place route of
TaskManager.tokens_to_notes_device against the uploaded route on the same notes."""
import itertools

import numpy as np
import pytest
import torch

import bar_cases as BC
import chord_cases as CC
from test_chords import CFG, _bytes, _count, _music
from test_gpu_parity import _model
from yourmt3_amd import bars as B
from yourmt3_amd import beats as T
from yourmt3_amd import chords as Ch
from yourmt3_amd import tracking as Tk
from yourmt3_amd.metrics import to_records

pytestmark = pytest.mark.gpu

SWITCHES = list(itertools.product((False, True), repeat=2))
POP, POP_FRAMES = CC.music("pop")[0], CC.music("pop")[2]
ONE = BC.records(np.array([0.5]), pitch=np.array([60]), length=np.array([0.3]))
INPUTS = {"pop": (POP, POP_FRAMES, None), "pop_under_a_count": (POP, POP_FRAMES, 201), "one_note": (ONE, 200, None), "no_records": (ONE[:0], 200, None)}


@pytest.fixture(scope="module")
def model():
    m = _model(CFG, max_batch=2)
    yield m
    m.close()


def _specification(rec, n_frames, bars, chords, n_rows=None):
    """what the chain must give on the live records `rec`; `n_rows`: the ticks' rows, -1 beyond the live ones"""
    beats, tempo, _ = T.track_beats(rec, n_frames)
    ticks = np.full((len(rec) if n_rows is None else n_rows, 2), -1, np.int32)
    ticks[:len(rec)] = T.beat_positions(rec, beats)
    want = {"beats": beats, "tempo": tempo, "ticks": ticks}
    if bars:
        want["metre"], want["bar_result"] = B.track_bars(rec, beats, n_frames)
    if chords:
        want["chord"], want["chord_result"] = Ch.track_chords(rec, beats, n_frames, metre=want.get("metre") if beats.size >= 2 else None)  # (no metre below 2)
    return want


def _same(got, want):
    assert set(got) == set(want)
    for name, v in want.items():
        assert got[name].dtype == v.dtype and got[name].shape == v.shape and got[name].tolist() == v.tolist(), name


@pytest.mark.parametrize("bars,chords", SWITCHES)
def test_the_chain_equals_the_specifications(model, bars, chords):
    assert T.track_beats(POP, POP_FRAMES)[0].size == 64 and T.track_beats(ONE, 200)[0].size < 2 and T.track_beats(ONE[:0], 200)[0].size == 0
    for frames in (POP_FRAMES, 200):
        with Tk.Chain(model, frames, len(POP), {}, {} if bars else None, {} if chords else None) as chain:
            assert (chain.bars is not None, chain.chords is not None) == (bars, chords)
            for name, (rec, n_frames, count) in INPUTS.items():
                if n_frames == frames:
                    _same(chain.run(_bytes(rec).cuda(), count=_count(count)), _specification(CC.live(rec, count), n_frames, bars, chords, len(rec)))
        with pytest.raises(ValueError, match="has been closed"):
            chain.beats.ptr


@pytest.mark.parametrize("bars,chords", SWITCHES)
def test_in_place_and_uploaded_give_the_same(model, bars, chords):
    from yourmt3_amd.task_manager import TaskManager
    tm = TaskManager("mt3_full_plus")
    seg = CFG.segment_samples / CFG.sample_rate
    starts, end_sec = [i * seg for i in range(13)], 13 * seg
    tokens = torch.from_numpy(tm.notes_to_tokens(_music(), starts, end_sec, max_len=CFG.max_decode_len)[0]).cuda()
    n_frames = T.n_frames_of(end_sec, 100.0)
    with Tk.Chain(model, n_frames, 13 * 48, None, {} if bars else None, {} if chords else None) as chain:
        notes, bad, in_place = tm.tokens_to_notes_device(model, tokens, starts, end_sec, beats=chain.beats, bars=chain.bars, chords=chain.chords)
        uploaded = chain.run(_bytes(to_records(notes)))
        assert bad == 0 and len(notes) > 40 and in_place["beats"].size >= 10
        _same(in_place, uploaded)
        _same(uploaded, _specification(to_records(notes), n_frames, bars, chords))
        none = tm.tokens_to_notes_device(model, tokens[:0], [], end_sec, beats=chain.beats, bars=chain.bars, chords=chain.chords)
        assert none[:2] == ([], 0)
        _same(none[2], Tk.empty(bars, chords))
