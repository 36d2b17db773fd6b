"""The tracking chain: beats, then positions, then bars, then chords, then sections on the same records, everything back in one copy
(DESIGN sections 27 and 31): what TaskManager.tokens_to_notes_device, transcribe() and estimate_beats / estimate_bars / estimate_chords /
estimate_sections share, and nothing else.
`Chain` compiles and closes the trackers; `launch_beats` and `launch_bars_chords` are the two phases of the device pass, around the place
where the in-place route copies the detokeniser's count back; `layout`, `pack` and `unpack` state once what rides back and in which
order, on anything with a dtype and a shape; `empty` is the result of no records; `render` makes the MIDI bytes and the info dict."""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

# the order of what rides back, after any records and velocities of the caller; the results are int64, the rest int32
ORDER = ("ticks", "beat_result", "tempo", "beats", "bar_result", "metre", "chord_result", "chord", "section_result", "section", "novelty")


def beats_fps(beat_params: Optional[dict]) -> float:
    from .beats import DEFAULTS
    return float((beat_params or {}).get("frames_per_second", DEFAULTS["frames_per_second"]))


def launch_beats(beats, records, n_frames: int, count=None, divisions: int = 0) -> Dict[str, object]:
    """Phase one: BeatTracker.track, then BeatTracker.positions, on `records` under the device `count` (None: all of them) -> the parts
    so far, device tensors by ORDER's names.  Asynchronous."""
    b, lags, result = beats.track(records, n_frames, count=count)
    return {"ticks": beats.positions(b, result, records, count, divisions), "beat_result": result, "tempo": lags, "beats": b}


def launch_bars_chords(parts: Dict[str, object], bars, chords, records, n_frames: int, count=None, sections=None) -> None:
    """Phase two, on the same stream: BarTracker.track if `bars`, then ChordTracker.track if `chords`, then SectionTracker.track if
    `sections`, the last two with the bars' metre where there is one.  `records`: the LIVE records only (the two objects' max_notes is sized for them, not for a detokeniser's capacity), so the
    in-place route calls this after it has copied the count back, and without a count.  Adds its parts to `parts`."""
    if bars is not None:
        parts["metre"], parts["bar_result"] = bars.track(parts["beats"], parts["beat_result"], records, n_frames, count)
    if chords is not None:
        parts["chord"], parts["chord_result"] = chords.track(parts["beats"], parts["beat_result"], parts.get("metre"), records, n_frames, count)
    if sections is not None:
        parts["section"], parts["section_result"], parts["novelty"] = sections.track(parts["beats"], parts["beat_result"], parts.get("metre"), records,
                                                                                    n_frames, count)


def layout(parts) -> List[Tuple[str, int]]:
    """-> [(name, int32 words)] of the parts present, in ORDER: what one copy brings back, and where"""
    return [(name, int(np.prod(parts[name].shape)) * (2 if "int64" in str(parts[name].dtype) else 1)) for name in ORDER if name in parts]


def pack(parts) -> list:
    """the parts as flat uint8 tensors in layout's order, for the caller's torch.cat"""
    import torch
    return [parts[name].reshape(-1).view(torch.uint8) for name, _ in layout(parts)]


def unpack(ints: np.ndarray, lay) -> dict:
    """layout's inverse: the copied-back int32 words -> {"beats" int32 (n_beats,), "tempo" int32 (nW,), "ticks" int32 (n, 2)} plus, where they
    rode along, "bar_result" / "chord_result" / "section_result" int64 (8,), "metre" / "chord" / "section" int32 (n_beats,) and "novelty"
    int64 (n_beats,), empty with fewer than two beats"""
    at, o = {}, 0
    for name, words in lay:
        at[name], o = ints[o:o + words], o + words
    n_beats = int(at["beat_result"].view(np.int64)[0])
    out = {"beats": at["beats"][:n_beats].copy(), "tempo": at["tempo"].copy(), "ticks": at["ticks"].reshape(-1, 2).copy()}
    for result, name in (("bar_result", "metre"), ("chord_result", "chord"), ("section_result", "section")):
        if name in at:
            out[result], out[name] = at[result].view(np.int64).copy(), at[name][:n_beats if n_beats >= 2 else 0].copy()
    if "novelty" in at:
        out["novelty"] = at["novelty"].view(np.int64)[:n_beats if n_beats >= 2 else 0].copy()
    return out


def empty(bars: bool, chords: bool, sections: bool = False) -> dict:
    """the result of no records: no beats, and what the specifications say of no records and no beats"""
    out = {"beats": np.zeros(0, np.int32), "tempo": np.zeros(0, np.int32), "ticks": np.zeros((0, 2), np.int32)}
    if bars:
        from .bars import track_bars
        out["metre"], out["bar_result"] = track_bars([], [], 1)
    if chords:
        from .chords import track_chords
        out["chord"], out["chord_result"] = track_chords([], [], 1)
    if sections:
        from .sections import track_sections
        out["section"], out["novelty"], out["section_result"] = track_sections([], [], 1)
    return out


class Chain(contextlib.ExitStack):
    """The trackers of one call, compiled together and closed together (in reverse, also when a later one fails to compile): a beat
    tracker for `n_frames` frames, and with `bar_params` / `chord_params` / `section_params` (a dict, possibly empty; None: none) a bar, a
    chord and a section tracker for max_beats(n_frames) beats and calls of up to `max_notes` records.  Their frames_per_second must be
    the beats'."""

    def __init__(self, model, n_frames: int, max_notes: int, beat_params: Optional[dict] = None, bar_params: Optional[dict] = None,
                 chord_params: Optional[dict] = None, section_params: Optional[dict] = None):
        from .beats import max_beats
        super().__init__()
        self.n_frames, self.fps, self.bars, self.chords, self.sections = int(n_frames), beats_fps(beat_params), None, None, None
        for noun, p in (("bars", bar_params), ("chords", chord_params), ("sections", section_params)):
            if p is not None and float(p.get("frames_per_second", self.fps)) != self.fps:
                raise ValueError(f"the {noun}' frames_per_second must be the beats'")
        try:
            self.beats = self.enter_context(model.compile_beat_tracker(self.n_frames, **(beat_params or {})))
            cap = max_beats(self.n_frames, self.beats.lag_min)
            if bar_params is not None:
                self.bars = self.enter_context(model.compile_bar_tracker(cap, max_notes, **{**bar_params, "frames_per_second": self.fps}))
            if chord_params is not None:
                self.chords = self.enter_context(model.compile_chord_tracker(cap, max_notes, **{**chord_params, "frames_per_second": self.fps}))
            if section_params is not None:
                self.sections = self.enter_context(model.compile_section_tracker(cap, max_notes, **{**section_params, "frames_per_second": self.fps}))
        except BaseException:
            self.close()
            raise

    def run(self, records, divisions: int = 0, count=None) -> dict:
        """Both phases on `records` (NOTE_RECORD bytes, uploaded once if they are on the host; `count`: a device count or None), then ONE
        copy back -> unpack's dict."""
        import torch
        rec = records.to(self.beats._live_model().device)
        parts = launch_beats(self.beats, rec, self.n_frames, count, divisions)
        launch_bars_chords(parts, self.bars, self.chords, rec, self.n_frames, count, self.sections)
        return unpack(torch.cat(pack(parts)).cpu().numpy().view(np.int32), layout(parts))


def render(notes, tracked: dict, fps: float, hands=None) -> Tuple[bytes, dict]:
    """-> (the bytes of the .mid on the bars when there is a metre, else on the beats, with one marker per chord when there are chords and
    one per section start, before a chord's of the same tick, when there are sections; the info dict: beat_summary, "ticks", then
    bar_summary, chord_summary and section_summary where they were tracked).  `hands`: every note's hand in the notes' order, or None:
    passed on to the writer (midi.notes_to_midi_bytes)."""
    from .beats import beat_summary
    from .midi import notes_to_midi_bytes_on_bars, notes_to_midi_bytes_on_beats
    b, ticks = tracked["beats"], tracked["ticks"]
    info = {**beat_summary(b, tracked["tempo"], fps), "ticks": ticks}
    markers = ()
    if "chord" in tracked:
        from .chords import chord_markers, chord_segments, chord_summary
        markers = chord_markers(chord_segments(tracked["chord"], b), b)
    if "section" in tracked:
        from .sections import merge_markers, section_markers, section_segments, section_summary
        markers = merge_markers(section_markers(section_segments(tracked["section"], b), b), markers)
    if "metre" in tracked:
        from .bars import bar_summary
        info.update(bar_summary(tracked["metre"], tracked["bar_result"], b, fps))
        midi = notes_to_midi_bytes_on_bars(notes, ticks, b, tracked["metre"], int(tracked["bar_result"][3]), fps, markers, hands)
    else:
        midi = notes_to_midi_bytes_on_beats(notes, ticks, b, fps, markers, hands)
    if "chord" in tracked:
        info.update(chord_summary(tracked["chord"], tracked["chord_result"], b, fps))
    if "section" in tracked:
        info.update(section_summary(tracked["section"], tracked["section_result"], b, fps))
    return midi, info


def estimate(model, notes_or_mid_path, end_sec: Optional[float], divisions: int, output_path: Optional[str], beat_params: Optional[dict],
             bar_params: Optional[dict] = None, chord_params: Optional[dict] = None, section_params: Optional[dict] = None) -> Tuple[dict, dict]:
    """The body of estimate_beats, estimate_bars, estimate_chords and estimate_sections: read the notes, derive `end_sec` and n_frames, run the chain, render,
    write the file -> (the info dict with "midi", the tracked dict)"""
    import torch
    from .beats import n_frames_of
    from .metrics import to_records
    from .midi import read_midi_notes
    notes = notes_or_mid_path
    if isinstance(notes, (str, os.PathLike)):
        with open(notes, "rb") as f:
            notes = read_midi_notes(f.read())
    notes = list(notes)
    if end_sec is None:
        end_sec = max([0.0] + [max(n.onset, n.offset) for n in notes if math.isfinite(n.onset) and math.isfinite(n.offset)])
    fps = beats_fps(beat_params)
    rec = torch.from_numpy(to_records(notes).view(np.uint8).reshape(-1).copy())
    with Chain(model, n_frames_of(end_sec, fps), max(1, len(notes)), beat_params, bar_params, chord_params, section_params) as chain:
        tracked = chain.run(rec, divisions)
    midi, out = render(notes, tracked, fps)
    out["midi"] = midi
    if output_path is not None:
        with open(output_path, "wb") as f:
            f.write(midi)
    return out, tracked
