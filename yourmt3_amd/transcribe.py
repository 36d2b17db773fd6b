"""`transcribe(model, audio_info)`: audio file or array -> MIDI file, the reference-shaped entry point
(BASELINE.json north_star; flow per SURVEY.md section 9, UNVERIFIED): load -> mono -> 16 kHz -> slice into
(n_seg, 1, 32767) -> model.inference_file(bsz, segments) -> TaskManager detokenise per channel -> notes -> MIDI."""
from __future__ import annotations

import math
import os
from typing import List, Optional, Union

import numpy as np
import torch

from .audio import load_wav_pcm
from .midi import read_midi_notes, write_midi
from .metrics import FrameMetricCounts, NoteMetricCounts, to_records
from .task_manager import DRUM_PROGRAM, NOTE_RECORD as NOTE_RECORD_DTYPE, Note, TaskManager, drop_low_confidence
from .velocity import estimate_velocities  # noqa: F401  (its home is velocity.py; it belongs with transcribe, evaluate and align)
from .beats import estimate_beats  # noqa: F401  (the same for beats.py)
from .bars import estimate_bars  # noqa: F401  (and for bars.py)
from .chords import estimate_chords  # noqa: F401  (and for chords.py)
from .sections import estimate_sections  # noqa: F401  (and for sections.py)
from .hands import estimate_hands  # noqa: F401  (and for hands.py)


def transcribe(model, audio_info: Union[str, dict, np.ndarray], task_manager: Optional[TaskManager] = None, bsz: int = 8,
               output_dir: str = ".", max_token_length: Optional[int] = None, return_notes: bool = False,
               continuous: bool = False, subtask: Optional[str] = None, confidence: bool = False,
               min_confidence: Optional[float] = None, constrained: bool = False, programs=None, num_beams: int = 1,
               length_penalty: float = 1.0, device_detok: bool = False, velocity: bool = False, velocity_params: Optional[dict] = None,
               beats: bool = False, quantize: int = 0, beat_params: Optional[dict] = None, bars: bool = False, bar_params: Optional[dict] = None,
               chords: bool = False, chord_params: Optional[dict] = None, sections: bool = False, section_params: Optional[dict] = None,
               hands: bool = False, hand_params: Optional[dict] = None):
    """`continuous=True` decodes the file's segments through `bsz` slots with continuous batching
    (YourMT3.inference_stream: segments leave at EOS and the next ones enter) instead of fixed batches; same ids.
    `subtask`: for a task-conditioned TaskManager (e.g. "singing_drum_v1"), the sub-task whose task tokens prompt every
    segment's decode (None: its "default"); tasks without task tokens take no prompt and refuse a subtask.
    `confidence=True` decodes with token scores (include/ymt3.h, token scores): every returned note carries
    `confidence` = the probability of its onset's token.  `min_confidence` implies it and drops the notes below it before
    the MIDI file is written.  The ids, and so the notes, are those of the unscored decode.
    `constrained=True` decodes under the TaskManager's segment grammar (TaskManager.event_automaton; include/ymt3.h,
    constraints): no invalid tokens, and with the 13-channel decoder every channel keeps to its own instrument group.
    `programs` (GM programs, 128 = drums, 129 = singing) implies it and limits the notes to those programs.
    `num_beams` > 1 decodes with beam search (include/ymt3.h, beam search; `length_penalty` as HF) and takes the best hypothesis of
    every (segment, channel); confidences are that hypothesis' token scores.  `bsz` still counts segments: the model needs
    max_batch >= bsz * num_beams.  Beams do not combine with `continuous=True` here yet: YourMT3.inference_stream(num_beams=...) is the
    beam search under continuous batching, and routing this call to it is a two-line follow-up (existing tests pin the refusal).
    `device_detok=True` keeps the ids (and scores) on the GPU and turns them into notes there (TaskManager.tokens_to_notes_device;
    include/ymt3.h, device detokeniser) in every mode above: the same notes and the same MIDI bytes, without the host's loop over every token.
    `velocity=True` fills every note's `velocity` from the audio under its onset (YourMT3.compile_note_velocity; include/ymt3.h, note
    velocities; the rules: yourmt3_amd/velocity.py) instead of the flat 100, in every mode above and with both detokenisers: the ingested
    buffer, still on the device, is the audio.  `velocity_params`: velocity.DEFAULTS' keys.  The notes `min_confidence` drops are gone
    before the measurement, so the loudest KEPT note gets peak_velocity.  Off, nothing changes by a byte.
    `beats=True` tracks the beats of the notes on the device (YourMT3.compile_beat_tracker; include/ymt3.h, beat tracking; the rules:
    yourmt3_amd/beats.py) and writes the .mid on them: its tempo track follows the music, a tick is a position in beats, and playback keeps
    the performance's timing after a lead-in of less than a beat.  `quantize` (a divisor of 480; 0: none) snaps every note to that many
    steps per beat.  `beat_params`: beats.DEFAULTS' keys.  With both detokenisers the same bytes: the device one is tracked on its records
    where they lie, the host's notes go up once.  After `min_confidence` and `velocity`, on the kept notes.  The return value gains a last
    element: {"beats_sec", "tempo_bpm" (one per window of hop_frames), "lead_sec", "ticks" ((n, 2), in the notes' order)}.  Off, nothing
    changes by a byte.
    `bars=True` (it needs `beats=True`) finds every beat's metre and place in its bar and the file's key on the device
    (YourMT3.compile_bar_tracker; include/ymt3.h, bars and key; the rules: yourmt3_amd/bars.py), on the same kept notes and the beats just
    tracked, and writes them into the .mid: time signatures at the bar lines where the metre changes, a key signature at tick 0.
    `bar_params`: bars.DEFAULTS' keys (frames_per_second is the beats').  In every decode mode and with both detokenisers the same bytes.
    The info dict gains "downbeats_sec", "time_signatures" ([(tick, numerator)] over 4), "key" (e.g. "F# minor", "none" without pitched
    notes) and "key_margin" (the best key's score minus the second best's).  Off, nothing changes by a byte.
    `chords=True` (it needs `beats=True`) gives every beat a chord on the device (YourMT3.compile_chord_tracker; include/ymt3.h, chords;
    the rules: yourmt3_amd/chords.py), on the same kept notes and beats, after the bars and with their metre when `bars=True`, and writes
    one marker (FF 06) per run of equal chords into the .mid's conductor track, at the tick of the run's first beat.  `chord_params`:
    chords.DEFAULTS' keys (frames_per_second is the beats').  In every decode mode and with both detokenisers the same bytes.  The info
    dict gains "chords" ([(start_sec, end_sec, name)], e.g. "Am", "G7", "C/E", "N") and "chord_labels" (every beat's 12 q + r, 255 for
    N).  Off, nothing changes by a byte.
    `sections=True` (it needs `beats=True`) finds the song's form on the device (YourMT3.compile_section_tracker; include/ymt3.h, sections;
    the rules: yourmt3_amd/sections.py), on the same kept notes and beats, after the bars and with their metre when `bars=True`, and
    writes one marker (FF 06) per section start into the .mid's conductor track, "[A]", "[B]" and so on, before a chord's marker of
    the same tick; a silent section gets none.  `section_params`: sections.DEFAULTS' keys (frames_per_second is the beats').  In every
    decode mode and with both detokenisers the same bytes.  The info dict gains "sections" ([(start_sec, end_sec, name)], "N" for a
    silent one) and "section_labels" (every beat's label, 255 in a silent section).  Off, nothing changes by a byte.
    `hands=True` gives every note of the piano programs a hand on the device (YourMT3.compile_hand_splitter; include/ymt3.h, hands; the
    rules: yourmt3_amd/hands.py) and writes such a program as two tracks on its one channel, "R.H." and then "L.H.": a notation program
    opens them as two staves.  It needs no beats and works with them: in every decode mode and with both detokenisers the same bytes
    (the device one's records get their hands where they lie, the host's notes go up once), after `min_confidence` and `velocity`, on
    the kept notes.  `hand_params`: hands.DEFAULTS' keys.  The info dict (made if there is none: the return value gains it as its last
    element) gains "hand" (one per note, in the notes' order: 1 right, 0 left, 255 none), "hand_splits" ([(sec, split point)] of every
    onset slice) and "hand_result" (hands.split_hands' eight numbers).  Off, nothing changes by a byte."""
    if velocity_params is not None and not velocity:
        raise ValueError("velocity_params without velocity=True")
    if (beat_params is not None or quantize) and not beats:
        raise ValueError("beat_params or quantize without beats=True")
    if bars and not beats:
        raise ValueError("bars=True without beats=True")
    if bar_params is not None and not bars:
        raise ValueError("bar_params without bars=True")
    if chords and not beats:
        raise ValueError("chords=True without beats=True")
    if chord_params is not None and not chords:
        raise ValueError("chord_params without chords=True")
    if sections and not beats:
        raise ValueError("sections=True without beats=True")
    if section_params is not None and not sections:
        raise ValueError("section_params without sections=True")
    if hand_params is not None and not hands:
        raise ValueError("hand_params without hands=True")
    num_beams = int(num_beams)
    if num_beams < 1:
        raise ValueError(f"num_beams={num_beams} must be >= 1")
    if num_beams > 1 and continuous:
        raise ValueError("beam search (num_beams > 1) does not run with continuous batching (continuous=True)")
    if num_beams > 1 and min(int(bsz), max(1, model.max_batch)) * num_beams > model.max_batch:
        raise ValueError(f"bsz={int(bsz)} x num_beams={num_beams} need max_batch >= {int(bsz) * num_beams}, "
                         f"the model was created with max_batch={model.max_batch}")
    cfg = model.cfg
    if task_manager is None:
        task_manager = TaskManager("mc13_full_plus_256" if cfg.n_channels == 13 else "mt3_full_plus")
    if task_manager.num_decoding_channels != cfg.n_channels:
        raise ValueError("TaskManager channel count does not match the model's decoder")
    if isinstance(audio_info, dict):
        path = audio_info["filepath"]
        name = audio_info.get("track_name") or os.path.splitext(os.path.basename(path))[0]
        x, sr = load_wav_pcm(path)
    elif isinstance(audio_info, str):
        path, name = audio_info, os.path.splitext(os.path.basename(audio_info))[0]
        x, sr = load_wav_pcm(path)
    else:
        x, sr, name = np.asarray(audio_info, dtype=np.float32), cfg.sample_rate, "audio"
    # mono mix, resample to the model rate, slice and zero-pad on the device (C ABI: ymt3_ingest)
    segments = model.ingest(torch.from_numpy(np.ascontiguousarray(x)), sr)
    n_samples = model.last_ingest_samples
    start_secs = [i * cfg.segment_samples / cfg.sample_rate for i in range(segments.shape[0])]
    prompt = None
    if task_manager.subtasks:
        prompt = torch.tensor(task_manager.task_prompt(subtask, 1)[0, 0])             # (P,): the same prefix for every segment
    elif subtask is not None:
        raise ValueError(f"task {task_manager.task_name!r} has no sub-tasks (asked for {subtask!r})")
    n_prompt = 0 if prompt is None else int(prompt.numel())
    L = min(max_token_length or task_manager.max_note_token_length, cfg.max_decode_len - n_prompt)
    kw = {} if prompt is None else {"task_tokens": prompt}
    scored = confidence or min_confidence is not None
    if scored:
        kw["return_scores"] = True
    constraint = None
    if constrained or programs is not None:
        aut, starts = task_manager.event_automaton(programs)
        constraint = model.compile_constraint(aut)
        kw["constraint"] = constraint
        kw["start_states"] = starts
    if num_beams > 1:
        kw.update(num_beams=num_beams, num_return_sequences=1, length_penalty=length_penalty)
    try:
        if device_detok:
            tokens, scores = _decode_device(model, segments, bsz, L, continuous, scored, kw)
        else:
            batches, score_batches = _decode(model, segments, bsz, L, continuous, scored, kw)
    finally:
        if constraint is not None:
            constraint.close()
    end_sec = n_samples / cfg.sample_rate
    measurer = model.compile_note_velocity(**(velocity_params or {})) if velocity else None
    chain = tracked = splitter = handed = None
    try:
        if hands:
            from .beats import n_frames_of
            from .hands import DEFAULTS as HAND_DEFAULTS, MAX_NOTES as HAND_MAX_NOTES, hand_summary
            hand_p = {**HAND_DEFAULTS, **(hand_params or {})}
            hand_frames = n_frames_of(end_sec, float(hand_p["frames_per_second"]))
            capacity = max(1, int(segments.shape[0]) * cfg.n_channels * L)
            splitter = model.compile_hand_splitter(hand_frames, min(HAND_MAX_NOTES, capacity), **(hand_params or {}))
        if beats:
            from .bars import MAX_NOTES as BAR_MAX_NOTES
            from .beats import n_frames_of
            from .tracking import Chain, beats_fps, render
            chain = Chain(model, n_frames_of(end_sec, beats_fps(beat_params)), min(BAR_MAX_NOTES, max(1, int(segments.shape[0]) * cfg.n_channels * L)),
                          beat_params, (bar_params or {}) if bars else None, (chord_params or {}) if chords else None,
                          (section_params or {}) if sections else None)
        in_place = device_detok and min_confidence is None                   # measured and tracked on the detokeniser's records where they lie
        if device_detok:
            extra = {}
            if in_place and measurer is not None:
                extra.update(velocity=measurer, audio=segments.view(-1))
            if in_place and chain is not None:
                extra.update(beats=chain.beats, quantize=quantize, bars=chain.bars, chords=chain.chords, sections=chain.sections)
            if in_place and splitter is not None and capacity <= splitter.max_notes:
                extra.update(hands=splitter)
            out = task_manager.tokens_to_notes_device(model, tokens, start_secs, end_sec, scores=scores, **extra)
            notes, tracked = out[0], (out[2] if len(out) > 2 else None)
            if "hands" in extra:
                handed = tuple(tracked.pop(k) for k in ("hand", "hand_split", "hand_result"))
                tracked = tracked if "beats" in extra else None
        else:
            notes = task_manager.tokens_to_notes(batches, start_secs, end_sec=end_sec, score_batches=score_batches)
        if min_confidence is not None:
            notes = drop_low_confidence(notes, float(min_confidence))
        if measurer is not None and not in_place:                           # the host's notes: one upload of their records, the same kernel
            notes = measurer.apply(segments.view(-1), notes)
        if chain is not None and tracked is None:                           # the same for the chain: up once, back once
            tracked = chain.run(torch.from_numpy(to_records(list(notes)).view(np.uint8).reshape(-1).copy()), quantize)
        if splitter is not None and handed is None:                         # and for the hands
            if len(notes) > splitter.max_notes:
                raise ValueError(f"{len(notes)} notes: the hands take at most {splitter.max_notes}")
            handed = splitter.run(torch.from_numpy(to_records(list(notes)).view(np.uint8).reshape(-1).copy()), hand_frames)
    finally:
        if splitter is not None:
            splitter.close()
        if measurer is not None:
            measurer.close()
        if chain is not None:
            chain.close()
    os.makedirs(output_dir, exist_ok=True)
    if tracked is None and handed is None:
        midi_path = write_midi(notes, os.path.join(output_dir, name + ".mid"))
        return (midi_path, notes) if return_notes else midi_path
    midi_path = os.path.join(output_dir, name + ".mid")
    hand = None if handed is None else [int(h) for h in handed[0].tolist()]
    if tracked is None:
        from .midi import notes_to_midi_bytes
        midi, info = notes_to_midi_bytes(notes, hands=hand), {}
    else:
        midi, info = render(notes, tracked, chain.fps, hands=hand)
    if handed is not None:
        info.update(hand_summary(*handed, hand_p))
    with open(midi_path, "wb") as f:
        f.write(midi)
    return (midi_path, notes, info) if return_notes else (midi_path, info)


def _decode(model, segments, bsz, L, continuous, scored, kw):
    """-> (token batches, score batches or None) through continuous batching or fixed batches"""
    score_batches = None
    if continuous:
        out = model.inference_stream(segments, max_token_length=L, slots=bsz, **kw)
        batches = [(out[0] if scored else out).cpu().numpy()]
        if scored:
            score_batches = [out[1].cpu().numpy()]
    else:
        out = model.inference_file(bsz, segments, max_token_length=L, **kw)
        if kw.get("num_beams", 1) > 1:                  # (b, K, 1, L): hypothesis 0 of every group
            batches = [t[:, :, 0] for t in (out[0] if scored else out)]
            score_batches = [t[:, :, 0] for t in out[1]] if scored else None
        else:
            batches, score_batches = out if scored else (out, None)
    return batches, score_batches


def _decode_device(model, segments, bsz, L, continuous, scored, kw):
    """_decode with everything left on the device -> ((n, K, L) ids, (n, K, L) scores or None); a beam call's (n, K, 1, L) is viewed
    through hypothesis 0's strides, not copied."""
    if continuous:
        out = model.inference_stream(segments, max_token_length=L, slots=bsz, **kw)
        tokens, scores = (out[0], out[1]) if scored else (out, None)
    else:
        step = max(1, min(int(bsz), model.max_batch))                   # inference_file's batches (its prompt and start states are per call here)
        outs = [model.inference(segments[i:i + step], max_token_length=L, **kw) for i in range(0, segments.shape[0], step)]
        tokens = torch.cat([o[0] if scored else o for o in outs], 0)
        scores = torch.cat([o[1] for o in outs], 0) if scored else None
    if kw.get("num_beams", 1) > 1:
        tokens = tokens[:, :, 0]
        scores = scores[:, :, 0] if scored else None
    return tokens, scores


class LiveTranscriber:
    """transcribe() for audio that arrives in chunks: a microphone, a network stream, a long recording read in blocks.

        live = LiveTranscriber(model, 44100, n_channels=2, dtype=torch.int16)
        for chunk in source:                    # (n_frames, n_channels) PCM, at most max_chunk_frames frames
            new_notes = live.push(chunk)        # the notes that became final
        new_notes = live.finish()
        live.write_midi("out.mid"); live.close()

    A push (1) ingests the chunk (IngestStream; include/ymt3.h, streaming ingest), (2) decodes the segments it completed, one
    model.inference call per at most `bsz` of them (None: as many as the model's max_batch allows), (3) pushes the ids, and the scores when
    confidences are asked for, to the incremental detokeniser on the device (include/ymt3.h, incremental detokeniser) and (4) copies back
    only the counters and the new records.  A note is returned once, when nothing later can change it: a pitched note when it ends, a
    drum hit when the next segment's start has passed it.  `finish()` pads the tail as the one-shot ingest does and closes what still
    sounds at the end of the audio.  The latency is one segment: the model decodes whole segments.

    Decode options are transcribe()'s except `continuous`: `subtask`, `confidence` / `min_confidence`, `constrained` / `programs`,
    `num_beams` / `length_penalty`, `max_token_length`.  `min_confidence` filters what push / finish return (and `notes`, and the MIDI
    file); the state on the device keeps every note.  `max_held` bounds the drum hits the state holds per (channel, pitch); `forced`
    counts the hits that had to leave early because of it (0 in any sane stream: a hit is held only while it lies past the start of a
    segment that has not come yet).

    The invariant: sorted(everything returned) and the MIDI bytes are those of transcribe(model, the whole PCM, device_detok=True, ...) with
    the same options -- both ends are exact, so this holds whenever the decode gives a segment the same ids here and there.  Rows are
    independent of batch composition only within a kernel regime (DESIGN, "Rows are independent of batch composition"): the two boundaries are 2048
    (row, head) pairs, beyond which self-attention sums with 2 waves per pair, and 512 rows, from which the decode GEMMs take mid-size tiles.
    A live session decodes a few segments per call and a file transcription up to `bsz`; the ids agree bit for bit as long as both stay on
    the same side of both boundaries.

    Note velocities (transcribe(velocity=True)) are not part of a live session: a pitched note becomes final when it ends, long after the
    audio of its onset has left the device.  estimate_velocities() on the recording puts them onto the session's MIDI file afterwards.
    Beats (transcribe(beats=True)) are not part of a live session either: the tempo path looks at the whole file.  estimate_beats() on the
    session's notes tracks them afterwards.  Bars and key (transcribe(bars=True)) build on the beats and are out of scope here for the same
    reason: estimate_bars() on the session's notes finds them afterwards; chords (transcribe(chords=True)) likewise, by estimate_chords(), and sections (transcribe(sections=True)) by estimate_sections().
    Hands (transcribe(hands=True)) are not part of a live session either: a split point is a path over the whole piece;
    estimate_hands() on the session's notes finds them afterwards."""

    def __init__(self, model, sample_rate: int, n_channels: int = 1, dtype=torch.int16, task_manager: Optional[TaskManager] = None,
                 max_chunk_frames: int = 1 << 16, bsz: Optional[int] = None, max_token_length: Optional[int] = None,
                 subtask: Optional[str] = None, confidence: bool = False, min_confidence: Optional[float] = None, constrained: bool = False,
                 programs=None, num_beams: int = 1, length_penalty: float = 1.0, max_held: int = 16, name: str = "audio"):
        cfg = model.cfg
        self.model, self.name = model, name
        self.num_beams = int(num_beams)
        if self.num_beams < 1:
            raise ValueError(f"num_beams={num_beams} must be >= 1")
        room = model.max_batch // self.num_beams
        if room < 1:
            raise ValueError(f"num_beams={self.num_beams} needs max_batch >= {self.num_beams}, the model was created with max_batch={model.max_batch}")
        self.bsz = room if bsz is None else max(1, min(int(bsz), room))
        if task_manager is None:
            task_manager = TaskManager("mc13_full_plus_256" if cfg.n_channels == 13 else "mt3_full_plus")
        if task_manager.num_decoding_channels != cfg.n_channels:
            raise ValueError("TaskManager channel count does not match the model's decoder")
        self.task_manager = task_manager
        prompt = None
        if task_manager.subtasks:
            prompt = torch.tensor(task_manager.task_prompt(subtask, 1)[0, 0])
        elif subtask is not None:
            raise ValueError(f"task {task_manager.task_name!r} has no sub-tasks (asked for {subtask!r})")
        n_prompt = 0 if prompt is None else int(prompt.numel())
        self.L = min(max_token_length or task_manager.max_note_token_length, cfg.max_decode_len - n_prompt)
        self.scored = bool(confidence) or min_confidence is not None
        self.min_confidence = None if min_confidence is None else float(min_confidence)
        self._kw = {} if prompt is None else {"task_tokens": prompt}
        if self.scored:
            self._kw["return_scores"] = True
        if self.num_beams > 1:
            self._kw.update(num_beams=self.num_beams, num_return_sequences=1, length_penalty=length_penalty)
        self._constraint = self._ingest = self._detok = self._state = None
        try:
            if constrained or programs is not None:
                aut, starts = task_manager.event_automaton(programs)
                self._constraint = model.compile_constraint(aut)
                self._kw["constraint"] = self._constraint
                self._kw["start_states"] = starts
            self._ingest = model.compile_ingest_stream(sample_rate, n_channels, dtype, max_chunk_frames)
            # the most segments one call can complete: a chunk's resampled samples on top of an almost whole partial segment
            per_chunk = -(-int(max_chunk_frames) * cfg.sample_rate // int(sample_rate)) // cfg.segment_samples + 2
            self._detok = model.compile_detokenizer(task_manager, per_chunk, self.L)
            self._state = self._detok.new_state(max_held=max_held)
        except Exception:
            self.close()
            raise
        self.notes: List = []               # everything returned so far, in the order it became final
        self.n_segments = 0                 # segments decoded so far
        self.n_invalid = self.forced = 0
        self.finished = False

    def _decode(self, segments):
        """(k, 1, S) segments -> ((k, K, L) ids, (k, K, L) scores or None) on the device, `bsz` segments per inference call"""
        outs = [self.model.inference(segments[i:i + self.bsz], max_token_length=self.L, **self._kw) for i in range(0, segments.shape[0], self.bsz)]
        tokens = torch.cat([o[0] if self.scored else o for o in outs], 0)
        scores = torch.cat([o[1] for o in outs], 0) if self.scored else None
        if self.num_beams > 1:              # (k, K, 1, L): hypothesis 0, read in place
            tokens = tokens[:, :, 0]
            scores = scores[:, :, 0] if self.scored else None
        return tokens, scores

    def _segments(self, segments, last: bool):
        cfg = self.model.cfg
        k = int(segments.shape[0])
        if k == 0 and not last:
            return []
        starts = [(self.n_segments + i) * cfg.segment_samples / cfg.sample_rate for i in range(k)]
        horizon = math.inf if last else (self.n_segments + k) * cfg.segment_samples / cfg.sample_rate
        tokens, scores = self._decode(segments) if k else (torch.zeros(0, cfg.n_channels, self.L, dtype=torch.int32, device=self.model.device), None)
        notes, bad, forced = self.task_manager.tokens_to_notes_stream(self.model, self._detok, self._state, tokens, starts, horizon, scores=scores,
                                                                      scored=self.scored)
        self.n_segments += k
        self.n_invalid += bad
        self.forced += forced
        return notes

    def _out(self, notes):
        if self.min_confidence is not None:
            notes = drop_low_confidence(notes, self.min_confidence)
        self.notes += notes
        return notes

    def push(self, pcm) -> list:
        """One chunk of (n_frames, n_channels) or (n_frames,) PCM -> the notes that became final, sorted."""
        if self.finished:
            raise ValueError("the session has been finished")
        pcm = torch.as_tensor(pcm) if not isinstance(pcm, torch.Tensor) else pcm
        return self._out(self._segments(self._ingest.push(pcm), last=False))

    def finish(self) -> list:
        """The end of the audio -> the remaining notes: the tail segments, every held hit, and what still sounds, closed at the end."""
        if self.finished:
            raise ValueError("the session has been finished")
        segments, n_samples = self._ingest.finish()
        notes = self._segments(segments, last=True)
        last, _, _ = self.task_manager.tokens_to_notes_stream(self.model, self._detok, self._state, end_sec=n_samples / self.model.cfg.sample_rate,
                                                              scored=self.scored)
        self.finished = True
        return self._out(sorted(notes + last))

    def write_midi(self, path: Optional[str] = None, output_dir: str = ".") -> str:
        """Write everything returned so far as a MIDI file -> its path (default: output_dir/name.mid, as transcribe())."""
        if path is None:
            os.makedirs(output_dir, exist_ok=True)
            path = os.path.join(output_dir, self.name + ".mid")
        return write_midi(sorted(self.notes), path)

    def close(self):
        for o in (getattr(self, "_state", None), getattr(self, "_detok", None), getattr(self, "_ingest", None), getattr(self, "_constraint", None)):
            if o is not None:
                o.close()
        self._state = self._detok = self._ingest = self._constraint = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def score_notes(model, audio_info: Union[str, dict, np.ndarray], notes, task_manager: Optional[TaskManager] = None, bsz: int = 8,
                subtask: Optional[str] = None) -> dict:
    """How likely are these notes for this audio: the teacher-forced log-likelihood of the notes' token ids (YourMT3.score; include/ymt3.h,
    sequence scoring).  `audio_info` as transcribe(); `notes`: a list of Note, or the path of a .mid file (midi.read_midi_notes).  The audio is
    ingested as transcribe() ingests it, the notes become ids on the device (TaskManager.notes_to_tokens_device; a row that does not fit
    the task's max_note_token_length raises ValueError), and every batch of `bsz` segments is one model.score call, prompted with
    `subtask`'s task tokens where the task has them; a row counts up to and including its EOS.  The MoE decoder is refused as
    YourMT3.score refuses it.
    -> {"log_likelihood": float, "segment_log_likelihood": (n, K) f64 array, "n_tokens": int (EOS included), "tokens": (n, K, L) int32 device tensor}"""
    cfg = model.cfg
    if task_manager is None:
        task_manager = TaskManager("mc13_full_plus_256" if cfg.n_channels == 13 else "mt3_full_plus")
    if task_manager.num_decoding_channels != cfg.n_channels:
        raise ValueError("TaskManager channel count does not match the model's decoder")
    if isinstance(audio_info, dict):
        x, sr = load_wav_pcm(audio_info["filepath"])
    elif isinstance(audio_info, str):
        x, sr = load_wav_pcm(audio_info)
    else:
        x, sr = np.asarray(audio_info, dtype=np.float32), cfg.sample_rate
    if isinstance(notes, (str, os.PathLike)):
        with open(notes, "rb") as f:
            notes = read_midi_notes(f.read())
    segments = model.ingest(torch.from_numpy(np.ascontiguousarray(x)), sr)
    n = int(segments.shape[0])
    start_secs = [i * cfg.segment_samples / cfg.sample_rate for i in range(n)]
    prompt = None
    if task_manager.subtasks:
        prompt = torch.tensor(task_manager.task_prompt(subtask, 1)[0, 0])
    elif subtask is not None:
        raise ValueError(f"task {task_manager.task_name!r} has no sub-tasks (asked for {subtask!r})")
    L = min(task_manager.max_note_token_length, cfg.max_decode_len - (0 if prompt is None else int(prompt.numel())))
    tokens, lengths = task_manager.notes_to_tokens_device(model, notes, start_secs, model.last_ingest_samples / cfg.sample_rate, max_len=L)
    step = max(1, min(int(bsz), model.max_batch))
    lls = [model.score(segments[i:i + step], tokens[i:i + step], task_tokens=prompt, lengths=lengths[i:i + step])[1] for i in range(0, n, step)]
    seg_ll = torch.cat(lls, 0).cpu().numpy() if lls else np.zeros((0, cfg.n_channels), np.float64)
    return {"log_likelihood": float(seg_ll.sum()), "segment_log_likelihood": seg_ll, "n_tokens": int(lengths.sum()), "tokens": tokens}


def _decode_against(model, audio_info, reference, task_manager, bsz, continuous, subtask, constrained, programs, num_beams, length_penalty):
    """What evaluate() and align() share: load the audio and the reference (a list of Note, a NOTE_RECORD array or the path of a .mid
    file), and decode the audio as transcribe(device_detok=True) does, the ids staying on the device.
    -> (task_manager, the audio's name, the reference as given or read, its records, n_programs, tokens, start_secs, L, end_sec)"""
    num_beams = int(num_beams)
    if num_beams < 1:
        raise ValueError(f"num_beams={num_beams} must be >= 1")
    if num_beams > 1 and continuous:
        raise ValueError("beam search (num_beams > 1) does not run with continuous batching (continuous=True)")
    cfg = model.cfg
    if task_manager is None:
        task_manager = TaskManager("mc13_full_plus_256" if cfg.n_channels == 13 else "mt3_full_plus")
    if task_manager.num_decoding_channels != cfg.n_channels:
        raise ValueError("TaskManager channel count does not match the model's decoder")
    name = "audio"
    if isinstance(audio_info, dict):
        name = audio_info.get("track_name") or os.path.splitext(os.path.basename(audio_info["filepath"]))[0]
        x, sr = load_wav_pcm(audio_info["filepath"])
    elif isinstance(audio_info, str):
        name = os.path.splitext(os.path.basename(audio_info))[0]
        x, sr = load_wav_pcm(audio_info)
    else:
        x, sr = np.asarray(audio_info, dtype=np.float32), cfg.sample_rate
    if isinstance(reference, (str, os.PathLike)):
        with open(reference, "rb") as f:
            reference = read_midi_notes(f.read())
    ref = to_records(reference)
    lo, hi = task_manager.codec.range_of("program")
    n_programs = hi - lo
    segments = model.ingest(torch.from_numpy(np.ascontiguousarray(x)), sr)
    n = int(segments.shape[0])
    start_secs = [i * cfg.segment_samples / cfg.sample_rate for i in range(n)]
    prompt = None
    if task_manager.subtasks:
        prompt = torch.tensor(task_manager.task_prompt(subtask, 1)[0, 0])
    elif subtask is not None:
        raise ValueError(f"task {task_manager.task_name!r} has no sub-tasks (asked for {subtask!r})")
    L = min(task_manager.max_note_token_length, cfg.max_decode_len - (0 if prompt is None else int(prompt.numel())))
    kw = {} if prompt is None else {"task_tokens": prompt}
    constraint = None
    if constrained or programs is not None:
        aut, starts = task_manager.event_automaton(programs)
        constraint = model.compile_constraint(aut)
        kw["constraint"] = constraint
        kw["start_states"] = starts
    if num_beams > 1:
        kw.update(num_beams=num_beams, num_return_sequences=1, length_penalty=length_penalty)
    try:
        tokens, _ = _decode_device(model, segments, bsz, L, continuous, False, kw)
    finally:
        if constraint is not None:
            constraint.close()
    return task_manager, name, reference, ref, n_programs, tokens, start_secs, L, model.last_ingest_samples / cfg.sample_rate


def evaluate(model, audio_info: Union[str, dict, np.ndarray], reference, task_manager: Optional[TaskManager] = None, bsz: int = 8,
             continuous: bool = False, subtask: Optional[str] = None, constrained: bool = False, programs=None, num_beams: int = 1,
             length_penalty: float = 1.0, frames: bool = False, frames_per_second: float = 100.0, align: bool = False, band_sec: float = 10.0,
             **tolerances) -> dict:
    """How right is the transcription of this audio: note-level onset, onset+offset and drum F1 against `reference` (a list of Note, or the
    path of a .mid file), by the rules of yourmt3_amd/metrics.py.  The audio is decoded as transcribe(device_detok=True) decodes it
    (`continuous`, `subtask`, `constrained`, `programs`, `num_beams`, `length_penalty` as there); the ids become note records on the device
    (Detokenizer.run_device) and are matched against the uploaded reference there (NoteMetrics.run, reading the number of transcribed notes
    from the detokeniser's counter on the device): one copy back, of the counts.  `tolerances`: onset_tol, offset_min_tol, offset_ratio.
    -> NoteMetricCounts.summary(): onset_f / offset_f (instrument-agnostic, with _p and _r), drum_onset_f, multi_f, per_program, skipped and
    "counts" (the (n_programs + 1, 2, 3) integers).
    `frames=True` adds frame-level F1 (PianoRoll.metrics; the rules: yourmt3_amd/metrics.py, frame metrics) over n_frames = max(1,
    ceil(end_sec * frames_per_second)) frames, end_sec being the audio's length as the detokeniser gets it.  It runs on the same records
    and counter on the device, after the note metrics, and the copy back is still one.  The summary gains frame_f, frame_p, frame_r,
    frame_acc (instrument-agnostic), frame_err ({"sub", "miss", "fa", "total"}), multi_frame_f, frame_counts (the (n_programs + 1, 6)
    integers) and n_frames.
    `align=True` first aligns the reference to the transcription (Aligner.align; the rules: yourmt3_amd/metrics.py, alignment: banded DTW
    over frame-wise pitch sets at frames_per_second under a band of band_sec seconds) and warps the uploaded reference records onto the
    audio's time axis on the device (Aligner.warp) before the metrics read them: for a reference that is a score, another performance
    or carries a lead-in.  n_est_frames = max(1, ceil(end_sec * frames_per_second)), n_ref_frames the same of the largest finite time of
    the reference.  The copy back is still one; the summary gains align_total and align_path_len."""
    task_manager, _, _, ref, n_programs, tokens, start_secs, L, end_sec = _decode_against(
        model, audio_info, reference, task_manager, bsz, continuous, subtask, constrained, programs, num_beams, length_penalty)
    n = len(start_secs)
    detok = model.compile_detokenizer(task_manager, max(n, 1), L)
    metrics = model.compile_note_metrics(n_programs, max(len(ref), 1), detok.capacity, **tolerances)
    roll = aligner = None
    try:
        if frames:
            n_frames = max(1, math.ceil(end_sec * float(frames_per_second)))
            roll = model.compile_piano_roll(n_programs, n_frames, frames_per_second, metrics.drum_program)
        if align:
            n_ref_frames, n_est_frames, band = _align_frames(ref, end_sec, frames_per_second, band_sec)
            aligner = model.compile_aligner(n_programs, max(n_ref_frames, n_est_frames), frames_per_second, band, metrics.drum_program)
        est, est_counts = detok.run_device(tokens, None, torch.tensor(start_secs, dtype=torch.float64), end_sec)
        ref_dev = torch.from_numpy(ref.view(np.uint8).reshape(-1).copy()).to(model.device)
        if align:
            warp, aligned = aligner.align(ref_dev, est, n_ref_frames, n_est_frames, est_count=est_counts)
            ref_dev = aligner.warp(ref_dev, warp)
        counts = metrics.run(ref_dev, est, est_count=est_counts)
        if frames:                                                       # int32 and int64 counts leave in one copy
            counts = torch.cat([counts.to(torch.int64), roll.metrics(ref_dev, est, n_frames, est_count=est_counts)])
        if align:
            counts = torch.cat([counts.to(torch.int64), aligned[:2]])
        flat = counts.cpu().numpy()
    finally:
        if aligner is not None:
            aligner.close()
        if roll is not None:
            roll.close()
        metrics.close()
        detok.close()
    n_note = (n_programs + 1) * 6 + 2
    out = NoteMetricCounts.from_flat(flat[:n_note], n_programs, metrics.drum_program).summary()
    if frames:
        out.update(FrameMetricCounts.from_flat(flat[n_note:n_note + n_note], n_programs, metrics.drum_program).summary(), n_frames=n_frames)
    if align:
        out.update(align_total=int(flat[-2]), align_path_len=int(flat[-1]))
    return out


def _align_frames(ref: np.ndarray, end_sec: float, frames_per_second: float, band_sec: float):
    """-> (n_ref_frames, n_est_frames, band_frames) of an alignment of the reference records `ref` to audio of end_sec seconds"""
    fps = float(frames_per_second)
    if not (np.isfinite(fps) and fps > 0):
        raise ValueError(f"frames_per_second={frames_per_second} must be finite and > 0")
    if not (np.isfinite(band_sec) and band_sec > 0):
        raise ValueError(f"band_sec={band_sec} must be finite and > 0")
    times = np.concatenate([ref["onset"], ref["offset"]])
    times = times[np.isfinite(times)]
    ref_end = max(float(times.max()), 0.0) if times.size else 0.0
    return max(1, math.ceil(ref_end * fps)), max(1, math.ceil(float(end_sec) * fps)), max(1, math.ceil(float(band_sec) * fps))


def align(model, audio_info: Union[str, dict, np.ndarray], reference, task_manager: Optional[TaskManager] = None, bsz: int = 8,
          frames_per_second: float = 100.0, band_sec: float = 10.0, output_dir: Optional[str] = None, continuous: bool = False,
          subtask: Optional[str] = None, constrained: bool = False, programs=None, num_beams: int = 1, length_penalty: float = 1.0,
          drum_program: int = DRUM_PROGRAM) -> dict:
    """Carry `reference` (a list of Note, or the path of a .mid file: a score, another performance, a file with a lead-in) onto the time
    axis of this audio.  The audio is transcribed as evaluate() transcribes it, the records staying on the device; the reference is
    aligned to them there by banded DTW over frame-wise pitch sets (Aligner.align; the rules: yourmt3_amd/metrics.py, alignment) with
    n_est_frames = max(1, ceil(end_sec * frames_per_second)), n_ref_frames the same of the largest finite onset or offset of the reference
    and a band of band_sec seconds, and warped along the path (Aligner.warp).  `drum_program` is evaluate()'s: the row of the drums.
    -> {"notes": the reference on the audio's time axis (a list of Note), "total", "path_len", "n_ref_frames", "n_est_frames", "warp"
    (the (n_ref_frames,) int32 array)}.  With `output_dir` the notes are also written to <name>.aligned.mid."""
    task_manager, name, reference, ref, n_programs, tokens, start_secs, L, end_sec = _decode_against(
        model, audio_info, reference, task_manager, bsz, continuous, subtask, constrained, programs, num_beams, length_penalty)
    n = len(start_secs)
    notes_in = reference if not isinstance(reference, np.ndarray) else None
    n_ref_frames, n_est_frames, band = _align_frames(ref, end_sec, frames_per_second, band_sec)
    detok = model.compile_detokenizer(task_manager, max(n, 1), L)
    aligner = None
    try:
        aligner = model.compile_aligner(n_programs, max(n_ref_frames, n_est_frames), frames_per_second, band, drum_program)
        est, est_counts = detok.run_device(tokens, None, torch.tensor(start_secs, dtype=torch.float64), end_sec)
        ref_dev = torch.from_numpy(ref.view(np.uint8).reshape(-1).copy()).to(model.device)
        warp, result = aligner.align(ref_dev, est, n_ref_frames, n_est_frames, est_count=est_counts)
        warped = aligner.warp(ref_dev, warp).cpu().numpy().view(NOTE_RECORD_DTYPE)
        warp, result = warp.cpu().numpy(), result.cpu().numpy()
    finally:
        if aligner is not None:
            aligner.close()
        detok.close()
    notes = [Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"]),
                  **({} if notes_in is None else {"velocity": notes_in[i].velocity})) for i, r in enumerate(warped)]
    out = {"notes": notes, "total": int(result[0]), "path_len": int(result[1]), "n_ref_frames": n_ref_frames, "n_est_frames": n_est_frames,
           "warp": warp}
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        out["midi_path"] = write_midi(notes, os.path.join(output_dir, name + ".aligned.mid"))
    return out


def piano_roll(model, notes, end_sec: float, frames_per_second: float = 100.0, per_program: bool = False,
               task_manager: Optional[TaskManager] = None) -> torch.Tensor:
    """The piano roll of `notes` (a list of Note, a NOTE_RECORD array, or the path of a .mid file) over n_frames = max(1, ceil(end_sec *
    frames_per_second)) frames, rasterised on the device (PianoRoll.roll; the rules: yourmt3_amd/metrics.py, frame metrics).
    -> the (n_frames, 128) uint8 instrument-agnostic roll (all pitched notes; drums are not in it), or with `per_program=True` all
    (n_programs + 1, n_frames, 128) rows, the agnostic one last; a device tensor.  The programs are the TaskManager's."""
    if task_manager is None:
        task_manager = TaskManager("mc13_full_plus_256" if model.cfg.n_channels == 13 else "mt3_full_plus")
    if isinstance(notes, (str, os.PathLike)):
        with open(notes, "rb") as f:
            notes = read_midi_notes(f.read())
    rec = to_records(notes)
    lo, hi = task_manager.codec.range_of("program")
    n_frames = max(1, math.ceil(float(end_sec) * float(frames_per_second)))
    roll = model.compile_piano_roll(hi - lo, n_frames, frames_per_second)
    try:
        out = roll.roll(torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()), n_frames, rows=None if per_program else "agnostic")
    finally:
        roll.close()
    return out if per_program else out[0]
