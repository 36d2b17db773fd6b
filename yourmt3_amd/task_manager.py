"""TaskManager: token ids <-> note events <-> notes (host, integer state machines).

Kept API names (BASELINE.json north_star; signatures per SURVEY section 9, UNVERIFIED -- the reference tree has
no code): `TaskManager(task_name, max_shift_steps)`, `.tokenizer`, `.num_decoding_channels`,
`.max_note_token_length`, `.detokenize_list_batches(list_batch_token_arrays, list_start_sec, return_events)`.

Token grammar of one segment (MT3 style):
    [program p, pitch k]*  TIE     notes still sounding from the previous segment (tie section)
    then events in time order:  SHIFT n (time += n*10 ms) | VELOCITY v | PROGRAM p | PITCH k | DRUM k
    EOS, then PAD.
VELOCITY 1 makes the following pitches onsets, VELOCITY 0 offsets; drums have onsets only.

Task-conditioned tasks (`singing_drum_v1`) prefix every segment's decode with task tokens that select a sub-task
("transcribe everything", "singing only", "drums only"): `task_prompt(subtask, n)` gives the ids, which
YourMT3.inference(audio, task_tokens=...) feeds to the decoder before it emits (include/ymt3.h, task prompts).
BUILD-DEFINED: the task-token names, their ids and the sub-task prefixes are shaped after an unverified recollection
of upstream; nothing in the reference pins them.  The ids sit right after the codec's events
(Codec.size ...) inside the 1536-wide head; a real checkpoint's ids are an entry of the `task_token_ids` table.

Confidences: with the token scores of YourMT3.inference(return_scores=True) (log-probabilities, include/ymt3.h, token
scores), every onset event carries the score of its pitch or drum token and every note `confidence = exp(score)` of its
onset.  Both fields are left out of comparisons, ordering and hashing: notes without scores are exactly what they were.

Device path: `tokens_to_notes_device` is `tokens_to_notes` for ids that are still on the GPU (include/ymt3.h, device detokeniser;
yourmt3_amd/csrc/detok.hip): the same notes, confidences and invalid-token count, one small copy back instead of a Python loop over
every token.  The host path here stays the specification; `token_table()` is all the kernels know of the codec.

Constraints: `event_automaton(programs)` is the grammar above as a token automaton (yourmt3_amd/constraint.py) for
YourMT3.inference(constraint=...): the decoder then emits only well-formed segments whose notes belong to the allowed programs.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .constraint import TokenAutomaton, stack
from .vocab import Codec, Event, EOS, NUM_SPECIAL, PAD, UNK

DRUM_PROGRAM = 128
DRUM_NOTE_SEC = 0.01          # drums carry no offset: fixed nominal duration
# the 32-byte note record of the device codec and the device metrics (include/ymt3.h)
NOTE_RECORD = np.dtype([("onset", "<f8"), ("offset", "<f8"), ("program", "<i4"), ("pitch", "<i4"), ("is_drum", "<i4"), ("score", "<f4")])

# token classes of TaskManager.token_table() (include/ymt3.h, device detokeniser): class << 12 | event value
TOKEN_CLASSES = {"invalid": 0, "stop": 1, "skip": 2, "shift": 3, "pitch": 4, "velocity": 5, "tie": 6, "program": 7, "drum": 8}


@dataclass(frozen=True, order=True)
class NoteEvent:
    time: float
    is_drum: bool
    program: int
    velocity: int             # 1 onset, 0 offset
    pitch: int
    score: Optional[float] = field(default=None, compare=False)      # onsets: log-probability of the pitch / drum token


@dataclass(frozen=True, order=True)
class Note:
    onset: float
    offset: float
    is_drum: bool
    program: int
    pitch: int
    velocity: int = 100
    confidence: Optional[float] = field(default=None, compare=False)  # exp(score) of the onset's token, if scored


# instrument classes of the 13-channel decoder (MT3 "FULL_PLUS" grouping + singing + drums)
MC13_GROUPS: List[Tuple[str, Sequence[int]]] = [
    ("piano", range(0, 8)), ("chromatic_percussion", range(8, 16)), ("organ", range(16, 24)),
    ("guitar", range(24, 32)), ("bass", range(32, 40)), ("strings", range(40, 56)), ("brass", range(56, 64)),
    ("reed", range(64, 72)), ("pipe", range(72, 80)), ("synth_lead", range(80, 88)), ("synth_pad", range(88, 96)),
    ("singing", (129,)), ("drums", (128,)),
]

# task-token names in id order: by default they take the ids Codec.size, Codec.size + 1, ... (build-defined, see above)
TASK_TOKEN_NAMES: Tuple[str, ...] = ("task", "transcribe_all", "transcribe_singing", "transcribe_drum")
DEFAULT_VOCAB = 1536          # YMT3Config.vocab: the head the ids must fit in

TASKS: Dict[str, dict] = {
    "mt3_full_plus": {"channels": 1, "max_tokens": 1024},
    "mc13_full_plus_256": {"channels": 13, "max_tokens": 256},
    # sub-task -> prefix of task-token names (build-defined, shaped after an unverified recollection of upstream)
    "singing_drum_v1": {"channels": 1, "max_tokens": 1024, "subtasks": {
        "default": ("transcribe_all", "task"),
        "singing-only": ("transcribe_singing", "task"),
        "drum-only": ("transcribe_drum", "task"),
    }},
}


def default_task_token_ids(codec: Codec) -> Dict[str, int]:
    return {name: codec.size + i for i, name in enumerate(TASK_TOKEN_NAMES)}


class NoteEventTokenizer:
    def __init__(self, codec: Codec, skip_ids: Iterable[int] = ()):
        self.codec = codec
        self.skip_ids = frozenset(int(i) for i in skip_ids)     # task-token ids: skipped when decoding (neither events nor invalid)

    # ---------------------------------------------------------------- notes -> tokens (for tests / data)
    def encode_segment(self, events: Sequence[NoteEvent], tie_notes: Sequence[Tuple[int, int]], start_sec: float,
                       max_len: Optional[int] = None) -> List[int]:
        c = self.codec
        toks: List[int] = []
        for prog, pitch in sorted(tie_notes):
            toks += [c.encode(Event("program", prog)), c.encode(Event("pitch", pitch))]
        toks.append(c.encode(Event("tie", 0)))
        cur_step, cur_vel, cur_prog = 0, None, None
        for ev in sorted(events):
            step = int(round((ev.time - start_sec) * c.steps_per_second))
            d = step - cur_step
            while d > 0:
                n = min(d, c.max_shift_steps)
                toks.append(c.encode(Event("shift", n)))
                d -= n
            cur_step = max(cur_step, step)
            if ev.is_drum:
                if cur_vel != 1:
                    toks.append(c.encode(Event("velocity", 1)))
                    cur_vel = 1
                toks.append(c.encode(Event("drum", ev.pitch)))
                continue
            if ev.velocity != cur_vel:
                toks.append(c.encode(Event("velocity", ev.velocity)))
                cur_vel = ev.velocity
            if ev.program != cur_prog:
                toks.append(c.encode(Event("program", ev.program)))
                cur_prog = ev.program
            toks.append(c.encode(Event("pitch", ev.pitch)))
        toks.append(EOS)
        if max_len is not None:
            if len(toks) > max_len:
                raise ValueError(f"segment needs {len(toks)} tokens > {max_len}")
            toks += [PAD] * (max_len - len(toks))
        return toks

    # ---------------------------------------------------------------- tokens -> note events
    def decode_segment(self, tokens: Iterable[int], start_sec: float, scores: Optional[Sequence[float]] = None):
        """-> (events, tie_notes, n_invalid).  Stops at EOS/PAD; malformed tokens are counted, not fatal.  `scores`: one
        log-probability per token (aligned with `tokens`); each onset event stores its pitch / drum token's as `score`."""
        c = self.codec
        events: List[NoteEvent] = []
        ties: List[Tuple[int, int]] = []
        in_tie, step, vel, prog, bad = True, 0, 1, 0, 0
        for i, tk in enumerate(tokens):
            tk = int(tk)
            sc = None if scores is None else float(scores[i])
            if tk in (EOS, PAD):
                break
            if tk in self.skip_ids:
                continue
            ev = c.decode(tk)
            if ev.type == "special":                       # UNK or an id beyond the codec
                bad += 1
            elif ev.type == "tie":
                in_tie = False
            elif ev.type == "shift":
                in_tie = False
                step += ev.value
            elif ev.type == "velocity":
                vel = ev.value
            elif ev.type == "program":
                prog = ev.value
            elif ev.type == "pitch":
                if prog == DRUM_PROGRAM:                    # a pitch under the drum program is a drum hit: no ties, no offsets
                    if in_tie:
                        bad += 1
                    elif vel:
                        events.append(NoteEvent(start_sec + step / c.steps_per_second, True, DRUM_PROGRAM, 1, ev.value, sc))
                elif in_tie:
                    ties.append((prog, ev.value))
                else:
                    events.append(NoteEvent(start_sec + step / c.steps_per_second, False, prog, vel, ev.value, sc if vel else None))
            elif ev.type == "drum":
                if in_tie:
                    bad += 1
                else:
                    events.append(NoteEvent(start_sec + step / c.steps_per_second, True, DRUM_PROGRAM, 1, ev.value, sc))
        return events, ties, bad


def note_events_to_notes(segments: Sequence[Tuple[float, List[NoteEvent], List[Tuple[int, int]]]], end_sec: float) -> List[Note]:
    """Merge per-segment (start_sec, events, tie_notes) into notes.

    A note sounding at a segment boundary stays open only if the next segment's tie section lists it;
    otherwise it is closed at that segment's start.  Offsets without an onset are dropped; a repeated
    onset re-triggers (closes the old note at the new onset); a drum hit repeated at the same time and
    pitch (the model emitting a token twice) is one hit.  A note's confidence is exp(score) of its onset event (None
    without one), carried across segments with the onset; a de-duplicated drum hit keeps the larger of its confidences.
    """
    active: Dict[Tuple[int, int], Tuple[float, Optional[float]]] = {}     # (program, pitch) -> (onset, confidence)
    notes: List[Note] = []
    drum_hits: Dict[Tuple[float, int], int] = {}                          # (time, pitch) -> index in notes
    for start, events, ties in sorted(segments, key=lambda s: s[0]):
        tie_set = set(ties)
        for key in [k for k in active if k not in tie_set]:
            on, conf = active.pop(key)
            if start > on:
                notes.append(Note(on, start, False, key[0], key[1], confidence=conf))
        for ev in sorted(events):
            conf = None if ev.score is None else math.exp(ev.score)
            if ev.is_drum:
                hit = (ev.time, ev.pitch)
                if hit not in drum_hits:
                    drum_hits[hit] = len(notes)
                    notes.append(Note(ev.time, ev.time + DRUM_NOTE_SEC, True, DRUM_PROGRAM, ev.pitch, confidence=conf))
                elif conf is not None:
                    old = notes[drum_hits[hit]]
                    if old.confidence is None or conf > old.confidence:
                        notes[drum_hits[hit]] = replace(old, confidence=conf)
                continue
            key = (ev.program, ev.pitch)
            if ev.velocity:
                if key in active and ev.time > active[key][0]:
                    notes.append(Note(active[key][0], ev.time, False, key[0], key[1], confidence=active[key][1]))
                active[key] = (ev.time, conf)
            elif key in active:
                on, oconf = active.pop(key)
                if ev.time > on:
                    notes.append(Note(on, ev.time, False, key[0], key[1], confidence=oconf))
    for key, (on, conf) in active.items():
        if end_sec > on:
            notes.append(Note(on, end_sec, False, key[0], key[1], confidence=conf))
    return sorted(notes)


class NoteStream:
    """note_events_to_notes for ONE channel whose segments arrive over time: the same merge with its state carried from call to call,
    and the specification of the incremental device detokeniser (include/ymt3.h).

    push(segments, horizon_sec): `segments` are (start_sec, events, tie_notes) as for note_events_to_notes, later than everything pushed
    before; `horizon_sec` is the start time of the next segment not yet pushed (+inf: none will come before finish).  The call returns
    every note the one-shot merge appends while it processes these segments, except drum hits with time >= horizon_sec: a hit of a
    later segment at the same f64 time and pitch is merged into them and may raise their confidence, and every event of a later segment
    lies at or after that segment's start, so those hits -- and only those -- can still change.  They are held, and returned by the
    first later push whose horizon exceeds their time, or by finish.  finish(end_sec) also closes what is still sounding, by the rule of
    the one-shot loop's tail.  A returned note never changes and is never returned again:
    sorted(everything returned) == note_events_to_notes(all the segments, end_sec), confidences included, for every split."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self._active: Dict[Tuple[int, int], Tuple[float, Optional[float]]] = {}   # (program, pitch) -> (onset, confidence)
        self._held: Dict[Tuple[float, int], Note] = {}                              # (time, pitch) -> the hit, still open
        self._last_start = -math.inf
        self._finished = False

    @property
    def n_held(self) -> int:
        return len(self._held)

    def _release(self, horizon_sec: float) -> List[Note]:
        out = [n for hit, n in self._held.items() if hit[0] < horizon_sec]
        self._held = {hit: n for hit, n in self._held.items() if not hit[0] < horizon_sec}
        return out

    def push(self, segments: Sequence[Tuple[float, List[NoteEvent], List[Tuple[int, int]]]], horizon_sec: float) -> List[Note]:
        if self._finished:
            raise ValueError("the stream has been finished: reset it first")
        segments = sorted(segments, key=lambda s: s[0])
        starts = [self._last_start] + [float(s[0]) for s in segments]
        if any(b <= a for a, b in zip(starts, starts[1:])):
            raise ValueError("segment start times must be strictly increasing over the whole stream")
        if not horizon_sec >= starts[-1] or horizon_sec == -math.inf:
            raise ValueError(f"horizon_sec={horizon_sec} lies before the last pushed segment's start {starts[-1]}")
        active, held = self._active, self._held
        notes: List[Note] = []
        for start, events, ties in segments:
            tie_set = set(ties)
            for key in [k for k in active if k not in tie_set]:
                on, conf = active.pop(key)
                if start > on:
                    notes.append(Note(on, start, False, key[0], key[1], confidence=conf))
            for ev in sorted(events):
                conf = None if ev.score is None else math.exp(ev.score)
                if ev.is_drum:
                    hit = (ev.time, ev.pitch)
                    if hit not in held:
                        held[hit] = Note(ev.time, ev.time + DRUM_NOTE_SEC, True, DRUM_PROGRAM, ev.pitch, confidence=conf)
                    elif conf is not None:
                        old = held[hit]
                        if old.confidence is None or conf > old.confidence:
                            held[hit] = replace(old, confidence=conf)
                    continue
                key = (ev.program, ev.pitch)
                if ev.velocity:
                    if key in active and ev.time > active[key][0]:
                        notes.append(Note(active[key][0], ev.time, False, key[0], key[1], confidence=active[key][1]))
                    active[key] = (ev.time, conf)
                elif key in active:
                    on, oconf = active.pop(key)
                    if ev.time > on:
                        notes.append(Note(on, ev.time, False, key[0], key[1], confidence=oconf))
        self._last_start = starts[-1]
        return sorted(notes + self._release(horizon_sec))

    def finish(self, end_sec: float) -> List[Note]:
        if self._finished:
            raise ValueError("the stream has been finished: reset it first")
        notes = list(self._held.values())
        for key, (on, conf) in self._active.items():
            if end_sec > on:
                notes.append(Note(on, end_sec, False, key[0], key[1], confidence=conf))
        self._held, self._active, self._finished = {}, {}, True
        return sorted(notes)


def drop_low_confidence(notes: Sequence[Note], min_confidence: float) -> List[Note]:
    """The notes whose confidence is at least `min_confidence`, in their order.  A note without a confidence (decoded without
    scores) has nothing to be judged by and is kept."""
    return [n for n in notes if n.confidence is None or n.confidence >= min_confidence]


class TaskManager:
    """`vocab_size`: the decoder head the task-token ids must fit in; `task_token_ids`: name -> id entries replacing the
    build-defined defaults (default_task_token_ids), e.g. the ids a real checkpoint was trained with."""

    def __init__(self, task_name: str = "mt3_full_plus", max_shift_steps: int = 206, debug_mode: bool = False,
                 vocab_size: int = DEFAULT_VOCAB, task_token_ids: Optional[Dict[str, int]] = None):
        if task_name not in TASKS:
            raise ValueError(f"unknown task {task_name!r}; known: {sorted(TASKS)}")
        self.task_name = task_name
        self.task = TASKS[task_name]
        self.codec = Codec(max_shift_steps=max_shift_steps)
        self.subtasks: Dict[str, Tuple[str, ...]] = dict(self.task.get("subtasks", {}))
        self.task_token_ids: Dict[str, int] = {}
        if self.subtasks:
            ids = default_task_token_ids(self.codec)
            for name, i in (task_token_ids or {}).items():
                if name not in ids:
                    raise ValueError(f"unknown task token {name!r}; known: {list(TASK_TOKEN_NAMES)}")
                ids[name] = int(i)
            bad = {n: i for n, i in ids.items() if not (NUM_SPECIAL <= i < vocab_size)}
            if bad:
                raise ValueError(f"task-token ids {bad} do not fit a vocabulary of {vocab_size} (specials below {NUM_SPECIAL})")
            if len(set(ids.values())) != len(ids) or any(i < self.codec.size for i in ids.values()):
                raise ValueError(f"task-token ids {ids} must be distinct and must not reuse a codec event id (< {self.codec.size})")
            self.task_token_ids = ids
        self.vocab_size = int(vocab_size)
        self.tokenizer = NoteEventTokenizer(self.codec, self.task_token_ids.values())
        self.num_decoding_channels = self.task["channels"]
        self.max_note_token_length = self.task["max_tokens"]
        self.debug_mode = debug_mode

    def task_prompt(self, subtask: Optional[str] = None, n_segments: int = 1) -> np.ndarray:
        """(n_segments, channels, P) int32 task-token prefix of `subtask` (None: "default") for YourMT3.inference(task_tokens=...).
        A task without task tokens has no prompt: it raises."""
        if not self.subtasks:
            raise ValueError(f"task {self.task_name!r} defines no task tokens")
        name = "default" if subtask is None else subtask
        if name not in self.subtasks:
            raise ValueError(f"unknown sub-task {name!r} of {self.task_name!r}; known: {sorted(self.subtasks)}")
        ids = np.array([self.task_token_ids[t] for t in self.subtasks[name]], np.int32)
        return np.array(np.broadcast_to(ids, (int(n_segments), self.num_decoding_channels, ids.size)))     # (a writable copy)

    def event_automaton(self, programs: Optional[Iterable[int]] = None) -> Tuple[TokenAutomaton, np.ndarray]:
        """The segment grammar as a token automaton for the allowed programs P (`programs`; None: all of 0..129, 128 = drums,
        129 = singing) -> (automaton, start states (channels,) int32).  With 13 channels channel k gets P & MC13_GROUPS[k]
        (stacked: every channel's own six states).  Tokens that decode_segment counts as invalid are never allowed (PAD, UNK,
        ids beyond the codec, task tokens included), nor are notes of programs outside P; a channel whose P is empty can only
        emit TIE, EOS."""
        n_prog = self.codec.range_of("program")[1] - self.codec.range_of("program")[0]
        P = set(range(n_prog)) if programs is None else {int(p) for p in programs}
        bad = sorted(p for p in P if not 0 <= p < n_prog)
        if bad:
            raise ValueError(f"programs {bad} outside [0, {n_prog})")
        if self.num_decoding_channels == 1:
            sets = [P]
        else:
            sets = [P & set(progs) for _, progs in MC13_GROUPS[:self.num_decoding_channels]]
        aut, offsets = stack([self._segment_grammar(p) for p in sets])
        return aut, np.array(offsets, np.int32)

    def _segment_grammar(self, P) -> TokenAutomaton:
        """Six states: section (0 tie, 1 body) x current program (0 unset -- decode_segment reads program 0 --, 1 pitched,
        2 drum); state = 3 * section + program, start 0."""
        c, V = self.codec, self.vocab_size
        rng = {t: c.range_of(t) for t in ("shift", "pitch", "velocity", "tie", "program", "drum")}
        prog0 = rng["program"][0]
        tie_tok = rng["tie"][0]
        allowed = np.zeros((6, V), bool)
        nxt = np.zeros((6, V), np.int32)
        for sec in (0, 1):
            for prog in (0, 1, 2):
                s = 3 * sec + prog
                a = allowed[s]
                pitch_ok = prog == 1 or (prog == 0 and 0 in P) or (sec == 1 and prog == 2)
                if pitch_ok:
                    a[slice(*rng["pitch"])] = True
                for p in P:
                    if sec == 1 or p != DRUM_PROGRAM:
                        a[prog0 + p] = True
                if sec == 0:
                    a[tie_tok] = True
                else:
                    if P:                           # (with nothing to transcribe a channel says TIE, EOS and nothing else)
                        a[slice(*rng["shift"])] = True
                        a[slice(*rng["velocity"])] = True
                    if DRUM_PROGRAM in P:
                        a[slice(*rng["drum"])] = True
                    a[EOS] = True
                # transitions, for every token (forced ids included): TIE and SHIFT open the body, PROGRAM sets the program
                nxt[s, :] = s
                nxt[s, tie_tok] = 3 + prog
                nxt[s, slice(*rng["shift"])] = 3 + prog
                nxt[s, slice(*rng["program"])] = 3 * sec + 1
                nxt[s, prog0 + DRUM_PROGRAM] = 3 * sec + 2
        return TokenAutomaton(allowed, nxt)

    def channel_of_program(self, program: int) -> int:
        if self.num_decoding_channels == 1:
            return 0
        for ch, (_, progs) in enumerate(MC13_GROUPS):
            if program in progs:
                return ch
        return 0

    def detokenize_list_batches(self, list_batch_token_arrays: Sequence[np.ndarray], list_start_sec: Sequence[float],
                                return_events: bool = False, list_batch_score_arrays: Optional[Sequence[np.ndarray]] = None):
        """list of (b, L) int arrays (ONE channel: pass arr[:, ch, :]) + start time of every segment ->
        per-segment (start, events, ties); with return_events also the invalid-token count.  `list_batch_score_arrays`:
        the matching (b, L) token scores; onset events then carry their token's score."""
        flat = np.concatenate([np.asarray(a) for a in list_batch_token_arrays], 0)
        if flat.shape[0] != len(list_start_sec):
            raise ValueError(f"{flat.shape[0]} segments but {len(list_start_sec)} start times")
        flat_sc = None
        if list_batch_score_arrays is not None:
            flat_sc = np.concatenate([np.asarray(a) for a in list_batch_score_arrays], 0)
            if flat_sc.shape != flat.shape:
                raise ValueError(f"scores {flat_sc.shape} do not match tokens {flat.shape}")
        segs, bad = [], 0
        for i, (row, start) in enumerate(zip(flat, list_start_sec)):
            ev, ties, b = self.tokenizer.decode_segment(row, float(start), None if flat_sc is None else flat_sc[i])
            segs.append((float(start), ev, ties))
            bad += b
        return (segs, bad) if return_events else segs

    def tokens_to_notes(self, token_batches: Sequence[np.ndarray], start_secs: Sequence[float], end_sec: float,
                        score_batches: Optional[Sequence[np.ndarray]] = None) -> List[Note]:
        """All channels: token_batches are (b, K, L); channels are decoded independently and mixed.  `score_batches`: the
        matching (b, K, L) token scores (YourMT3.inference_file(return_scores=True)); every note then has
        confidence = exp(score of its onset's token)."""
        notes: List[Note] = []
        for ch in range(self.num_decoding_channels):
            sc = None if score_batches is None else [np.asarray(a)[:, ch, :] for a in score_batches]
            segs = self.detokenize_list_batches([np.asarray(a)[:, ch, :] for a in token_batches], start_secs, list_batch_score_arrays=sc)
            notes += note_events_to_notes(segs, end_sec)
        return sorted(notes)

    def notes_to_tokens(self, notes: Sequence[Note], start_secs: Sequence[float], end_sec: float,
                        max_len: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Notes -> (tokens (n, K, L) int32 PAD-filled, lengths (n, K) int32, EOS included): the inverse of tokens_to_notes and the
        specification of the device tokeniser (notes_to_tokens_device; include/ymt3.h, device tokeniser).  L = max_len or
        max_note_token_length; `start_secs` must be strictly increasing.  Rules:
          - a note whose onset is not in [start_secs[0], end_sec) is dropped (so is one with a NaN onset, or a pitched one with a NaN
            offset); a drum note counts as program DRUM_PROGRAM; the channel is channel_of_program(program);
          - the onset belongs to the last segment s with start[s] <= onset, at step int(round((onset - start[s]) * steps_per_second))
            (f64, half to even), and every event's time is the canonical start[s] + step / steps_per_second;
          - a drum note is one onset event (velocity 1), no offset, no ties;
          - a pitched note is in the tie section of every later segment s' with start[s'] < offset; a tie section lists a (program,
            pitch) once;
          - its offset event (velocity 0) goes to the segment that contains `offset`, except: offset >= end_sec gives none (the
            detokeniser closes the note at end_sec), offset == start[s'] of a later segment gives none (the missing tie closes it
            there), and an offset that would land in the onset's segment at or before the onset's step (or before that segment) is
            placed at the onset's step + 1, even past the segment's nominal end: a note never loses its own onset;
          - every (segment, channel) row is encode_segment(events, sorted(ties), start[s]); an empty row is TIE, EOS.
        A row that needs more than L tokens raises ValueError naming the segment, the channel and the count.
        Round trip: for notes on the 10 ms grid of their segment (onset and offset are start[s] + k / steps_per_second of the segment
        they fall in, or offset == end_sec), with no two notes of one (program, pitch) overlapping, no duplicate drum hits, drum notes
        of program DRUM_PROGRAM and DRUM_NOTE_SEC long, tokens_to_notes([notes_to_tokens(...)[0]], start_secs, end_sec) ==
        sorted(notes), f64 times included.  Outside these preconditions the function still defines the ids."""
        import bisect

        starts = [float(s) for s in start_secs]
        n, K = len(starts), self.num_decoding_channels
        L = int(max_len or self.max_note_token_length)
        if any(b <= a for a, b in zip(starts, starts[1:])):
            raise ValueError("start_secs must be strictly increasing")
        end_sec = float(end_sec)
        sps = self.codec.steps_per_second
        events: List[List[List[NoteEvent]]] = [[[] for _ in range(K)] for _ in range(n)]
        ties: List[List[set]] = [[set() for _ in range(K)] for _ in range(n)]
        time_of = lambda s, step: starts[s] + step / sps
        for note in notes if n else ():
            onset, offset = float(note.onset), float(note.offset)
            if not (starts[0] <= onset < end_sec):
                continue
            prog = DRUM_PROGRAM if note.is_drum else int(note.program)
            pitch = int(note.pitch)
            ch = self.channel_of_program(prog)
            s = bisect.bisect_right(starts, onset) - 1
            step = int(round((onset - starts[s]) * sps))
            if note.is_drum:
                events[s][ch].append(NoteEvent(time_of(s, step), True, DRUM_PROGRAM, 1, pitch))
                continue
            if offset != offset:
                continue
            events[s][ch].append(NoteEvent(time_of(s, step), False, prog, 1, pitch))
            for s2 in range(s + 1, n):
                if not starts[s2] < offset:
                    break
                ties[s2][ch].add((prog, pitch))
            if offset >= end_sec:
                continue
            so = bisect.bisect_right(starts, offset) - 1
            if so <= s:
                d = (offset - starts[s]) * sps
                so, ostep = s, (int(round(d)) if d > step else step + 1)
                if ostep <= step:
                    ostep = step + 1
            elif offset == starts[so]:
                continue
            else:
                ostep = int(round((offset - starts[so]) * sps))
            events[so][ch].append(NoteEvent(time_of(so, ostep), False, prog, 0, pitch))
        tokens = np.full((n, K, L), PAD, np.int32)
        lengths = np.zeros((n, K), np.int32)
        for s in range(n):
            for ch in range(K):
                row = self.tokenizer.encode_segment(events[s][ch], sorted(ties[s][ch]), starts[s])
                if len(row) > L:
                    raise ValueError(f"segment {s} channel {ch} needs {len(row)} tokens > {L}")
                tokens[s, ch, :len(row)] = row
                lengths[s, ch] = len(row)
        return tokens, lengths

    def tok_params(self) -> Tuple[Dict[str, int], np.ndarray]:
        """All the device tokeniser knows of the codec (include/ymt3.h, ymt3_tok_params): the first id of every event range, the
        shift limit, the step rate, the drum program, EOS and PAD -> (fields, program -> channel (n_programs,) uint8)."""
        c = self.codec
        f = {t + "_base": c.range_of(t)[0] for t in ("shift", "pitch", "velocity", "tie", "program", "drum")}
        f.update(max_shift_steps=c.max_shift_steps, steps_per_second=c.steps_per_second, drum_program=DRUM_PROGRAM, eos_id=EOS, pad_id=PAD)
        n_prog = c.range_of("program")[1] - c.range_of("program")[0]
        return f, np.array([self.channel_of_program(p) for p in range(n_prog)], np.uint8)

    def token_table(self) -> np.ndarray:
        """(vocab_size,) uint16: TOKEN_CLASSES[class] << 12 | event value for every id, as decode_segment reads it: PAD / EOS stop,
        the tokenizer's skip_ids (task tokens) skip, UNK and every id Codec.decode calls `special` invalid, events their type and value."""
        table = np.zeros(self.vocab_size, np.uint16)
        for i in range(self.vocab_size):
            if i in (EOS, PAD):
                cls, val = "stop", 0
            elif i in self.tokenizer.skip_ids:
                cls, val = "skip", 0
            else:
                ev = self.codec.decode(i)
                cls, val = ("invalid", 0) if ev.type == "special" else (ev.type, ev.value)
            if not 0 <= val < 4096:
                raise ValueError(f"event value {val} of token {i} does not fit 12 bits")
            table[i] = TOKEN_CLASSES[cls] << 12 | val
        return table

    def tokens_to_notes_device(self, model, tokens, start_secs: Sequence[float], end_sec: float, scores=None,
                               detokenizer=None, velocity=None, audio=None, beats=None, quantize: int = 0, bars=None, chords=None,
                               sections=None, hands=None):
        """tokens_to_notes on the device -> (notes, n_invalid).  `tokens`: (n, K, L) integer ids on `model`'s GPU (any strides whose
        last dimension is contiguous, e.g. hypothesis 0 of a beam call's (n, K, N, L)); `scores`: the matching (n, K, L) f32 token scores
        or None; `start_secs` must be strictly increasing.  `detokenizer`: a YourMT3.compile_detokenizer object to reuse (None: one is
        made for this call and closed).  One copy back of the counters and the notes' records; confidence = exp(score) on the host.
        `velocity`: a YourMT3.compile_note_velocity object, with `audio` the flat f32 samples the segments were cut from, on the GPU
        (YourMT3.ingest's buffer as it is): every note's velocity is measured on the records where they lie, their number read from the
        detokeniser's counter on the device, and the bytes come back in the records' copy.
        `beats`: a YourMT3.compile_beat_tracker object: the beats are tracked on the records where they lie (over the frames of `end_sec`,
        beats.n_frames_of), every note gets its ticks (snapped to `quantize` steps per beat if that is not 0), and beats, tempo and ticks
        come back in the same copy: the result gains a third element, {"beats" (frames), "tempo" (lags per window), "ticks" ((n, 2), in
        the returned notes' order)}.
        `bars`: a YourMT3.compile_bar_tracker object (it needs `beats`, and the beat tracker's frames_per_second): metres, downbeats and
        key are tracked on the same records and beats where they lie, and ride back in the same copy: the third element gains "metre"
        (int32 (n_beats,), 256 m + k) and "bar_result" (int64 (8,), bars.track_bars' result).
        `chords`: a YourMT3.compile_chord_tracker object (it needs `beats`; with `bars` it uses their metre): a chord per beat, tracked on
        the same records and beats where they lie, riding back in the same copy: the third element gains "chord" (int32 (n_beats,),
        256 bass + label) and "chord_result" (int64 (8,), chords.track_chords' result).
        `sections`: a YourMT3.compile_section_tracker object (it needs `beats`; with `bars` it uses their metre): the song's form, tracked
        on the same records and beats where they lie, riding back in the same copy: the third element gains "section" (int32 (n_beats,),
        65536 start + 256 s + label), "novelty" (int64 (n_beats,)) and "section_result" (int64 (8,), sections.track_sections' result).
        `hands`: a YourMT3.compile_hand_splitter object whose max_notes holds the detokeniser's capacity (it needs no beats): every note's
        hand, found on the records where they lie under the device count (over the frames of `end_sec`), the bytes riding back in the
        same copy: the last element (a third one is made if there is none) gains "hand" (uint8 (n,), in the returned notes' order, as
        "ticks" are), "hand_result" (int64 (8,), hands.split_hands' result) and "hand_split" (int32 (T,), 256 slot + split point of every slice)."""
        import torch

        if bars is not None and beats is None:
            raise ValueError("bars without beats: the bar tracker works on the beat tracker's beats")
        if chords is not None and beats is None:
            raise ValueError("chords without beats: the chord tracker works on the beat tracker's beats")
        if sections is not None and beats is None:
            raise ValueError("sections without beats: the section tracker works on the beat tracker's beats")
        starts = np.asarray(list(start_secs), np.float64)
        if tokens.dim() != 3 or tokens.shape[1] != self.num_decoding_channels:
            raise ValueError(f"tokens must be (n, {self.num_decoding_channels}, L), got {tuple(tokens.shape)}")
        n, K, L = (int(v) for v in tokens.shape)
        if starts.shape != (n,):
            raise ValueError(f"{n} segments but {starts.size} start times")
        if n > 1 and not bool(np.all(starts[1:] > starts[:-1])):
            raise ValueError("start_secs must be strictly increasing")
        if scores is not None and tuple(scores.shape) != tuple(tokens.shape):
            raise ValueError(f"scores {tuple(scores.shape)} do not match tokens {tuple(tokens.shape)}")
        if (velocity is None) != (audio is None):
            raise ValueError("velocity and audio go together")
        if n == 0 or L == 0:
            if beats is not None or hands is not None:
                from .tracking import empty
                none = empty(bars is not None, chords is not None, sections is not None) if beats is not None else {}
                if hands is not None:
                    none.update(hand=np.zeros(0, np.uint8), hand_result=np.zeros(8, np.int64), hand_split=np.zeros(0, np.int32))
                return [], 0, none
            return [], 0
        own = detokenizer is None
        if own:
            detokenizer = model.compile_detokenizer(self, n, L)
        try:
            tracked = hand = None
            if velocity is None and beats is None and hands is None:
                rec, n_invalid = detokenizer.run(tokens, scores, torch.from_numpy(starts), float(end_sec))
                vel = None
            else:
                rec_dev, counts = detokenizer.run_device(tokens, scores, torch.from_numpy(starts), float(end_sec))
                vel_dev = velocity.run(audio, rec_dev, count=counts)[0] if velocity is not None else None
                if beats is not None:                                    # under the device count, before it is copied back
                    from . import tracking
                    from .beats import n_frames_of
                    n_frames = n_frames_of(end_sec, beats.params["frames_per_second"])
                    parts = tracking.launch_beats(beats, rec_dev, n_frames, counts, quantize)
                if hands is not None:                                    # under the device count too
                    from .beats import n_frames_of
                    hand_dev, hand_split, hand_result = hands.split(rec_dev, n_frames_of(end_sec, hands.params["frames_per_second"]), count=counts)
                n_notes, n_invalid = (int(v) for v in counts.cpu().tolist())
                nb = n_notes * NOTE_RECORD.itemsize
                riders = [rec_dev[:nb]] + ([vel_dev[:n_notes]] if velocity is not None else [])
                if beats is not None:                                    # bars and chords on the live records: their number is known by now, the beats' is not
                    parts["ticks"] = parts["ticks"][:n_notes]
                    tracking.launch_bars_chords(parts, bars, chords, rec_dev[:nb], n_frames, sections=sections)
                    riders += tracking.pack(parts)
                if hands is not None:                                    # last: the tracking parts keep their place
                    riders += [hand_dev[:n_notes], hand_result.view(torch.uint8), hand_split.view(torch.uint8)]
                both = torch.cat(riders).cpu().numpy()
                rec, o = both[:nb].view(NOTE_RECORD), nb
                vel = None
                if velocity is not None:
                    vel, o = both[o:o + n_notes].tolist(), o + n_notes
                if beats is not None:
                    lay = tracking.layout(parts)
                    words = sum(w for _, w in lay)
                    tracked, o = tracking.unpack(both[o:o + 4 * words].view(np.int32), lay), o + 4 * words
                if hands is not None:
                    hand, hand_result = both[o:o + n_notes].copy(), both[o + n_notes:o + n_notes + 64].copy().view(np.int64)
                    hand_split = both[o + n_notes + 64:].copy().view(np.int32)[:int(hand_result[0])]
        finally:
            if own:
                detokenizer.close()
        scored = scores is not None
        notes = [Note(on, off, bool(dr), pg, pt, confidence=math.exp(sc) if scored else None)
                 for on, off, pg, pt, dr, sc in zip(rec["onset"].tolist(), rec["offset"].tolist(), rec["program"].tolist(),
                                                    rec["pitch"].tolist(), rec["is_drum"].tolist(), rec["score"].astype(np.float64).tolist())]
        if vel is not None:
            notes = [replace(x, velocity=v) for x, v in zip(notes, vel)]
        if tracked is not None or hand is not None:
            order = sorted(range(len(notes)), key=notes.__getitem__)
            tracked = {} if tracked is None else tracked
            if "ticks" in tracked:
                tracked["ticks"] = tracked["ticks"][order]
            if hand is not None:
                tracked["hand"], tracked["hand_result"], tracked["hand_split"] = hand[order], hand_result, hand_split
            return [notes[i] for i in order], n_invalid, tracked
        return sorted(notes), n_invalid

    def tokens_to_notes_stream(self, model, detokenizer, state, tokens=None, start_secs: Sequence[float] = (), horizon_sec: float = math.inf,
                               scores=None, end_sec: Optional[float] = None, scored: Optional[bool] = None) -> Tuple[List[Note], int, int]:
        """One call of the incremental device detokeniser (include/ymt3.h; the specification is NoteStream, per channel) ->
        (notes that became final, n_invalid, n_forced).  `detokenizer` / `state`: YourMT3.compile_detokenizer and its new_state().
        A push: `tokens` (n, K, L) ids on the GPU, later than everything pushed before, `start_secs` their strictly increasing start
        times, `horizon_sec` the start of the next segment not yet pushed (+inf: none before the end).  The finish: `end_sec` and no
        tokens.  Notes carry confidence = exp(score) iff scores are in use (`scored`; by default whether `scores` is given -- pass it
        at the finish).  One copy back of the counters and the new records.  n_forced != 0: the state's max_held was reached and the
        result may differ from the one-shot one."""
        import torch

        if end_sec is not None:
            if tokens is not None:
                raise ValueError("the finish takes no tokens")
            rec_dev, counts = detokenizer.finish_device(state, float(end_sec))
        else:
            starts = np.asarray(list(start_secs), np.float64)
            if tokens is None or tokens.dim() != 3 or tokens.shape[1] != self.num_decoding_channels:
                raise ValueError(f"tokens must be (n, {self.num_decoding_channels}, L)")
            n = int(tokens.shape[0])
            if starts.shape != (n,):
                raise ValueError(f"{n} segments but {starts.size} start times")
            last = getattr(state, "last_start", -math.inf)
            if n and not (bool(np.all(np.diff(starts) > 0)) and starts[0] > last):
                raise ValueError("start_secs must be strictly increasing over the whole stream")
            if not float(horizon_sec) >= (starts[-1] if n else last) or float(horizon_sec) == -math.inf:
                raise ValueError(f"horizon_sec={horizon_sec} lies before the last pushed segment's start")
            if scores is not None and tuple(scores.shape) != tuple(tokens.shape):
                raise ValueError(f"scores {tuple(scores.shape)} do not match tokens {tuple(tokens.shape)}")
            rec_dev, counts = detokenizer.push_device(state, tokens, scores, torch.from_numpy(starts), float(horizon_sec))
            if n:
                state.last_start = float(starts[-1])
        n_notes, n_invalid, n_forced = (int(v) for v in counts.cpu().tolist())
        from .model import NOTE_RECORD
        rec = rec_dev[:n_notes * NOTE_RECORD.itemsize].cpu().numpy().view(NOTE_RECORD)
        if scored is None:
            scored = scores is not None
        notes = [Note(on, off, bool(dr), pg, pt, confidence=math.exp(sc) if scored else None)
                 for on, off, pg, pt, dr, sc in zip(rec["onset"].tolist(), rec["offset"].tolist(), rec["program"].tolist(),
                                                    rec["pitch"].tolist(), rec["is_drum"].tolist(), rec["score"].astype(np.float64).tolist())]
        return sorted(notes), n_invalid, n_forced

    def notes_to_tokens_device(self, model, notes, start_secs: Sequence[float], end_sec: float, max_len: Optional[int] = None,
                               tokenizer=None):
        """notes_to_tokens on the device -> (tokens (n, K, L) int32, lengths (n, K) int32) as tensors on `model`'s GPU.  `notes`: a
        list of Note, or a uint8 tensor of NOTE_RECORD bytes already on the GPU (e.g. the records ymt3_detokenize wrote: nothing of
        them touches the host).  `start_secs` must be strictly increasing.  `tokenizer`: a YourMT3.compile_tokenizer object to reuse
        (None: one is made for this call and closed).  A note list is checked like the host path checks it (program and pitch inside
        the codec's ranges, ValueError); records outside them are dropped on the device (include/ymt3.h, device tokeniser).  One copy
        back of the lengths: a row that needs more than L tokens raises the host path's ValueError (its count is a lower bound when the
        row has more than L events or a gap of more than L shift tokens)."""
        import torch
        from .model import NOTE_RECORD

        starts = np.asarray(list(start_secs), np.float64)
        n, K = int(starts.size), self.num_decoding_channels
        L = int(max_len or self.max_note_token_length)
        if n > 1 and not bool(np.all(starts[1:] > starts[:-1])):
            raise ValueError("start_secs must be strictly increasing")
        if isinstance(notes, torch.Tensor):
            records = notes
        else:
            n_prog = self.codec.range_of("program")[1] - self.codec.range_of("program")[0]
            rec = np.zeros(len(notes), NOTE_RECORD)
            for i, nt in enumerate(notes):
                prog = DRUM_PROGRAM if nt.is_drum else int(nt.program)
                if not (0 <= prog < n_prog and 0 <= int(nt.pitch) < 128):
                    raise ValueError(f"{nt}: program outside [0, {n_prog}) or pitch outside [0, 128)")
                rec[i] = (nt.onset, nt.offset, prog, nt.pitch, bool(nt.is_drum), 0.0)
            records = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(model.device)
        own = tokenizer is None
        if own:
            tokenizer = model.compile_tokenizer(self, max(n, 1), L)
        try:
            tokens, lengths = tokenizer.run(records, torch.from_numpy(starts), float(end_sec), L)
            over = (lengths > L).nonzero().cpu().tolist()
            if over:
                s, ch = over[0]
                raise ValueError(f"segment {s} channel {ch} needs {int(lengths[s, ch])} tokens > {L}")
        finally:
            if own:
                tokenizer.close()
        return tokens, lengths
