"""Minimal Standard MIDI File (format 1) writer/reader for Note lists (mido / pretty_midi are absent)."""
from __future__ import annotations

import bisect
import struct
from typing import Dict, List, Sequence

from .task_manager import Note, DRUM_PROGRAM

TICKS_PER_BEAT = 480
TEMPO_US = 500000                      # 120 bpm -> 960 ticks per second


def _vlq(n: int) -> bytes:
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def _ticks(sec: float) -> int:
    return int(round(sec * TICKS_PER_BEAT * 1e6 / TEMPO_US))


SINGING_PROGRAM = 129
SINGING_GM_PROGRAM = 53                # GM "Voice Oohs": the defined stand-in for the vocabulary's singing-voice program


def gm_program(program: int) -> int:
    """Vocabulary program -> General MIDI program number of the program-change event."""
    if program == SINGING_PROGRAM:
        return SINGING_GM_PROGRAM
    if not 0 <= program <= 127:
        raise ValueError(f"program {program} has no General MIDI number")
    return program


def _fit_melodic_channels(by_prog: Dict[int, List[Note]]) -> Dict[int, List[Note]]:
    """A Standard MIDI File has 15 melodic channels (16 minus the drum channel) and ONE program per channel at a time.
    With more than 15 melodic programs, programs of one GM instrument family (program // 8) are merged onto the family's
    lowest program present, largest families first, until 15 remain -- deterministic, and never two programs on one
    channel.  Still more than 15 distinct families (only with all 16 GM families plus singing present): error."""
    melodic = sorted(p for p in by_prog if p != DRUM_PROGRAM)
    if len(melodic) <= 15:
        return by_prog
    family = lambda p: 16 if p == SINGING_PROGRAM else p // 8
    groups: Dict[int, List[int]] = {}
    for p in melodic:
        groups.setdefault(family(p), []).append(p)
    merged = {p: p for p in melodic}
    n = len(melodic)
    for fam in sorted(groups, key=lambda f: (-len(groups[f]), f)):
        if n <= 15:
            break
        members = groups[fam]
        if len(members) > 1:
            for p in members[1:]:
                merged[p] = members[0]
            n -= len(members) - 1
    if n > 15:
        raise ValueError(f"{n} instrument families do not fit the 15 melodic MIDI channels")
    out: Dict[int, List[Note]] = {}
    for p, ns in by_prog.items():
        out.setdefault(merged.get(p, p), []).extend(ns)
    return out


HAND_TRACKS = ((1, b"R.H."), (0, b"L.H."))  # (hand, track name) in the order of a split program's tracks: hands.RIGHT, hands.LEFT


def notes_to_midi_bytes(notes: Sequence[Note], hands=None) -> bytes:
    """`hands`: None, or every note's hand in the notes' order (hands.split_hands: 1 right, 0 left, 255 none): a melodic program with a
    note of hand 0 or 1 is written as two tracks on its one channel (_smf_bytes).  Without them the bytes are the same as before."""
    return _smf_bytes(notes, {id(n): (_ticks(n.onset), _ticks(n.offset)) for n in notes}, [(0, TEMPO_US)], hands=hands)


def _smf_bytes(notes: Sequence[Note], ticks: Dict[int, tuple], tempos, conductor_events=(), hands=None) -> bytes:
    """The file of `notes`: ticks[id(note)] = (onset tick, offset tick); `tempos` = [(tick, microseconds per beat)], ascending;
    `conductor_events` = [(tick, the bytes of a meta event)], ascending, merged into the conductor track before the tempo of the same tick.  The
    ticks are keyed by the note objects' identity: everything below, _fit_melodic_channels included, regroups the SAME objects and never
    copies a note (equal notes may carry different ticks, so the notes' values cannot be the key).  `hands`: None, or a hand per note in
    the notes' order, keyed by identity in the same way.  A melodic program with any note of hand 0 or 1 becomes two tracks on its one
    channel, the right hand's and then the left's, each opening with its name (FF 03, "R.H." / "L.H."), the program change in the first
    of them only.  The one-voice-per-(channel, pitch) rule runs over the program's notes together, before they are divided: a span
    belongs to the hand of the note that opened it, a note of hand 255 in such a program goes with the right, a hand without a span
    gets no track."""
    if hands is not None and len(hands) != len(notes):
        raise ValueError(f"{len(notes)} notes but {len(hands)} hands")
    hand_of = {} if hands is None else {id(n): int(h) for n, h in zip(notes, hands)}
    by_prog: Dict[int, List[Note]] = {}
    for n in notes:
        by_prog.setdefault(DRUM_PROGRAM if n.is_drum else n.program, []).append(n)
    conductor, last = bytearray(), 0
    events = [(tick, 1, b"\xff\x51\x03" + int(us).to_bytes(3, "big")) for tick, us in tempos]
    if conductor_events:
        events = sorted(events + [(int(tick), 0, bytes(ev)) for tick, ev in conductor_events], key=lambda e: (e[0], e[1]))   # (stable: the given order at one tick)
    for tick, _, ev in events:
        conductor += _vlq(tick - last) + ev
        last = tick
    tracks = [bytes(conductor) + b"\x00\xff\x2f\x00"]
    by_prog = _fit_melodic_channels(by_prog)
    melodic_channels = [c for c in range(16) if c != 9]
    melodic = [p for p in sorted(by_prog) if p != DRUM_PROGRAM]
    for prog, ns in sorted(by_prog.items()):
        ch = 9 if prog == DRUM_PROGRAM else melodic_channels[melodic.index(prog)]
        ev = []
        # one voice per (channel, pitch): a note still sounding when the same pitch starts again ends at that onset, and a
        # second note starting on the same tick is dropped -- otherwise the note-ons and note-offs of the file do not pair up
        spans: Dict[int, List[List[int]]] = {}
        for n in sorted(ns, key=lambda x: (x.pitch, x.onset, x.offset)):
            on, off = ticks[id(n)][0], max(ticks[id(n)][1], ticks[id(n)][0] + 1)
            sp = spans.setdefault(n.pitch, [])
            if sp and sp[-1][0] == on:
                sp[-1][1] = max(sp[-1][1], off)
                continue
            if sp and sp[-1][1] > on:
                sp[-1][1] = on
            sp.append([on, off, n.velocity, 0 if hand_of.get(id(n)) == 0 else 1])
        split = prog != DRUM_PROGRAM and any(hand_of.get(id(n)) in (0, 1) for n in ns)
        first = True
        for hand, name in HAND_TRACKS if split else ((None, b""),):
            ev = []
            for pitch, sp in spans.items():
                for on, off, vel, h in sp:
                    if hand is None or h == hand:
                        ev.append((on, 1, pitch, vel))
                        ev.append((off, 0, pitch, 0))
            if split and not ev:
                continue
            ev.sort(key=lambda e: (e[0], e[1]))        # offsets before onsets at the same tick
            body = bytearray()
            if split:
                body += b"\x00\xff\x03" + bytes([len(name)]) + name
            if prog != DRUM_PROGRAM and first:
                body += b"\x00" + bytes([0xC0 | ch, gm_program(prog)])
            first = False
            last = 0
            for tick, on, pitch, vel in ev:
                body += _vlq(tick - last) + bytes([(0x90 if on else 0x80) | ch, pitch & 0x7F, vel & 0x7F])
                last = tick
            body += b"\x00\xff\x2f\x00"
            tracks.append(bytes(body))
    out = b"MThd" + struct.pack(">IHHH", 6, 1, len(tracks), TICKS_PER_BEAT)
    for t in tracks:
        out += b"MTrk" + struct.pack(">I", len(t)) + t
    return out


def _marker_events(markers):
    """[(tick, text)] -> conductor events FF 06 (marker), in the given order"""
    out = []
    for tick, text in markers:
        raw = str(text).encode("utf-8")
        if not 0 < len(raw) < 128:
            raise ValueError(f"marker {text!r}: 1 to 127 bytes")
        out.append((int(tick), b"\xff\x06" + bytes([len(raw)]) + raw))
    return out


def notes_to_midi_bytes_on_beats(notes: Sequence[Note], ticks, beats, frames_per_second: float = 100.0, markers=(), hands=None) -> bytes:
    """notes_to_midi_bytes with a tempo map: `ticks` (n, 2), every note's onset and offset tick at 480 per beat (beats.beat_positions or
    BeatTracker.positions, in the notes' order), `beats` the beats' frames at `frames_per_second`.  The tempo track starts with the first
    interval's tempo at tick 0 and sets interval i's, rint((b[i+1] - b[i]) / fps 1e6) microseconds per beat, at tick (n0 + i) 480
    (beats.tempo_map); played back, the file keeps the performance's timing, after a lead-in of beats.lead_sec.  A note without ticks
    (-1: a NaN time) is left out.  With fewer than two beats there is no map: the bytes are notes_to_midi_bytes'.  `markers` = [(tick,
    text)], ascending (chords.chord_markers: a chord symbol at its first beat), go into the conductor track as FF 06 events; without
    them the bytes are the same as before.  `hands` as notes_to_midi_bytes takes them."""
    from .beats import tempo_map
    notes = list(notes)
    tempos = tempo_map(beats, frames_per_second)
    if not tempos:
        return notes_to_midi_bytes(notes, hands)
    pairs = [(int(a), int(b)) for a, b in ticks]
    if len(pairs) != len(notes):
        raise ValueError(f"{len(notes)} notes but {len(pairs)} tick pairs")
    kept, kept_hands = _with_ticks(notes, pairs, hands)
    return _smf_bytes([n for n, _ in kept], {id(n): t for n, t in kept}, tempos, _marker_events(markers), kept_hands)


def _with_ticks(notes, pairs, hands):
    """the notes that have ticks with them, and those notes' hands (None without hands)"""
    if hands is not None and len(hands) != len(notes):
        raise ValueError(f"{len(notes)} notes but {len(hands)} hands")
    keep = [t[0] >= 0 and (t[1] >= 0 or n.is_drum) for n, t in zip(notes, pairs)]
    kept = [(n, t) for n, t, k in zip(notes, pairs, keep) if k]
    return kept, None if hands is None else [h for h, k in zip(hands, keep) if k]


def notes_to_midi_bytes_on_bars(notes: Sequence[Note], ticks, beats, metre, key: int = -1, frames_per_second: float = 100.0, markers=(), hands=None) -> bytes:
    """notes_to_midi_bytes_on_beats with bar lines and a key: `metre` (256 m + k of every beat) and `key` as bars.track_bars or
    BarTracker give them.  The conductor track gains one FF 58 04 nn 02 18 08 (nn/4) per entry of bars.time_signatures and one
    FF 59 02 sf mi at tick 0 (bars.key_signature; none for key -1), in tick order with the tempo events.  Without downbeats (fewer
    than two beats among them) the bytes are exactly notes_to_midi_bytes_on_beats'.  `markers` as there: at one tick after the time and
    key signatures and before the tempo.  `hands` as notes_to_midi_bytes takes them."""
    from .bars import key_signature, time_signatures
    from .beats import tempo_map
    notes = list(notes)
    signatures = time_signatures(metre, beats)
    tempos = tempo_map(beats, frames_per_second)
    if not signatures or not tempos:
        return notes_to_midi_bytes_on_beats(notes, ticks, beats, frames_per_second, markers, hands)
    pairs = [(int(a), int(b)) for a, b in ticks]
    if len(pairs) != len(notes):
        raise ValueError(f"{len(notes)} notes but {len(pairs)} tick pairs")
    kept, kept_hands = _with_ticks(notes, pairs, hands)
    events = [(tick, b"\xff\x58\x04" + bytes([nn, 2, 24, 8])) for tick, nn in signatures]
    if int(key) >= 0:
        sf, mi = key_signature(key)
        events.insert(1 if events[0][0] == 0 else 0, (0, b"\xff\x59\x02" + bytes([sf & 0xFF, mi])))
    return _smf_bytes([n for n, _ in kept], {id(n): t for n, t in kept}, tempos, events + _marker_events(markers), kept_hands)


def write_midi(notes: Sequence[Note], path: str) -> str:
    with open(path, "wb") as f:
        f.write(notes_to_midi_bytes(notes))
    return path


def read_midi_notes(data: bytes) -> List[Note]:
    """Parse what notes_to_midi_bytes writes (round-trip tests): note on/off + program change only."""
    assert data[:4] == b"MThd"
    _, fmt, ntrk, tpb = struct.unpack(">IHHH", data[4:14])
    pos, notes = 14, []
    sec = lambda t: t * TEMPO_US / (tpb * 1e6)
    progs: Dict[int, int] = {}                          # by channel: a split program's second track has no program change of its own
    for _ in range(ntrk):
        assert data[pos:pos + 4] == b"MTrk"
        ln = struct.unpack(">I", data[pos + 4:pos + 8])[0]
        p, end, tick, open_ = pos + 8, pos + 8 + ln, 0, {}
        while p < end:
            d = 0
            while True:
                b = data[p]; p += 1
                d = (d << 7) | (b & 0x7F)
                if not b & 0x80:
                    break
            tick += d
            st = data[p]; p += 1
            if st == 0xFF:
                ml = data[p + 1]; p += 2 + ml
            elif st & 0xF0 == 0xC0:
                progs[st & 0x0F] = data[p]; p += 1
            elif st & 0xF0 in (0x90, 0x80):
                pitch, vel = data[p], data[p + 1]; p += 2
                drum = (st & 0x0F) == 9
                if st & 0xF0 == 0x90 and vel > 0:
                    open_[pitch] = (tick, vel)
                elif pitch in open_:
                    on, v = open_.pop(pitch)
                    notes.append(Note(sec(on), sec(tick), drum, DRUM_PROGRAM if drum else progs.get(st & 0x0F, 0), pitch, v))
        pos = end
    return sorted(notes)


def _track_events(data: bytes):
    """The events of a Standard MIDI File as notes_to_midi_bytes and notes_to_midi_bytes_on_beats write it -> (ticks per beat, an
    iterator of (track, absolute tick, status byte, payload bytes)); a meta event's payload starts with its type byte."""
    assert data[:4] == b"MThd"
    _, fmt, ntrk, tpb = struct.unpack(">IHHH", data[4:14])

    def events():
        pos = 14
        for track in range(ntrk):
            assert data[pos:pos + 4] == b"MTrk"
            ln = struct.unpack(">I", data[pos + 4:pos + 8])[0]
            p, end, tick = pos + 8, pos + 8 + ln, 0
            while p < end:
                d = 0
                while True:
                    b = data[p]; p += 1
                    d = (d << 7) | (b & 0x7F)
                    if not b & 0x80:
                        break
                tick += d
                st = data[p]; p += 1
                if st == 0xFF:
                    n = 2 + data[p + 1]
                    payload = data[p:p + 1] + data[p + 2:p + n]
                else:
                    n = 1 if st & 0xF0 == 0xC0 else 2
                    payload = data[p:p + n]
                p += n
                yield track, tick, st, payload
            pos = end

    return tpb, events()


def note_on_ticks(data: bytes) -> List[int]:
    """the absolute tick of every note-on of a file, track by track"""
    return [tick for _, tick, st, payload in _track_events(data)[1] if st & 0xF0 == 0x90 and payload[1] > 0]


def read_midi_on_beats(data: bytes):
    """Parse what notes_to_midi_bytes_on_beats writes -> (notes in seconds through the file's tempo map, the map as [(tick, microseconds
    per beat)]).  A file without tempo events plays at 120 bpm."""
    tpb, events = _track_events(data)
    raw, tempos, prog, open_ = [], [], {}, {}
    for track, tick, st, payload in events:
        if st == 0xFF:
            if payload[0] == 0x51:
                tempos.append((tick, int.from_bytes(payload[1:], "big")))
        elif st & 0xF0 == 0xC0:
            prog[st & 0x0F] = payload[0]                # by channel: a split program's second track has no program change of its own
        elif st & 0xF0 in (0x90, 0x80):
            pitch, vel = payload[0], payload[1]
            drum = (st & 0x0F) == 9
            if st & 0xF0 == 0x90 and vel > 0:
                open_[track, pitch] = (tick, vel)
            elif (track, pitch) in open_:
                on, v = open_.pop((track, pitch))
                raw.append((on, tick, drum, DRUM_PROGRAM if drum else prog.get(st & 0x0F, 0), pitch, v))
    tempos = sorted(tempos) or [(0, TEMPO_US)]
    if tempos[0][0] != 0:
        tempos.insert(0, (0, TEMPO_US))
    starts, t = [], 0.0                                 # the time at which every tempo event takes hold
    for i, (tk, us) in enumerate(tempos):
        if i:
            t += (tk - tempos[i - 1][0]) * tempos[i - 1][1] / (tpb * 1e6)
        starts.append(t)

    at = [tk for tk, _ in tempos]

    def sec(tick):
        i = bisect.bisect_right(at, tick) - 1
        return starts[i] + (tick - at[i]) * tempos[i][1] / (tpb * 1e6)

    return sorted(Note(sec(on), sec(off), drum, prog, pitch, v) for on, off, drum, prog, pitch, v in raw), tempos


def read_midi_on_bars(data: bytes):
    """Parse what notes_to_midi_bytes_on_bars writes -> (notes, tempo map) as read_midi_on_beats, then the time signatures as [(tick,
    numerator)] (denominator 4 is asserted) and the key signature as (sf, mi), or None if the file has none."""
    notes, tempos = read_midi_on_beats(data)
    signatures, key = [], None
    for _, tick, st, payload in _track_events(data)[1]:
        if st == 0xFF and payload[0] == 0x58:
            assert payload[2] == 2, "a denominator other than 4"
            signatures.append((tick, payload[1]))
        elif st == 0xFF and payload[0] == 0x59:
            key = (payload[1] - 256 if payload[1] > 127 else payload[1], payload[2])
    return notes, tempos, signatures, key


def read_midi_markers(data: bytes):
    """the markers (FF 06) of a file, as the writers on the beats and on the bars write them -> [(tick, text)]"""
    return [(tick, bytes(payload[1:]).decode("utf-8")) for _, tick, st, payload in _track_events(data)[1] if st == 0xFF and payload[0] == 0x06]


def read_midi_track_names(data: bytes) -> List[str]:
    """the track names (FF 03) of a file, track by track"""
    return [bytes(payload[1:]).decode("utf-8") for _, _, st, payload in _track_events(data)[1] if st == 0xFF and payload[0] == 0x03]


def read_midi_open_notes(data: bytes) -> List[int]:
    """per track, the note-ons and note-offs that do not pair up inside it: a note-on of a pitch that is sounding, a note-off of one that
    is not, and what still sounds at the track's end.  All zero in a file of this module's writers."""
    tpb, events = _track_events(data)
    bad: Dict[int, int] = {}
    sounding: Dict[int, set] = {}
    for track, _, st, payload in events:
        bad.setdefault(track, 0)
        if st & 0xF0 in (0x90, 0x80):
            on = st & 0xF0 == 0x90 and payload[1] > 0
            held = sounding.setdefault(track, set())
            if on == (payload[0] in held):
                bad[track] += 1
            (held.add if on else held.discard)(payload[0])
    return [bad[t] + len(sounding.get(t, ())) for t in sorted(bad)]


def read_midi_hands(data: bytes):
    """Parse what notes_to_midi_bytes writes with `hands` -> [(note, hand)], sorted: the notes as read_midi_notes reads them, hand 1 for a
    track named "R.H.", 0 for "L.H.", 255 for any other track."""
    names = {name.decode(): hand for hand, name in HAND_TRACKS}
    tpb, events = _track_events(data)
    sec = lambda t: t * TEMPO_US / (tpb * 1e6)
    out, progs, hand, open_ = [], {}, {}, {}
    for track, tick, st, payload in events:
        if st == 0xFF:
            if payload[0] == 0x03:
                hand[track] = names.get(bytes(payload[1:]).decode("utf-8"), 255)
        elif st & 0xF0 == 0xC0:
            progs[st & 0x0F] = payload[0]
        elif st & 0xF0 in (0x90, 0x80):
            pitch, vel = payload[0], payload[1]
            drum = (st & 0x0F) == 9
            if st & 0xF0 == 0x90 and vel > 0:
                open_[track, pitch] = (tick, vel)
            elif (track, pitch) in open_:
                on, v = open_.pop((track, pitch))
                out.append((Note(sec(on), sec(tick), drum, DRUM_PROGRAM if drum else progs.get(st & 0x0F, 0), pitch, v), hand.get(track, 255)))
    return sorted(out)
