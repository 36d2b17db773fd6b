"""Tokeniser, the parts that need no GPU (include/ymt3.h, device tokeniser):
  1. TaskManager.notes_to_tokens, the specification: the round trip tokens_to_notes(notes_to_tokens(notes)) == sorted(notes) under its stated
     preconditions, rows that the segment grammar accepts, rows equal to encode_segment on hand-written cases, the overflow and start-time errors;
  2. tests/tok_model.py -- the kernels' algorithm in plain Python -- equals the host path on the cases of tests/tok_cases.py;
  3. the C ABI: the three entry points are declared, listed and exported, the ABI version is still 3."""
import os
import re

import numpy as np
import pytest

import tok_cases as C
import tok_model as M
from yourmt3_amd.task_manager import DRUM_PROGRAM, Note, NoteEvent, TaskManager
from yourmt3_amd.vocab import EOS, PAD, Event

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"zero_notes", "one_note", "spans_all_segments", "offset_on_segment_start", "onset_and_offset_in_one_step", "touches_its_successor",
         "duplicate_notes_and_ties", "drums_at_equal_times", "programs_128_and_129", "programs_96_to_127", "gap_longer_than_max_shift",
         "row_of_exactly_L"}


def test_every_listed_case_is_present_for_both_channel_counts():
    for K in (1, 13):
        assert {c["name"] for c in C.special_cases() if c["task"] == C.TASK_OF_K[K]} == NAMES


@pytest.mark.parametrize("case", C.grid_cases(), ids=lambda c: c["id"])
def test_round_trip_gives_the_notes_back(case):
    tm = C.task_manager(case["task"], case["ms"])
    tokens, lengths = C.reference(case)
    back = tm.tokens_to_notes([tokens], case["starts"], case["end_sec"])
    assert back == sorted(case["notes"])
    assert [(n.onset, n.offset) for n in back] == [(n.onset, n.offset) for n in sorted(case["notes"])]         # f64 times, bit for bit
    again, lengths2 = tm.notes_to_tokens(back, case["starts"], case["end_sec"], max_len=case["L"])              # tokens -> notes -> tokens
    assert np.array_equal(again, tokens) and np.array_equal(lengths2, lengths)


ROUND_TRIP_SPECIALS = {"zero_notes", "one_note", "spans_all_segments", "offset_on_segment_start", "touches_its_successor",
                       "gap_longer_than_max_shift", "row_of_exactly_L"}


@pytest.mark.parametrize("case", [c for c in C.special_cases() if c["name"] in ROUND_TRIP_SPECIALS], ids=lambda c: c["id"])
def test_special_cases_inside_the_preconditions_round_trip(case):
    tm = C.task_manager(case["task"], case["ms"])
    tokens, _ = C.reference(case)
    want = sorted(Note(n.onset, min(n.offset, case["end_sec"]), n.is_drum, n.program, n.pitch) for n in case["notes"])
    assert tm.tokens_to_notes([tokens], case["starts"], case["end_sec"]) == want


@pytest.mark.parametrize("case", list(C.special_cases()) + list(C.grid_cases()), ids=lambda c: c["id"])
def test_rows_are_accepted_by_the_segment_grammar(case):
    """Every row walks event_automaton() from its channel's start state through allowed tokens and ends where EOS is allowed.  The one
    exception is stated, not skipped over: with 13 channels programs 96-127 fall to channel 0 (channel_of_program), whose automaton admits
    the piano group only, so those rows are checked against the grammar of all programs instead."""
    tm = C.task_manager(case["task"], case["ms"])
    tokens, lengths = C.reference(case)
    aut, start = tm.event_automaton()
    if case["name"] == "programs_96_to_127" and tm.num_decoding_channels == 13:
        one = TaskManager("mt3_full_plus", max_shift_steps=case["ms"])
        aut, start = one.event_automaton()
        start = np.repeat(start, 13)
    for s in range(tokens.shape[0]):
        for ch in range(tokens.shape[1]):
            state, ln = int(start[ch]), int(lengths[s, ch])
            row = tokens[s, ch]
            assert row[ln - 1] == EOS and (row[ln:] == PAD).all() and EOS not in row[:ln - 1]
            for tk in row[:ln]:
                assert aut.allowed[state, tk], (case["id"], s, ch, int(tk))
                state = int(aut.next[state, tk])


def test_literal_example():
    """Two segments of 0.5 s.  A piano note from 0.10 s over the boundary to 0.62 s, a drum hit at 0.10 s, a short guitar note."""
    tm = TaskManager("mt3_full_plus")
    enc = lambda t, v: tm.codec.encode(Event(t, v))
    notes = [Note(0.10, 0.62, False, 0, 60), Note(0.10, 0.11, True, DRUM_PROGRAM, 36), Note(0.30, 0.30, False, 24, 50)]
    tokens, lengths = tm.notes_to_tokens(notes, [0.0, 0.5], 1.0, max_len=16)
    row0 = [enc("tie", 0), enc("shift", 10), enc("velocity", 1), enc("program", 0), enc("pitch", 60), enc("drum", 36),
            enc("shift", 20), enc("program", 24), enc("pitch", 50), enc("shift", 1), enc("velocity", 0), enc("pitch", 50), EOS]
    row1 = [enc("program", 0), enc("pitch", 60), enc("tie", 0), enc("shift", 12), enc("velocity", 0), enc("program", 0), enc("pitch", 60), EOS]
    assert tokens[0, 0].tolist() == row0 + [PAD] * 3 and tokens[1, 0].tolist() == row1 + [PAD] * 8
    assert lengths.tolist() == [[13], [8]]
    assert (tokens.dtype, lengths.dtype) == (np.int32, np.int32)


def test_rows_equal_encode_segment_on_hand_written_events():
    tm = TaskManager("mc13_full_plus_256", max_shift_steps=7)
    starts = [1.0, 1.5, 2.25]
    notes = [Note(1.2, 2.3, False, 33, 40), Note(1.2, 2.3, False, 33, 40), Note(1.49, 1.5, False, 0, 70), Note(2.25, 9.0, False, 0, 71),
             Note(0.99, 1.2, False, 0, 1), Note(2.6, 2.7, False, 0, 2), Note(2.3, 2.3, True, 5, 38)]
    tokens, lengths = tm.notes_to_tokens(notes, starts, 2.6, max_len=32)
    ev = lambda s, step, drum, prog, vel, pitch: NoteEvent(starts[s] + step / 100, drum, prog, vel, pitch)
    want = {(0, 4): ([ev(0, 20, False, 33, 1, 40)] * 2, []), (1, 4): ([], [(33, 40)]), (2, 4): ([ev(2, 5, False, 33, 0, 40)] * 2, [(33, 40)]),
            (0, 0): ([ev(0, 49, False, 0, 1, 70)], []), (2, 0): ([ev(2, 0, False, 0, 1, 71)], []), (2, 12): ([ev(2, 5, True, DRUM_PROGRAM, 1, 38)], [])}
    for s in range(3):
        for ch in range(13):
            events, ties = want.get((s, ch), ([], []))
            row = tm.tokenizer.encode_segment(events, ties, starts[s], max_len=32)
            assert tokens[s, ch].tolist() == row, (s, ch)
            assert lengths[s, ch] == row.index(EOS) + 1
    assert tokens[1, 3].tolist() == [tm.codec.encode(Event("tie", 0)), EOS] + [PAD] * 30


@pytest.mark.parametrize("K", [1, 13])
def test_overflow_fires_at_exactly_one_token_more_than_fits(K):
    case = next(c for c in C.special_cases() if c["name"] == "row_of_exactly_L" and c["task"] == C.TASK_OF_K[K])
    tm = C.task_manager(case["task"], case["ms"])
    tokens, lengths = C.reference(case)
    assert int(lengths.max()) == case["L"] == 8 and tokens[0, 0, -1] == EOS
    more = list(case["notes"]) + [Note(0.05, 9.0, False, 0, 65)]
    with pytest.raises(ValueError, match=r"segment 0 channel 0 needs 9 tokens > 8"):
        tm.notes_to_tokens(more, case["starts"], case["end_sec"], max_len=8)
    assert int(tm.notes_to_tokens(more, case["starts"], case["end_sec"], max_len=9)[1].max()) == 9


def test_non_increasing_start_times_are_refused():
    tm = TaskManager("mt3_full_plus")
    for starts in ([0.0, 2.0, 2.0], [0.0, 3.0, 1.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            tm.notes_to_tokens([], starts, 9.0)


def test_default_length_and_empty_inputs():
    tm = TaskManager("mc13_full_plus_256")
    tokens, lengths = tm.notes_to_tokens([], [0.0, 1.0], 2.0)
    assert tokens.shape == (2, 13, 256) and (lengths == 2).all() and (tokens[:, :, 1] == EOS).all()
    tokens, lengths = tm.notes_to_tokens([Note(0.0, 1.0, False, 0, 60)], [], 2.0)
    assert tokens.shape == (0, 13, 256) and lengths.shape == (0, 13)


MODEL_CASES = list(C.special_cases()) + list(C.grid_cases()) + [C.matrix_case(n, K, L, ms) for (n, K, L, ms) in C.MATRIX if L <= 256]


@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: c["id"])
def test_model_equals_host_path(case):
    tm = C.task_manager(case["task"], case["ms"])
    tokens, lengths = C.reference(case)
    p, chan = tm.tok_params()
    got, got_len = M.tokenize(p, chan, M.records_of(case["notes"]), case["starts"], case["end_sec"], tm.num_decoding_channels, case["L"])
    assert np.array_equal(got_len, lengths)
    assert np.array_equal(got, tokens)


def test_model_reports_overflow_and_counts_a_tie_once():
    tm = TaskManager("mt3_full_plus")
    p, chan = tm.tok_params()
    # 40 copies of one note over the boundary: 40 onset items overflow L = 16 in segment 0, one tie item in segment 1
    notes = [Note(0.1, 0.9, False, 0, 60)] * 40
    _, ln = M.tokenize(p, chan, M.records_of(notes), [0.0, 0.5], 1.0, 1, 16)
    assert ln[0, 0] > 16
    with pytest.raises(ValueError, match="segment 0 channel 0"):
        tm.notes_to_tokens(notes, [0.0, 0.5], 1.0, max_len=16)
    # with room for them: segment 1 lists the tie once (2 ids), then TIE, one shift, velocity 0, the program, 40 offsets, EOS
    tokens, lengths = tm.notes_to_tokens(notes, [0.0, 0.5], 1.0, max_len=64)
    got, got_len = M.tokenize(p, chan, M.records_of(notes), [0.0, 0.5], 1.0, 1, 64)
    assert np.array_equal(got, tokens) and np.array_equal(got_len, lengths) and lengths[1, 0] == 2 + 1 + 3 + 40 + 1
    # a gap of more shift tokens than the row has columns: the length is a lower bound, still > L
    far = [Note(0.0, 0.01, False, 0, 60), Note(400.0, 400.01, False, 0, 61)]
    tm7 = TaskManager("mt3_full_plus", max_shift_steps=7)
    p7, chan7 = tm7.tok_params()
    _, ln = M.tokenize(p7, chan7, M.records_of(far), [0.0], 500.0, 1, 32)
    assert ln[0, 0] > 32


def test_entry_points_declared_listed_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    lib = _lib.load()
    for name in ("ymt3_tok_create", "ymt3_tok_destroy", "ymt3_tokenize"):
        assert re.search(r"\b" + name + r"\s*\(ymt3_", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct ymt3_tok_s* ymt3_tok;" in header and "} ymt3_tok_params;" in header
    assert lib.ymt3_abi_version() == 3 and "#define YMT3_ABI_VERSION 3" in header
    body = header[header.index("typedef struct ymt3_tok_params {"):header.index("} ymt3_tok_params;")]
    assert re.findall(r"\b([a-z_]+)(?=[,;])", body) == [n for n, _ in _lib.TokParams._fields_]
