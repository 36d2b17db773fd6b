"""The note side's shared pieces on the GPU (yourmt3_amd/csrc/note_rule.h, note_objects.hip).

  1. One table of records, one per edge of the rule for which record counts and which frames it covers, through every consumer of the
     rule: ymt3_note_metrics, ymt3_frame_metrics, ymt3_piano_roll and ymt3_align_notes each equal their host specification
     (yourmt3_amd/metrics.py) exactly, under count tensors of 0, a negative value, a value inside the array and one above n; the three
     skipped-record counts of a side are equal and are what metrics.classify says.
  2. One table of refusals over the six note-side objects: a NULL object, an object of a second handle, a record pointer 4 bytes off, a
     count one above the object's maximum.  Every refusal is error code 1 with its exact text, and the same object's next valid call gives
     the right answer.
  3. YourMT3.close() closes every object the model created."""
import ctypes

import numpy as np
import pytest
import torch

import detok_cases as DC
import roll_cases as RC
import tok_cases as TC
from test_gpu_parity import _model
from test_roll import CFG, _dev
from yourmt3_amd.metrics import classify, dtw_align, frame_metrics, note_metrics, piano_roll, warp_notes
from yourmt3_amd.task_manager import NOTE_RECORD, Note

pytestmark = pytest.mark.gpu

NAN, INF = RC.NAN, RC.INF
P = dict(n_programs=3, drum_program=1)
N_FRAMES, FPS = 65, 100.0                 # one past the wave's 64-frame stride: the raster loop runs twice for a long note
# (onset, offset, program, pitch, is_drum), and whether the record counts
REF = [((NAN, 0.5, 0, 60, False), 0),                 # NaN onset
       ((0.1, NAN, 0, 60, False), 0),                 # NaN offset on a pitched note
       ((0.1, NAN, 1, 36, True), 1),                  # NaN offset on a drum
       ((0.1, 0.5, 0, -1, False), 0), ((0.1, 0.5, 0, 128, False), 0),       # pitch -1 and 128
       ((0.1, 0.5, -1, 60, False), 0), ((0.1, 0.5, 3, 60, False), 0),       # program -1 and n_programs
       ((0.2, 0.9, 7, 38, True), 1), ((0.3, NAN, -3, 42, True), 1),         # is_drum with an out-of-range program: the drum
       ((-INF, 0.10, 0, 61, False), 1), ((INF, INF, 0, 62, False), 1), ((1e300, 2e300, 0, 68, False), 1),
       ((0.30, 0.10, 0, 64, False), 1),               # an offset before the onset: one frame
       ((0.005, 0.30, 0, 65, False), 1), ((0.015, 0.30, 0, 66, False), 1),  # .5 frames: 0.5 -> 0, 1.5 -> 2
       ((-0.004, 0.05, 0, 63, False), 1), ((-0.006, 0.05, 2, 63, False), 1),   # slightly below 0: frame -0, and frame -1 clipped
       ((0.60, 0.70, 2, 31, False), 1),               # ends beyond n_frames
       ((0.0, 0.65, 0, 0, False), 1),                 # every frame: more than one pass of the wave
       ((0.20, 0.40, 2, 127, False), 1), ((0.21, 0.22, 1, 36, True), 1)]
EST = [((0.0, 0.66, 0, 0, False), 1), ((0.1, NAN, 1, 36, True), 1), ((NAN, NAN, 1, 36, True), 0), ((0.1, 0.5, 0, 128, False), 0),
       ((0.21, 0.41, 2, 127, False), 1), ((0.2, 0.3, 999, 38, True), 1), ((0.1, 0.2, 1, 128, True), 0), ((0.1, NAN, 2, 60, False), 0),
       ((-INF, 0.12, 0, 61, False), 1), ((0.62, INF, 2, 31, False), 1), ((+INF, 0.1, 0, 62, False), 1), ((-1e300, 1e300, 0, 69, False), 1),
       ((0.31, 0.10, 0, 64, False), 1), ((0.015, 0.29, 0, 65, False), 1), ((0.005, 0.31, 0, 66, False), 1), ((-0.004, 0.05, 2, 63, False), 1),
       ((0.1, 0.5, -1, 60, False), 0), ((0.1, 0.5, 3, 60, False), 0), ((0.64, 0.65, 0, 1, False), 1), ((0.65, 0.66, 0, 2, False), 1)]


@pytest.fixture(scope="module")
def rig():
    """the model of the roll tests, and one object per consumer of the rule"""
    m = _model(CFG, max_batch=2)
    objs = dict(nm=m.compile_note_metrics(P["n_programs"], 64, 64, drum_program=P["drum_program"]),
                pr=m.compile_piano_roll(P["n_programs"], N_FRAMES, FPS, P["drum_program"]),
                al=m.compile_aligner(P["n_programs"], N_FRAMES, FPS, N_FRAMES, P["drum_program"]))
    yield m, objs
    m.close()


def test_the_table_has_every_edge_and_counts_as_written():
    for rows in (REF, EST):
        rec = RC.records([r for r, _ in rows])
        assert classify(rec, **P)[0].tolist() == [bool(c) for _, c in rows]
    assert 0 < sum(c for _, c in REF) < len(REF)


def test_one_record_table_through_every_consumer(rig):
    m, o = rig
    ref, est = RC.records([r for r, _ in REF]), RC.records([r for r, _ in EST])
    n_r, n_e = ref.size, est.size
    rd, ed = _dev(ref), _dev(est)
    count = lambda v: None if v is None else torch.tensor([v, 12345], dtype=torch.int32).cuda()
    seen = set()
    # no count tensors; then 0, a negative value, a value inside the array and one above n, on either side
    for cr, ce in ((None, None), (0, 7), (-3, n_e), (9, n_e + 5), (n_r + 9, 0), (n_r, -1), (14, 11)):
        hr = ref[:n_r if cr is None else min(max(cr, 0), n_r)]
        he = est[:n_e if ce is None else min(max(ce, 0), n_e)]
        skipped = [int(r.size - classify(r, **P)[0].sum()) for r in (hr, he)]
        seen.add(tuple(skipped))
        notes = o["nm"].run(rd, ed, count(cr), count(ce)).cpu().numpy()
        frames = o["pr"].metrics(rd, ed, N_FRAMES, count(cr), count(ce)).cpu().numpy()
        rolls = [o["pr"].roll(d, N_FRAMES, count(c)).cpu().numpy() for d, c in ((rd, cr), (ed, ce))]
        warp, result, path = (t.cpu().numpy() for t in o["al"].align(rd, ed, N_FRAMES, N_FRAMES, count(cr), count(ce), path=True))
        print(f"counts {cr}, {ce}: {hr.size} and {he.size} records, skipped {skipped}; device {notes[-2:].tolist()} {frames[-2:].tolist()} {result[2:].tolist()}")
        assert np.array_equal(notes, note_metrics(hr, he, **P).flat()), (cr, ce)
        assert np.array_equal(frames, frame_metrics(hr, he, N_FRAMES, frames_per_second=FPS, **P).flat()), (cr, ce)
        for got, h in zip(rolls, (hr, he)):
            assert np.array_equal(got, piano_roll(h, N_FRAMES, frames_per_second=FPS, **P)), (cr, ce)
        want = dtw_align(hr, he, N_FRAMES, N_FRAMES, frames_per_second=FPS, band_frames=N_FRAMES, **P)
        assert result.tolist() == [want.total, want.path_len] + want.skipped.tolist() and np.array_equal(warp, want.warp), (cr, ce)
        assert np.array_equal(path[:want.path_len], want.path), (cr, ce)
        assert notes[-2:].tolist() == frames[-2:].tolist() == result[2:].tolist() == skipped, (cr, ce)
    assert len(seen) > 3                                                  # the counts moved the skipped records


# ---------------------------------------------------------------------------------------------- refusals
MAX_NOTES = 1 << 29                       # ROLL_MAX_NOTES and TOK_MAX_NOTES of csrc/kernels.h
# (entry point, what is wrong, the text of ymt3_last_error): every one is YMT3_ERR_ARG
REFUSALS = [
    ("detokenize", dict(obj=None), "null detokeniser"),
    ("detokenize", dict(obj="foreign"), "the detokeniser belongs to another handle"),
    ("detokenize", dict(n=2), "n_segments=2 outside [0, max_segments=1]"),
    ("state_reset", dict(obj=None), "null detokeniser state"),
    ("state_reset", dict(obj="foreign"), "the detokeniser state belongs to another handle"),
    ("push", dict(obj=None), "null detokeniser state"),
    ("push", dict(obj="foreign"), "the detokeniser state was created for another detokeniser"),
    ("push", dict(n=2), "n_segments=2 outside [0, max_segments=1]"),
    ("tokenize", dict(obj=None), "null tokeniser"),
    ("tokenize", dict(obj="foreign"), "the tokeniser belongs to another handle"),
    ("tokenize", dict(notes="+4"), "notes_dev is not aligned to 8 bytes"),
    ("tokenize", dict(n_notes=MAX_NOTES + 1), "n_notes=536870913 outside [0, 536870912]"),
    ("tokenize", dict(n=2), "n_segments=2 outside [0, max_segments=1]"),
    ("note_metrics", dict(obj=None), "null metrics object"),
    ("note_metrics", dict(obj="foreign"), "the metrics object belongs to another handle"),
    ("note_metrics", dict(ref="+4"), "ref_notes_dev is not aligned to 8 bytes"),
    ("note_metrics", dict(est="+4"), "est_notes_dev is not aligned to 8 bytes"),
    ("note_metrics", dict(n_ref=5), "n_ref=5 outside [0, max_ref=4]"),
    ("note_metrics", dict(n_est=5), "n_est=5 outside [0, max_est=4]"),
    ("frame_metrics", dict(obj=None), "null roll object"),
    ("frame_metrics", dict(obj="foreign"), "the roll object belongs to another handle"),
    ("frame_metrics", dict(ref="+4"), "ref_notes_dev is not aligned to 8 bytes"),
    ("frame_metrics", dict(est="+4"), "est_notes_dev is not aligned to 8 bytes"),
    ("frame_metrics", dict(n_frames=9), "n_frames=9 outside [0, max_frames=8]"),
    ("frame_metrics", dict(n_est=MAX_NOTES + 1), "n_est=536870913 outside [0, 536870912]"),
    ("piano_roll", dict(obj=None), "null roll object"),
    ("piano_roll", dict(obj="foreign"), "the roll object belongs to another handle"),
    ("piano_roll", dict(ref="+4"), "notes_dev is not aligned to 8 bytes"),
    ("piano_roll", dict(n_frames=9), "n_frames=9 outside [0, max_frames=8]"),
    ("piano_roll", dict(n_ref=MAX_NOTES + 1), "n_notes=536870913 outside [0, 536870912]"),
    ("align_notes", dict(obj=None), "null aligner object"),
    ("align_notes", dict(obj="foreign"), "the aligner object belongs to another handle"),
    ("align_notes", dict(ref="+4"), "ref_notes_dev is not aligned to 8 bytes"),
    ("align_notes", dict(est="+4"), "est_notes_dev is not aligned to 8 bytes"),
    ("align_notes", dict(n_frames=9), "n_ref_frames=9 outside [1, max_frames=8]"),
    ("align_notes", dict(n_ref=MAX_NOTES + 1), "n_ref=536870913 outside [0, 536870912]"),
    ("warp_notes", dict(obj=None), "null aligner object"),
    ("warp_notes", dict(obj="foreign"), "the aligner object belongs to another handle"),
    ("warp_notes", dict(ref="+4"), "notes_dev is not aligned to 8 bytes"),
    ("warp_notes", dict(out="+4"), "notes_out_dev is not aligned to 8 bytes"),
    ("warp_notes", dict(n_frames=9), "n_ref_frames=9 outside [1, max_frames=8]"),
    ("warp_notes", dict(n_ref=MAX_NOTES + 1), "n_notes=536870913 outside [0, 536870912]"),
]
OBJECT_OF = dict(detokenize="detok", state_reset="state", push="state", tokenize="tok", note_metrics="nm", frame_metrics="pr", piano_roll="pr",
                 align_notes="al", warp_notes="al")
F, L = 8, 8                               # max_frames and max_steps; max_ref = max_est = 4, max_segments = 1
NOTES = [Note(0.0, 9.0, False, 0, 60), Note(0.05, 9.0, False, 0, 62), Note(0.05, 9.0, False, 0, 64)]       # a row of exactly L = 8 tokens (tests/tok_cases.py)
SMALL_REF = [(0.00, 0.05, 0, 60, False), (0.02, 0.06, 2, 62, False), (0.03, NAN, 1, 36, True), (NAN, 0.1, 0, 60, False)]
SMALL_EST = [(0.01, 0.05, 0, 60, False), (0.02, 0.08, 2, 63, False), (0.03, 0.04, 7, 36, True)]


@pytest.fixture(scope="module")
def six():
    """two handles with the six objects each, at the smallest sizes, and the inputs of one valid call per entry point"""
    tm = TC.task_manager("mt3_full_plus")
    models = [_model(CFG, max_batch=2), _model(CFG, max_batch=1)]
    sets = []
    for m in models:
        detok = m.compile_detokenizer(tm, 1, L)
        sets.append(dict(detok=detok, state=detok.new_state(4), tok=m.compile_tokenizer(tm, 1, L),
                         nm=m.compile_note_metrics(P["n_programs"], 4, 4, drum_program=P["drum_program"]),
                         pr=m.compile_piano_roll(P["n_programs"], F, FPS, P["drum_program"]),
                         al=m.compile_aligner(P["n_programs"], F, FPS, F, P["drum_program"])))
    yield tm, models[0], sets[0], sets[1]
    for m in models:
        m.close()


def _calls(tm, m, own, foreign):
    """-> {entry point: call(**what is wrong) -> error code}, {object: check()}: the raw C calls and the objects' valid calls"""
    lib, h, stream = m._lib, m._handle, m._stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ref, est = RC.records(SMALL_REF), RC.records(SMALL_EST)
    # (views: the bytes around a pointer that is 4 off exist)
    rd, ed = (torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _dev(r)])[16:] for r in (ref, est))
    out = rd.clone()
    tokens_host, _ = tm.notes_to_tokens(NOTES, [0.0], 0.4, max_len=L)
    tokens = torch.from_numpy(np.concatenate([tokens_host, tokens_host])).cuda()              # (room for the refused n_segments = 2)
    starts = torch.tensor([0.0, 0.5], dtype=torch.float64).cuda()
    records = torch.empty(64 * NOTE_RECORD.itemsize, dtype=torch.uint8).cuda()
    counts32, counts64 = torch.zeros(64, dtype=torch.int32).cuda(), torch.zeros(64, dtype=torch.int64).cuda()
    toks, lengths = torch.empty(2, 1, L, dtype=torch.int32).cuda(), torch.empty(2, 1, dtype=torch.int32).cuda()
    roll = torch.empty(4 * F * 128, dtype=torch.uint8).cuda()
    warp = torch.zeros(F, dtype=torch.int32).cuda()

    def arg(a, name, tensor):
        return ctypes.c_void_p(tensor.data_ptr() + 4) if a.get(name) == "+4" else p(tensor)

    def obj(a, kind):
        return a["obj"] if a.get("obj", "") is None else (foreign if a.get("obj") == "foreign" else own)[kind].ptr

    calls = dict(
        detokenize=lambda **a: lib.ymt3_detokenize(h, obj(a, "detok"), p(tokens), None, a.get("n", 1), L, L, L, p(starts), 0.4, p(records), 64, p(counts32), stream),
        state_reset=lambda **a: lib.ymt3_detok_state_reset(h, obj(a, "state"), stream),
        push=lambda **a: own["state"].reset() or lib.ymt3_detokenize_push(h, own["detok"].ptr, obj(a, "state"), p(tokens), None, a.get("n", 1), L, L, L, p(starts),
                                                                          9.0, p(own["state"]._notes), own["state"].capacity, p(own["state"]._counts), stream),   # (a finished state refuses first)
        tokenize=lambda **a: lib.ymt3_tokenize(h, obj(a, "tok"), arg(a, "notes", rd), a.get("n_notes", ref.size), p(starts), a.get("n", 1), 0.4, L, p(toks),
                                               p(lengths), stream),
        note_metrics=lambda **a: lib.ymt3_note_metrics(h, obj(a, "nm"), arg(a, "ref", rd), a.get("n_ref", ref.size), None, arg(a, "est", ed),
                                                       a.get("n_est", est.size), None, p(counts32), stream),
        frame_metrics=lambda **a: lib.ymt3_frame_metrics(h, obj(a, "pr"), arg(a, "ref", rd), a.get("n_ref", ref.size), None, arg(a, "est", ed),
                                                         a.get("n_est", est.size), None, a.get("n_frames", F), p(counts64), stream),
        piano_roll=lambda **a: lib.ymt3_piano_roll(h, obj(a, "pr"), arg(a, "ref", rd), a.get("n_ref", ref.size), None, a.get("n_frames", F), 0, 4, p(roll), stream),
        align_notes=lambda **a: lib.ymt3_align_notes(h, obj(a, "al"), arg(a, "ref", rd), a.get("n_ref", ref.size), None, a.get("n_frames", F), arg(a, "est", ed),
                                                     a.get("n_est", est.size), None, F, p(warp), None, p(counts64), stream),
        warp_notes=lambda **a: lib.ymt3_warp_notes(h, obj(a, "al"), arg(a, "ref", rd), a.get("n_ref", ref.size), None, p(warp), a.get("n_frames", F),
                                                   arg(a, "out", out), stream))

    host_notes = tm.tokens_to_notes([tokens_host], [0.0], 0.4)
    assert len(host_notes) == len(NOTES)
    host_tokens, host_lengths = tm.notes_to_tokens(NOTES, [0.0], 0.4, max_len=L)
    kw = dict(frames_per_second=FPS, **P)
    alignment = dtw_align(ref, est, F, F, band_frames=F, **kw)

    def check_state():
        own["state"].reset()
        first = tm.tokens_to_notes_stream(m, own["detok"], own["state"], tokens[:1], [0.0], float("inf"))
        last = tm.tokens_to_notes_stream(m, own["detok"], own["state"], end_sec=0.4)
        assert DC.same_notes(sorted(first[0] + last[0]), host_notes) is None and first[1:] == last[1:] == (0, 0)

    def check_tok():
        got, lens = tm.notes_to_tokens_device(m, NOTES, [0.0], 0.4, max_len=L, tokenizer=own["tok"])
        assert np.array_equal(got.cpu().numpy(), host_tokens) and np.array_equal(lens.cpu().numpy(), host_lengths)

    def check_al():
        got_warp, result = own["al"].align(rd, ed, F, F)
        assert result.tolist() == [alignment.total, alignment.path_len] + alignment.skipped.tolist() and np.array_equal(got_warp.cpu().numpy(), alignment.warp)
        got = own["al"].warp(rd, got_warp).cpu().numpy().view(NOTE_RECORD)
        want = warp_notes(ref, alignment.warp, FPS)
        assert all(np.array_equal(got[f], want[f], equal_nan=True) for f in NOTE_RECORD.names)

    def check_detok():
        got, bad = tm.tokens_to_notes_device(m, tokens[:1], [0.0], 0.4, detokenizer=own["detok"])
        assert DC.same_notes(got, host_notes) is None and bad == 0

    def check_nm():
        assert np.array_equal(own["nm"].run(rd, ed).cpu().numpy(), note_metrics(ref, est, **P).flat())

    def check_pr():
        assert np.array_equal(own["pr"].metrics(rd, ed, F).cpu().numpy(), frame_metrics(ref, est, F, **kw).flat())
        assert np.array_equal(own["pr"].roll(ed, F).cpu().numpy(), piano_roll(est, F, **kw))

    checks = dict(detok=check_detok, state=check_state, tok=check_tok, nm=check_nm, pr=check_pr, al=check_al)
    return calls, checks


def test_every_refusal_has_its_code_and_text_and_the_object_goes_on(six):
    tm, m, own, foreign = six
    calls, checks = _calls(tm, m, own, foreign)
    for kind, check in checks.items():
        check()
    for entry, wrong, text in REFUSALS:
        rc = calls[entry](**wrong)
        got = m._lib.ymt3_last_error().decode()
        print(f"{entry}{wrong}: {rc} {got!r}")
        assert rc == 1 and got == text, (entry, wrong, rc, got)
        checks[OBJECT_OF[entry]]()
    assert {OBJECT_OF[e] for e, _, _ in REFUSALS} == set(checks)
    assert calls["frame_metrics"]() == 0 and calls["warp_notes"]() == 0     # the table's calls are valid but for what a row changes


def test_close_closes_everything_the_model_owns():
    from yourmt3_amd.constraint import TokenAutomaton
    tm = TC.task_manager("mt3_full_plus")
    m = _model(CFG, max_batch=1)
    V = m.cfg.vocab
    detok = m.compile_detokenizer(tm, 1, L)
    made = [m.compile_constraint(TokenAutomaton(np.ones((1, V), bool), np.zeros((1, V), np.int32))), detok, detok.new_state(4),
            m.compile_tokenizer(tm, 1, L), m.compile_note_metrics(3, 4, 4, drum_program=1), m.compile_piano_roll(3, F, drum_program=1),
            m.compile_aligner(3, F, drum_program=1), m.compile_ingest_stream(16000)]
    assert set(m._owned) == set(made) and all(o.ptr.value for o in made)
    with m.compile_aligner(3, F, drum_program=1) as extra:                                   # `with` frees at the end of the block
        assert extra.ptr.value
    with pytest.raises(ValueError, match="the aligner object has been closed"):
        extra.ptr
    m.close()
    nouns = ["constraint", "detokenizer", "detokenizer state", "tokenizer", "note metrics object", "piano roll object", "aligner object", "ingest stream"]
    for o, noun in zip(made, nouns):
        with pytest.raises(ValueError, match=f"^the {noun} has been closed$"):
            o.ptr
        o.close()                                                            # a second close is a no-op
