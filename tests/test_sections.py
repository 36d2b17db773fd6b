"""The device section tracker (include/ymt3.h, sections; yourmt3_amd/csrc/sections.hip) against the host specification,
yourmt3_amd/sections.py, which is always the reference:
  1. every case of tests/section_cases.py: section, novelty and result EQUAL, the outputs pre-filled with sentinels and 8 entries longer,
     with and without a metre, with novelty_dev given and NULL, with and without a count; the wrapper's run the same;
  2. the same call twice, a small call after a large one against a fresh object, two parameter sets alive together;
  3. the refused arguments with their texts, the object usable afterwards; destroy before and after the handle's destruction;
  4. the handle's decode state left alone; transcribe(beats=True, bars=True, chords=True, sections=True) and estimate_sections() end to end."""
import ctypes

import numpy as np
import pytest
import torch

import section_cases as SC
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd import bars as B
from yourmt3_amd import beats as T
from yourmt3_amd import chords as Ch
from yourmt3_amd import midi as M
from yourmt3_amd import sections as S
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.task_manager import Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
CASES = SC.all_cases()
IDS = [c[0] for c in CASES]
MAX_BEATS, MAX_NOTES = 1024, 1024
SENTINEL = -7
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def rig():
    """the model, and one tracker per parameter set"""
    m = _model(CFG, max_batch=2)
    yield m, {}
    m.close()


@pytest.fixture(scope="module")
def reference():
    """the specification's answer of every case, computed once: name -> ((section, novelty, result) with the case's metre, the same without)"""
    out = {}
    for name, rec, beats, n_frames, metre, params, count in CASES:
        plain = S.track_sections(SC.live(rec, count), beats, n_frames, **params)
        out[name] = (plain if metre is None else S.track_sections(SC.live(rec, count), beats, n_frames, metre=metre, **params), plain)
    return out


def _tracker(rig, params):
    m, objs = rig
    key = repr(sorted(params.items()))
    if key not in objs:
        objs[key] = m.compile_section_tracker(MAX_BEATS, MAX_NOTES, **params)
    return m, objs[key]


def _bytes(rec: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())


def _count(count):
    return None if count is None else torch.tensor([count, 12345], dtype=torch.int32).cuda()     # (a detokeniser's counter has a second element)


def _beats(beats):
    """-> (beats on the device, one spare entry so that K = 0 has a pointer; the beat tracker's result with K in it)"""
    b = torch.from_numpy(np.concatenate([np.asarray(beats, np.int32), np.array([SENTINEL], np.int32)])).cuda()
    return b, torch.tensor([len(beats), 11, 22, 33], dtype=torch.int64).cuda()


def _metre(metre):
    return None if metre is None else torch.from_numpy(np.concatenate([np.asarray(metre, np.int32), np.array([0], np.int32)])).cuda()


def _raw(m, st, rec, beats, n_frames, metre=None, count=None, novelty=True):
    """the C call itself -> (section, novelty or None, result), pre-filled with the sentinel and 8 entries longer"""
    n = rec.numel() // 32
    b, beat_result = _beats(beats)
    md = _metre(metre)
    section = torch.full((st.max_beats + 8,), SENTINEL, dtype=torch.int32).cuda()
    nov = torch.full((st.max_beats + 8,), SENTINEL, dtype=torch.int64).cuda() if novelty else None
    result = torch.full((8 + 8,), SENTINEL, dtype=torch.int64).cuda()
    rc = m._lib.ymt3_track_sections(m._handle, st.ptr, _p(b), _p(beat_result), _p(md), _p(rec) if n else None, n, _p(count), n_frames, _p(section),
                                    st.max_beats, _p(nov), _p(result), m._stream())
    assert rc == 0, m._lib.ymt3_last_error().decode()
    return section, nov, result


def check(ref, out):
    """the device's outputs (as _raw returns them) against the specification's, sentinels included"""
    want_section, want_nov, want_result = ref
    section, nov, result = (None if t is None else t.cpu().numpy() for t in out)
    assert result[:8].tolist() == want_result.tolist() and (result[8:] == SENTINEL).all()
    k = want_section.size
    assert section[:k].tolist() == want_section.tolist() and (section[k:] == SENTINEL).all()     # beyond K: left alone
    if nov is not None:
        assert nov[:k].tolist() == want_nov.tolist() and (nov[k:] == SENTINEL).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_equals_the_specification(rig, reference, case):
    name, rec, beats, n_frames, metre, params, count = case
    m, st = _tracker(rig, params)
    dev = _bytes(rec).cuda()
    with_metre, plain = reference[name]
    check(with_metre, _raw(m, st, dev, beats, n_frames, metre, _count(count)))
    check(plain, _raw(m, st, dev, beats, n_frames, None, _count(count), novelty=False))             # metre_dev and novelty_dev NULL
    if count is None:                                                       # a count that leaves every record: the same
        check(with_metre, _raw(m, st, dev, beats, n_frames, metre, _count(len(rec) + 3), novelty=False))
    # the wrapper, records given on the host
    section, nov, result = st.run(beats, _bytes(rec), n_frames, metre=metre, count=_count(count))
    assert section.dtype == np.int32 and nov.dtype == np.int64 and result.dtype == np.int64
    assert section.tolist() == with_metre[0].tolist() and nov.tolist() == with_metre[1].tolist() and result.tolist() == with_metre[2].tolist()


def _named(name):
    return next(c for c in CASES if c[0] == name)


def test_the_same_call_twice_a_small_call_after_a_large_one_and_two_objects(rig, reference):
    m = rig[0]
    big, small, other = _named("records_1024"), _named("beats2"), _named("second_params")
    st = m.compile_section_tracker(MAX_BEATS, MAX_NOTES)
    second = m.compile_section_tracker(MAX_BEATS, MAX_NOTES, **other[5])    # another parameter set, alive at the same time
    for case in (big, big, small, big):
        check(reference[case[0]][0], _raw(m, st, _bytes(case[1]).cuda(), case[2], case[3], case[4]))
        check(reference[other[0]][0], _raw(m, second, _bytes(other[1]).cuda(), other[2], other[3], other[4]))
    fresh = m.compile_section_tracker(MAX_BEATS, MAX_NOTES)                 # the small call after the large one against a fresh object
    a = _raw(m, st, _bytes(small[1]).cuda(), small[2], small[3], small[4])
    b = _raw(m, fresh, _bytes(small[1]).cuda(), small[2], small[3], small[4])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for o in (st, second, fresh):
        o.close()


def test_more_peaks_than_the_select_kernel_ranks_in_lds(rig):
    """4 999 peaks, above the 4 096 keys the select kernel ranks in LDS: its other path, rounds of a block-wide maximum; ten blocks of the
    prefix count; 157 tiles of the novelty kernel"""
    m = rig[0]
    rec, beats, n_frames = SC.blocks(10000, block=2, step=10)
    params = dict(max_sections=64, min_len=1, peak_div=1024, kernel_beats=2, context=1)
    want = S.track_sections(rec, beats, n_frames, **params)
    assert want[2][4] == 4999 > 4096 and want[2][0] == 64
    with m.compile_section_tracker(16384, 16384, **params) as st:
        check(want, _raw(m, st, _bytes(rec).cuda(), beats, n_frames))
        few = S.track_sections(rec, beats, n_frames, **{**params, "max_sections": 3})
    with m.compile_section_tracker(16384, 16384, **{**params, "max_sections": 3}) as st:
        check(few, _raw(m, st, _bytes(rec).cuda(), beats, n_frames, novelty=False))


def test_argument_errors_leave_everything_usable(rig, reference):
    name, rec_np, beats_np, n_frames, metre_np, params, _ = _named("AABA")
    m, st = _tracker(rig, params)
    n = len(rec_np)
    rec = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _bytes(rec_np).cuda()])[16:]       # (a view: its misaligned neighbours exist)
    beats, beat_result = _beats(beats_np)
    metre = _metre(metre_np)
    section, nov, result = torch.empty(MAX_BEATS + 8, dtype=torch.int32).cuda(), torch.empty(MAX_BEATS + 8, dtype=torch.int64).cuda(), torch.empty(16, dtype=torch.int64).cuda()
    cnt = torch.tensor([n, 0, 0], dtype=torch.int32).cuda()
    m2 = _model(CFG, max_batch=1)
    foreign = m2.compile_section_tracker(16, 16)

    def track(**over):
        a = dict(h=m._handle, obj=st.ptr, beats=_p(beats), beat_result=_p(beat_result), metre=_p(metre), notes=_p(rec), n=n, count=_p(cnt),
                 n_frames=n_frames, section=_p(section), cap=MAX_BEATS, nov=_p(nov), result=_p(result))
        a.update(over)
        rc = m._lib.ymt3_track_sections(a["h"], a["obj"], a["beats"], a["beat_result"], a["metre"], a["notes"], a["n"], a["count"], a["n_frames"],
                                        a["section"], a["cap"], a["nov"], a["result"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def fill():
        section.fill_(SENTINEL), nov.fill_(SENTINEL), result.fill_(SENTINEL)

    def good():
        fill()
        rc, msg = track()
        assert rc == 0, msg
        check(reference[name][0], (section, nov, result))

    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    table = [({"beats": None}, "beats_dev is NULL"), ({"beats": off(beats, 2)}, "beats_dev is not aligned to 4 bytes"),
             ({"beat_result": None}, "beat_result_dev is NULL"), ({"beat_result": off(beat_result, 4)}, "beat_result_dev is not aligned to 8 bytes"),
             ({"metre": off(metre, 2)}, "metre_dev is not aligned to 4 bytes"),
             ({"n": -1}, f"n_notes=-1 outside [0, max_notes={MAX_NOTES}]"), ({"n": MAX_NOTES + 1}, f"n_notes={MAX_NOTES + 1} outside [0, max_notes={MAX_NOTES}]"),
             ({"notes": None}, "notes_dev is NULL"), ({"notes": off(rec, 4)}, "notes_dev is not aligned to 8 bytes"),
             ({"count": off(cnt, 2)}, "count_dev is not aligned to 4 bytes"),
             ({"n_frames": 0}, "n_frames=0 outside [1, 1048576]"), ({"n_frames": (1 << 20) + 1}, "n_frames=1048577 outside [1, 1048576]"),
             ({"section": None}, "section_dev is NULL"), ({"section": off(section, 2)}, "section_dev is not aligned to 4 bytes"),
             ({"cap": MAX_BEATS - 1}, f"section_cap={MAX_BEATS - 1} below the section tracker's max_beats={MAX_BEATS}"),
             ({"nov": off(nov, 4)}, "novelty_dev is not aligned to 8 bytes"),
             ({"result": None}, "result_dev is NULL"), ({"result": off(result, 4)}, "result_dev is not aligned to 8 bytes"),
             ({"obj": None}, "null section tracker"), ({"h": None}, "null handle"), ({"obj": foreign.ptr}, "the section tracker belongs to another handle")]
    for over, text in table:
        fill()
        rc, msg = track(**over)
        assert rc == 1 and msg == text and int((section != SENTINEL).sum()) == 0 and int((nov != SENTINEL).sum()) == 0 and int((result != SENTINEL).sum()) == 0, \
            (over, rc, msg)
        good()                                                              # the object's next call is right
    # no records: no pointer is needed; one silent section
    fill()
    assert track(n=0, notes=None, count=None)[0] == 0
    want = S.track_sections([], beats_np, n_frames, metre=metre_np)
    check(want, (section, nov, result))
    assert want[2].tolist() == [1, 0, 0, 0, 0, 1, 0, 0]
    # ymt3_sections_create refuses what it cannot serve, and the handle goes on
    for change, text in [({"frames_per_second": 0.0}, "frames_per_second=0 must be finite and > 0"), ({"near_div": 1}, "near_div=1 outside [2, 64]"),
                         ({"context": 0}, "context=0 outside [1, 16]"), ({"context": 17}, "context=17 outside [1, 16]"),
                         ({"kernel_beats": 1}, "kernel_beats=1 outside [2, 64]"), ({"kernel_beats": 65}, "kernel_beats=65 outside [2, 64]"),
                         ({"min_len": 0}, "min_len=0 outside [1, 256]"), ({"min_len": 257}, "min_len=257 outside [1, 256]"),
                         ({"peak_div": 0}, "peak_div=0 outside [1, 1024]"), ({"peak_div": 1025}, "peak_div=1025 outside [1, 1024]"),
                         ({"same_dist": -1}, "same_dist=-1 outside [0, 32768]"), ({"same_dist": 32769}, "same_dist=32769 outside [0, 32768]"),
                         ({"len_num": 0}, "len_num=0 outside [1, 16]"), ({"len_num": 17}, "len_num=17 outside [1, 16]"),
                         ({"max_sections": 0}, "max_sections=0 outside [1, 64]"), ({"max_sections": 65}, "max_sections=65 outside [1, 64]"),
                         ({"n_programs": 257}, "n_programs=257: at most 256 programs"), ({"drum_program": 130}, "drum_program=130 outside [0, n_programs=130)")]:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_section_tracker(16, 16, **change)
        assert str(e.value) == "ymt3 error " + ("4" if "n_programs" in change else "1") + ": " + text
        with pytest.raises(ValueError):                                    # the specification refuses the same
            S.check_params(**{**S.DEFAULTS, **change})
    for sizes, text in [((0, 1), "max_beats=0 outside [1, 1048577]"), (((1 << 20) + 2, 1), "max_beats=1048578 outside [1, 1048577]"),
                        ((1, 0), "max_notes=0 outside [1, 1048576]"), ((1, (1 << 20) + 1), "max_notes=1048577 outside [1, 1048576]")]:
        with pytest.raises(_lib.YMT3Error) as e:
            m.compile_section_tracker(*sizes)
        assert str(e.value) == "ymt3 error 1: " + text
        with pytest.raises(ValueError):
            S.check_sizes(*sizes)
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_sections_create(m._handle, None, 16, 16, ctypes.byref(obj)) == 1 and m._lib.ymt3_last_error().decode() == "params is NULL"
    assert obj.value is None
    m._lib.ymt3_sections_destroy(None)                                      # NULL is a no-op
    m2.close()
    good()


def test_destroy_before_and_after_the_handle_and_close_with_the_model(rig, reference):
    m2 = _model(CFG, max_batch=1)
    early = m2.compile_section_tracker(64, 64)
    early.close()                                                           # before the handle's destruction
    kept = m2.compile_section_tracker(64, 64, context=2)
    raw = ctypes.c_void_p()
    params = _lib.SectionParams(100.0, *(int(S.DEFAULTS[k]) for k in S._INTS))
    assert m2._lib.ymt3_sections_create(m2._handle, ctypes.byref(params), 64, 64, ctypes.byref(raw)) == 0 and raw.value
    assert kept in m2._owned
    m2.close()                                                              # closes `kept` with the model
    with pytest.raises(ValueError, match="^the section tracker has been closed$"):
        kept.ptr
    m2._lib.ymt3_sections_destroy(raw)                                      # after the handle's destruction
    name, rec, beats, n_frames, metre, params, _ = _named("ABAB")          # the first model is untouched
    m, st = _tracker(rig, params)
    check(reference[name][0], _raw(m, st, _bytes(rec).cuda(), beats, n_frames, metre))


def test_decode_is_the_same_before_and_after(rig, reference):
    name, rec, beats, n_frames, metre, params, _ = _named("ABCA")
    m, st = _tracker(rig, params)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    out = _raw(m, st, _bytes(rec).cuda(), beats, n_frames, metre)
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    check(reference[name][0], out)


def _music():
    """known music for the small configuration: C, F, G, C at 120 bpm for 6 s, three beats each: the triad on every beat and a kick on
    every change"""
    out = []
    for k in range(12):
        t, root = 0.3 + 0.5 * k, (0, 5, 7, 0)[k // 3]
        out += [Note(t, t + 0.4, False, 0, 60 + (root + s) % 12) for s in (0, 4, 7)]
        if k % 3 == 0:
            out += [Note(t, t + 0.01, True, 128, 36)]
    return out


SHORT = {"min_len": 2, "kernel_beats": 2}                                   # twelve beats of music: sections of three beats


def test_transcribe_with_sections_end_to_end(rig, tmp_path, monkeypatch):
    from yourmt3_amd import transcribe as Tr
    from yourmt3_amd.task_manager import TaskManager
    transcribe = Tr.transcribe
    m = rig[0]
    out = lambda name: str(tmp_path / name)
    read = lambda path: open(path, "rb").read()
    # Random weights transcribe no music, so the decode is replaced by the ids of known music (the tokeniser's): ingest, both detokenisers,
    # the four trackers, the positions and the writer run as they are.
    tm = TaskManager("mt3_full_plus")

    def ids(model, segments, L):
        n = int(segments.shape[0])
        starts = [i * model.cfg.segment_samples / model.cfg.sample_rate for i in range(n)]
        return tm.notes_to_tokens(_music(), starts, model.last_ingest_samples / model.cfg.sample_rate, max_len=L)[0]

    def decode(model, segments, bsz, L, continuous, scored, kw):
        t = ids(model, segments, L)
        return [t], ([np.zeros(t.shape, np.float32)] if scored else None)

    def decode_device(model, segments, bsz, L, continuous, scored, kw):
        t = torch.from_numpy(ids(model, segments, L)).cuda()
        return t, (torch.zeros(t.shape, dtype=torch.float32).cuda() if scored else None)

    monkeypatch.setattr(Tr, "_decode", decode)
    monkeypatch.setattr(Tr, "_decode_device", decode_device)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=13 * 8191), seed=3)[0].numpy()
    kw = dict(bsz=2, return_notes=True, beats=True, bars=True, chords=True)
    chords_only, notes_chords, info_chords = transcribe(m, audio, output_dir=out("chords"), **kw)
    off, _, info_off = transcribe(m, audio, output_dir=out("off"), sections=False, **kw)
    assert read(chords_only) == read(off) and set(info_off) == set(info_chords) and "sections" not in info_off
    host, notes_host, info_host = transcribe(m, audio, output_dir=out("host"), sections=True, section_params=SHORT, **kw)
    dev, notes_dev, info_dev = transcribe(m, audio, output_dir=out("dev"), sections=True, section_params=SHORT, device_detok=True, **kw)
    scored, _, info_scored = transcribe(m, audio, output_dir=out("scored"), sections=True, section_params=SHORT, device_detok=True, min_confidence=0.0, **kw)
    assert read(host) == read(dev) == read(scored) != read(off) and notes_host == notes_dev == notes_chords
    for a in (info_dev, info_scored):
        assert set(a) == set(info_host) == set(info_chords) | {"sections", "section_labels"}
        assert all(a[k] == info_host[k] for k in a if k != "ticks") and a["ticks"].tolist() == info_host["ticks"].tolist()
    assert all(info_host[k] == info_chords[k] for k in info_chords if k != "ticks")
    # against the specification on the same notes
    n_frames = T.n_frames_of(m.last_ingest_samples / CFG.sample_rate, 100.0)
    beats = T.track_beats(notes_host, n_frames)[0]
    metre, bar_result = B.track_bars(notes_host, beats, n_frames)
    chord, _ = Ch.track_chords(notes_host, beats, n_frames, metre=metre)
    section, nov, result = S.track_sections(notes_host, beats, n_frames, metre=metre, **SHORT)
    want = S.section_summary(section, result, beats, 100.0)
    print(f"{len(notes_host)} notes, {beats.size} beats, sections {[name for _, _, name in want['sections']]}")
    assert beats.size >= 10 and info_host["sections"] == want["sections"] and info_host["section_labels"] == want["section_labels"]
    assert result[0] >= 2 and want["sections"][0][2] == "A"
    marks = S.section_markers(S.section_segments(section, beats), beats)
    chord_marks = Ch.chord_markers(Ch.chord_segments(chord, beats), beats)
    written = M.read_midi_markers(read(host))
    assert written == S.merge_markers(marks, chord_marks) and [x for x in written if x[1].startswith("[")] == marks and marks
    assert [t for t, _ in written] == sorted(t for t, _ in written) and M.read_midi_markers(read(off)) == chord_marks
    ticks = T.beat_positions(notes_host, beats)
    assert read(host) == M.notes_to_midi_bytes_on_bars(notes_host, ticks, beats, metre, int(bar_result[3]), 100.0, written)
    assert M.read_midi_on_bars(read(host)) == M.read_midi_on_bars(read(off)) and M.read_midi_notes(read(host)) == M.read_midi_notes(read(off))
    # without the bars and the chords: no metre, the file on the beats with the sections' markers alone, by both detokenisers
    nb_host, _, info_nb = transcribe(m, audio, bsz=2, output_dir=out("nb_host"), return_notes=True, beats=True, sections=True, section_params=SHORT)
    nb_dev, _, info_nb_dev = transcribe(m, audio, bsz=2, output_dir=out("nb_dev"), return_notes=True, beats=True, sections=True, section_params=SHORT, device_detok=True)
    plain = S.track_sections(notes_host, beats, n_frames, **SHORT)
    assert read(nb_host) == read(nb_dev) == M.notes_to_midi_bytes_on_beats(notes_host, ticks, beats, 100.0, S.section_markers(S.section_segments(plain[0], beats), beats))
    assert info_nb["section_labels"] == info_nb_dev["section_labels"] == [int(v) & 255 for v in plain[0]] and "key" not in info_nb and "chords" not in info_nb
    # other parameters reach the kernels; the switches are checked
    _, _, one = transcribe(m, audio, bsz=2, output_dir=out("params"), return_notes=True, beats=True, sections=True, section_params={"max_sections": 1}, device_detok=True)
    assert len(one["sections"]) == 1 and set(one["section_labels"]) == {0}
    with pytest.raises(ValueError, match="sections=True without beats=True"):
        transcribe(m, audio, bsz=2, output_dir=out("bad"), sections=True)
    with pytest.raises(ValueError, match="section_params without sections=True"):
        transcribe(m, audio, bsz=2, output_dir=out("bad"), beats=True, section_params={})


def test_the_detokenisers_records_get_their_sections_in_place(rig):
    from yourmt3_amd.task_manager import TaskManager
    m = rig[0]
    tm = TaskManager("mt3_full_plus")
    seg = CFG.segment_samples / CFG.sample_rate
    starts = [i * seg for i in range(13)]
    end_sec = 13 * seg
    tokens, _ = tm.notes_to_tokens(_music(), starts, end_sec, max_len=CFG.max_decode_len)
    host_notes = tm.tokens_to_notes([tokens], starts, end_sec=end_sec)
    n_frames = T.n_frames_of(end_sec, 100.0)
    beats = T.track_beats(host_notes, n_frames)[0]
    metre, _ = B.track_bars(host_notes, beats, n_frames)
    with m.compile_beat_tracker(n_frames) as bt:
        cap = T.max_beats(n_frames, bt.lag_min)
        with m.compile_bar_tracker(cap, 13 * 48) as br, m.compile_section_tracker(cap, 13 * 48, **SHORT) as st:
            toks = torch.from_numpy(tokens).cuda()
            dev_notes, bad, tracked = tm.tokens_to_notes_device(m, toks, starts, end_sec, beats=bt, bars=br, sections=st)
            section, nov, result = S.track_sections(host_notes, beats, n_frames, metre=metre, **SHORT)
            assert dev_notes == host_notes and bad == 0 and tracked["beats"].tolist() == beats.tolist() and tracked["metre"].tolist() == metre.tolist()
            assert tracked["section"].tolist() == section.tolist() and tracked["novelty"].tolist() == nov.tolist() and tracked["section_result"].tolist() == result.tolist()
            no_bars = tm.tokens_to_notes_device(m, toks, starts, end_sec, beats=bt, sections=st)[2]
            plain = S.track_sections(host_notes, beats, n_frames, **SHORT)
            assert set(no_bars) == {"beats", "tempo", "ticks", "section", "novelty", "section_result"}
            assert no_bars["section"].tolist() == plain[0].tolist() and no_bars["novelty"].tolist() == plain[1].tolist() and no_bars["section_result"].tolist() == plain[2].tolist()
            assert set(tm.tokens_to_notes_device(m, toks, starts, end_sec, beats=bt, bars=br)[2]) == {"beats", "tempo", "ticks", "metre", "bar_result"}
            with pytest.raises(ValueError, match="sections without beats"):
                tm.tokens_to_notes_device(m, toks, starts, end_sec, sections=st)


def test_estimate_sections_finds_aaba_in_a_midi_file(rig, tmp_path):
    from yourmt3_amd.transcribe import estimate_sections
    m = rig[0]
    rec, _, n_frames, _, truth = SC.music("AABA", True)
    made = sorted(Note(float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"])) for r in rec)
    path = M.write_midi(made, str(tmp_path / "aaba_in.mid"))
    notes = M.read_midi_notes(open(path, "rb").read())                      # what the file holds: its ticks' times
    end_sec = n_frames / 100.0
    n_frames = T.n_frames_of(end_sec, 100.0)
    beats = T.track_beats(notes, n_frames)[0]
    metre, bar_result = B.track_bars(notes, beats, n_frames)
    section, nov, result = S.track_sections(notes, beats, n_frames, metre=metre)
    got = estimate_sections(m, path, end_sec=end_sec, output_path=str(tmp_path / "sections.mid"), lab_path=str(tmp_path / "sections.lab"))
    assert [round(t * 100) for t in got["beats_sec"]] == beats.tolist() and got["metre"].tolist() == metre.tolist()
    assert got["section"].tolist() == section.tolist() and got["novelty"].tolist() == nov.tolist()
    assert "".join(name for _, _, name in got["sections"]) == "AABA" and result[:2].tolist() == [4, 2]
    wanted = [j for j, _ in SC.truth_beats(beats, truth)]
    seg = S.section_segments(section, beats)
    assert [s for s, _, _ in seg] == wanted and got["section_labels"] == [int(v) & 255 for v in section]
    assert got["lab"] == S.section_lab(seg, beats, 100.0) == open(str(tmp_path / "sections.lab")).read() and got["lab"].startswith(f"{beats[0] / 100:.3f} ")
    assert [line.split()[2] for line in got["lab"].splitlines()] == ["A", "A", "B", "A"]
    data = open(str(tmp_path / "sections.mid"), "rb").read()
    assert data == got["midi"] and M.read_midi_markers(data) == S.section_markers(seg, beats)
    assert [text for _, text in M.read_midi_markers(data)] == ["[A]", "[A]", "[B]", "[A]"]
    assert M.read_midi_on_bars(data)[3] == B.key_signature(int(bar_result[3])) and got["key"] == B.key_name(bar_result[3])
    other = estimate_sections(m, notes, end_sec=end_sec, max_sections=2, bar_params={"metres": (4,)})
    assert len(other["sections"]) == 2
    empty = estimate_sections(m, [], end_sec=1.0)
    assert empty["beats_sec"] == [] and empty["sections"] == [] and empty["section_labels"] == [] and empty["lab"] == "" and M.read_midi_markers(empty["midi"]) == []
