"""Alignment on the GPU (include/ymt3.h, alignment; yourmt3_amd/csrc/align.hip).  The reference of every comparison is the host
specification, dtw_align and warp_notes of yourmt3_amd/metrics.py, never the device path itself, and every comparison is an equality:

  1. every case of tests/align_cases.py: warp, path, path_len, total and skipped; the warped records byte for byte (NaN payloads aside);
  2. the sides' sizes read on the device through count pointers; path=None; notes_out_dev == notes_dev;
  3. the object's state: the same call twice, a small call after a large one against a fresh object;
  4. the refused arguments, with handle and object usable afterwards;
  5. the handle's decode state left alone; evaluate(align=True, frames=True) and align() end to end."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

import align_cases as C
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.metrics import dtw_align, frame_metrics, note_metrics, warp_notes
from yourmt3_amd.task_manager import NOTE_RECORD, Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
MAX_FRAMES = 3000
CASES = C.cases()
IDS = [c["id"] for c in CASES]
_p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def rig():
    """the model, and per parameter set an aligner with room for the largest case"""
    m = _model(CFG, max_batch=2)
    yield m, {}
    m.close()


def _aligner(rig, case):
    m, objs = rig
    key = (case["n_programs"], case["drum_program"], case["fps"], case["band"])
    if key not in objs:
        objs[key] = m.compile_aligner(case["n_programs"], MAX_FRAMES, case["fps"], case["band"], case["drum_program"])
    return m, objs[key]


def to_pad(n: int) -> np.ndarray:
    """records that would count, and sound, if they were read"""
    pad = np.zeros(n, NOTE_RECORD)
    pad["onset"], pad["offset"], pad["pitch"] = 0.0, 0.2, 60
    return pad


def _dev(rec: np.ndarray, capacity: int = 0) -> torch.Tensor:
    return torch.from_numpy(np.concatenate([rec, to_pad(max(capacity - rec.size, 0))]).view(np.uint8).reshape(-1).copy()).cuda()


def _records(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(NOTE_RECORD)


def same_records(got: np.ndarray, want: np.ndarray) -> bool:
    return (got.shape == want.shape and all(np.array_equal(got[f], want[f], equal_nan=True) for f in ("onset", "offset", "score"))
            and all(np.array_equal(got[f], want[f]) for f in ("program", "pitch", "is_drum")))


def check(got, want, na, nb):
    """(warp, result, path) of the device against an Alignment"""
    warp, result, path = got
    assert warp.dtype == torch.int32 and warp.is_cuda and tuple(warp.shape) == (na,)
    assert result.dtype == torch.int64 and tuple(result.shape) == (4,) and path.dtype == torch.int32 and tuple(path.shape) == (na + nb - 1, 2)
    result = result.cpu().numpy()
    assert result.tolist() == [want.total, want.path_len] + want.skipped.tolist(), (result, want)
    assert np.array_equal(warp.cpu().numpy(), want.warp)
    assert np.array_equal(path[:want.path_len].cpu().numpy(), want.path)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_alignment_equals_dtw_align(rig, case):
    m, al = _aligner(rig, case)
    want = C.reference(case)
    rd, ed = _dev(case["ref"]), _dev(case["est"])
    got = al.align(rd, ed, case["na"], case["nb"], path=True)
    print(f"{case['id']}: {case['na']} x {case['nb']} frames, band {case['band']}: total {want.total}, path_len {want.path_len}, skipped {want.skipped.tolist()}")
    check(got, want, case["na"], case["nb"])
    # the records along the warp; records given on the host are uploaded
    for side in ("ref", "est"):
        out = al.warp(_dev(case[side]), got[0])
        assert out.dtype == torch.uint8 and out.is_cuda and same_records(_records(out), warp_notes(case[side], want.warp, case["fps"])), side
    out = al.warp(torch.from_numpy(case["ref"].view(np.uint8).reshape(-1).copy()), got[0])
    assert same_records(_records(out), warp_notes(case["ref"], want.warp, case["fps"]))


@pytest.mark.parametrize("name", ["frames_300x257_band7", "skipped_records", "frames_65x64_band7"])
def test_the_sizes_read_on_the_device(rig, name):
    """n is the buffers' capacity; the count pointers say how many records each side has"""
    case = C.case(name)
    m, al = _aligner(rig, case)
    ref, est, na, nb = case["ref"], case["est"], case["na"], case["nb"]
    cap_r, cap_e = ref.size + 37, est.size + 5
    rd, ed = _dev(ref, cap_r), _dev(est, cap_e)
    full_r, full_e = np.concatenate([ref, to_pad(37)]), np.concatenate([est, to_pad(5)])
    count = lambda v: torch.tensor([v, 12345], dtype=torch.int32).cuda()                 # (a detokeniser's counter has a second element)
    kw = dict(band_frames=case["band"], **C.params(case))
    for cr, ce in ((ref.size, est.size), (ref.size // 2, est.size), (ref.size, est.size // 3), (0, est.size), (ref.size, -4), (cap_r, cap_e),
                   (cap_r + 100, cap_e + 100)):
        hr, he = full_r[:max(cr, 0)], full_e[:max(ce, 0)]
        want = dtw_align(hr, he, na, nb, **kw)
        got = al.align(rd, ed, na, nb, ref_count=count(cr), est_count=count(ce), path=True)
        check(got, want, na, nb)
        out = _records(al.warp(rd, got[0], count=count(cr)))                             # records past the count stay as they are
        n = min(max(cr, 0), cap_r)
        assert same_records(out[:n], warp_notes(full_r[:n], want.warp, case["fps"])) and same_records(out[n:], full_r[n:]), (cr, ce)
    check(al.align(rd, ed, na, nb, ref_count=count(ref.size), est_count=count(est.size), path=True), C.reference(case), na, nb)


def test_the_same_call_twice_and_a_small_call_after_a_large_one(rig):
    big = C.case("tempo_curve")
    m, al = _aligner(rig, big)
    rd, ed = _dev(big["ref"]), _dev(big["est"])
    first = al.align(rd, ed, big["na"], big["nb"], path=True)
    again = al.align(rd, ed, big["na"], big["nb"], path=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    check(again, C.reference(big), big["na"], big["nb"])
    # small calls on the object that has just held 3000 x 2750 frames under a band of 400, and on a fresh one: both orientations, and a
    # call with nothing sounding, whose every step is a tie
    fresh = m.compile_aligner(big["n_programs"], MAX_FRAMES, big["fps"], big["band"], big["drum_program"])
    for name in ("frames_300x257_band40", "frames_200x513_band40", "frames_65x64_band7", "both_empty"):
        small = C.case(name)
        ref, est = small["ref"].copy(), small["est"].copy()
        ref["program"], est["program"] = ref["program"] * 2, est["program"] * 2         # the small cases' programs 0, 1, 2 under the big case's parameters
        want = dtw_align(ref, est, small["na"], small["nb"], band_frames=big["band"], **C.params(big))
        assert want.path_len > 0
        for obj in (al, fresh):
            check(obj.align(_dev(ref), _dev(est), small["na"], small["nb"], path=True), want, small["na"], small["nb"])
    check(al.align(rd, ed, big["na"], big["nb"], path=True), C.reference(big), big["na"], big["nb"])
    with fresh as f:
        assert f is fresh
    with pytest.raises(ValueError, match="closed"):
        fresh.ptr


def test_frames_up_to_max_frames_and_no_path(rig):
    case = next(c for c in CASES if (c["na"], c["nb"]) == (257, 200))
    m = rig[0]
    want = C.reference(case)
    rd, ed = _dev(case["ref"]), _dev(case["est"])
    with m.compile_aligner(case["n_programs"], 257, case["fps"], case["band"], case["drum_program"]) as al:
        check(al.align(rd, ed, 257, 200, path=True), want, 257, 200)
        got = al.align(rd, ed, 257, 200)                                                 # path=None
        assert len(got) == 2 and np.array_equal(got[0].cpu().numpy(), want.warp)
        assert got[1].cpu().numpy().tolist() == [want.total, want.path_len] + want.skipped.tolist()
        for call, word in ((lambda: al.align(rd, ed, 258, 200), "n_ref_frames"), (lambda: al.align(rd, ed, 257, 258), "n_est_frames"),
                           (lambda: al.align(rd, ed, 0, 200), "n_ref_frames"), (lambda: al.align(rd, ed, 257, 0), "n_est_frames")):
            with pytest.raises(_lib.YMT3Error, match="ymt3 error 1: " + word):
                call()
        check(al.align(ed, rd, 200, 257, path=True), dtw_align(case["est"], case["ref"], 200, 257, band_frames=case["band"], **C.params(case)), 200, 257)


def test_argument_errors_leave_everything_usable(rig):
    case = C.case("frames_300x257_band7")
    m, al = _aligner(rig, case)
    want = C.reference(case)
    na, nb = case["na"], case["nb"]
    ref = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _dev(case["ref"])])[16:]  # (a view: its misaligned neighbours exist)
    est = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _dev(case["est"])])[16:]
    warp = torch.empty(na + 2, dtype=torch.int32).cuda()
    path = torch.empty((na + nb + 1, 2), dtype=torch.int32).cuda()
    result = torch.empty(5, dtype=torch.int64).cuda()
    out = torch.empty(ref.numel() + 16, dtype=torch.uint8).cuda()

    def align(**over):
        a = dict(ref=_p(ref), n_ref=case["ref"].size, na=na, est=_p(est), n_est=case["est"].size, nb=nb, warp=_p(warp), path=_p(path), result=_p(result))
        a.update(over)
        rc = m._lib.ymt3_align_notes(m._handle, al.ptr, a["ref"], a["n_ref"], None, a["na"], a["est"], a["n_est"], None, a["nb"], a["warp"], a["path"],
                                     a["result"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def warped(**over):
        a = dict(notes=_p(ref), n=case["ref"].size, warp=_p(warp), na=na, out=_p(out))
        a.update(over)
        rc = m._lib.ymt3_warp_notes(m._handle, al.ptr, a["notes"], a["n"], None, a["warp"], a["na"], a["out"], m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    def good():
        rc, msg = align()
        assert rc == 0, msg
        assert result[:4].cpu().numpy().tolist() == [want.total, want.path_len] + want.skipped.tolist()
        assert np.array_equal(warp[:na].cpu().numpy(), want.warp) and np.array_equal(path[:want.path_len].cpu().numpy(), want.path)

    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)
    for over, word in [({"na": MAX_FRAMES + 1}, "n_ref_frames"), ({"na": 0}, "n_ref_frames"), ({"nb": MAX_FRAMES + 1}, "n_est_frames"), ({"nb": 0}, "n_est_frames"),
                       ({"nb": -1}, "n_est_frames"), ({"n_ref": -1}, "n_ref"), ({"n_est": -1}, "n_est"), ({"n_ref": (1 << 29) + 1}, "n_ref"),
                       ({"n_est": (1 << 29) + 1}, "n_est"), ({"warp": None}, "warp_dev"), ({"result": None}, "result_dev"),
                       ({"ref": None}, "ref_notes_dev"), ({"est": None}, "est_notes_dev"), ({"ref": off(ref, 4)}, "ref_notes_dev is not aligned"),
                       ({"est": off(est, 4)}, "est_notes_dev is not aligned"), ({"warp": off(warp, 2)}, "warp_dev is not aligned"),
                       ({"result": off(result, 4)}, "result_dev is not aligned"), ({"path": off(path, 4)}, "path_dev is not aligned")]:
        warp.fill_(-7), path.fill_(-7), result.fill_(-7)
        rc, msg = align(**over)
        assert rc == 1 and word in msg, (over, rc, msg)                  # YMT3_ERR_ARG, naming the argument
        assert int((warp != -7).sum()) == 0 and int((path != -7).sum()) == 0 and int((result != -7).sum()) == 0       # nothing was launched
        good()
        assert int(warp[na]) == -7 and int(result[4]) == -7 and int((path[want.path_len:] != -7).sum()) == 0          # and nothing past the ends
    host = warp_notes(case["ref"], want.warp, case["fps"])
    for over, word in [({"na": MAX_FRAMES + 1}, "n_ref_frames"), ({"na": 0}, "n_ref_frames"), ({"n": -1}, "n_notes"), ({"n": (1 << 29) + 1}, "n_notes"),
                       ({"warp": None}, "warp_dev"), ({"warp": off(warp, 2)}, "warp_dev is not aligned"), ({"notes": None}, "notes_dev"),
                       ({"out": None}, "notes_out_dev"), ({"notes": off(ref, 4)}, "notes_dev is not aligned"), ({"out": off(out, 4)}, "notes_out_dev is not aligned")]:
        out.fill_(7)
        rc, msg = warped(**over)
        assert rc == 1 and word in msg, (over, rc, msg)
        assert int((out != 7).sum()) == 0
        rc, msg = warped()
        assert rc == 0, msg
        assert same_records(_records(out[:ref.numel()]), host) and int((out[ref.numel():] != 7).sum()) == 0
    # in place: notes_out_dev == notes_dev
    mine = ref.clone()
    assert warped(notes=_p(mine), out=_p(mine))[0] == 0 and same_records(_records(mine), host)
    # an empty side needs no pointer, and no records need none
    assert align(ref=None, n_ref=0)[0] == 0
    empty = dtw_align(case["ref"][:0], case["est"], na, nb, band_frames=case["band"], **C.params(case))
    assert result[:4].cpu().numpy().tolist() == [empty.total, empty.path_len, 0, 0] and np.array_equal(warp[:na].cpu().numpy(), empty.warp)
    assert warped(notes=None, out=None, n=0)[0] == 0
    # ymt3_aligner_create refuses what it cannot serve, and the handle goes on
    ok = dict(frames_per_second=100.0, n_programs=130, drum_program=128, band_frames=10)
    for change, max_frames, code, word in [({"frames_per_second": float("nan")}, 8, 1, "frames_per_second"), ({"frames_per_second": 0.0}, 8, 1, "frames_per_second"),
                                           ({"frames_per_second": -1.0}, 8, 1, "frames_per_second"), ({"frames_per_second": float("inf")}, 8, 1, "frames_per_second"),
                                           ({"n_programs": 0, "drum_program": 0}, 8, 1, "n_programs"), ({"drum_program": 130}, 8, 1, "drum_program"),
                                           ({"drum_program": -1}, 8, 1, "drum_program"), ({"band_frames": 0}, 8, 1, "band_frames"),
                                           ({"band_frames": -5}, 8, 1, "band_frames"), ({}, 0, 1, "max_frames"), ({}, (1 << 20) + 1, 1, "max_frames"),
                                           ({"n_programs": 257}, 8, 4, "n_programs")]:
        params = _lib.AlignParams(**{**ok, **change})
        obj = ctypes.c_void_p(1)
        rc = m._lib.ymt3_aligner_create(m._handle, ctypes.byref(params), max_frames, ctypes.byref(obj))
        assert rc == code and obj.value is None and word in m._lib.ymt3_last_error().decode(), (change, rc, m._lib.ymt3_last_error().decode())
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_aligner_create(m._handle, None, 8, ctypes.byref(obj)) == 1 and "params" in m._lib.ymt3_last_error().decode()
    m._lib.ymt3_aligner_destroy(None)                                    # NULL is a no-op
    good()
    with pytest.raises(ValueError, match="NOTE_RECORD"):
        al.align(torch.zeros(33, dtype=torch.uint8).cuda(), est, na, nb)
    with pytest.raises(ValueError, match="int32"):
        al.warp(ref, warp.to(torch.int64))


def test_decode_is_the_same_before_and_after(rig):
    case = C.case("frames_300x257_band7")
    m, al = _aligner(rig, case)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    got = al.align(_dev(case["ref"]), _dev(case["est"]), case["na"], case["nb"], path=True)
    out = al.warp(_dev(case["ref"]), got[0])
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    check(got, C.reference(case), case["na"], case["nb"])
    assert same_records(_records(out), warp_notes(case["ref"], C.reference(case).warp, case["fps"]))


def test_evaluate_with_align_and_align_end_to_end(rig, tmp_path):
    from yourmt3_amd.midi import read_midi_notes
    from yourmt3_amd.transcribe import align, evaluate, transcribe
    m = rig[0]
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=5 * 8191), seed=3)[0].numpy()
    _, notes = transcribe(m, audio, bsz=2, output_dir=str(tmp_path), return_notes=True, device_detok=True)
    assert len(notes) > 0
    end_sec = audio.shape[-1] / CFG.sample_rate
    nb = max(1, math.ceil(end_sec * 100.0))
    # the reference: the transcription with a lead-in of 0.5 s, played 10 % slower, a pitch wrong here and there and a note of its own
    reference = [dataclasses.replace(x, onset=0.5 + 1.1 * x.onset, offset=0.5 + 1.1 * x.offset, pitch=(x.pitch + 1) % 128 if i % 7 == 6 else x.pitch)
                 for i, x in enumerate(notes)]
    reference += [Note(0.10, 0.30, False, 7, 1)]
    ref_end = max(max(x.onset, x.offset) for x in reference)
    na, band = max(1, math.ceil(ref_end * 100.0)), 200
    want = dtw_align(reference, notes, na, nb, 130, band_frames=band)
    warped = warp_notes(reference, want.warp)
    res = evaluate(m, audio, reference, bsz=2, align=True, band_sec=2.0, frames=True)
    note_want, frame_want = note_metrics(warped, notes, 130), frame_metrics(warped, notes, nb, 130)
    print(f"{len(notes)} notes, {na} x {nb} frames: total {want.total}, path_len {want.path_len}; {note_want}; {frame_want}")
    assert res["align_total"] == want.total and res["align_path_len"] == want.path_len and res["n_frames"] == nb
    assert np.array_equal(res["counts"], note_want.counts) and np.array_equal(res["skipped"], note_want.skipped)
    assert np.array_equal(res["frame_counts"], frame_want.counts)
    plain = evaluate(m, audio, reference, bsz=2, frames=True)
    off = evaluate(m, audio, reference, bsz=2, frames=True, align=False)
    assert set(off) == set(plain) == set(res) - {"align_total", "align_path_len"}
    assert np.array_equal(off["counts"], plain["counts"]) and np.array_equal(off["frame_counts"], plain["frame_counts"])
    assert all(off[k] == plain[k] for k in ("onset_f", "offset_f", "drum_onset_f", "multi_f", "frame_f", "multi_frame_f", "n_frames"))
    assert np.array_equal(plain["counts"], note_metrics(reference, notes, 130).counts)
    # align(): the warped reference as notes, and as a MIDI file
    got = align(m, audio, reference, bsz=2, band_sec=2.0, output_dir=str(tmp_path))
    assert got["total"] == want.total and got["path_len"] == want.path_len and (got["n_ref_frames"], got["n_est_frames"]) == (na, nb)
    assert np.array_equal(got["warp"], want.warp)
    assert [(n.onset, n.offset, n.is_drum, n.program, n.pitch) for n in got["notes"]] == [
        (float(r["onset"]), float(r["offset"]), bool(r["is_drum"]), int(r["program"]), int(r["pitch"])) for r in warped]
    assert got["midi_path"].endswith("audio.aligned.mid")
    from yourmt3_amd.midi import notes_to_midi_bytes
    assert open(got["midi_path"], "rb").read() == notes_to_midi_bytes(got["notes"])
    assert len(read_midi_notes(open(got["midi_path"], "rb").read())) > 0
    assert "midi_path" not in align(m, audio, reference, bsz=2, band_sec=2.0)
