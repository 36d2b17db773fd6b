"""Note velocities on the GPU (include/ymt3.h, note velocities; yourmt3_amd/csrc/velocity.hip).  The reference of every comparison is the
host specification, note_velocities of yourmt3_amd/velocity.py, never the device path itself:

  1. every case of tests/velocity_cases.py: counts, the measured / unmeasured split, the bytes of unmeasured records and of records
     beyond the count exactly; energies and peaks within TAU * max(P, 1e-12); every velocity among the admissible ones, and no more
     records off the specification's own byte than have two admissible values.  With and without an energy buffer;
  2. the object's state: the same call twice, a small call after a large one against a fresh object, two parameter sets alive together,
     records and audio given on the host;
  3. the refused arguments with their texts, the object usable afterwards; destroy before and after the handle's destruction;
  4. the handle's decode state left alone; transcribe(velocity=True) and estimate_velocities() end to end.

Measured on an MI355X when this was written: the largest |E_dev - E_spec| / max(P, 1e-12) over all cases is 1.61e-7 (window_96; TAU =
4.8e-6), and no velocity of any case differs from the specification's.  Every test prints its own figures before it asserts."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

import velocity_cases as C
from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd import _lib
from yourmt3_amd import velocity as V
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.task_manager import NOTE_RECORD, Note

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=48, n_enc_layers=1, n_dec_layers=1)
CASES = C.cases()
IDS = [c["id"] for c in CASES]
_p = lambda t: ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def rig():
    """the model, and one velocity object per parameter set"""
    assert CFG.sample_rate == C.SR
    m = _model(CFG, max_batch=2)
    yield m, {}
    m.close()


def _nv(rig, case):
    m, objs = rig
    key = repr(sorted(case["params"].items()))
    if key not in objs:
        objs[key] = m.compile_note_velocity(**case["params"])
    return m, objs[key]


def _case(name):
    return next(c for c in CASES if c["id"] == name)


def _bytes(rec: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())


def _count(case):
    return None if case["count"] is None else torch.tensor([case["count"], 12345], dtype=torch.int32).cuda()     # (a detokeniser's counter has a second element)


def _raw(m, nv, audio, rec, count=None, energy=True):
    """ymt3_note_velocities itself -> (rc, velocity, energy or None, peaks, counts), the outputs pre-filled with sentinels"""
    n = rec.numel() // 32
    vel = torch.full((n + 8,), 7, dtype=torch.uint8).cuda()
    en = torch.full((n + 8,), -7.0).cuda() if energy else None
    peaks, counts = torch.full((2,), -7.0).cuda(), torch.full((2,), -7, dtype=torch.int32).cuda()
    rc = m._lib.ymt3_note_velocities(m._handle, nv.ptr, _p(audio) if audio.numel() else None, audio.numel(), _p(rec) if n else None, n,
                                     None if count is None else _p(count), _p(vel), None if en is None else _p(en), _p(peaks), _p(counts), m._stream())
    return rc, vel, en, peaks, counts


def check(case, vel, en, peaks, counts, label=""):
    """the device's answer for the case against the specification; -> the largest energy error in units of max(P, 1e-12)"""
    ref = C.reference(case)
    n, live = case["rec"].size, C.live(case)
    vel, peaks, counts = vel.cpu().numpy(), peaks.cpu().numpy().astype(np.float64), counts.cpu().numpy()
    assert vel.dtype == np.uint8 and vel.shape == (n,)
    assert counts.tolist() == ref["counts"].tolist(), label
    assert (vel[live:] == 0).all(), label                                  # at or beyond the count
    spec_measured = ~np.isnan(ref["E"])
    default = int(V.check_params(C.SR, **case["params"])["default_velocity"])
    assert (vel[:live][~spec_measured] == default).all(), label
    worst = 0.0
    if en is not None:
        en = en.cpu().numpy()
        assert en.dtype == np.float32 and en.shape == (n,) and np.isnan(en[live:]).all()
        assert np.array_equal(~np.isnan(en[:live]), spec_measured), label   # the split
        err = np.abs(en[:live][spec_measured].astype(np.float64) - ref["E"][spec_measured]) / np.maximum(ref["P"][spec_measured], 1e-12)
        worst = float(err.max()) if err.size else 0.0
    slack = C.peak_slack(case)
    peak_err = [abs(peaks[c] - ref["peaks"][c]) for c in (0, 1)]
    spans = C.admissible(case)
    off = [i for i in range(live) if vel[i] != ref["vel"][i]]
    print(f"{case['id']}{label}: {live} live of {n}, {int(spec_measured.sum())} measured; largest |E_dev - E_spec| / P = {worst:.3g} (TAU {C.TAU:.3g}); "
          f"peaks off by {peak_err[0]:.3g}, {peak_err[1]:.3g} (allowed {slack[0]:.3g}, {slack[1]:.3g}); "
          f"{len(off)} velocities differ from the specification's, {sum(hi > lo for lo, hi in spans)} have two admissible values")
    assert worst <= C.TAU, label
    assert all(peak_err[c] <= slack[c] for c in (0, 1)), label
    assert all(spans[i][0] <= int(vel[i]) <= spans[i][1] for i in range(live)), [(i, int(vel[i]), spans[i]) for i in range(live) if not spans[i][0] <= int(vel[i]) <= spans[i][1]]
    assert all(spans[i][1] > spans[i][0] for i in off)                      # equality wherever the interval rounds to one value
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_reproduces_the_specification(rig, case):
    m, nv = _nv(rig, case)
    audio, rec = torch.from_numpy(case["audio"]).cuda(), _bytes(case["rec"]).cuda()
    vel, en, peaks, counts = nv.run(audio, rec, count=_count(case), energies=True)
    assert all(t.is_cuda for t in (vel, en, peaks, counts)) and peaks.dtype == torch.float32 and counts.dtype == torch.int32
    check(case, vel, en, peaks, counts)
    three = nv.run(audio, rec, count=_count(case))
    assert len(three) == 3 and torch.equal(three[0], vel) and torch.equal(three[1], peaks) and torch.equal(three[2], counts)
    # without an energy buffer the second kernel measures again: the same bytes, and nothing written past n
    rc, vel2, _, peaks2, counts2 = _raw(m, nv, audio, rec, _count(case), energy=False)
    n = case["rec"].size
    assert rc == 0 and torch.equal(vel2[:n], vel) and int((vel2[n:] != 7).sum()) == 0
    assert torch.equal(peaks2, peaks) and torch.equal(counts2, counts)
    rc, vel3, en3, _, _ = _raw(m, nv, audio, rec, _count(case))
    assert rc == 0 and torch.equal(vel3[:n], vel) and int((vel3[n:] != 7).sum()) == 0 and int((en3[n:] != -7.0).sum()) == 0
    assert torch.equal(en3[:n].view(torch.int32), en.view(torch.int32))


def test_the_same_call_twice_a_small_call_after_a_large_one_and_two_objects(rig):
    big, small = _case("n_257"), _case("n_5")
    m, nv = _nv(rig, big)
    other_case = _case("mapping")
    _, other = _nv(rig, other_case)                                        # two parameter sets alive together
    audio = torch.from_numpy(big["audio"]).cuda()
    first = nv.run(audio, _bytes(big["rec"]).cuda(), energies=True)
    mapped = other.run(audio, _bytes(other_case["rec"]).cuda(), energies=True)
    again = nv.run(audio, _bytes(big["rec"]).cuda(), energies=True)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    check(big, *first)
    check(other_case, *mapped)
    fresh = m.compile_note_velocity()
    for obj in (nv, fresh):
        check(small, *obj.run(audio, _bytes(small["rec"]).cuda(), energies=True))
    a, b = nv.run(audio, _bytes(small["rec"]).cuda(), energies=True), fresh.run(audio, _bytes(small["rec"]).cuda(), energies=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    # records and audio given on the host are uploaded; the audio may have any shape
    host = nv.run(torch.from_numpy(big["audio"]).view(-1, 1000), _bytes(big["rec"]), energies=True)
    for x, y in zip(first, host):
        assert x.is_cuda and y.is_cuda and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    # the order of the records does not matter
    perm = np.random.default_rng(2).permutation(big["rec"].size)
    shuffled = nv.run(audio, _bytes(big["rec"][perm]).cuda(), energies=True)
    assert torch.equal(shuffled[0].cpu(), first[0].cpu()[perm]) and torch.equal(shuffled[1].cpu().view(torch.int32), first[1].cpu().view(torch.int32)[perm])
    assert torch.equal(shuffled[2], first[2]) and torch.equal(shuffled[3], first[3])
    fresh.close()
    with pytest.raises(ValueError, match="^the note velocity object has been closed$"):
        fresh.ptr
    with pytest.raises(ValueError, match="NOTE_RECORD"):
        nv.run(audio, torch.zeros(33, dtype=torch.uint8))
    with pytest.raises(ValueError, match="float32"):
        nv.run(audio.double(), _bytes(small["rec"]))
    with pytest.raises(TypeError, match="window"):
        m.compile_note_velocity(window=64)


def test_argument_errors_leave_everything_usable(rig):
    case = _case("n_65")
    m, nv = _nv(rig, case)
    n = case["rec"].size
    audio = torch.cat([torch.zeros(4).cuda(), torch.from_numpy(case["audio"]).cuda()])[4:]       # (views: their misaligned neighbours exist)
    rec = torch.cat([torch.zeros(16, dtype=torch.uint8).cuda(), _bytes(case["rec"]).cuda()])[16:]
    vel = torch.empty(n + 8, dtype=torch.uint8).cuda()
    en, peaks, counts, cnt = torch.empty(n + 2).cuda(), torch.empty(4).cuda(), torch.empty(4, dtype=torch.int32).cuda(), torch.tensor([n, 0, 0], dtype=torch.int32).cuda()
    m2 = _model(CFG, max_batch=1)
    foreign = m2.compile_note_velocity()

    def call(**over):
        a = dict(h=m._handle, obj=nv.ptr, audio=_p(audio), n_audio=audio.numel(), notes=_p(rec), n=n, count=_p(cnt), vel=_p(vel), en=_p(en), peaks=_p(peaks),
                 counts=_p(counts))
        a.update(over)
        rc = m._lib.ymt3_note_velocities(a["h"], a["obj"], a["audio"], a["n_audio"], a["notes"], a["n"], a["count"], a["vel"], a["en"], a["peaks"], a["counts"],
                                         m._stream())
        return rc, m._lib.ymt3_last_error().decode()

    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    table = [({"n_audio": -1}, "n_audio=-1 must be >= 0"), ({"audio": None}, "audio_dev is NULL"), ({"audio": off(audio, 2)}, "audio_dev is not aligned to 4 bytes"),
             ({"n": -1}, "n_notes=-1 outside [0, 536870912]"), ({"n": (1 << 29) + 1}, "n_notes=536870913 outside [0, 536870912]"),
             ({"notes": None}, "notes_dev is NULL"), ({"notes": off(rec, 4)}, "notes_dev is not aligned to 8 bytes"),
             ({"count": off(cnt, 2)}, "count_dev is not aligned to 4 bytes"), ({"vel": None}, "velocity_dev is NULL"),
             ({"en": off(en, 2)}, "energy_dev is not aligned to 4 bytes"), ({"peaks": None}, "peaks_dev is NULL"),
             ({"peaks": off(peaks, 2)}, "peaks_dev is not aligned to 4 bytes"), ({"counts": None}, "counts_dev is NULL"),
             ({"counts": off(counts, 1)}, "counts_dev is not aligned to 4 bytes"), ({"obj": None}, "null note velocity object"),
             ({"h": None}, "null handle"), ({"obj": foreign.ptr}, "the note velocity object belongs to another handle")]
    for over, text in table:
        vel.fill_(7), en.fill_(-7.0), peaks.fill_(-7.0), counts.fill_(-7)
        rc, msg = call(**over)
        assert rc == 1 and msg == text, (over, rc, msg)                    # YMT3_ERR_ARG and its text
        assert int((vel != 7).sum()) == 0 and int((en != -7.0).sum()) == 0 and int((peaks != -7.0).sum()) == 0 and int((counts != -7).sum()) == 0
        rc, msg = call()                                                    # the object's next call is right
        assert rc == 0, msg
        check(case, vel[:n], en[:n], peaks[:2], counts[:2])
        assert int((vel[n:] != 7).sum()) == 0 and int((en[n:] != -7.0).sum()) == 0 and int((peaks[2:] != -7.0).sum()) == 0 and int((counts[2:] != -7).sum()) == 0
    # n_notes = 0 only zeroes the outputs and needs no record or velocity pointer; audio of no samples needs no pointer
    vel.fill_(7), peaks.fill_(-7.0), counts.fill_(-7)
    assert call(n=0, notes=None, vel=None, en=None, count=None)[0] == 0
    assert peaks[:2].tolist() == [0.0, 0.0] and counts[:2].tolist() == [0, 0] and int((vel != 7).sum()) == 0
    assert call(audio=None, n_audio=0)[0] == 0 and counts[:2].tolist() == [n, 0] and peaks[:2].tolist() == [0.0, 0.0]
    # ymt3_velocity_create refuses what it cannot serve, and the handle goes on
    good = dict(velocity_per_db=2.0, peak_db=float("nan"), sample_rate=16000, window_samples=1024, n_harmonics=4, peak_velocity=120, min_velocity=1,
                default_velocity=100, drum_program=128)
    for change, text in [({"sample_rate": 8000}, "sample_rate=8000 != the model's sample_rate=16000"), ({"window_samples": 63}, "window_samples=63 outside [64, 4096]"),
                         ({"window_samples": 4097}, "window_samples=4097 outside [64, 4096]"), ({"n_harmonics": 0}, "n_harmonics=0 outside [1, 8]"),
                         ({"n_harmonics": 9}, "n_harmonics=9 outside [1, 8]"), ({"velocity_per_db": 0.0}, "velocity_per_db=0 must be finite and > 0"),
                         ({"velocity_per_db": -1.0}, "velocity_per_db=-1 must be finite and > 0"), ({"velocity_per_db": float("nan")}, "velocity_per_db=nan must be finite and > 0"),
                         ({"velocity_per_db": float("inf")}, "velocity_per_db=inf must be finite and > 0"), ({"peak_velocity": 0}, "peak_velocity=0 outside [1, 127]"),
                         ({"peak_velocity": 128}, "peak_velocity=128 outside [1, 127]"), ({"min_velocity": 0}, "min_velocity=0 outside [1, peak_velocity=120]"),
                         ({"min_velocity": 121}, "min_velocity=121 outside [1, peak_velocity=120]"), ({"default_velocity": 0}, "default_velocity=0 outside [1, 127]"),
                         ({"default_velocity": 128}, "default_velocity=128 outside [1, 127]"),
                         ({"peak_db": float("inf")}, "peak_db=inf must be finite, or NaN for the loudest measured note"),
                         ({"peak_db": float("-inf")}, "peak_db=-inf must be finite, or NaN for the loudest measured note"),
                         ({"drum_program": -1}, "drum_program=-1 must be >= 0")]:
        params = _lib.VelocityParams(**{**good, **change})
        obj = ctypes.c_void_p(1)
        rc = m._lib.ymt3_velocity_create(m._handle, ctypes.byref(params), ctypes.byref(obj))
        assert rc == 1 and obj.value is None and m._lib.ymt3_last_error().decode() == text, (change, rc, m._lib.ymt3_last_error().decode())
        if "sample_rate" not in change:                                     # (the wrapper takes the rate from the model)
            with pytest.raises(_lib.YMT3Error) as e:
                m.compile_note_velocity(**change)
            assert str(e.value) == "ymt3 error 1: " + text
    obj = ctypes.c_void_p(1)
    assert m._lib.ymt3_velocity_create(m._handle, None, ctypes.byref(obj)) == 1 and m._lib.ymt3_last_error().decode() == "params is NULL" and obj.value is None
    params = _lib.VelocityParams(**good)
    assert m._lib.ymt3_velocity_create(None, ctypes.byref(params), ctypes.byref(obj)) == 1 and m._lib.ymt3_last_error().decode() == "null handle"
    assert m._lib.ymt3_velocity_create(m._handle, ctypes.byref(params), None) == 1 and m._lib.ymt3_last_error().decode() == "null output pointer"
    m._lib.ymt3_velocity_destroy(None)                                     # NULL is a no-op
    m2.close()
    rc, msg = call()
    assert rc == 0, msg
    check(case, vel[:n], en[:n], peaks[:2], counts[:2])


def test_destroy_before_and_after_the_handle_and_close_with_the_model(rig):
    m2 = _model(CFG, max_batch=1)
    early = m2.compile_note_velocity()
    early.close()                                                           # before the handle's destruction
    kept = m2.compile_note_velocity(window_samples=96)
    raw = ctypes.c_void_p()
    params = _lib.VelocityParams(2.0, float("nan"), 16000, 1024, 4, 120, 1, 100, 128)
    assert m2._lib.ymt3_velocity_create(m2._handle, ctypes.byref(params), ctypes.byref(raw)) == 0 and raw.value
    assert kept in m2._owned
    m2.close()                                                              # closes `kept` with the model
    with pytest.raises(ValueError, match="^the note velocity object has been closed$"):
        kept.ptr
    m2._lib.ymt3_velocity_destroy(raw)                                      # after the handle's destruction
    # the first model is untouched
    case = _case("edges")
    m, nv = _nv(rig, case)
    check(case, *nv.run(torch.from_numpy(case["audio"]), _bytes(case["rec"]), energies=True))


def test_decode_is_the_same_before_and_after(rig):
    case = _case("n_257")
    m, nv = _nv(rig, case)
    audio = O.synthetic_audio(2, m.cfg)
    before = m.inference(audio, max_token_length=24)
    out = nv.run(torch.from_numpy(case["audio"]).cuda(), _bytes(case["rec"]).cuda(), energies=True)
    after = m.inference(audio, max_token_length=24)
    assert torch.equal(before, after)
    check(case, *out)


def _same_but_velocity(a, b):
    return len(a) == len(b) and all(dataclasses.replace(x, velocity=100) == dataclasses.replace(y, velocity=100) and x.confidence == y.confidence
                                    for x, y in zip(a, b))


def test_transcribe_with_velocities_end_to_end(rig, tmp_path):
    from yourmt3_amd.transcribe import transcribe
    m = rig[0]
    # 5 segments of the small config, as tests/test_roll.py transcribes them
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=5 * 8191), seed=3)[0].numpy()
    out = lambda name: str(tmp_path / name)
    read = lambda path: open(path, "rb").read()
    never, flat = transcribe(m, audio, bsz=2, output_dir=out("never"), return_notes=True)       # a call that never heard of the argument
    off, flat_off = transcribe(m, audio, bsz=2, output_dir=out("off"), return_notes=True, velocity=False)
    assert read(never) == read(off) and flat == flat_off and len(flat) > 0 and {n.velocity for n in flat} == {100}
    host, notes_host = transcribe(m, audio, bsz=2, output_dir=out("host"), return_notes=True, velocity=True)
    dev, notes_dev = transcribe(m, audio, bsz=2, output_dir=out("dev"), return_notes=True, velocity=True, device_detok=True)
    scored, notes_scored = transcribe(m, audio, bsz=2, output_dir=out("scored"), return_notes=True, velocity=True, device_detok=True, min_confidence=0.0)
    cont, notes_cont = transcribe(m, audio, bsz=2, output_dir=out("cont"), return_notes=True, velocity=True, continuous=True)
    assert read(host) == read(dev) == read(scored) == read(cont) != read(never)
    assert notes_host == notes_dev == notes_cont and [n.velocity for n in notes_scored] == [n.velocity for n in notes_host]
    assert _same_but_velocity(notes_host, flat) and all(n.confidence is not None for n in notes_scored)
    # admissible against the specification run on the ingested buffer
    buf = m.ingest(torch.from_numpy(audio), CFG.sample_rate).view(-1).cpu().numpy()
    from yourmt3_amd.metrics import to_records
    case = {"id": None, "audio": buf, "rec": to_records(notes_host), "params": {}, "count": None}
    spans, ref = C.admissible(case), C.reference(case)
    got = [n.velocity for n in notes_host]
    print(f"{len(got)} notes, velocities {min(got)} .. {max(got)}; {sum(g != w for g, w in zip(got, ref['vel'].tolist()))} differ from the specification's, "
          f"{sum(hi > lo for lo, hi in spans)} have more than one admissible value")
    assert all(lo <= g <= hi for g, (lo, hi) in zip(got, spans)) and max(got) == 120 and len(set(got)) > 1
    # other parameters reach the kernel; parameters without the switch are refused
    _, louder = transcribe(m, audio, bsz=2, output_dir=out("params"), return_notes=True, velocity=True, velocity_params={"peak_velocity": 127, "velocity_per_db": 1.0})
    assert max(n.velocity for n in louder) == 127 and _same_but_velocity(louder, flat)
    with pytest.raises(ValueError, match="velocity_params"):
        transcribe(m, audio, bsz=2, output_dir=out("bad"), velocity_params={})


def test_estimate_velocities_puts_the_loud_half_above_the_quiet_half(rig, tmp_path):
    from yourmt3_amd.midi import read_midi_notes, write_midi
    from yourmt3_amd.transcribe import estimate_velocities
    m = rig[0]
    t = np.arange(2 * C.SR) / C.SR
    audio = (np.where(t < 1.0, 0.05, 0.2) * np.sin(2 * np.pi * V.pitch_hz(60) * t)).astype(np.float32)     # two levels, 12.04 dB apart
    flat = [Note(0.1 + 0.2 * i, 0.25 + 0.2 * i, False, 0, 60) for i in range(5)] + [Note(1.1 + 0.2 * i, 1.25 + 0.2 * i, False, 0, 60) for i in range(4)]
    path = write_midi(flat, str(tmp_path / "flat.mid"))
    notes = estimate_velocities(m, audio, path, output_dir=str(tmp_path))
    step = int(np.rint(2.0 * 20 * math.log10(4.0)))
    assert [n.velocity for n in notes] == [120 - step] * 5 + [120] * 4 and step == 24
    back = sorted(read_midi_notes(open(tmp_path / "audio.velocity.mid", "rb").read()))
    assert [n.velocity for n in back] == [96] * 5 + [120] * 4
    assert [n.velocity for n in estimate_velocities(m, audio, flat, velocity_per_db=1.0, peak_velocity=100)] == [88] * 5 + [100] * 4
    assert estimate_velocities(m, audio, []) == []
