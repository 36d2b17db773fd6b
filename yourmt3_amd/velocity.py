"""Note velocities from the audio: how loud is each note at its onset (include/ymt3.h, note velocities).

The vocabulary carries no dynamics (its `velocity` events are 0 / 1, offset / onset), so every transcribed Note has velocity 100 until the
audio under its onset is looked at.  The rules below are this repository's own.  `note_velocities` is their host specification: plain
numpy, f64 throughout, on the same f32 samples and the same two tables the device reads.  `NoteVelocity` is the device object
(YourMT3.compile_note_velocity; yourmt3_amd/csrc/velocity.hip), which reproduces it within the tolerance DESIGN section 21 measures.

The rules.  x[0 .. n_audio) is f32 mono at `sample_rate`; samples outside that range read as 0.

  tables    window w[k] = f32(0.5 - 0.5 cos(2 pi (k + 0.5) / W)), k < W; phase steps step[p][h - 1] = uint32(rint(h f(p) / sr * 2^32)) with
            f(p) = 440 * 2^((p - 69) / 12), h = 1 .. H, kept only where h f(p) < sr / 2 and 0 ("absent") elsewhere.
  measured  a record is measured iff its onset is finite, its pitch lies in [0, 128) and it is a drum (is_drum != 0 or program ==
            drum_program) or f(pitch) < sr / 2.  Every other record gets default_velocity and energy NaN.
  window    n0 = rint(onset * sr) in f64, that one multiply, half to even; W samples from n0, whatever the note's offset; clamped in f64
            before any conversion to an integer, so a window wholly outside the audio is all zeros.
  energy    a[k] = w[k] x[n0 + k].  Window power P = 2 sum a^2 / sum w^2.  Drum: E = P.  Pitched: E = 4 sum_h |sum_k a[k] e^(-i theta)|^2 /
            (sum w)^2 over the harmonics present, theta = phi 2 pi / 2^32 with the exact integer phase word phi = (step * k) mod 2^32.  A
            steady sinusoid of amplitude A at f(p) gives E ~ A^2.  A non-finite E makes the record unmeasured after all.
  peaks     peaks[0] / peaks[1]: the largest E over the measured pitched / drum records, 0 for an empty class.  counts[0] / counts[1]:
            measured / unmeasured records.
  velocity  u = peak_velocity + velocity_per_db * (10 log10(max(E, 1e-12)) - 10 log10(max(ref, 1e-12))), ref the peak of the record's
            class or, with a finite peak_db (dB re full scale), 10^(peak_db / 10) for both classes; velocity = clamp(rint(u),
            min_velocity, 127)."""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
from typing import List, Optional, Tuple

import numpy as np

from .model import _Owned
from .task_manager import DRUM_PROGRAM, Note

DEFAULTS = dict(window_samples=1024, n_harmonics=4, velocity_per_db=2.0, peak_velocity=120, min_velocity=1, default_velocity=100,
                peak_db=float("nan"), drum_program=DRUM_PROGRAM)
MAX_HARMONICS = 8
ENERGY_FLOOR = 1e-12


def check_params(sample_rate: int, **params) -> dict:
    """the parameters with their defaults, refused (ValueError naming the parameter) outside the ranges the C ABI accepts"""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown velocity parameter(s): {sorted(unknown)}")
    p = {**DEFAULTS, **params}
    if int(sample_rate) < 1:
        raise ValueError(f"sample_rate={sample_rate} must be >= 1")
    if not 64 <= int(p["window_samples"]) <= 4096:
        raise ValueError(f"window_samples={p['window_samples']} outside [64, 4096]")
    if not 1 <= int(p["n_harmonics"]) <= MAX_HARMONICS:
        raise ValueError(f"n_harmonics={p['n_harmonics']} outside [1, {MAX_HARMONICS}]")
    if not (math.isfinite(p["velocity_per_db"]) and p["velocity_per_db"] > 0):
        raise ValueError(f"velocity_per_db={p['velocity_per_db']} must be finite and > 0")
    if not 1 <= int(p["peak_velocity"]) <= 127:
        raise ValueError(f"peak_velocity={p['peak_velocity']} outside [1, 127]")
    if not 1 <= int(p["min_velocity"]) <= int(p["peak_velocity"]):
        raise ValueError(f"min_velocity={p['min_velocity']} outside [1, peak_velocity={p['peak_velocity']}]")
    if not 1 <= int(p["default_velocity"]) <= 127:
        raise ValueError(f"default_velocity={p['default_velocity']} outside [1, 127]")
    if math.isinf(p["peak_db"]):
        raise ValueError(f"peak_db={p['peak_db']} must be finite, or NaN for the loudest measured note")
    if int(p["drum_program"]) < 0:
        raise ValueError(f"drum_program={p['drum_program']} must be >= 0")
    return p


def pitch_hz(pitch: int) -> float:
    return 440.0 * math.pow(2.0, (pitch - 69) / 12.0)


def velocity_tables(sample_rate: int, window_samples: int, n_harmonics: int):
    """-> (window f32 (W,), steps uint32 (128, n_harmonics), sum w, sum w^2): every value as ymt3_velocity_create builds it (libm's cos
    and pow, element by element, and the two sums in index order)"""
    W, H, sr = int(window_samples), int(n_harmonics), float(sample_rate)
    w = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (k + 0.5) / W) for k in range(W)], np.float64).astype(np.float32)
    steps = np.zeros((128, H), np.uint32)
    for p in range(128):
        f = pitch_hz(p)
        for h in range(1, H + 1):
            if h * f < sr / 2.0:
                steps[p, h - 1] = int(np.rint(h * f / sr * 4294967296.0))
    sw = sw2 = 0.0
    for v in w.tolist():
        sw += v
        sw2 += v * v
    return w, steps, sw, sw2


def _records(notes) -> np.ndarray:
    from .metrics import to_records
    return to_records(notes)


def note_energies(audio, sample_rate: int, notes, **params):
    """The measurement alone -> (E f64 (n,), NaN where the record is not measured; P f64 (n,), the window power of every record with a
    finite onset, NaN otherwise; is_drum bool (n,))."""
    p = check_params(sample_rate, **params)
    rec = _records(notes)
    x = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
    n_audio, sr, W, H = x.size, float(int(sample_rate)), int(p["window_samples"]), int(p["n_harmonics"])
    w, steps, sw, sw2 = velocity_tables(sample_rate, W, H)
    w64 = w.astype(np.float64)
    k = np.arange(W, dtype=np.uint64)
    E = np.full(rec.size, np.nan)
    P = np.full(rec.size, np.nan)
    drum = (rec["is_drum"] != 0) | (rec["program"] == int(p["drum_program"]))
    with np.errstate(all="ignore"):
        for i, r in enumerate(rec):
            on = float(r["onset"])
            if not math.isfinite(on):
                continue
            n0 = np.rint(np.float64(on) * np.float64(sr))
            lo = int(min(max(n0, -float(W)), float(n_audio)))               # clamped in f64: the window [lo, lo + W) meets the audio or not
            seg = np.zeros(W, np.float64)
            a0, a1 = max(lo, 0), min(lo + W, n_audio)
            if a0 < a1:
                seg[a0 - lo:a1 - lo] = x[a0:a1]
            a = w64 * seg
            P[i] = 2.0 * np.sum(a * a) / sw2
            pitch = int(r["pitch"])
            if not 0 <= pitch < 128:
                continue
            if drum[i]:
                e = P[i]
            else:
                if not pitch_hz(pitch) < sr / 2.0:
                    continue
                e = 0.0
                for h in range(H):
                    step = int(steps[pitch, h])
                    if step == 0:
                        continue
                    phi = (np.uint64(step) * k) & np.uint64(0xffffffff)
                    theta = phi.astype(np.float64) * (2.0 * math.pi / 4294967296.0)
                    re, im = np.sum(a * np.cos(theta)), -np.sum(a * np.sin(theta))
                    e += re * re + im * im
                e = 4.0 * e / (sw * sw)
            if math.isfinite(e):
                E[i] = e
    return E, P, drum


def reference_energies(peaks, peak_db: float):
    """the energy a note at peak_velocity has, per class: the class's peak, or 10^(peak_db / 10) for both"""
    if math.isfinite(peak_db):
        return [math.pow(10.0, peak_db / 10.0)] * 2
    return [float(peaks[0]), float(peaks[1])]


def velocity_of(e: float, ref: float, velocity_per_db: float, peak_velocity: int, min_velocity: int) -> int:
    u = peak_velocity + velocity_per_db * (10.0 * math.log10(max(e, ENERGY_FLOOR)) - 10.0 * math.log10(max(ref, ENERGY_FLOOR)))
    return int(min(max(np.rint(u), float(min_velocity)), 127.0))


def note_velocities(audio, sample_rate: int, notes, **params) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The host specification -> (velocities uint8 (n,), energies f64 (n,), peaks f64 (2,), counts int64 (2,)).  `audio`: f32 mono at
    `sample_rate`, any shape, read flat; `notes`: a list of Note or a NOTE_RECORD array, in any order; `params`: DEFAULTS' keys."""
    p = check_params(sample_rate, **params)
    E, _, drum = note_energies(audio, sample_rate, notes, **params)
    measured = ~np.isnan(E)
    peaks = np.array([E[measured & ~drum].max() if (measured & ~drum).any() else 0.0, E[measured & drum].max() if (measured & drum).any() else 0.0])
    ref = reference_energies(peaks, float(p["peak_db"]))
    vel = np.full(E.size, int(p["default_velocity"]), np.uint8)
    for i in np.flatnonzero(measured):
        vel[i] = velocity_of(float(E[i]), ref[int(drum[i])], float(p["velocity_per_db"]), int(p["peak_velocity"]), int(p["min_velocity"]))
    return vel, E, peaks, np.array([int(measured.sum()), int((~measured).sum())], np.int64)


class NoteVelocity(_Owned):
    """The device note velocities of one model (YourMT3.compile_note_velocity; include/ymt3.h, note velocities): the parameters and the
    two tables on the device.  `params`: DEFAULTS' keys, checked by the C ABI.  Freed by close(), by leaving a `with` block, or by the
    model's close()."""
    _destroy, _noun = "ymt3_velocity_destroy", "note velocity object"

    def __init__(self, model, **params):
        from . import _lib
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown velocity parameter(s): {sorted(unknown)}")
        self.params = {**DEFAULTS, **params}
        self.sample_rate = int(model.cfg.sample_rate)
        self._own(model)
        p = self.params
        c = _lib.VelocityParams(float(p["velocity_per_db"]), float(p["peak_db"]), self.sample_rate, int(p["window_samples"]), int(p["n_harmonics"]),
                                int(p["peak_velocity"]), int(p["min_velocity"]), int(p["default_velocity"]), int(p["drum_program"]))
        _lib.check(self._lib.ymt3_velocity_create(model._handle, ctypes.byref(c), ctypes.byref(self._c)))

    def run(self, audio, records, count=None, energies: bool = False):
        """`audio`: f32 samples at the model's rate, any shape, read flat (YourMT3.ingest's segments as they are); `records`: NOTE_RECORD
        bytes (uint8, a multiple of 32); both are uploaded if they are on the host.  `count`: an int32 device tensor whose FIRST element
        is the number of records, read on the device (a Detokenizer.run_device counts tensor as it is).
        -> (velocities uint8 (n,), peaks f32 (2,), counts int32 (2,)), with `energies=True` (velocities, energies f32 (n,), peaks,
        counts): device tensors.  Records at or beyond the count have velocity 0 and energy NaN.  Asynchronous: nothing is copied back."""
        import torch
        from . import _lib
        from .model import _ptr, _records_side
        model = self._live_model()
        if audio.dtype != torch.float32:
            raise ValueError("audio must be float32")
        audio = audio.to(model.device).contiguous().view(-1)
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        vel = torch.empty(n, device=model.device, dtype=torch.uint8)
        en = torch.empty(n, device=model.device, dtype=torch.float32)
        peaks = torch.empty(2, device=model.device, dtype=torch.float32)
        counts = torch.empty(2, device=model.device, dtype=torch.int32)
        _lib.check(self._lib.ymt3_note_velocities(model._handle, self.ptr, _ptr(audio) if audio.numel() else None, int(audio.numel()),
                                                  _ptr(rec) if n else None, n, _ptr(cnt), _ptr(vel) if n else None, _ptr(en) if n else None,
                                                  _ptr(peaks), _ptr(counts), model._stream()))
        return (vel, en, peaks, counts) if energies else (vel, peaks, counts)

    def apply(self, audio, notes: List[Note]) -> List[Note]:
        """`notes` with the velocity of each measured from `audio`: one upload of the records, one copy back of the bytes"""
        import torch
        if not notes:
            return []
        rec = torch.from_numpy(_records(list(notes)).view(np.uint8).reshape(-1).copy())
        vel = self.run(audio, rec)[0].cpu().tolist()
        return [dataclasses.replace(n, velocity=v) for n, v in zip(notes, vel)]


def estimate_velocities(model, audio_info, notes_or_mid_path, output_dir: Optional[str] = None, **params) -> List[Note]:
    """Put dynamics onto notes that have none: `notes_or_mid_path` (a list of Note, or the path of a .mid file of this audio -- a flat
    transcription, or a score carried onto the audio's time axis by align()) with every velocity measured from the audio under the
    note's onset (NoteVelocity; the rules: this module's docstring).  `audio_info` as transcribe(); `params`: DEFAULTS' keys.
    -> the notes, in their order.  With `output_dir` they are also written to <name>.velocity.mid."""
    import torch
    from .audio import load_wav_pcm
    from .midi import read_midi_notes, write_midi
    name = "audio"
    if isinstance(audio_info, dict):
        name = audio_info.get("track_name") or os.path.splitext(os.path.basename(audio_info["filepath"]))[0]
        x, sr = load_wav_pcm(audio_info["filepath"])
    elif isinstance(audio_info, str):
        name = os.path.splitext(os.path.basename(audio_info))[0]
        x, sr = load_wav_pcm(audio_info)
    else:
        x, sr = np.asarray(audio_info, dtype=np.float32), model.cfg.sample_rate
    notes = notes_or_mid_path
    if isinstance(notes, (str, os.PathLike)):
        with open(notes, "rb") as f:
            notes = read_midi_notes(f.read())
    segments = model.ingest(torch.from_numpy(np.ascontiguousarray(x)), sr)
    with model.compile_note_velocity(**params) as nv:
        out = nv.apply(segments, list(notes))
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        write_midi(out, os.path.join(output_dir, name + ".velocity.mid"))
    return out
