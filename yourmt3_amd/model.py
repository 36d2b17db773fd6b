"""Host-side mirror of the model object on the reference's inference path.

SURVEY.md section 9 (unverified recollection; nothing in /root/reference to cite) has upstream
`model/ymt3.py` exposing `inference(x, task_tokens, max_token_length)` and
`inference_file(bsz, audio_segments)` returning a list of (B, K, L) int arrays.  `YourMT3` keeps
those names and shapes; every tensor operation is a call through the C ABI (include/ymt3.h) into
the gfx950 kernels.  torch is used for device buffers and the current HIP stream only.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .config import YMT3Config, to_c
from .constraint import TokenAutomaton
from .tables import derived_tables
from .task_manager import DRUM_PROGRAM, NOTE_RECORD
from .weights import make_weights, pack_blob


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _records_side(device, label: str, rec: torch.Tensor, cnt: Optional[torch.Tensor] = None, count_label: str = ""):
    """One side of a call that reads NOTE_RECORDs -> (records on the device, their number, the count tensor on the device or None)."""
    if rec.dtype != torch.uint8 or rec.dim() != 1 or rec.numel() % NOTE_RECORD.itemsize:
        raise ValueError(f"{label} must be a 1-D uint8 tensor of {NOTE_RECORD.itemsize}-byte NOTE_RECORDs")
    rec = rec.to(device).contiguous()
    if rec.numel() and rec.data_ptr() % 8:
        rec = rec.clone()
    if cnt is not None:
        if cnt.dtype != torch.int32 or not cnt.numel():
            raise ValueError(f"{count_label} must be an int32 tensor")
        cnt = cnt.to(device)
    return rec, rec.numel() // NOTE_RECORD.itemsize, cnt


def _two_sides(device, ref_records, est_records, ref_count, est_count):
    """The reference and the estimate of PianoRoll.metrics and Aligner.align."""
    return (_records_side(device, "ref_records", ref_records, ref_count, "the count of ref_records"),
            _records_side(device, "est_records", est_records, est_count, "the count of est_records"))


class _Owned:
    """What every device object of a model shares: the C pointer, the library, a weak reference to the model, and one way to end.  A
    subclass names its C destroy function and itself; YourMT3.close() closes every object the model created (YourMT3._owned)."""
    _destroy = ""
    _noun = ""                 # "the <noun> has been closed"
    _gone = None               # "the <_gone>'s model is gone": the noun, unless the class says otherwise

    def _own(self, model: "YourMT3") -> None:
        """In every __init__, before the C create call: close() and __del__ are safe whether or not that call succeeds."""
        self._model = weakref.ref(model)
        self._lib = model._lib
        self._c = ctypes.c_void_p()
        model._owned.add(self)

    @property
    def ptr(self):
        if not self._c.value:
            raise ValueError(f"the {self._noun} has been closed")
        return self._c

    def _live_model(self) -> "YourMT3":
        model = self._model()
        if model is None:
            raise ValueError(f"the {self._gone or self._noun}'s model is gone")
        return model

    def close(self):
        if getattr(self, "_c", None) is not None and self._c.value:
            getattr(self._lib, self._destroy)(self._c)
            self._c = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecodeConstraint(_Owned):
    """A token automaton uploaded to one model's device (YourMT3.compile_constraint; include/ymt3.h, constraints).  Freed by
    close(), or by the model's close()."""
    _destroy, _noun = "ymt3_constraint_destroy", "constraint"

    def __init__(self, model: "YourMT3", automaton: TokenAutomaton):
        self.automaton = automaton
        self.n_states = automaton.n_states
        self._own(model)
        bits = np.ascontiguousarray(automaton.bits())
        nxt = np.ascontiguousarray(automaton.next, dtype=np.int32)
        _lib.check(self._lib.ymt3_constraint_create(model._handle, automaton.n_states, automaton.vocab, bits.ctypes.data,
                                                    nxt.ctypes.data, ctypes.byref(self._c)))


class Detokenizer(_Owned):
    """The device detokeniser of one model for one TaskManager (YourMT3.compile_detokenizer; include/ymt3.h, device detokeniser): the
    token table and all scratch for up to `max_segments` segments of `max_steps` columns.  Freed by close(), or by the model's close()."""
    _destroy, _noun = "ymt3_detok_destroy", "detokenizer"

    def __init__(self, model: "YourMT3", task_manager, max_segments: int, max_steps: int):
        self.max_segments, self.max_steps = int(max_segments), int(max_steps)
        self.n_channels = model.cfg.n_channels
        self._own(model)
        table = np.ascontiguousarray(task_manager.token_table(), dtype=np.uint16)
        _lib.check(self._lib.ymt3_detok_create(model._handle, table.ctypes.data, int(table.size), int(task_manager.codec.steps_per_second),
                                               DRUM_PROGRAM, self.max_segments, self.max_steps, ctypes.byref(self._c)))
        self.capacity = self.max_segments * self.n_channels * self.max_steps
        self._notes = torch.empty(self.capacity * NOTE_RECORD.itemsize, device=model.device, dtype=torch.uint8)
        self._counts = torch.zeros(2, device=model.device, dtype=torch.int32)
        self._states = weakref.WeakSet()

    def run(self, tokens: torch.Tensor, scores: Optional[torch.Tensor], start_secs: torch.Tensor, end_sec: float):
        """(n, K, L) ids (+ scores) on the device, (n,) f64 strictly increasing start times -> (records: NOTE_RECORD array, n_invalid)."""
        notes, counts = self.run_device(tokens, scores, start_secs, end_sec)
        n_notes, n_invalid = (int(v) for v in counts.cpu().tolist())
        rec = notes[:n_notes * NOTE_RECORD.itemsize].cpu().numpy().view(NOTE_RECORD)
        return rec, n_invalid

    @staticmethod
    def _inputs(model, tokens: torch.Tensor, scores: Optional[torch.Tensor], start_secs: torch.Tensor):
        """-> (tokens, scores, start times) as the C calls read them, on the device, and the tokens' n and L"""
        n, K, L = (int(v) for v in tokens.shape)
        if tokens.dtype != torch.int32:
            tokens = tokens.to(torch.int32)
        tokens = tokens.to(model.device)
        if L > 1 and tokens.stride(2) != 1:
            tokens = tokens.contiguous()
        if scores is not None:
            scores = scores.to(model.device, torch.float32)
            if tuple(scores.stride()) != tuple(tokens.stride()):         # one pair of strides serves both
                tokens, scores = tokens.contiguous(), scores.contiguous()
        return tokens, scores, start_secs.to(model.device, torch.float64).contiguous(), n, L

    def run_device(self, tokens: torch.Tensor, scores: Optional[torch.Tensor], start_secs: torch.Tensor, end_sec: float):
        """run() without the copy back -> (records: uint8 tensor of `capacity` NOTE_RECORDs, counts: int32 tensor [n_notes, n_invalid]),
        both on the device and both the detokeniser's own buffers: the next call overwrites them.  Asynchronous; the first n_notes records
        are valid, which NoteMetrics.run reads from `counts` on the device."""
        model = self._live_model()
        tokens, scores, starts, n, L = self._inputs(model, tokens, scores, start_secs)
        _lib.check(self._lib.ymt3_detokenize(model._handle, self.ptr, _ptr(tokens), _ptr(scores), n, L, tokens.stride(0), tokens.stride(1),
                                             _ptr(starts), float(end_sec), _ptr(self._notes), self.capacity, _ptr(self._counts),
                                             model._stream()))
        return self._notes, self._counts

    # ------------------------------------------------------------------ incremental form (include/ymt3.h, incremental detokeniser)
    def new_state(self, max_held: int = 16) -> "DetokState":
        """The carried state of one stream of segments for push_device / finish_device: the notes still sounding and the drum hits not
        yet final, at most `max_held` per (channel, drum pitch).  Freed by its close(), or with this detokeniser."""
        model = self._live_model()
        st = DetokState(self, model, max_held)
        self._states.add(st)
        return st

    def push_device(self, state: "DetokState", tokens: torch.Tensor, scores: Optional[torch.Tensor], start_secs: torch.Tensor, horizon_sec: float):
        """One push of (n, K, L) ids (+ scores) with their (n,) f64 start times; `horizon_sec` is the start of the next segment not yet
        pushed.  -> (records: uint8 tensor of `state.capacity` NOTE_RECORDs, counts: int32 tensor [n_notes, n_invalid, n_forced]), the
        state's own device buffers, overwritten by its next call.  Asynchronous; nothing is checked against the start times here."""
        model = self._live_model()
        tokens, scores, starts, n, L = self._inputs(model, tokens, scores, start_secs)
        _lib.check(self._lib.ymt3_detokenize_push(model._handle, self.ptr, state.ptr, _ptr(tokens) if n else None, _ptr(scores) if n else None,
                                                  n, L, tokens.stride(0), tokens.stride(1), _ptr(starts) if n else None, float(horizon_sec),
                                                  _ptr(state._notes), state.capacity, _ptr(state._counts), model._stream()))
        return state._notes, state._counts

    def finish_device(self, state: "DetokState", end_sec: float):
        """The end of the stream: every held hit, and every sounding note closed at `end_sec` -> (records, counts) as push_device."""
        model = self._live_model()
        _lib.check(self._lib.ymt3_detokenize_finish(model._handle, self.ptr, state.ptr, float(end_sec), _ptr(state._notes), state.capacity,
                                                    _ptr(state._counts), model._stream()))
        return state._notes, state._counts

    def close(self):
        for st in list(getattr(self, "_states", ())):
            st.close()
        super().close()
        self._notes = self._counts = None


class DetokState(_Owned):
    """What one stream of segments carries between Detokenizer.push_device calls (Detokenizer.new_state; include/ymt3.h, incremental
    detokeniser), with the record and counter buffers its calls write."""
    _destroy, _noun, _gone = "ymt3_detok_state_destroy", "detokenizer state", "state"

    def __init__(self, detok: Detokenizer, model: "YourMT3", max_held: int):
        self.max_held = int(max_held)
        self._own(model)
        _lib.check(self._lib.ymt3_detok_state_create(model._handle, detok.ptr, self.max_held, ctypes.byref(self._c)))
        self.carry = int(self._lib.ymt3_detok_state_carry(self._c))
        self.capacity = detok.capacity + self.carry
        self._notes = torch.empty(self.capacity * NOTE_RECORD.itemsize, device=model.device, dtype=torch.uint8)
        self._counts = torch.zeros(3, device=model.device, dtype=torch.int32)
        self.last_start = float("-inf")              # start of the last pushed segment (TaskManager.tokens_to_notes_stream checks against it)

    def reset(self) -> None:
        model = self._live_model()
        _lib.check(self._lib.ymt3_detok_state_reset(model._handle, self.ptr, model._stream()))
        self.last_start = float("-inf")

    def close(self):
        super().close()
        self._notes = self._counts = None


class Tokenizer(_Owned):
    """The device tokeniser of one model for one TaskManager (YourMT3.compile_tokenizer; include/ymt3.h, device tokeniser): the codec's
    parameter block, the program -> channel table and all scratch for up to `max_segments` segments of `max_steps` columns.  Freed by
    close(), or by the model's close()."""
    _destroy, _noun = "ymt3_tok_destroy", "tokenizer"

    def __init__(self, model: "YourMT3", task_manager, max_segments: int, max_steps: int):
        self.max_segments, self.max_steps = int(max_segments), int(max_steps)
        self.n_channels = model.cfg.n_channels
        self._own(model)
        fields, chan = task_manager.tok_params()
        self.n_programs = int(chan.size)
        params = _lib.TokParams(**fields)
        chan = np.ascontiguousarray(chan, dtype=np.uint8)
        _lib.check(self._lib.ymt3_tok_create(model._handle, ctypes.byref(params), chan.ctypes.data, self.n_programs, self.max_segments,
                                             self.max_steps, ctypes.byref(self._c)))

    def run(self, records: torch.Tensor, start_secs: torch.Tensor, end_sec: float, n_steps: Optional[int] = None):
        """NOTE_RECORD bytes on the device (uint8, a multiple of 32), (n,) f64 strictly increasing start times -> (tokens (n, K, L)
        int32, lengths (n, K) int32) on the device, L = n_steps or max_steps.  Asynchronous: nothing is copied back."""
        model = self._live_model()
        records, n_notes, _ = _records_side(model.device, "records", records)
        starts = start_secs.to(model.device, torch.float64).contiguous()
        n, L = int(starts.shape[0]), int(n_steps or self.max_steps)
        tokens = torch.empty(n, self.n_channels, L, device=model.device, dtype=torch.int32)
        lengths = torch.empty(n, self.n_channels, device=model.device, dtype=torch.int32)
        _lib.check(self._lib.ymt3_tokenize(model._handle, self.ptr, _ptr(records) if n_notes else None, n_notes, _ptr(starts) if n else None, n,
                                           float(end_sec), L, _ptr(tokens) if n else None, _ptr(lengths) if n else None, model._stream()))
        return tokens, lengths


class NoteMetrics(_Owned):
    """The device note metrics of one model (YourMT3.compile_note_metrics; include/ymt3.h, note metrics; the rules and the host
    specification: yourmt3_amd/metrics.py): the parameters and all scratch for up to `max_ref` reference and `max_est` estimated notes.
    Freed by close(), or by the model's close()."""
    _destroy, _noun = "ymt3_metrics_destroy", "note metrics object"

    def __init__(self, model: "YourMT3", n_programs: int, max_ref: int, max_est: int, drum_program: int = DRUM_PROGRAM, onset_tol: float = 0.05,
                 offset_min_tol: float = 0.05, offset_ratio: float = 0.2):
        self.n_programs, self.drum_program = int(n_programs), int(drum_program)
        self.max_ref, self.max_est = int(max_ref), int(max_est)
        self._own(model)
        params = _lib.MetricsParams(float(onset_tol), float(offset_min_tol), float(offset_ratio), self.n_programs, self.drum_program)
        _lib.check(self._lib.ymt3_metrics_create(model._handle, ctypes.byref(params), self.max_ref, self.max_est, ctypes.byref(self._c)))

    def run(self, ref_records: torch.Tensor, est_records: torch.Tensor, ref_count: Optional[torch.Tensor] = None,
            est_count: Optional[torch.Tensor] = None) -> torch.Tensor:
        """NOTE_RECORD bytes on the device (uint8, a multiple of 32) for both sides -> the ((n_programs + 1) * 6 + 2,) int32 counts tensor on
        the device (metrics.NoteMetricCounts.from_flat reads it).  `ref_count` / `est_count`: int32 device tensors whose FIRST element is
        the side's number of records, read on the device (a Detokenizer.run_device counts tensor as it is); the tensor's size is then only the
        buffer's capacity.  Asynchronous: nothing is copied back."""
        model = self._live_model()
        r, nr, rc = _records_side(model.device, "ref_records", ref_records, ref_count, "ref_count")
        e, ne, ec = _records_side(model.device, "est_records", est_records, est_count, "est_count")
        counts = torch.empty((self.n_programs + 1) * 6 + 2, device=model.device, dtype=torch.int32)
        _lib.check(self._lib.ymt3_note_metrics(model._handle, self.ptr, _ptr(r) if nr else None, nr, _ptr(rc), _ptr(e) if ne else None, ne, _ptr(ec),
                                               _ptr(counts), model._stream()))
        return counts


class PianoRoll(_Owned):
    """The device piano roll and frame metrics of one model (YourMT3.compile_piano_roll; include/ymt3.h, piano roll and frame metrics; the
    rules and the host specification: piano_roll and frame_metrics of yourmt3_amd/metrics.py): the parameters and the bit-set scratch for up
    to `max_frames` frames.  Freed by close(), or by the model's close()."""
    _destroy, _noun = "ymt3_roll_destroy", "piano roll object"

    def __init__(self, model: "YourMT3", n_programs: int, max_frames: int, frames_per_second: float = 100.0, drum_program: int = DRUM_PROGRAM):
        self.n_programs, self.drum_program = int(n_programs), int(drum_program)
        self.max_frames, self.frames_per_second = int(max_frames), float(frames_per_second)
        self._own(model)
        params = _lib.RollParams(self.frames_per_second, self.n_programs, self.drum_program)
        _lib.check(self._lib.ymt3_roll_create(model._handle, ctypes.byref(params), self.max_frames, ctypes.byref(self._c)))

    def roll(self, records: torch.Tensor, n_frames: int, count: Optional[torch.Tensor] = None, rows=None) -> torch.Tensor:
        """NOTE_RECORD bytes (uint8, a multiple of 32; on the host: uploaded) -> the (n_rows, n_frames, 128) uint8 roll on the device.
        `rows`: None for all n_programs + 1 rows, "agnostic" for the last row only, or (first_row, n_rows).  `count`: an int32 device
        tensor whose FIRST element is the number of records, read on the device (a Detokenizer.run_device counts tensor as it is).
        Asynchronous: nothing is copied back."""
        model = self._live_model()
        if rows is None:
            first, n_rows = 0, self.n_programs + 1
        elif isinstance(rows, str):
            if rows != "agnostic":
                raise ValueError(f"rows={rows!r}: None, \"agnostic\" or (first_row, n_rows)")
            first, n_rows = self.n_programs, 1
        else:
            first, n_rows = (int(v) for v in rows)
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        out = torch.empty(max(n_rows, 0), max(int(n_frames), 0), 128, device=model.device, dtype=torch.uint8)
        if int(n_frames) == 0 and n_rows > 0:                            # an empty roll has no buffer to hand over
            return out
        _lib.check(self._lib.ymt3_piano_roll(model._handle, self.ptr, _ptr(rec) if n else None, n, _ptr(cnt), int(n_frames), first, n_rows,
                                             _ptr(out) if out.numel() else None, model._stream()))
        return out

    def metrics(self, ref_records: torch.Tensor, est_records: torch.Tensor, n_frames: int, ref_count: Optional[torch.Tensor] = None,
                est_count: Optional[torch.Tensor] = None) -> torch.Tensor:
        """NOTE_RECORD bytes for both sides -> the ((n_programs + 1) * 6 + 2,) int64 counts tensor on the device
        (metrics.FrameMetricCounts.from_flat reads it).  Records and counts as roll() takes them.  Asynchronous: nothing is copied back."""
        model = self._live_model()
        (r, nr, rc), (e, ne, ec) = _two_sides(model.device, ref_records, est_records, ref_count, est_count)
        counts = torch.empty((self.n_programs + 1) * 6 + 2, device=model.device, dtype=torch.int64)
        _lib.check(self._lib.ymt3_frame_metrics(model._handle, self.ptr, _ptr(r) if nr else None, nr, _ptr(rc), _ptr(e) if ne else None, ne,
                                                _ptr(ec), int(n_frames), _ptr(counts), model._stream()))
        return counts


class Aligner(_Owned):
    """The device alignment of one model (YourMT3.compile_aligner; include/ymt3.h, alignment; the rules and the host specification: dtw_align
    and warp_notes of yourmt3_amd/metrics.py): the parameters and all scratch for sides of up to `max_frames` frames under a band of
    `band_frames`.  Freed by close(), by leaving a `with` block, or by the model's close()."""
    _destroy, _noun = "ymt3_aligner_destroy", "aligner object"

    def __init__(self, model: "YourMT3", n_programs: int, max_frames: int, frames_per_second: float = 100.0, band_frames: int = 1000,
                 drum_program: int = DRUM_PROGRAM):
        self.n_programs, self.drum_program = int(n_programs), int(drum_program)
        self.max_frames, self.frames_per_second, self.band_frames = int(max_frames), float(frames_per_second), int(band_frames)
        self._own(model)
        params = _lib.AlignParams(self.frames_per_second, self.n_programs, self.drum_program, max(min(self.band_frames, 2 ** 31 - 1), -1))
        _lib.check(self._lib.ymt3_aligner_create(model._handle, ctypes.byref(params), self.max_frames, ctypes.byref(self._c)))

    def align(self, ref_records: torch.Tensor, est_records: torch.Tensor, n_ref_frames: int, n_est_frames: int,
              ref_count: Optional[torch.Tensor] = None, est_count: Optional[torch.Tensor] = None, path: bool = False):
        """NOTE_RECORD bytes for both sides (uint8, a multiple of 32; on the host: uploaded) -> (warp, result) or, with `path=True`,
        (warp, result, path), device tensors: warp (n_ref_frames,) int32; result (4,) int64 = total, path_len, skipped ref, skipped est;
        path (n_ref_frames + n_est_frames - 1, 2) int32, of which the first path_len rows are written.  Counts as PianoRoll.metrics takes
        them.  Asynchronous: nothing is copied back."""
        model = self._live_model()
        (r, nr, rc), (e, ne, ec) = _two_sides(model.device, ref_records, est_records, ref_count, est_count)
        na, nb = int(n_ref_frames), int(n_est_frames)
        warp = torch.empty(max(na, 1), device=model.device, dtype=torch.int32)
        result = torch.empty(4, device=model.device, dtype=torch.int64)
        cells = torch.empty((max(na + nb - 1, 1), 2), device=model.device, dtype=torch.int32) if path else None
        _lib.check(self._lib.ymt3_align_notes(model._handle, self.ptr, _ptr(r) if nr else None, nr, _ptr(rc), na, _ptr(e) if ne else None, ne,
                                              _ptr(ec), nb, _ptr(warp), _ptr(cells), _ptr(result), model._stream()))
        return (warp, result, cells) if path else (warp, result)

    def warp(self, records: torch.Tensor, warp: torch.Tensor, count: Optional[torch.Tensor] = None) -> torch.Tensor:
        """NOTE_RECORD bytes and the warp of align() -> the records with W applied to onset and offset (metrics.warp_notes), a new uint8
        tensor on the device; with `count`, records past it are copied as they are.  Asynchronous."""
        model = self._live_model()
        rec, n, cnt = _records_side(model.device, "records", records, count, "the count of records")
        if warp.dtype != torch.int32 or warp.dim() != 1 or not warp.numel():
            raise ValueError("warp must be a 1-D int32 tensor of n_ref_frames elements")
        warp = warp.to(model.device).contiguous()
        out = rec.clone()
        _lib.check(self._lib.ymt3_warp_notes(model._handle, self.ptr, _ptr(out) if n else None, n, _ptr(cnt), _ptr(warp), int(warp.numel()),
                                             _ptr(out) if n else None, model._stream()))
        return out


class IngestStream(_Owned):
    """Streaming ingest of one model for one PCM format (YourMT3.compile_ingest_stream; include/ymt3.h, streaming ingest): PCM arrives
    in chunks of at most `max_chunk_frames` frames, whole segments come out as soon as their last sample is final, and all of them
    together are model.ingest() of the concatenated PCM bit for bit.  Freed by close(), or by the model's close()."""
    _destroy, _noun = "ymt3_ingest_stream_destroy", "ingest stream"

    def __init__(self, model: "YourMT3", sample_rate: int, n_channels: int, dtype, max_chunk_frames: int):
        if dtype in (torch.int16, np.int16, "int16"):
            self.dtype, fmt = torch.int16, 0
        elif dtype in (torch.float32, np.float32, "float32"):
            self.dtype, fmt = torch.float32, 1
        else:
            raise ValueError("pcm must be int16 or float32")
        self.sample_rate, self.n_channels, self.max_chunk_frames = int(sample_rate), int(n_channels), int(max_chunk_frames)
        self.segment_samples = model.cfg.segment_samples
        self._own(model)
        self._frames = self._delivered = 0          # frames pushed, segments returned: what finish() sizes its result from
        _lib.check(self._lib.ymt3_ingest_stream_create(model._handle, self.sample_rate, self.n_channels, fmt, self.max_chunk_frames,
                                                       ctypes.byref(self._c)))

    def plan(self, n_frames: int) -> int:
        """How many whole segments a push of `n_frames` frames would complete now (host arithmetic only)."""
        k = ctypes.c_int(0)
        _lib.check(self._lib.ymt3_ingest_stream_plan(self.ptr, int(n_frames), ctypes.byref(k)))
        return k.value

    def push(self, pcm: torch.Tensor) -> torch.Tensor:
        """(n_frames, n_channels) or (n_frames,) PCM of the stream's dtype -> (k, 1, S) float32: the k >= 0 segments this chunk
        completed, on the device.  Asynchronous; k is known without a synchronisation."""
        model = self._live_model()
        if pcm.dim() == 1:
            pcm = pcm[:, None]
        if pcm.dim() != 2 or int(pcm.shape[1]) != self.n_channels:
            raise ValueError(f"pcm must be (n_frames, {self.n_channels})")
        if pcm.dtype != self.dtype:
            raise ValueError(f"pcm must be {self.dtype}, got {pcm.dtype}")
        n_frames = int(pcm.shape[0])
        k = self.plan(n_frames)
        pcm = pcm.to(model.device).contiguous()
        segs = torch.empty(k, 1, self.segment_samples, device=model.device, dtype=torch.float32)
        got = ctypes.c_int(0)
        _lib.check(self._lib.ymt3_ingest_stream_push(model._handle, self.ptr, _ptr(pcm) if n_frames else None, n_frames,
                                                     _ptr(segs) if k else None, k, ctypes.byref(got), model._stream()))
        assert got.value == k
        self._frames += n_frames
        self._delivered += k
        return segs

    def finish(self):
        """-> ((k, 1, S) float32: the remaining segments, the last one zero padded; the stream's total resampled samples)."""
        model = self._live_model()
        S = self.segment_samples
        n_out, n_seg, k = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(self._lib.ymt3_ingest_plan(model._handle, self._frames, self.sample_rate, ctypes.byref(n_out), ctypes.byref(n_seg)))
        rows = n_seg.value - self._delivered
        segs = torch.empty(rows, 1, S, device=model.device, dtype=torch.float32)
        _lib.check(self._lib.ymt3_ingest_stream_finish(model._handle, self.ptr, _ptr(segs) if rows else None, rows, ctypes.byref(k),
                                                       ctypes.byref(n_out), model._stream()))
        assert k.value == rows
        self._delivered += rows
        return segs, int(n_out.value)

    def reset(self) -> None:
        """Forget the stream so far; the next push starts a new one."""
        model = self._live_model()
        _lib.check(self._lib.ymt3_ingest_stream_reset(model._handle, self.ptr, model._stream()))
        self._frames = self._delivered = 0


class YourMT3:
    def __init__(self, cfg: YMT3Config, weights: Optional[Dict[str, torch.Tensor]] = None, *, seed: int = 1234,
                 device: int = 0, max_batch: int = 64):
        if not torch.cuda.is_available():
            raise _lib.YMT3Error("no GPU visible: the MI355X HIP path cannot run (there is no CPU fallback)")
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.max_batch = int(max_batch)
        self._lib = _lib.load()
        self.weights = weights if weights is not None else make_weights(cfg, seed)
        blob = pack_blob({**self.weights, **derived_tables(self.weights, cfg)})
        self._handle = ctypes.c_void_p()
        ccfg = to_c(cfg, self.max_batch)
        # `blob` is immutable bytes: c_char_p points at its buffer (no second ~91 MB host copy); ymt3_create only reads it
        _lib.check(self._lib.ymt3_create(ctypes.byref(ccfg), ctypes.c_char_p(blob), len(blob), device, ctypes.byref(self._handle)))
        # every object created for this handle, which close() must free with it (_Owned._own adds them)
        self._owned = weakref.WeakSet()

    def close(self):
        for o in list(getattr(self, "_owned", ())):
            o.close()
        if getattr(self, "_handle", None) and self._handle.value:
            self._lib.ymt3_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    @property
    def device_bytes(self) -> int:
        return int(self._lib.ymt3_device_bytes(self._handle))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _audio2d(self, audio: torch.Tensor) -> torch.Tensor:
        if audio.dim() == 3:                       # (B, 1, S) as upstream slices it
            audio = audio[:, 0, :]
        if audio.shape[-1] != self.cfg.segment_samples:
            raise ValueError(f"segments must have {self.cfg.segment_samples} samples, got {audio.shape[-1]}")
        if audio.shape[0] > self.max_batch:
            raise ValueError(f"batch {audio.shape[0]} exceeds max_batch {self.max_batch}")
        return audio.to(self.device, torch.float32).contiguous()

    def _prompt(self, task_tokens, B: int, n_steps: int) -> Optional[torch.Tensor]:
        """task_tokens -> (B, K, P) int32 device prompt (include/ymt3.h, task prompts), or None for None.  Accepted shapes: (P,)
        for every row, (B, P) per segment (repeated over the channels) or (B, K, P); ids must lie in [0, vocab)."""
        if task_tokens is None:
            return None
        cfg = self.cfg
        t = torch.as_tensor(task_tokens)
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"task_tokens must be integer ids, got {t.dtype}")
        K = cfg.n_channels
        if t.dim() == 1:
            t = t[None, None, :].expand(B, K, t.shape[0])
        elif t.dim() == 2:
            if t.shape[0] != B:
                raise ValueError(f"task_tokens (B, P) needs B = {B} rows, got {tuple(t.shape)}")
            t = t[:, None, :].expand(B, K, t.shape[1])
        elif t.dim() == 3:
            if tuple(t.shape[:2]) != (B, K):
                raise ValueError(f"task_tokens (B, K, P) must be ({B}, {K}, P), got {tuple(t.shape)}")
        else:
            raise ValueError(f"task_tokens must be (P,), (B, P) or (B, K, P), got {tuple(t.shape)}")
        P = int(t.shape[-1])
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= cfg.vocab):
            raise ValueError(f"task_tokens ids must lie in [0, {cfg.vocab})")
        if P + n_steps > cfg.max_decode_len:
            raise ValueError(f"{P} prompt + {n_steps} emitted steps exceed max_decode_len {cfg.max_decode_len}")
        return t.to(self.device, torch.int32).contiguous()

    BEAM_MAX = 8

    def _beam_params(self, B: int, num_beams, num_return_sequences, length_penalty) -> Optional["_lib.BeamParams"]:
        """Validated ymt3_beam_params, or None for the plain greedy call (num_beams = num_return_sequences = 1).  Needs no GPU."""
        W, N = int(num_beams), int(num_return_sequences)
        if W != num_beams or N != num_return_sequences:
            raise ValueError("num_beams and num_return_sequences must be integers")
        alpha = float(length_penalty)
        if not 1 <= W <= self.BEAM_MAX:
            raise ValueError(f"num_beams={W} outside [1, {self.BEAM_MAX}]")
        if not 1 <= N <= W:
            raise ValueError(f"num_return_sequences={N} outside [1, num_beams={W}]")
        if not (alpha >= 0.0) or alpha == float("inf"):
            raise ValueError(f"length_penalty={alpha} must be finite and >= 0")
        if W == 1 and N == 1:
            return None
        if B * W > self.max_batch:
            raise ValueError(f"{B} segments x num_beams={W} need max_batch >= {B * W}, the model was created with max_batch={self.max_batch}")
        if self.cfg.n_channels * W > 255:
            raise ValueError(f"n_channels * num_beams = {self.cfg.n_channels * W} exceeds 255 rows per segment")
        return _lib.BeamParams(W, N, alpha)

    def beam_trace(self, n_steps: int, n_groups: int, num_beams: int, logits: bool = False):
        """Debug hook (needs YMT3_DEBUG_HOOKS=1 at construction): from now on beam calls record, per emitted step and group, the new
        running beams.  Returns (trace (n_steps, n_groups, W, 2) int32 = (parent, token), -1 where nothing was recorded; run (n_steps,
        n_groups, W) f32; logits (n_steps, n_groups, W, V) f32 raw logits of the running beams, or None).  W must be the calls' num_beams."""
        W = int(num_beams)
        tr = torch.full((n_steps, n_groups, W, 2), -1, device=self.device, dtype=torch.int32)
        run = torch.full((n_steps, n_groups, W), float("nan"), device=self.device, dtype=torch.float32)
        lg = torch.full((n_steps, n_groups, W, self.cfg.vocab), float("nan"), device=self.device, dtype=torch.float32) if logits else None
        _lib.check(self._lib.ymt3_debug_beam_trace(self._handle, _ptr(tr), _ptr(run), _ptr(lg), n_steps, n_groups))
        self._beam_trace = (tr, run, lg)
        return self._beam_trace

    def compile_constraint(self, automaton: TokenAutomaton) -> DecodeConstraint:
        """Validate and upload a token automaton (yourmt3_amd/constraint.py) for decode / inference(constraint=...)."""
        if automaton.vocab != self.cfg.vocab:
            raise ValueError(f"automaton vocab {automaton.vocab} != the model's {self.cfg.vocab}")
        return DecodeConstraint(self, automaton)

    def _task_steps(self, task_manager, max_steps: Optional[int]) -> int:
        """What compile_detokenizer and compile_tokenizer ask of a TaskManager -> max_steps, or its default."""
        if task_manager.num_decoding_channels != self.cfg.n_channels:
            raise ValueError("TaskManager channel count does not match the model's decoder")
        if task_manager.vocab_size != self.cfg.vocab:
            raise ValueError(f"TaskManager vocab {task_manager.vocab_size} != the model's {self.cfg.vocab}")
        return min(task_manager.max_note_token_length, self.cfg.max_decode_len) if max_steps is None else max_steps

    def compile_detokenizer(self, task_manager, max_segments: int, max_steps: Optional[int] = None) -> Detokenizer:
        """The device detokeniser for `task_manager`'s vocabulary (TaskManager.tokens_to_notes_device), with scratch for `max_segments`
        segments of up to `max_steps` columns (None: the task's max_note_token_length, at most max_decode_len)."""
        return Detokenizer(self, task_manager, max_segments, self._task_steps(task_manager, max_steps))

    def compile_tokenizer(self, task_manager, max_segments: int, max_steps: Optional[int] = None) -> Tokenizer:
        """The device tokeniser for `task_manager`'s vocabulary (TaskManager.notes_to_tokens_device), with scratch for `max_segments`
        segments of up to `max_steps` columns (None: the task's max_note_token_length, at most max_decode_len)."""
        return Tokenizer(self, task_manager, max_segments, self._task_steps(task_manager, max_steps))

    def compile_note_metrics(self, n_programs: int, max_ref: int, max_est: int, **tolerances) -> NoteMetrics:
        """The device note metrics (include/ymt3.h, note metrics) for records of `n_programs` programs, with scratch for up to `max_ref`
        reference and `max_est` estimated notes.  `tolerances`: drum_program, onset_tol, offset_min_tol, offset_ratio (metrics.note_metrics'
        defaults)."""
        return NoteMetrics(self, n_programs, max_ref, max_est, **tolerances)

    def compile_piano_roll(self, n_programs: int, max_frames: int, frames_per_second: float = 100.0, drum_program: int = DRUM_PROGRAM) -> PianoRoll:
        """The device piano roll and frame metrics (include/ymt3.h, piano roll and frame metrics) for records of `n_programs` programs,
        with bit-set scratch for up to `max_frames` frames: 32 * (n_programs + 1) bytes per frame."""
        return PianoRoll(self, n_programs, max_frames, frames_per_second, drum_program)

    def compile_aligner(self, n_programs: int, max_frames: int, frames_per_second: float = 100.0, band_frames: int = 1000,
                        drum_program: int = DRUM_PROGRAM) -> Aligner:
        """The device alignment (include/ymt3.h, alignment) for records of `n_programs` programs: banded DTW of a reference onto an
        estimate, each of up to `max_frames` frames, under a band of `band_frames`; the step bits take max_frames * (band_frames / 8 + 2)
        * 4 bytes."""
        return Aligner(self, n_programs, max_frames, frames_per_second, band_frames, drum_program)

    def compile_note_velocity(self, **params):
        """The device note velocities (include/ymt3.h, note velocities; the rules and the host specification: yourmt3_amd/velocity.py)
        at the model's sample rate.  `params`: window_samples, n_harmonics, velocity_per_db, peak_velocity, min_velocity,
        default_velocity, peak_db, drum_program (velocity.DEFAULTS).  -> a velocity.NoteVelocity, closed with the model like every
        other device object."""
        from .velocity import NoteVelocity                              # (not a name of this module: velocity.py builds on it)
        return NoteVelocity(self, **params)

    def compile_beat_tracker(self, max_frames: int, **params):
        """The device beat tracker (include/ymt3.h, beat tracking; the rules and the host specification: yourmt3_amd/beats.py) with
        scratch for up to `max_frames` frames.  `params`: frames_per_second, bpm_min, bpm_max, bpm_prior, prior_octaves, tightness,
        window_frames, hop_frames, lag_step_max, onset_cap, n_programs, drum_program (beats.DEFAULTS).  -> a beats.BeatTracker, closed
        with the model like every other device object."""
        from .beats import BeatTracker                                  # (not a name of this module: beats.py builds on it)
        return BeatTracker(self, max_frames, **params)

    def compile_bar_tracker(self, max_beats: int, max_notes: int, **params):
        """The device bar tracker (include/ymt3.h, bars and key; the rules and the host specification: yourmt3_amd/bars.py) with scratch
        for up to `max_beats` beats, for calls of up to `max_notes` records.  `params`: frames_per_second, metres, near_div, accent_cap,
        w_long, w_kick, kick_lo, kick_hi, w_accent, switch_cost, n_programs, drum_program (bars.DEFAULTS).  -> a bars.BarTracker, closed
        with the model like every other device object."""
        from .bars import BarTracker                                    # (not a name of this module: bars.py builds on it)
        return BarTracker(self, max_beats, max_notes, **params)

    def compile_chord_tracker(self, max_beats: int, max_notes: int, **params):
        """The device chord tracker (include/ymt3.h, chords; the rules and the host specification: yourmt3_amd/chords.py) with scratch
        for `max_beats` beats, taking at most `max_notes` records a call.  `params`: frames_per_second, near_div, qualities, bass_div,
        w_bass, w_none, change_cost, change_cost_down, n_programs, drum_program (chords.DEFAULTS).  -> a chords.ChordTracker, closed
        with the model at the latest."""
        from .chords import ChordTracker                                # (not a name of this module: chords.py builds on it)
        return ChordTracker(self, max_beats, max_notes, **params)

    def compile_section_tracker(self, max_beats: int, max_notes: int, **params):
        """The device section tracker (include/ymt3.h, sections; the rules and the host specification: yourmt3_amd/sections.py) with
        scratch for `max_beats` beats and calls of up to `max_notes` records.  `params`: frames_per_second, near_div, context,
        kernel_beats, min_len, peak_div, same_dist, len_num, max_sections, n_programs, drum_program (sections.DEFAULTS).  -> a
        sections.SectionTracker, closed with the model."""
        from .sections import SectionTracker                            # (not a name of this module: sections.py builds on it)
        return SectionTracker(self, max_beats, max_notes, **params)

    def compile_hand_splitter(self, max_frames: int, max_notes: int, **params):
        """The device hand splitter (include/ymt3.h, hands; the rules and the host specification: yourmt3_amd/hands.py) with scratch for
        `max_frames` frames and calls of up to `max_notes` records.  `params`: hands.DEFAULTS' keys.  -> a hands.HandSplitter, closed
        with the model."""
        from .hands import HandSplitter                                 # (not a name of this module: hands.py builds on it)
        return HandSplitter(self, max_frames, max_notes, **params)

    def compile_ingest_stream(self, sample_rate: int, n_channels: int = 1, dtype=torch.int16, max_chunk_frames: int = 1 << 16) -> IngestStream:
        """Streaming form of ingest() (include/ymt3.h, streaming ingest) for `n_channels`-channel PCM of `dtype` (int16 or float32) at
        `sample_rate`, pushed in chunks of at most `max_chunk_frames` frames."""
        return IngestStream(self, sample_rate, n_channels, dtype, max_chunk_frames)

    def _start_states(self, constraint: Optional[DecodeConstraint], start_states, B: int) -> Optional[torch.Tensor]:
        """start_states -> (B, K) int32 device tensor, or None (state 0).  (K,) is every segment's; (B, K) per segment."""
        if constraint is None:
            if start_states is not None:
                raise ValueError("start_states without a constraint")
            return None
        if start_states is None:
            return None
        K = self.cfg.n_channels
        t = torch.as_tensor(start_states)
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"start_states must be integer states, got {t.dtype}")
        if t.dim() == 1 and t.shape[0] == K:
            t = t[None, :].expand(B, K)
        elif not (t.dim() == 2 and tuple(t.shape) == (B, K)):
            raise ValueError(f"start_states must be ({K},) or ({B}, {K}), got {tuple(t.shape)}")
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= constraint.n_states):
            raise ValueError(f"start states must lie in [0, {constraint.n_states})")
        return t.to(self.device, torch.int32).contiguous()

    @property
    def last_decode_steps(self) -> int:
        """Decoder steps the last decode / inference call launched (fewer than asked for after an early stop; a task prompt's
        steps included)."""
        return int(self._lib.ymt3_last_decode_steps(self._handle))

    @property
    def merged_fallbacks(self) -> int:
        """How often this handle left the merged decode kernels for the separate launches after one gave up waiting (0 or 1)."""
        return int(self._lib.ymt3_merged_fallbacks(self._handle))

    @property
    def last_decode_chains(self) -> int:
        """Concurrent row ranges the last decode call cut its batch into (include/ymt3.h: 2 for 168-256 rows of one channel, else 1)."""
        return int(self._lib.ymt3_last_decode_chains(self._handle))

    @property
    def qkv0_table_active(self) -> bool:
        """Whether the last decode call took layer 0's q / k / v from the per-token table built at construction and launched no
        layer-0 projection (include/ymt3.h; YMT3_NO_QKV0_TABLE=1 at construction keeps the launch)."""
        return bool(self._lib.ymt3_qkv0_table_active(self._handle))

    def set_abort_recovery(self, mode: int) -> None:
        """1 (default): decode calls verify at their end that no merged kernel gave up and re-run through the separate launches if
        one did; 0: fully asynchronous calls, an aborted call's ids are INT32_MIN and the next call switches over (include/ymt3.h)."""
        _lib.check(self._lib.ymt3_set_abort_recovery(self._handle, int(mode)))

    def set_early_stop(self, interval: int) -> None:
        """Check every `interval` steps whether all rows have emitted EOS and stop decoding once they have (0 = off)."""
        _lib.check(self._lib.ymt3_set_early_stop(self._handle, int(interval)))

    # ------------------------------------------------------------------ stages (C ABI, 1:1)
    def ingest(self, pcm: torch.Tensor, sample_rate: int) -> torch.Tensor:
        """(n_frames, n_channels) or (n_frames,) int16 / float32 PCM at `sample_rate` -> (n_seg, 1, S) float32 mono
        segments at cfg.sample_rate on the device (mix, resample, slice and zero-pad in one kernel)."""
        if pcm.dim() == 1:
            pcm = pcm[:, None]
        if pcm.dim() != 2:
            raise ValueError("pcm must be (n_frames, n_channels)")
        if pcm.dtype == torch.int16:
            fmt = 0
        elif pcm.dtype == torch.float32:
            fmt = 1
        else:
            raise ValueError("pcm must be int16 or float32")
        pcm = pcm.to(self.device).contiguous()
        n_frames, n_ch = int(pcm.shape[0]), int(pcm.shape[1])
        n_out, n_seg = ctypes.c_int64(0), ctypes.c_int(0)
        _lib.check(self._lib.ymt3_ingest_plan(self._handle, n_frames, int(sample_rate), ctypes.byref(n_out), ctypes.byref(n_seg)))
        segs = torch.empty(n_seg.value, 1, self.cfg.segment_samples, device=self.device, dtype=torch.float32)
        _lib.check(self._lib.ymt3_ingest(self._handle, _ptr(pcm) if n_frames else None, fmt, n_frames, n_ch, int(sample_rate),
                                         _ptr(segs), n_seg.value, self._stream()))
        self.last_ingest_samples = int(n_out.value)
        return segs

    def logmel(self, audio: torch.Tensor) -> torch.Tensor:
        a = self._audio2d(audio)
        B = a.shape[0]
        mel = torch.empty(B, self.cfg.n_frames, self.cfg.n_mels, device=self.device, dtype=torch.float32)
        _lib.check(self._lib.ymt3_logmel(self._handle, _ptr(a), B, _ptr(mel), self._stream()))
        return mel

    def encode(self, mel: torch.Tensor) -> torch.Tensor:
        mel = mel.to(self.device, torch.float32).contiguous()
        B = mel.shape[0]
        enc = torch.empty(B, self.cfg.n_frames, self.cfg.d_model, device=self.device, dtype=torch.bfloat16)
        _lib.check(self._lib.ymt3_encode(self._handle, _ptr(mel), B, _ptr(enc), self._stream()))
        return enc

    def decode(self, enc: torch.Tensor, n_steps: Optional[int] = None, forced: Optional[torch.Tensor] = None,
               return_logits: bool = False, prompt=None, return_scores: bool = False, constraint: Optional[DecodeConstraint] = None,
               start_states=None, num_beams: int = 1, num_return_sequences: int = 1, length_penalty: float = 1.0, _force_beam: bool = False):
        """Greedy decode of n_steps emitted tokens per row; with num_beams > 1 (or num_return_sequences > 1) beam search, see below.  `prompt` ((P,), (B, P) or (B, K, P) ids): fed after the start id before
        anything is emitted (HF decoder_input_ids = [pad, *prompt]); tokens / forced / logits index emitted steps only.
        Returns tokens, then logits if `return_logits`, then scores if `return_scores`: (B, K, n_steps) f32 log-probabilities of
        the fed ids (the emitted ones, or `forced`'s), include/ymt3.h, token scores.  `constraint` (compile_constraint) with
        `start_states` ((K,) or (B, K); None: state 0): every row emits only what its automaton allows (include/ymt3.h,
        constraints); scores are then those of the masked distribution, logits stay raw.
        Beam search (include/ymt3.h, beam search; HF generate(num_beams, num_return_sequences, length_penalty, early_stopping=True)):
        tokens are (B, K, N, n_steps), best hypothesis first, and with `return_scores` the call returns (tokens, token_scores (B, K, N,
        n_steps), sequence_scores (B, K, N)).  `forced` and `return_logits` do not combine with beams.  The model needs max_batch >=
        B * num_beams.  (`_force_beam`: take the beam path for num_beams = 1 too -- greedy search through the beam kernels, for tests.)"""
        cfg = self.cfg
        enc = enc.to(self.device, torch.bfloat16).contiguous()
        B = enc.shape[0]
        bp = self._beam_params(B, num_beams, num_return_sequences, length_penalty)
        if bp is None and _force_beam:
            bp = _lib.BeamParams(1, 1, float(length_penalty))
        p = self._prompt(prompt, B, int(n_steps or 1))
        n_steps = int(n_steps or cfg.max_decode_len - (p.shape[-1] if p is not None else 0))
        if bp is not None:
            if forced is not None or return_logits:
                raise ValueError("forced ids and return_logits do not combine with beam search")
            N = bp.num_return
            tokens = torch.empty(B, cfg.n_channels, N, n_steps, device=self.device, dtype=torch.int32)
            ts = torch.empty(B, cfg.n_channels, N, n_steps, device=self.device, dtype=torch.float32) if return_scores else None
            ss = torch.empty(B, cfg.n_channels, N, device=self.device, dtype=torch.float32) if return_scores else None
            st = self._start_states(constraint, start_states, B)
            _lib.check(self._lib.ymt3_decode_beam(self._handle, _ptr(enc), B, n_steps, _ptr(p), 0 if p is None else int(p.shape[-1]),
                                                  ctypes.byref(bp), _ptr(tokens), _ptr(ss), _ptr(ts),
                                                  constraint.ptr if constraint is not None else None, _ptr(st), self._stream()))
            return (tokens, ts, ss) if return_scores else tokens
        tokens = torch.empty(B, cfg.n_channels, n_steps, device=self.device, dtype=torch.int32)
        f = forced.to(self.device, torch.int32).contiguous() if forced is not None else None
        if f is not None and tuple(f.shape) != (B, cfg.n_channels, n_steps):
            raise ValueError("forced must be (B, n_channels, n_steps)")
        lg = torch.empty(B, cfg.n_channels, n_steps, cfg.vocab, device=self.device, dtype=torch.float32) if return_logits else None
        sc = torch.empty(B, cfg.n_channels, n_steps, device=self.device, dtype=torch.float32) if return_scores else None
        st = self._start_states(constraint, start_states, B)
        if constraint is not None:
            _lib.check(self._lib.ymt3_decode_constrained(self._handle, _ptr(enc), B, n_steps, _ptr(p), 0 if p is None else int(p.shape[-1]),
                                                         _ptr(tokens), _ptr(sc), _ptr(f), _ptr(lg), constraint.ptr, _ptr(st),
                                                         self._stream()))
        elif sc is not None:
            _lib.check(self._lib.ymt3_decode_scored(self._handle, _ptr(enc), B, n_steps, _ptr(p), 0 if p is None else int(p.shape[-1]),
                                                    _ptr(tokens), _ptr(sc), _ptr(f), _ptr(lg), self._stream()))
        elif p is None:
            _lib.check(self._lib.ymt3_decode_greedy(self._handle, _ptr(enc), B, n_steps, _ptr(tokens), _ptr(f), _ptr(lg), self._stream()))
        else:
            _lib.check(self._lib.ymt3_decode_prompted(self._handle, _ptr(enc), B, n_steps, _ptr(p), int(p.shape[-1]), _ptr(tokens), _ptr(f),
                                                      _ptr(lg), self._stream()))
        out = (tokens,) + ((lg,) if return_logits else ()) + ((sc,) if return_scores else ())
        return out if len(out) > 1 else tokens

    # ------------------------------------------------------------------ sequence scoring (include/ymt3.h)
    def _score_args(self, tokens, lengths, B: int):
        """tokens -> (B, K, L) int32 on the device; lengths ("eos", None or a tensor) -> (B, K) int32 on the device, or None."""
        cfg = self.cfg
        t = torch.as_tensor(tokens)
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"tokens must be integer ids, got {t.dtype}")
        if t.dim() != 3 or tuple(t.shape[:2]) != (B, cfg.n_channels) or t.shape[2] < 1:
            raise ValueError(f"tokens must be ({B}, {cfg.n_channels}, L) with L >= 1, got {tuple(t.shape)}")
        t = t.to(self.device, torch.int32).contiguous()
        L = int(t.shape[2])
        if isinstance(lengths, str):
            if lengths != "eos":
                raise ValueError(f"lengths must be 'eos', None or a (B, K) tensor, got {lengths!r}")
            if cfg.eos_id >= 0:
                hit = t == cfg.eos_id                                           # the first EOS, inclusive; L where there is none
                lengths = torch.where(hit.any(-1), hit.int().argmax(-1) + 1, torch.full_like(hit[..., 0], L, dtype=torch.int64))
            else:
                lengths = None
        if lengths is not None:
            ln = torch.as_tensor(lengths)
            if ln.dtype.is_floating_point or ln.dtype == torch.bool or ln.dtype.is_complex:
                raise ValueError(f"lengths must be integers, got {ln.dtype}")
            if tuple(ln.shape) != (B, cfg.n_channels):
                raise ValueError(f"lengths must be ({B}, {cfg.n_channels}), got {tuple(ln.shape)}")
            lengths = ln.to(self.device, torch.int32).contiguous()
        return t, lengths

    def decode_score(self, enc: torch.Tensor, tokens: torch.Tensor, prompt=None, lengths=None, return_logits: bool = False):
        """Teacher-forced scores of GIVEN ids in one pass over all positions (include/ymt3.h, sequence scoring; HF forward with labels):
        scores (B, K, L) f32 = log_softmax(logits of position P + j)[tokens[..., j]] -- what decode(enc, L, forced=tokens,
        return_scores=True) returns after P + L dependent steps.  `prompt` as decode(); `lengths` ((B, K) ints, clamped into [0, L]):
        columns at or past a row's length score exactly 0.0 (None: every column counts).  `return_logits`: (scores, logits (B, K, L,
        vocab) f32).  Dense decoder FFN only."""
        enc = enc.to(self.device, torch.bfloat16).contiguous()
        B = enc.shape[0]
        t, ln = self._score_args(tokens, lengths, B)
        L = int(t.shape[2])
        p = self._prompt(prompt, B, L)
        sc = torch.empty(B, self.cfg.n_channels, L, device=self.device, dtype=torch.float32)
        lg = torch.empty(B, self.cfg.n_channels, L, self.cfg.vocab, device=self.device, dtype=torch.float32) if return_logits else None
        _lib.check(self._lib.ymt3_score_tokens(self._handle, _ptr(enc), B, L, _ptr(p), 0 if p is None else int(p.shape[-1]), _ptr(t),
                                               _ptr(ln), _ptr(sc), _ptr(lg), self._stream()))
        return (sc, lg) if return_logits else sc

    def score(self, audio: torch.Tensor, tokens: torch.Tensor, task_tokens=None, lengths="eos"):
        """(B, 1, S) or (B, S) audio + (B, K, L) ids -> (scores (B, K, L) f32, log_likelihood (B, K) f64): how likely is this
        transcription for this audio, the whole path in one C call.  `lengths="eos"`: a row counts up to and including its first
        eos_id (all L columns when it has none, or when eos_id < 0); None: every column; or a (B, K) integer tensor.  Columns past a
        row's length score 0.0, so log_likelihood = scores.sum(-1) is the likelihood of the sequence up to its end."""
        a = self._audio2d(audio)
        B = a.shape[0]
        t, ln = self._score_args(tokens, lengths, B)
        L = int(t.shape[2])
        p = self._prompt(task_tokens, B, L)
        sc = torch.empty(B, self.cfg.n_channels, L, device=self.device, dtype=torch.float32)
        if B:
            _lib.check(self._lib.ymt3_transcribe_segments_score(self._handle, _ptr(a), B, L, _ptr(p), 0 if p is None else int(p.shape[-1]),
                                                                _ptr(t), _ptr(ln), _ptr(sc), self._stream()))
        return sc, sc.double().sum(-1)

    # ------------------------------------------------------------------ reference-shaped API
    def inference(self, audio: torch.Tensor, task_tokens=None, max_token_length: Optional[int] = None, return_scores: bool = False,
                  constraint: Optional[DecodeConstraint] = None, start_states=None, num_beams: int = 1, num_return_sequences: int = 1,
                  length_penalty: float = 1.0):
        """(B, 1, S) or (B, S) audio -> (B, K, L) int32 token ids: the whole hot path, one C call.  `task_tokens` ((P,), (B, P) or
        (B, K, P) ids, e.g. TaskManager.task_prompt): the decoder is prompted with them and L tokens are emitted after them.
        `return_scores`: returns (tokens, scores), scores (B, K, L) f32 the log-probability of every emitted token (0.0 for the
        PAD after a row's EOS), as HF compute_transition_scores(normalize_logits=True).  `constraint` / `start_states`: as
        decode().  `num_beams` / `num_return_sequences` / `length_penalty`: beam search as in decode() -- tokens (B, K, N, L), and
        with `return_scores` (tokens, token_scores, sequence_scores)."""
        a = self._audio2d(audio)
        B = a.shape[0]
        L = int(max_token_length or self.cfg.max_decode_len)
        bp = self._beam_params(B, num_beams, num_return_sequences, length_penalty)
        p = self._prompt(task_tokens, B, L)
        if bp is not None:
            N = bp.num_return
            tokens = torch.empty(B, self.cfg.n_channels, N, L, device=self.device, dtype=torch.int32)
            ts = torch.empty(B, self.cfg.n_channels, N, L, device=self.device, dtype=torch.float32) if return_scores else None
            ss = torch.empty(B, self.cfg.n_channels, N, device=self.device, dtype=torch.float32) if return_scores else None
            st = self._start_states(constraint, start_states, B)
            if B:
                _lib.check(self._lib.ymt3_transcribe_segments_beam(
                    self._handle, _ptr(a), B, L, _ptr(p), 0 if p is None else int(p.shape[-1]), ctypes.byref(bp), _ptr(tokens), _ptr(ss),
                    _ptr(ts), constraint.ptr if constraint is not None else None, _ptr(st), self._stream()))
            return (tokens, ts, ss) if return_scores else tokens
        tokens = torch.empty(B, self.cfg.n_channels, L, device=self.device, dtype=torch.int32)
        st = self._start_states(constraint, start_states, B)
        if constraint is not None:
            scores = torch.empty(B, self.cfg.n_channels, L, device=self.device, dtype=torch.float32) if return_scores else None
            if B:
                _lib.check(self._lib.ymt3_transcribe_segments_constrained(
                    self._handle, _ptr(a), B, L, _ptr(p), 0 if p is None else int(p.shape[-1]), _ptr(tokens), _ptr(scores),
                    constraint.ptr, _ptr(st), self._stream()))
            return (tokens, scores) if return_scores else tokens
        if return_scores:
            scores = torch.empty(B, self.cfg.n_channels, L, device=self.device, dtype=torch.float32)
            if B:
                _lib.check(self._lib.ymt3_transcribe_segments_scored(self._handle, _ptr(a), B, L, _ptr(p), 0 if p is None else int(p.shape[-1]),
                                                                     _ptr(tokens), _ptr(scores), self._stream()))
            return tokens, scores
        if p is None:
            _lib.check(self._lib.ymt3_transcribe_segments(self._handle, _ptr(a), B, L, _ptr(tokens), self._stream()))
        elif B:
            _lib.check(self._lib.ymt3_transcribe_segments_prompted(self._handle, _ptr(a), B, L, _ptr(p), int(p.shape[-1]), _ptr(tokens),
                                                                   self._stream()))
        return tokens

    def inference_stream(self, audio_segments: torch.Tensor, max_token_length: Optional[int] = None, slots: int = 0,
                         interval: int = 8, task_tokens=None, return_scores: bool = False,
                         constraint: Optional[DecodeConstraint] = None, start_states=None, num_beams: int = 1,
                         num_return_sequences: int = 1, length_penalty: float = 1.0):
        """(N, 1, S) or (N, S) audio, any N -> (N, K, L) int32 ids with continuous batching: `slots` decoder slots are
        refilled from the queue as segments emit EOS (needs eos_id >= 0 to gain anything).  Ids equal inference()'s, with the
        same `task_tokens` ((P,), (N, P) or (N, K, P)).  `return_scores`: (tokens, scores) as inference().  `constraint` /
        `start_states` ((K,) or (N, K)): as inference(); each segment's rows start from its own states when it is admitted.
        Beam search (`num_beams` / `num_return_sequences` / `length_penalty`, as inference()): tokens (N, K, Nret, L), with
        `return_scores` (tokens, token_scores, sequence_scores), equal to inference()'s on the same segments; a slot then holds a
        segment's n_channels * num_beams rows and is refilled once all its groups are done, so `slots` * num_beams may not exceed
        max_batch (slots = 0: max_batch // num_beams).  (transcribe(continuous=True) still refuses beams: tests pin that refusal;
        routing it here is a two-line follow-up.)"""
        bp = self._beam_params(0, num_beams, num_return_sequences, length_penalty)
        if bp is not None:
            if int(slots) * bp.num_beams > self.max_batch:
                raise ValueError(f"slots={int(slots)} x num_beams={bp.num_beams} need max_batch >= {int(slots) * bp.num_beams}, "
                                 f"the model was created with max_batch={self.max_batch}")
            if bp.num_beams > self.max_batch:
                raise ValueError(f"num_beams={bp.num_beams} needs max_batch >= {bp.num_beams}, the model was created with max_batch={self.max_batch}")
            if self.cfg.n_channels * bp.num_beams > 255:
                raise ValueError(f"n_channels * num_beams = {self.cfg.n_channels * bp.num_beams} exceeds 255 rows per segment")
        a = audio_segments[:, 0, :] if audio_segments.dim() == 3 else audio_segments
        if a.shape[-1] != self.cfg.segment_samples:
            raise ValueError(f"segments must have {self.cfg.segment_samples} samples, got {a.shape[-1]}")
        a = a.to(self.device, torch.float32).contiguous()
        N = a.shape[0]
        L = int(max_token_length or self.cfg.max_decode_len)
        p = self._prompt(task_tokens, N, L)
        if bp is not None:
            K, Nret = self.cfg.n_channels, bp.num_return
            tokens = torch.empty(N, K, Nret, L, device=self.device, dtype=torch.int32)
            ts = torch.empty(N, K, Nret, L, device=self.device, dtype=torch.float32) if return_scores else None
            ss = torch.empty(N, K, Nret, device=self.device, dtype=torch.float32) if return_scores else None
            st = self._start_states(constraint, start_states, N)
            if N:
                _lib.check(self._lib.ymt3_transcribe_stream_beam(
                    self._handle, _ptr(a), N, L, _ptr(p), 0 if p is None else int(p.shape[-1]), ctypes.byref(bp), _ptr(tokens), _ptr(ss),
                    _ptr(ts), int(slots), int(interval), constraint.ptr if constraint is not None else None, _ptr(st), self._stream()))
            return (tokens, ts, ss) if return_scores else tokens
        tokens = torch.empty(N, self.cfg.n_channels, L, device=self.device, dtype=torch.int32)
        st = self._start_states(constraint, start_states, N)
        if constraint is not None:
            scores = torch.empty(N, self.cfg.n_channels, L, device=self.device, dtype=torch.float32) if return_scores else None
            if N:
                _lib.check(self._lib.ymt3_transcribe_stream_constrained(
                    self._handle, _ptr(a), N, L, _ptr(p), 0 if p is None else int(p.shape[-1]), _ptr(tokens), _ptr(scores), int(slots),
                    int(interval), constraint.ptr, _ptr(st), self._stream()))
            return (tokens, scores) if return_scores else tokens
        if return_scores:
            scores = torch.empty(N, self.cfg.n_channels, L, device=self.device, dtype=torch.float32)
            if N:
                _lib.check(self._lib.ymt3_transcribe_stream_scored(self._handle, _ptr(a), N, L, _ptr(p), 0 if p is None else int(p.shape[-1]),
                                                                   _ptr(tokens), _ptr(scores), int(slots), int(interval), self._stream()))
            return tokens, scores
        if p is None:
            _lib.check(self._lib.ymt3_transcribe_stream(self._handle, _ptr(a) if N else None, N, L, _ptr(tokens) if N else None,
                                                        int(slots), int(interval), self._stream()))
        elif N:
            _lib.check(self._lib.ymt3_transcribe_stream_prompted(self._handle, _ptr(a), N, L, _ptr(p), int(p.shape[-1]), _ptr(tokens),
                                                                 int(slots), int(interval), self._stream()))
        return tokens

    def inference_file(self, bsz: int, audio_segments: torch.Tensor, max_token_length: Optional[int] = None,
                       task_tokens=None, return_scores: bool = False, constraint: Optional[DecodeConstraint] = None,
                       start_states=None, num_beams: int = 1, num_return_sequences: int = 1, length_penalty: float = 1.0):
        """Split (N, 1, S) segments into batches of `bsz`; one (b, K, L) int array per batch.  `task_tokens`: (P,) for every
        segment, or (N, P) / (N, K, P), sliced with the batches.  `return_scores`: (token_batches, score_batches), the second a
        list of (b, K, L) float32 arrays (inference(return_scores=True)).  `constraint` / `start_states` ((K,) or (N, K),
        sliced with the batches): as inference().  Beam search (`num_beams` / `num_return_sequences` / `length_penalty`, as
        inference()): the arrays are (b, K, N, L), `return_scores` gives (token_batches, token_score_batches, sequence_score_batches),
        and `bsz` counts segments: the model must have been created with max_batch >= bsz * num_beams."""
        beams = self._beam_params(0, num_beams, num_return_sequences, length_penalty) is not None
        if beams and int(bsz) * int(num_beams) > self.max_batch:
            raise ValueError(f"bsz={int(bsz)} x num_beams={int(num_beams)} need max_batch >= {int(bsz) * int(num_beams)}, "
                             f"the model was created with max_batch={self.max_batch}")
        bsz = min(int(bsz), self.max_batch)
        N = audio_segments.shape[0]
        tt = None if task_tokens is None else torch.as_tensor(task_tokens)
        if tt is not None and tt.dim() > 1 and tt.shape[0] != N:
            raise ValueError(f"task_tokens has {tt.shape[0]} rows for {N} segments")
        ss = None if start_states is None else torch.as_tensor(start_states)
        if ss is not None and ss.dim() == 2 and ss.shape[0] != N:
            raise ValueError(f"start_states has {ss.shape[0]} rows for {N} segments")
        out, scores, seq_scores = [], [], []
        for i in range(0, N, bsz):
            ti = tt if tt is None or tt.dim() == 1 else tt[i:i + bsz]
            kw = {}
            if constraint is not None or ss is not None:
                kw = {"constraint": constraint, "start_states": ss if ss is None or ss.dim() != 2 else ss[i:i + bsz]}
            if beams:
                kw.update(num_beams=num_beams, num_return_sequences=num_return_sequences, length_penalty=length_penalty)
                r = self.inference(audio_segments[i:i + bsz], task_tokens=ti, max_token_length=max_token_length, return_scores=return_scores, **kw)
                if return_scores:
                    out.append(r[0].cpu().numpy()); scores.append(r[1].cpu().numpy()); seq_scores.append(r[2].cpu().numpy())
                else:
                    out.append(r.cpu().numpy())
            elif return_scores:
                t, sc = self.inference(audio_segments[i:i + bsz], task_tokens=ti, max_token_length=max_token_length, return_scores=True,
                                       **kw)
                out.append(t.cpu().numpy())
                scores.append(sc.cpu().numpy())
            else:
                out.append(self.inference(audio_segments[i:i + bsz], task_tokens=ti, max_token_length=max_token_length, **kw).cpu().numpy())
        if beams and return_scores:
            return out, scores, seq_scores
        return (out, scores) if return_scores else out

    PROFILE_CLASSES = ["qkv_cache_gemm", "self_attn", "self_o_gemm", "cross_q_gemm", "cross_attn", "cross_o_gemm",
                       "ffn_wi_gemm", "ffn_wo_gemm", "lm_head_gemm", "argmax_embed", "unsampled_span", "gemm_chain", "attn_pair", "step_layers"]

    def profile_decode(self, enc: torch.Tensor, n_steps: int, stride: int = 16) -> Dict[str, dict]:
        """Eager decode with HIP events around each kernel of every `stride`-th step (include/ymt3.h)."""
        enc = enc.to(self.device, torch.bfloat16).contiguous()
        B = enc.shape[0]
        tokens = torch.empty(B, self.cfg.n_channels, n_steps, device=self.device, dtype=torch.int32)
        ms = (ctypes.c_float * 16)()
        cnt = (ctypes.c_int32 * 16)()
        _lib.check(self._lib.ymt3_profile_decode(self._handle, _ptr(enc), B, n_steps, stride, _ptr(tokens), ms, cnt, self._stream()))
        return {n: {"ms_total": float(ms[i]), "launches": int(cnt[i])} for i, n in enumerate(self.PROFILE_CLASSES)}

    def moe_trace(self, n_steps: int) -> torch.Tensor:
        """Debug hook (needs YMT3_DEBUG_HOOKS=1 at construction, MoE decoder): from now on lock-step decode calls record the router's
        choices in the returned (n_steps, n_dec_layers, max_batch * n_channels, 2) int32 device tensor (-1 where nothing was recorded)."""
        rows = self.max_batch * self.cfg.n_channels
        self._moe_trace = torch.full((n_steps, self.cfg.n_dec_layers, rows, 2), -1, device=self.device, dtype=torch.int32)
        _lib.check(self._lib.ymt3_debug_moe_trace(self._handle, _ptr(self._moe_trace), n_steps, rows))
        return self._moe_trace

    def step_stamps(self):
        """Measurement (needs YMT3_STAMP=1 at construction): per kernel of the last decode step, in launch order:
        (class name, workgroups, first entry, last entry, first exit, last exit) in microseconds from the step's start."""
        cls = np.zeros(64, np.int32); grid = np.zeros(64, np.int32); st = np.zeros((64, 4), np.uint64)
        n = ctypes.c_int(0)
        _lib.check(self._lib.ymt3_debug_step_stamps(self._handle, cls.ctypes.data, grid.ctypes.data, st.ctypes.data, ctypes.byref(n)))
        t0 = int(st[0, 0])
        return [(self.PROFILE_CLASSES[int(cls[i])], int(grid[i])) + tuple((int(v) - t0) / 100.0 for v in st[i]) for i in range(n.value)]

    def kernel_stamps(self, kernel: int, grid: int) -> np.ndarray:
        """Measurement: (grid, 2) raw 100 MHz (entry, exit) stamps of kernel `kernel` of the last decode step."""
        out = np.zeros((grid, 2), np.uint64)
        _lib.check(self._lib.ymt3_debug_kernel_stamps(self._handle, int(kernel), out.ctypes.data, int(grid)))
        return out

    def test_gemm(self, a_bf16: torch.Tensor, w_bf16: torch.Tensor) -> torch.Tensor:
        M, K = a_bf16.shape
        N = w_bf16.shape[0]
        c = torch.empty(M, N, device=self.device, dtype=torch.float32)
        _lib.check(self._lib.ymt3_test_gemm(self._handle, _ptr(a_bf16.contiguous()), _ptr(w_bf16.contiguous()), _ptr(c), M, N, K, self._stream()))
        return c

    # ------------------------------------------------------------------ per-kernel test doors (include/ymt3.h)
    # Debug entry points: each runs ONE production launcher on caller-owned tensors.  The C side refuses what it can see from a raw pointer;
    # the extent every tensor must have is computed HERE from the shape and the strides, and a smaller tensor is refused before the call.
    def _door(self, name: str, t: torch.Tensor, dtype, need: int) -> torch.Tensor:
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name}: needs a contiguous {dtype} tensor on {self.device}")
        if need <= 0 or t.numel() < need:
            raise ValueError(f"{name}: {t.numel()} elements, the shape and strides reach {need}")
        return t

    def test_gemm_ex(self, epilogue: int, a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, M: int, N: int, K: int, lda: Optional[int] = None,
                     ldw: Optional[int] = None, ldc: Optional[int] = None, bias: Optional[torch.Tensor] = None, T: int = 0, H: int = 0,
                     n_seg: int = 0) -> torch.Tensor:
        """out (+)= a[M][K] (row stride lda) w[N][K]^T with epilogue 0 f32 (+ bias), 1 bf16, 2 bf16 relu, 3 f32 +=, 4 bf16 head-major
        [N / (H 64)][n_seg][H][T][64]; `out` is written in place (row stride ldc) and returned."""
        lda, ldw, ldc = K if lda is None else lda, K if ldw is None else ldw, N if ldc is None else ldc
        self._door("a", a, torch.bfloat16, (M - 1) * lda + K)
        self._door("w", w, torch.bfloat16, (N - 1) * ldw + K)
        self._door("out", out, torch.float32 if epilogue in (0, 3) else torch.bfloat16, M * N if epilogue == 4 else (M - 1) * ldc + N)
        if bias is not None:
            self._door("bias", bias, torch.float32, N)
        _lib.check(self._lib.ymt3_test_gemm_ex(self._handle, int(epilogue), _ptr(a), _ptr(w), _ptr(out), _ptr(bias), M, N, K, lda, ldw, ldc, T, H,
                                               n_seg, self._stream()))
        return out

    def test_rmsnorm(self, x: torch.Tensor, gain: torch.Tensor, out: torch.Tensor, M: int, d: int, eps: float) -> torch.Tensor:
        self._door("x", x, torch.float32, M * d)
        self._door("gain", gain, torch.float32, d)
        self._door("out", out, torch.bfloat16, M * d)
        _lib.check(self._lib.ymt3_test_rmsnorm(self._handle, _ptr(x), _ptr(gain), _ptr(out), M, d, float(eps), self._stream()))
        return out

    def test_enc_attention(self, q: torch.Tensor, ldq: int, k: torch.Tensor, v: torch.Tensor, ldkv: int, bias_off: torch.Tensor, out: torch.Tensor,
                           B: int, T: int, H: int) -> torch.Tensor:
        """rows q + (b T + t) ldq + 64 h, k|v + (b T + t) ldkv + 64 h; out [B T][64 H].  q, k, v may be views into one fused buffer."""
        self._door("q", q, torch.bfloat16, (B * T - 1) * ldq + H * 64)
        self._door("k", k, torch.bfloat16, (B * T - 1) * ldkv + H * 64)
        self._door("v", v, torch.bfloat16, (B * T - 1) * ldkv + H * 64)
        self._door("bias_off", bias_off, torch.float32, H * (2 * T - 1))
        self._door("out", out, torch.bfloat16, B * T * H * 64)
        _lib.check(self._lib.ymt3_test_enc_attention(self._handle, _ptr(q), ldq, _ptr(k), _ptr(v), ldkv, _ptr(bias_off), _ptr(out), B, T, H,
                                                     self._stream()))
        return out

    def test_seq_attention(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, bias_off: Optional[torch.Tensor], n_seq: int,
                           H: int, Tq: int, Tk: int, inner_n: int, q_strides, kv_strides, o_strides) -> torch.Tensor:
        """SeqAttnArgs of csrc/kernels.h; every *_strides is (outer, inner, step) in elements."""
        def reach(st, n_pos):
            last = n_seq - 1                                      # the furthest start: the last sequence, or the last of the row before it
            starts = [(s // inner_n) * st[0] + (s % inner_n) * st[1] for s in (last, last - last % inner_n - 1) if s >= 0]
            return max(starts) + (n_pos - 1) * st[2] + H * 64
        if min(n_seq, H, Tq, Tk, inner_n) <= 0 or min(tuple(q_strides) + tuple(kv_strides) + tuple(o_strides)) < 0:
            raise ValueError("counts must be positive and strides non-negative")
        self._door("q", q, torch.bfloat16, reach(q_strides, Tq))
        self._door("k", k, torch.bfloat16, reach(kv_strides, Tk))
        self._door("v", v, torch.bfloat16, reach(kv_strides, Tk))
        self._door("out", out, torch.bfloat16, reach(o_strides, Tq))
        if bias_off is not None:
            self._door("bias_off", bias_off, torch.float32, H * (2 * Tk - 1))
        a = _lib.SeqAttnArgs(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), bias_off.data_ptr() if bias_off is not None else None,
                             n_seq, H, Tq, Tk, inner_n, *[int(s) for s in tuple(q_strides) + tuple(kv_strides) + tuple(o_strides)])
        _lib.check(self._lib.ymt3_test_seq_attention(self._handle, ctypes.byref(a), self._stream()))
        return out

    def test_spec_embed(self, mel: torch.Tensor, w: torch.Tensor, pos: torch.Tensor, gain: torch.Tensor, out: torch.Tensor, n_rows: int, F: int,
                        d: int, eps: float) -> torch.Tensor:
        self._door("mel", mel, torch.float32, n_rows)
        self._door("w", w, torch.float32, d)
        self._door("pos", pos, torch.bfloat16, F * d)
        self._door("gain", gain, torch.float32, d)
        self._door("out", out, torch.bfloat16, n_rows * d)
        _lib.check(self._lib.ymt3_test_spec_embed(self._handle, _ptr(mel), _ptr(w), _ptr(pos), _ptr(gain), _ptr(out), n_rows, F, d, float(eps),
                                                  self._stream()))
        return out

    # ---- decoder step kernels (separate launches).  Everything is validated BEFORE the library is touched, so the refusals can be tested
    # without a device: geometry first (ValueError), then every tensor's extent, then the position values.
    @staticmethod
    def _need(cond: bool, text: str) -> None:
        if not cond:
            raise ValueError("needs " + text)

    def _positions(self, row_pos: Optional[torch.Tensor], step: int, row0: int, R: int, L: int) -> None:
        if row_pos is None:
            self._need(0 <= step < L, f"0 <= step < {L}")
            return
        self._door("row_pos", row_pos, torch.int32, row0 + R)
        p = row_pos[row0:row0 + R]
        self._need(bool(((p >= 0) & (p < L)).all()), f"every row_pos in [0, {L})")

    def test_dec_gemm(self, mode: int, *, W: torch.Tensor, R: int, N: int, K: int, row0: int = 0, eps: float = 1e-6,
                      x: Optional[torch.Tensor] = None, a: Optional[torch.Tensor] = None, gain: Optional[torch.Tensor] = None,
                      out_bf16: Optional[torch.Tensor] = None, out_f32: Optional[torch.Tensor] = None, kcache: Optional[torch.Tensor] = None,
                      vcache: Optional[torch.Tensor] = None, H: int = 0, L: int = 0, ssq: Optional[torch.Tensor] = None, ssq_stride: int = 0,
                      part: Optional[torch.Tensor] = None, pend_y: Optional[torch.Tensor] = None, h_out: Optional[torch.Tensor] = None,
                      table: Optional[torch.Tensor] = None, mid_rows: int = 0, step: int = 0, row_pos: Optional[torch.Tensor] = None) -> None:
        """ymt3_test_dec_gemm (include/ymt3.h): mode 0 QKV + cache append, 1 bf16, 2 bf16 relu, 3 f32 logits, 4 residual.  Every row-indexed
        tensor starts at row 0 and must reach row0 + R; outputs are written in place."""
        need, rows = self._need, row0 + R
        need(0 <= mode <= 4 and R > 0 and 0 <= row0 <= 0xffff and R <= 0xffff and N > 0 and N % 16 == 0, "a mode in 0..4, R > 0, 0 <= row0, N % 16 == 0")
        need(K == 512 if mode != 4 else K in (512, 1024, 2048), "K = 512 (mode 4: 512, 1024 or 2048)")
        need(pend_y is None or mode in (0, 3), "pend_y with modes 0 and 3 only")
        need(part is None or mode == 4, "part with mode 4 only")
        need(table is None or (mode == 0 and pend_y is None), "table with mode 0 and without pend_y only")
        need(h_out is None or (mode == 0 and pend_y is not None), "h_out with mode 0 and pend_y only")
        mid = mid_rows if mid_rows >= 0 else 512
        if mid > 0 and R >= mid:
            need(N % 64 == 0 and part is None and pend_y is None and table is None and (K == 512 or (K == 2048 and mode == 4)),
                 "a shape the mid-size tile kernel is instantiated for")
        self._door("W", W, torch.bfloat16, N * K)
        if mode == 4:
            need(N == 512, "N == 512 in mode 4")
            need(a is not None and out_f32 is not None and ssq is not None, "a, out_f32 and ssq in mode 4")
            self._door("a", a, torch.bfloat16, rows * K)
            if part is not None:
                self._door("part", part, torch.float32, rows * 8 * N)
        else:
            need(x is not None and gain is not None, "x and gain")
            self._door("x", x, torch.float32, rows * K)
            self._door("gain", gain, torch.float32, K)
            if pend_y is not None:
                self._door("pend_y", pend_y, torch.float32, 2 * rows * K)
            else:
                need(ssq is not None, "ssq")
        if ssq is not None:
            need(ssq_stride >= rows, "ssq_stride >= row0 + R")
            self._door("ssq", ssq, torch.float32, 31 * ssq_stride + rows)
        if mode == 0:
            need(H > 0 and L > 0 and N == 3 * H * 64, "N == 3 * H * 64")
            if table is not None:
                self._door("table", table, torch.bfloat16, rows * N)
            else:
                need(out_bf16 is not None and kcache is not None and vcache is not None, "out_bf16, kcache and vcache")
                self._door("out_bf16", out_bf16, torch.bfloat16, rows * H * 64)
                self._door("kcache", kcache, torch.bfloat16, rows * H * L * 64)
                self._door("vcache", vcache, torch.bfloat16, rows * H * L * 64)
                self._positions(row_pos, step, row0, R, L)
            if pend_y is not None:
                need(h_out is not None and h_out.data_ptr() != x.data_ptr(), "h_out, another buffer than x")
                self._door("h_out", h_out, torch.float32, rows * K)
        elif mode in (3, 4):
            need(out_f32 is not None, "out_f32")
            self._door("out_f32", out_f32, torch.float32, rows * N)
        else:
            need(out_bf16 is not None, "out_bf16")
            self._door("out_bf16", out_bf16, torch.bfloat16, rows * N)
        p = lambda t: t.data_ptr() if t is not None else None
        c = _lib.DecGemmArgs(p(x), p(a), p(gain), p(W), p(out_bf16), p(out_f32), p(kcache), p(vcache), p(ssq), p(part), p(pend_y), p(h_out),
                             p(table), p(row_pos), row0, R, N, K, H, L, ssq_stride, mid_rows, step, float(eps))
        _lib.check(self._lib.ymt3_test_dec_gemm(self._handle, int(mode), ctypes.byref(c), self._stream()))

    def test_dec_attention(self, *, self_attn: bool, k: torch.Tensor, v: torch.Tensor, R: int, H: int, slab_keys: int, row0: int = 0,
                           q: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                           step: int = 0, row_pos: Optional[torch.Tensor] = None, n_keys_const: int = 0, rows_per_kv: int = 1,
                           force_many: bool = False, wo: Optional[torch.Tensor] = None, opart: Optional[torch.Tensor] = None,
                           wq: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None, gain: Optional[torch.Tensor] = None,
                           ssq: Optional[torch.Tensor] = None, ssq_stride: int = 0, ipart: Optional[torch.Tensor] = None, eps: float = 1e-6,
                           anc: Optional[torch.Tensor] = None, anc_rows: int = 0, anc_pitch: int = 0, W: int = 0) -> None:
        """ymt3_test_dec_attention (include/ymt3.h).  k / v hold the slabs of kv rows 0 .. (row0 + R - 1) / rows_per_kv (beam: of rows
        0 .. row0 + R - 1, whole groups)."""
        need, rows = self._need, row0 + R
        need(R > 0 and 0 <= row0 <= 0xffff and R <= 0xffff and 1 <= H <= 255 and 1 <= slab_keys <= 0xfffff and 1 <= rows_per_kv <= 255,
             "R > 0, 0 <= row0, 1 <= H <= 255, 1 <= slab_keys, 1 <= rows_per_kv <= 255")
        many = force_many or R * H > 2048
        kv_rows = rows if anc is not None else (rows - 1) // rows_per_kv + 1
        self._door("k", k, torch.bfloat16, kv_rows * H * slab_keys * 64)
        self._door("v", v, torch.bfloat16, kv_rows * H * slab_keys * 64)
        if self_attn:
            need(q is not None and bias is not None and n_keys_const == 0, "q and bias, n_keys_const == 0 (self-attention)")
            need(wq is None and x is None and gain is None and ssq is None and ipart is None, "no fused query projection (self-attention)")
            self._door("q", q, torch.bfloat16, rows * H * 64)
            self._door("bias", bias, torch.float32, H * slab_keys)
            self._positions(row_pos, step, row0, R, slab_keys)
            if wo is not None:
                need(H == 8 and not many and anc is None and opart is not None and out is None, "H == 8, the 8-wave form, opart and no out (wo)")
                self._door("wo", wo, torch.bfloat16, 512 * H * 64)
                self._door("opart", opart, torch.float32, rows * 8 * 512)
            else:
                need(out is not None and opart is None, "out")
            if anc is not None:
                need(1 <= W <= 8 and R % W == 0 and row0 % W == 0 and rows_per_kv == 1, "1 <= W <= 8 dividing R and row0, rows_per_kv == 1 (beam)")
                need(anc_pitch % 16 == 0 and slab_keys < anc_pitch <= 48 * 1024 and rows <= anc_rows,
                     "anc_pitch % 16 == 0, slab_keys < anc_pitch <= 48 KiB, row0 + R <= anc_rows (beam)")
                self._door("anc", anc, torch.uint8, 2 * anc_rows * anc_pitch)
        else:
            need(bias is None and row_pos is None and anc is None and wo is None and opart is None and out is not None,
                 "out and neither bias, row_pos, anc nor wo (cross-attention)")
            need(1 <= n_keys_const <= min(slab_keys, 0xfff), "1 <= n_keys_const <= min(slab_keys, 4095)")
            if wq is not None:
                need(x is not None and gain is not None and not force_many, "x and gain, the 8-wave form (wq)")
                need(x.numel() % 512 == 0 and gain.numel() == 512, "residual rows of 512 elements (wq)")
                self._door("wq", wq, torch.bfloat16, H * 64 * 512)
                self._door("x", x, torch.float32, rows * 512)
                self._door("gain", gain, torch.float32, 512)
                if ipart is not None:
                    need(H == 8 and ssq is None and not many, "H == 8, no ssq, at most 2048 (row, head) pairs (ipart)")
                    self._door("ipart", ipart, torch.float32, rows * 8 * 512)
                else:
                    need(ssq is not None and ssq_stride >= rows, "ssq with ssq_stride >= row0 + R")
                    self._door("ssq", ssq, torch.float32, 31 * ssq_stride + rows)
            else:
                need(q is not None and x is None and gain is None and ssq is None and ipart is None, "q and no projection operands")
                self._door("q", q, torch.bfloat16, rows * H * 64)
        if out is not None:
            self._door("out", out, torch.bfloat16, rows * H * 64)
        p = lambda t: t.data_ptr() if t is not None else None
        c = _lib.DecAttnArgs(p(q), p(k), p(v), p(out), p(bias), p(row_pos), p(wq), p(x), p(gain), p(ssq), p(ipart), p(wo), p(opart), p(anc),
                             int(bool(self_attn)), step, n_keys_const, slab_keys, rows_per_kv, row0, R, H, slab_keys if self_attn else 0, ssq_stride,
                             int(bool(force_many)), anc_rows, anc_pitch, W, 512 if wq is not None else 0, float(eps))
        _lib.check(self._lib.ymt3_test_dec_attention(self._handle, ctypes.byref(c), self._stream()))

    def test_mc_cross_attention(self, *, x: torch.Tensor, gain: torch.Tensor, ssq: torch.Tensor, ssq_stride: int, wq: torch.Tensor,
                                k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, n_seg: int, n_channels: int, H: int, T: int, row0: int = 0,
                                eps: float = 1e-6) -> None:
        """ymt3_test_mc_cross_attention (include/ymt3.h): rows row0 + seg * n_channels + channel; k / v [n_seg][H][T][64]."""
        need = self._need
        need(0 < n_seg <= 65535 and 1 <= H <= 255 and 0 <= row0 <= 0xffff, "0 < n_seg, 1 <= H <= 255, 0 <= row0")
        need(2 <= n_channels <= 16, "2 <= n_channels <= 16")
        need(T in (128, 256, 512), "T in {128, 256, 512}")
        rows = row0 + n_seg * n_channels
        need(ssq_stride >= rows, "ssq_stride >= row0 + n_seg * n_channels")
        need(gain.numel() == 512 and x.numel() % 512 == 0, "residual rows of 512 elements")
        self._door("x", x, torch.float32, rows * 512)
        self._door("gain", gain, torch.float32, 512)
        self._door("ssq", ssq, torch.float32, 31 * ssq_stride + rows)
        self._door("wq", wq, torch.bfloat16, H * 64 * 512)
        self._door("k", k, torch.bfloat16, n_seg * H * T * 64)
        self._door("v", v, torch.bfloat16, n_seg * H * T * 64)
        self._door("out", out, torch.bfloat16, rows * H * 64)
        c = _lib.McCrossArgs(x.data_ptr(), gain.data_ptr(), ssq.data_ptr(), wq.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), row0, n_seg,
                             n_channels, H, T, ssq_stride, 512, float(eps))
        _lib.check(self._lib.ymt3_test_mc_cross_attention(self._handle, ctypes.byref(c), self._stream()))

    def test_moe_stage(self, stage: int, *, R: int, E: int, row0: int = 0, eps: float = 1e-6, fp8: bool = False,
                       ssq_stride: Optional[int] = None, h: Optional[torch.Tensor] = None, gain: Optional[torch.Tensor] = None,
                       ssq: Optional[torch.Tensor] = None, router: Optional[torch.Tensor] = None, wi: Optional[torch.Tensor] = None,
                       wo: Optional[torch.Tensor] = None, wi_q8: Optional[torch.Tensor] = None, wo_q8: Optional[torch.Tensor] = None,
                       wi_s: Optional[torch.Tensor] = None, wo_s: Optional[torch.Tensor] = None, xn: Optional[torch.Tensor] = None,
                       sel: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, hidden: Optional[torch.Tensor] = None,
                       y: Optional[torch.Tensor] = None, d_model: int = 512, d_ff: int = 2048, top_k: int = 2) -> None:
        """ymt3_test_moe_stage (include/ymt3.h): stage 0 router, 1 expert wi, 2 expert wo, 3 combine.  Every row-indexed tensor starts at row 0
        (pair-indexed ones at pair 0) and must reach row0 + R (2 (row0 + R)); outputs are written in place.  Only the tensors the stage reads
        or writes are needed."""
        need, rows = self._need, row0 + R
        need(0 <= stage <= 3, "a stage in 0..3")
        need(d_model == 512 and d_ff == 2048 and top_k == 2, "d_model == 512, d_ff == 2048, top_k == 2")
        need(2 <= E <= 16, "2 <= E <= 16")
        need(1 <= R <= 1536 and 0 <= row0 <= 0xffff, "1 <= R <= 1536, 0 <= row0")
        ssq_stride = rows if ssq_stride is None else ssq_stride
        need(ssq_stride >= rows, "ssq_stride >= row0 + R")
        bf, f32 = torch.bfloat16, torch.float32
        want = {0: ("h", "gain", "ssq", "router", "xn", "sel", "gate"),
                1: ("xn", "sel", "hidden") + (("wi_q8", "wi_s") if fp8 else ("wi",)),
                2: ("hidden", "sel", "gate", "y") + (("wo_q8", "wo_s") if fp8 else ("wo",)),
                3: ("h", "y", "ssq")}[stage]
        spec = dict(h=(h, f32, rows * d_model), gain=(gain, f32, d_model), ssq=(ssq, f32, 31 * ssq_stride + rows), router=(router, bf, E * d_model),
                    wi=(wi, bf, E * d_ff * d_model), wo=(wo, bf, E * d_ff * d_model), wi_q8=(wi_q8, torch.uint8, E * d_ff * d_model),
                    wo_q8=(wo_q8, torch.uint8, E * d_ff * d_model), wi_s=(wi_s, f32, E), wo_s=(wo_s, f32, E), xn=(xn, bf, rows * d_model),
                    sel=(sel, torch.int32, 2 * rows), gate=(gate, f32, 2 * rows), hidden=(hidden, bf, 2 * rows * d_ff), y=(y, f32, 2 * rows * d_model))
        for name in want:
            t, dtype, n = spec[name]
            need(t is not None, f"{name} in stage {stage}")
            self._door(name, t, dtype, n)
        p = lambda name: spec[name][0].data_ptr() if name in want else None
        c = _lib.MoeArgs(*[p(n) for n in ("h", "gain", "ssq", "router", "wi", "wo", "wi_q8", "wo_q8", "wi_s", "wo_s", "xn", "sel", "gate", "hidden", "y")],
                         ssq_stride, int(bool(fp8)), row0, R, E, top_k, d_model, d_ff, float(eps))
        _lib.check(self._lib.ymt3_test_moe_stage(self._handle, int(stage), ctypes.byref(c), self._stream()))

    # ---- full-sequence scoring pass (csrc/dec_seq.hip), validated before the library is touched like the decoder doors above
    def test_seq_embed(self, *, h: torch.Tensor, embed: torch.Tensor, tokens: torch.Tensor, n_rows: int, n_prompt: int, n_steps: int, V: int,
                       pad_id: int, row0: int = 0, L: Optional[int] = None, prompt: Optional[torch.Tensor] = None,
                       chan_embed: Optional[torch.Tensor] = None, n_channels: int = 1, d: int = 512) -> None:
        """ymt3_test_seq_embed (include/ymt3.h): h [n_rows * L][512] starts at the launch's first row; prompt / tokens are indexed by the
        absolute row and must reach row0 + n_rows."""
        need, rows = self._need, row0 + n_rows
        L = n_prompt + n_steps if L is None else L
        need(row0 >= 0 and n_rows >= 1 and n_prompt >= 0 and n_steps >= 1 and V >= 1 and d == 512, "0 <= row0, n_rows >= 1, n_prompt >= 0, n_steps >= 1, V >= 1, d == 512")
        need(L == n_prompt + n_steps, "L == n_prompt + n_steps")
        need(chan_embed is None or n_channels >= 1, "n_channels >= 1 with chan_embed")
        need(n_prompt == 0 or prompt is not None, "a prompt when n_prompt > 0")
        self._door("h", h, torch.float32, n_rows * L * d)
        self._door("embed", embed, torch.bfloat16, V * d)
        self._door("tokens", tokens, torch.int32, rows * n_steps)
        if n_prompt > 0:
            self._door("prompt", prompt, torch.int32, rows * n_prompt)
        if chan_embed is not None:
            self._door("chan_embed", chan_embed, torch.bfloat16, n_channels * d)
        p = lambda t: t.data_ptr() if t is not None else None
        c = _lib.SeqEmbedArgs(p(h), p(embed), p(chan_embed), p(prompt) if n_prompt > 0 else None, p(tokens), row0, n_rows, L, n_prompt, n_steps, V, d,
                              n_channels, pad_id)
        _lib.check(self._lib.ymt3_test_seq_embed(self._handle, ctypes.byref(c), self._stream()))

    def test_dec_seq_attention(self, *, causal: bool, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, n_rows: int, L: int,
                               n_keys: int, H: int, ldq: int, ldkv: int, ldo: int, kv_head: int, q_seq: int, kv_seq: int, o_seq: int,
                               row0: int = 0, rows_per_kv: int = 1, bias: Optional[torch.Tensor] = None, bias_stride: int = 0) -> None:
        """ymt3_test_dec_seq_attention (include/ymt3.h).  q / out start at the launch's first row; k / v hold the slabs of kv rows
        0 .. (row0 + n_rows - 1) / rows_per_kv.  q, k, v may be views into one fused buffer."""
        need = self._need
        need(row0 >= 0 and 1 <= n_rows <= 65535 and L >= 1 and n_keys >= 1 and rows_per_kv >= 1 and 1 <= H <= 65535,
             "0 <= row0, 1 <= n_rows <= 65535, L >= 1, n_keys >= 1, rows_per_kv >= 1, 1 <= H <= 65535")
        need(ldq >= H * 64 and ldo >= H * 64 and ldkv >= 64 and kv_head >= 64 and min(q_seq, kv_seq, o_seq) >= 0,
             "ldq, ldo >= H * 64, ldkv, kv_head >= 64, non-negative row strides")
        need(ldkv >= (H - 1) * kv_head + 64 or kv_head >= (n_keys - 1) * ldkv + 64, "ldkv >= H * 64 (kv_head == 64), or head-major slabs")
        need(all(x % 8 == 0 for x in (ldq, ldkv, ldo, kv_head, q_seq, kv_seq, o_seq)), "strides that are multiples of 8 elements")
        if causal:
            need(bias is not None and n_keys == L and L <= bias_stride, "a bias and n_keys == L <= bias_stride (causal)")
            self._door("bias", bias, torch.float32, H * bias_stride)
        else:
            need(bias is None, "no bias (cross-attention)")
        kv_rows = (row0 + n_rows - 1) // rows_per_kv + 1
        kv_reach = (kv_rows - 1) * kv_seq + (H - 1) * kv_head + (n_keys - 1) * ldkv + 64
        self._door("q", q, torch.bfloat16, (n_rows - 1) * q_seq + (L - 1) * ldq + H * 64)
        self._door("k", k, torch.bfloat16, kv_reach)
        self._door("v", v, torch.bfloat16, kv_reach)
        self._door("out", out, torch.bfloat16, (n_rows - 1) * o_seq + (L - 1) * ldo + H * 64)
        c = _lib.DecSeqAttnArgs(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), bias.data_ptr() if causal else None, q_seq, kv_seq, o_seq,
                                ldq, ldkv, ldo, kv_head, row0, n_rows, L, n_keys, rows_per_kv, H, bias_stride if causal else 0, int(bool(causal)))
        _lib.check(self._lib.ymt3_test_dec_seq_attention(self._handle, ctypes.byref(c), self._stream()))

    def test_seq_lm_head(self, *, xn: torch.Tensor, W: torch.Tensor, tokens: torch.Tensor, scores: torch.Tensor, M: int, L: int, n_prompt: int,
                         n_steps: int, V: int, row0: int = 0, lengths: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None,
                         d: int = 512) -> None:
        """ymt3_test_seq_lm_head (include/ymt3.h): xn [M][512] starts at the launch's first row; tokens / lengths / scores / logits are indexed
        by the absolute row and must reach row0 + M / L."""
        need = self._need
        need(row0 >= 0 and M >= 1 and L >= 1 and n_prompt >= 0 and n_steps >= 1 and d == 512, "0 <= row0, M >= 1, L >= 1, n_prompt >= 0, n_steps >= 1, d == 512")
        need(M % L == 0 and L == n_prompt + n_steps, "M % L == 0 and L == n_prompt + n_steps")
        need(V >= 16 and V % 16 == 0, "V a positive multiple of 16")
        rows = row0 + M // L
        self._door("xn", xn, torch.bfloat16, M * d)
        self._door("W", W, torch.bfloat16, V * d)
        self._door("tokens", tokens, torch.int32, rows * n_steps)
        self._door("scores", scores, torch.float32, rows * n_steps)
        if lengths is not None:
            self._door("lengths", lengths, torch.int32, rows)
        if logits is not None:
            self._door("logits", logits, torch.float32, rows * n_steps * V)
        p = lambda t: t.data_ptr() if t is not None else None
        c = _lib.SeqLmHeadArgs(p(xn), p(W), p(tokens), p(lengths), p(scores), p(logits), M, L, n_prompt, n_steps, V, d, row0)
        _lib.check(self._lib.ymt3_test_seq_lm_head(self._handle, ctypes.byref(c), self._stream()))

    # ---- token selection (csrc/decode.hip: argmax_embed_kernel and its companions; csrc/beam.hip), validated before the library is touched like
    # the doors above: geometry, every tensor's extent, then the VALUES the kernels follow (positions, offsets, states, next-state tables)
    TOKEN_OPS = ("decode_init", "argmax_embed", "slot_start", "slot_retire", "pad_tail", "qkv0_embed")
    BEAM_OPS = ("beam_init", "beam_select", "beam_finalize", "beam_slot_start", "beam_slot_finalize")

    def _automaton(self, c_allowed, c_next, c_start, row_state, V: int, n_states: int, rows: int, n_start: int, lo: int = 0) -> int:
        """extents and values of a raw automaton -> its words per state (0: none)"""
        need = self._need
        if c_allowed is None:
            need(c_next is None, "c_next with c_allowed only")
            words = 0
        else:
            words = (V + 31) // 32
            need(n_states >= 1 and c_next is not None and row_state is not None, "c_next, row_state and c_n_states >= 1 (c_allowed)")
            self._door("c_allowed", c_allowed, torch.int32, n_states * words)
            self._door("c_next", c_next, torch.int32, n_states * V)
            nx = c_next[:n_states * V]
            need(bool(((nx >= 0) & (nx < n_states)).all()), f"every c_next in [0, {n_states})")
        if row_state is not None:
            self._door("row_state", row_state, torch.int32, rows)
        if c_start is not None:
            need(row_state is not None and n_states >= 1 and n_start >= 1, "row_state and c_n_states >= 1 (c_start)")
            self._door("c_start", c_start, torch.int32, n_start)
        elif c_allowed is not None and n_start == 0:             # a step: the states the kernel indexes the tables with
            st = row_state[lo:rows]
            need(bool(((st >= 0) & (st < n_states)).all()), f"every row_state in [0, {n_states})")
        return words

    def test_token_step(self, op: int, *, R: int, n_steps: int, row0: int = 0, V: int = 0, d: int = 512, n_channels: int = 1, eos_id: int = -1,
                        pad_id: int = 0, n_prompt: int = 0, step: int = 0, step0: int = 0, keep_shared: bool = False,
                        logits: Optional[torch.Tensor] = None, h: Optional[torch.Tensor] = None, embed: Optional[torch.Tensor] = None,
                        chan_embed: Optional[torch.Tensor] = None, finished: Optional[torch.Tensor] = None, ssq: Optional[torch.Tensor] = None,
                        ssq_stride: int = 0, row_pos: Optional[torch.Tensor] = None, row_out: Optional[torch.Tensor] = None,
                        row_prompt: Optional[torch.Tensor] = None, row_state: Optional[torch.Tensor] = None, ticket: Optional[torch.Tensor] = None,
                        zero_sync: Optional[torch.Tensor] = None, zero_lines: int = 0, qkv0: Optional[torch.Tensor] = None,
                        q0: Optional[torch.Tensor] = None, kcache0: Optional[torch.Tensor] = None, vcache0: Optional[torch.Tensor] = None, L: int = 0,
                        tokens_out: Optional[torch.Tensor] = None, forced: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None,
                        scores_out: Optional[torch.Tensor] = None, prompt: Optional[torch.Tensor] = None, c_allowed: Optional[torch.Tensor] = None,
                        c_next: Optional[torch.Tensor] = None, c_start: Optional[torch.Tensor] = None, c_n_states: int = 0,
                        state_out: Optional[torch.Tensor] = None, first_out: int = 0, first_prompt: int = 0, from_: int = 0, v0: int = 0) -> None:
        """ymt3_test_token_step (include/ymt3.h): op 0 decode_init, 1 argmax_embed, 2 slot_start, 3 slot_retire, 4 pad_tail, 5 qkv0_embed.  Every
        row-indexed tensor starts at row 0 and must reach the launch's last row; outputs are written in place.  With keep_shared the loop
        state is the previous call's: step, step0 and the output pointers of this call are not used."""
        need = self._need
        need(0 <= op <= 5 and 1 <= R <= 0xffff and 0 <= row0 <= 0xffff and n_steps >= 1 and n_prompt >= 0, "an op in 0..5, 1 <= R, 0 <= row0, n_steps >= 1, n_prompt >= 0")
        slot = row_pos is not None
        need(slot if op in (2, 3) else (not slot or op == 1), "row_pos with ops 1, 2 and 3 only, always with 2 and 3")
        need(slot or (row_out is None and row_prompt is None), "row_out and row_prompt with row_pos only")
        rows = row0 + (n_channels if op == 2 else R)
        cells = rows * n_steps                                      # lock-step: [rows][n_steps]; slot mode: whatever the offsets reach
        if op in (0, 1, 2, 5):
            need(V >= 1 and d >= 1 and n_channels >= 1 and 0 <= pad_id < V and eos_id < V, "V, d, n_channels >= 1, pad_id in [0, V), eos_id < V")
            need(h is not None and embed is not None and ssq is not None and ssq_stride >= rows, "h, embed, ssq with ssq_stride >= the last row")
            need(op != 0 or row0 == 0, "row0 == 0 (decode_init)")
            need(op != 5 or (row0 == 0 and chan_embed is None and v0 >= 0 and v0 + R <= V), "row0 == 0, no chan_embed, [v0, v0 + R) inside [0, V) (qkv0_embed)")
            self._door("h", h, torch.float32, rows * d)
            self._door("embed", embed, torch.bfloat16, V * d)
            self._door("ssq", ssq, torch.float32, 31 * ssq_stride + rows)
            if chan_embed is not None:
                self._door("chan_embed", chan_embed, torch.bfloat16, n_channels * d)
        words = 0
        if op in (0, 1, 2):
            need(finished is not None, "finished")
            self._door("finished", finished, torch.int32, rows)
            need(c_start is None or op != 1, "c_start with the init kernels only")
            words = self._automaton(c_allowed, c_next, c_start, row_state, V, c_n_states, rows, 0 if op == 1 else (rows if op == 0 else n_channels), row0)
            if qkv0 is not None:
                need(q0 is not None and kcache0 is not None and vcache0 is not None and d == 512 and L >= 1 and chan_embed is None and n_channels == 1,
                     "q0, kcache0, vcache0, d == 512, L >= 1, one channel without chan_embed (qkv0)")
                self._door("qkv0", qkv0, torch.bfloat16, V * 1536)
                self._door("q0", q0, torch.bfloat16, rows * 512)
                self._door("kcache0", kcache0, torch.bfloat16, rows * 8 * L * 64)
                self._door("vcache0", vcache0, torch.bfloat16, rows * 8 * L * 64)
                need(op != 0 or 0 <= step0 < L, f"0 <= step0 < {L} (qkv0)")
        if slot:
            need(row_out is not None and (row_prompt is not None or (op == 1 and n_prompt == 0) or op == 3), "row_out, and row_prompt where prompts are read or written")
            self._door("row_pos", row_pos, torch.int32, rows)
            self._door("row_out", row_out, torch.int64, rows)
            if row_prompt is not None:
                self._door("row_prompt", row_prompt, torch.int64, rows)
        if op != 5 and (op != 0 or tokens_out is not None) and op != 2:
            need(tokens_out is not None, "tokens_out")
            if not slot:
                self._door("tokens_out", tokens_out, torch.int32, cells)
        if op in (0, 1) and not slot:
            for name, t, dt, n in (("forced", forced, torch.int32, cells), ("logits_out", logits_out, torch.float32, cells * V),
                                   ("scores_out", scores_out, torch.float32, cells)):
                if t is not None:
                    self._door(name, t, dt, n)
            need(n_prompt == 0 or prompt is not None, "prompt with n_prompt > 0")
            if prompt is not None and n_prompt > 0:
                self._door("prompt", prompt, torch.int32, rows * n_prompt)
        if op == 4:
            need(0 <= from_ <= n_steps, "0 <= from <= n_steps")
            if scores_out is not None:
                self._door("scores_out", scores_out, torch.float32, cells)
        if slot and op in (1, 3):
            need(forced is None and logits_out is None, "neither forced nor logits_out in slot mode")
            for name, t, dt in (("tokens_out", tokens_out, torch.int32), ("scores_out", scores_out, torch.float32)):
                if t is not None:
                    self._door(name, t, dt, n_steps)
            o, p = row_out[row0:rows], row_pos[row0:rows]
            reach = min(t.numel() for t in (tokens_out, scores_out) if t is not None)
            need(bool(((o >= 0) & (o + n_steps <= reach)).all()), "every row_out inside tokens_out (and scores_out)")
            need(bool((p >= 0).all()), "every row_pos >= 0")
            if op == 1:
                live = finished[row0:rows] == 0
                need(bool((p[live] < n_prompt + n_steps).all()), "every live row_pos < n_prompt + n_steps")
                need(qkv0 is None or bool((p[live] < L).all()), "every live row_pos < L (qkv0)")
                if n_prompt > 0:
                    need(prompt is not None, "prompt with n_prompt > 0")
                    self._door("prompt", prompt, torch.int32, n_prompt)
                    q = row_prompt[row0:rows]
                    need(bool(((q >= 0) & (q + n_prompt <= prompt.numel())).all()), "every row_prompt inside prompt")
        if op == 1:
            need(logits is not None, "logits")
            self._door("logits", logits, torch.float32, rows * V)
            need(slot or keep_shared or (0 <= step0 <= step and step - step0 - n_prompt < n_steps and (qkv0 is None or step < L)),
                 "step0 <= step, the emitted column below n_steps, step < L with qkv0")
            if ticket is not None:
                self._door("ticket", ticket, torch.int32, (R // 32 + 1) * 32)
            need((zero_sync is None) == (zero_lines == 0) and zero_lines >= 0, "zero_lines >= 1 with zero_sync, 0 without")
            if zero_sync is not None:
                self._door("zero_sync", zero_sync, torch.int32, zero_lines * 32)
        if state_out is not None:
            self._door("state_out", state_out, torch.int32, 4)
        p = lambda t: t.data_ptr() if t is not None else None
        c = _lib.TokenStepArgs(p(logits), p(h), p(embed), p(chan_embed), p(finished), p(ssq), p(row_pos), p(row_out), p(row_prompt), p(row_state),
                               p(ticket), p(zero_sync), p(qkv0), p(q0), p(kcache0), p(vcache0), p(tokens_out), p(forced), p(logits_out),
                               p(scores_out), p(prompt), p(c_allowed), p(c_next), p(c_start), p(state_out), first_out, first_prompt, ssq_stride, row0,
                               R, V, d, n_channels, eos_id, pad_id, zero_lines, 8 if qkv0 is not None else 0, L, step, step0, n_steps, n_prompt, words,
                               c_n_states, int(bool(keep_shared)), from_, v0)
        _lib.check(self._lib.ymt3_test_token_step(self._handle, int(op), ctypes.byref(c), self._stream()))

    def test_beam_step(self, op: int, *, R: int, W: int, V: int, n_steps: int, anc_rows: int, anc_pitch: int, fed_pitch: int, h: torch.Tensor,
                       embed: torch.Tensor, finished: torch.Tensor, ssq: torch.Tensor, ssq_stride: int, anc: torch.Tensor, slot_anc: torch.Tensor,
                       fed_tok: torch.Tensor, fed_lp: torch.Tensor, run: torch.Tensor, fin_score: torch.Tensor, fin_len: torch.Tensor,
                       fin_store: torch.Tensor, fin_tok: torch.Tensor, fin_lp: torch.Tensor, n_fin: torch.Tensor, d: int = 512, n_channels: int = 1,
                       eos_id: int = -1, pad_id: int = 0, n_prompt: int = 0, step: int = 0, keep_shared: bool = False, N: int = 1, row0: int = 0,
                       alpha: float = 1.0, first_group: int = 0, logits: Optional[torch.Tensor] = None, chan_embed: Optional[torch.Tensor] = None,
                       row_state: Optional[torch.Tensor] = None, row_pos: Optional[torch.Tensor] = None, row_out: Optional[torch.Tensor] = None,
                       row_prompt: Optional[torch.Tensor] = None, prompt: Optional[torch.Tensor] = None, c_allowed: Optional[torch.Tensor] = None,
                       c_next: Optional[torch.Tensor] = None, c_start: Optional[torch.Tensor] = None, c_n_states: int = 0,
                       tokens_out: Optional[torch.Tensor] = None, seq_out: Optional[torch.Tensor] = None, tok_out: Optional[torch.Tensor] = None,
                       state_out: Optional[torch.Tensor] = None, n_queue: int = 0) -> None:
        """ymt3_test_beam_step (include/ymt3.h): op 0 beam_init, 1 beam_select, 2 beam_finalize, 3 beam_slot_start, 4 beam_slot_finalize over
        rows [0, R) = R / W groups.  n_queue (slot mode): the groups the result tensors hold (row_out must stay below it)."""
        need = self._need
        need(0 <= op <= 4 and 1 <= W <= 8 and 1 <= R <= 0xffff and R % W == 0 and R <= anc_rows, "an op in 0..4, 1 <= W <= 8 dividing R, R <= anc_rows")
        need(V >= 1 and d >= 1 and n_channels >= 1 and 0 <= pad_id < V and eos_id < V and ssq_stride >= R, "V, d, n_channels >= 1, pad_id in [0, V), eos_id < V, ssq_stride >= R")
        need(n_steps >= 1 and n_prompt >= 0 and anc_pitch % 16 == 0 and anc_pitch <= 48 * 1024 and n_prompt + n_steps < min(anc_pitch, fed_pitch),
             "n_prompt + n_steps below anc_pitch (a multiple of 16, at most 48 KiB) and fed_pitch")
        need(1 <= N <= W and 0.0 <= alpha <= 16.0, "1 <= N <= W, 0 <= alpha <= 16")
        slot = row_pos is not None
        need(slot if op in (3, 4) else (not slot or op == 1), "row_pos with ops 1, 3 and 4 only, always with 3 and 4")
        G = R // W
        self._door("h", h, torch.float32, R * d)
        self._door("embed", embed, torch.bfloat16, V * d)
        self._door("ssq", ssq, torch.float32, 31 * ssq_stride + R)
        self._door("anc", anc, torch.uint8, 2 * anc_rows * anc_pitch)
        self._door("slot_anc", slot_anc, torch.uint8, R * anc_pitch)
        self._door("fed_tok", fed_tok, torch.int32, R * fed_pitch)
        self._door("fed_lp", fed_lp, torch.float32, R * fed_pitch)
        for name, t, dt in (("finished", finished, torch.int32), ("run", run, torch.float32), ("fin_score", fin_score, torch.float32),
                            ("fin_len", fin_len, torch.int32), ("fin_store", fin_store, torch.int32), ("fin_tok", fin_tok, torch.int32),
                            ("fin_lp", fin_lp, torch.float32)):
            self._door(name, t, dt, R)
        self._door("n_fin", n_fin, torch.int32, G)
        if chan_embed is not None:
            self._door("chan_embed", chan_embed, torch.bfloat16, n_channels * d)
        need(c_start is None or op in (0, 3), "c_start with the init kernels only")
        words = self._automaton(c_allowed, c_next, c_start, row_state, V, c_n_states, R, 0 if op not in (0, 3) else (G if op == 0 else n_channels))
        if slot:
            need(row_out is not None and row_prompt is not None, "row_out and row_prompt (slot mode)")
            for name, t in (("row_pos", row_pos), ("row_out", row_out), ("row_prompt", row_prompt)):
                self._door(name, t, torch.int32 if t is row_pos else torch.int64, R)
            need(op == 1 or (row0 >= 0 and row0 % (n_channels * W) == 0 and row0 + n_channels * W <= R), "row0 a slot boundary inside [0, R)")
            n_groups = n_queue
            need(op != 3 or (first_group >= 0 and first_group + n_channels <= n_queue), "the slot's queue indices below n_queue")
            # what the launch follows: a stopped group (finished != 0: done, or an empty slot) reads neither its offsets nor its position
            live = (finished[:R] == 0) if op == 1 else None
            if op in (1, 4):
                o = row_out[:R][live] if op == 1 else row_out[row0:row0 + n_channels * W]
                need(bool(((o >= 0) & (o < n_queue)).all()), "every row_out in [0, n_queue)")
            if op == 1:
                p = row_pos[:R][live]
                need(bool(((p >= 0) & (p < n_prompt + n_steps)).all()), "every live row_pos in [0, n_prompt + n_steps)")
        else:
            n_groups = G
        if n_prompt > 0:
            need(prompt is not None, "prompt with n_prompt > 0")
            self._door("prompt", prompt, torch.int32, n_groups * n_prompt)
            if slot and op == 1:
                q = row_prompt[:R][live]
                need(bool(((q >= 0) & (q + n_prompt <= prompt.numel())).all()), "every row_prompt inside prompt")
        if op == 0 or not keep_shared:
            need(tokens_out is not None, "tokens_out")
            self._door("tokens_out", tokens_out, torch.int32, n_groups * N * n_steps)
            if seq_out is not None:
                self._door("seq_out", seq_out, torch.float32, n_groups * N)
            if tok_out is not None:
                self._door("tok_out", tok_out, torch.float32, n_groups * N * n_steps)
        if op == 1:
            need(logits is not None, "logits")
            self._door("logits", logits, torch.float32, R * V)
            need(slot or keep_shared or (0 <= step and step - n_prompt < n_steps), "0 <= step, the emitted column below n_steps")
        if op in (2, 4):
            lo, hi = (0, R) if op == 2 else (row0, row0 + n_channels * W)
            fs, fl = fin_store[lo:hi], fin_len[lo:hi]
            need(bool(((fs >= 0) & (fs < W)).all()) and bool(((fl >= 0) & (fl <= n_steps)).all()), "fin_store in [0, W), fin_len in [0, n_steps]")
        if state_out is not None:
            self._door("state_out", state_out, torch.int32, 4)
        p = lambda t: t.data_ptr() if t is not None else None
        c = _lib.BeamStepArgs(p(logits), p(h), p(embed), p(chan_embed), p(finished), p(ssq), p(row_state), p(anc), p(fed_tok), p(fed_lp), p(run),
                              p(fin_score), p(fin_len), p(fin_store), p(fin_tok), p(fin_lp), p(n_fin), p(slot_anc), p(row_pos), p(row_out),
                              p(row_prompt), p(prompt), p(c_allowed), p(c_next), p(c_start), p(tokens_out), p(seq_out), p(tok_out), p(state_out),
                              first_group, ssq_stride, R, V, d, n_channels, eos_id, pad_id, W, anc_rows, anc_pitch, fed_pitch, step, n_steps, n_prompt,
                              words, c_n_states, int(bool(keep_shared)), N, row0, float(alpha))
        _lib.check(self._lib.ymt3_test_beam_step(self._handle, int(op), ctypes.byref(c), self._stream()))
