"""Beam search under continuous batching, CPU side (include/ymt3.h, ymt3_transcribe_stream_beam): the ABI surface, the wrapper's argument
checks and the host model of the slot scheduler that the GPU test's step counts come from."""
import ctypes
import os
import re

import numpy as np
import pytest

from beam_stream_model import lockstep_steps, stream_steps
from yourmt3_amd.config import YMT3Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ymt3_transcribe_stream_beam"


def test_header_library_and_binding_agree_on_the_entry_point():
    h = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    assert "#define YMT3_ABI_VERSION 3" in h
    body = h[h.index('extern "C" {'):h.rindex("#ifdef __cplusplus")]
    m = re.search(r"\bint " + NAME + r"\(([^;]*?)\);", body, re.S)
    assert m, "the header does not declare " + NAME
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 15, params
    assert params[0] == "ymt3_handle h" and params[6] == "const ymt3_beam_params* params" and params[10:12] == ["int slots", "int interval"]
    assert params[-1] == "void* stream"
    # the combination is no longer listed as unsupported; what the beam tests look for in the header is still there
    unsupported = h[h.index("- not supported:"):]
    unsupported = unsupported[:unsupported.index("\n * Rows:")]
    assert "stream" not in unsupported, unsupported
    for word in ("lower flat index", "num_beams <= 8", "early_stopping False", "255"):
        assert word in h, word
    from yourmt3_amd import _lib
    from yourmt3_amd.build import build
    raw = ctypes.CDLL(build())
    assert hasattr(raw, NAME) and NAME in _lib.SYMBOLS
    raw.ymt3_abi_version.restype = ctypes.c_int
    assert raw.ymt3_abi_version() == 3
    src = open(os.path.join(ROOT, "yourmt3_amd", "_lib.py")).read()
    m = re.search(r"lib\." + NAME + r"\.argtypes = \[(.*?)\]", src)
    assert m and len(m.group(1).split(",")) == 15


def test_inference_stream_rejects_bad_beam_arguments_without_a_gpu():
    from yourmt3_amd.model import YourMT3
    m = YourMT3.__new__(YourMT3)                        # argument checks only: no handle, no device
    m.cfg, m.max_batch = YMT3Config(segment_samples=8191, max_decode_len=64), 8
    audio = np.zeros((3, 8191), np.float32)             # (never touched: the checks come first)
    for kw in (dict(num_beams=0), dict(num_beams=9), dict(num_beams=4, num_return_sequences=5), dict(num_beams=4, num_return_sequences=0),
               dict(num_beams=4, length_penalty=-0.5), dict(num_beams=4, length_penalty=float("nan")),
               dict(num_beams=4, length_penalty=float("inf")), dict(num_beams=2.5)):
        with pytest.raises(ValueError):
            m.inference_stream(audio, **kw)
    with pytest.raises(ValueError, match=r"slots=3.*num_beams=4.*max_batch >= 12.*max_batch=8"):
        m.inference_stream(audio, slots=3, num_beams=4)
    m.max_batch = 2
    with pytest.raises(ValueError, match=r"num_beams=4.*max_batch=2"):
        m.inference_stream(audio, num_beams=4)
    m.cfg, m.max_batch = YMT3Config(segment_samples=8191, max_decode_len=64, n_channels=64), 8
    with pytest.raises(ValueError, match="255"):
        m.inference_stream(audio, num_beams=4)


DONE = [24, 3, 17, 0, 9, 24, 5]                          # the GPU test's queue: emitted step at which each segment's groups are done


def test_scheduler_model_on_hand_worked_cases():
    # one slot: the segments run one after the other, each for the first multiple of the interval that covers its d + 1 steps
    assert stream_steps([5], 1, 4) == 8 and stream_steps([3], 1, 4) == 4 and stream_steps([4], 1, 4) == 8
    assert stream_steps([5, 0, 7], 1, 4) == 8 + 4 + 8
    assert stream_steps([5, 0, 7], 1, 1) == 6 + 1 + 8
    assert stream_steps([5, 0, 7], 1, 4, n_prompt=3) == 12 + 4 + 12         # 9, 4 and 11 steps
    assert stream_steps([], 4, 4) == 0
    # more slots than segments: the slowest segment decides; interval 0 means 8; slots <= 0 means "as many as there are segments"
    assert stream_steps([5, 0, 7], 8, 4) == 8 and stream_steps([5, 0, 7], 8, 0) == 8 and stream_steps([5, 0, 9], 0, 4) == 12
    # two slots, interval 4, steps needed 25 4 18 1 10 25 6.  Rounds end at 4, 8, ...: segment 1 leaves at 4 (slot 1 takes 2), 2 at
    # 4 + 20 = 24 (slot 1 takes 3), 0 at 28 and 3 at 24 + 4 = 28 (slots take 4 and 5), 4 at 28 + 12 = 40 (slot 0 takes 6), 6 at 40 + 8 = 48,
    # 5 at 28 + 28 = 56
    assert stream_steps(DONE, 2, 4) == 56
    # three slots, interval 8: 1 leaves at 8 (3 in), 3 at 16 (4 in), 2 at 24 (5 in), 0 at 32 (6 in) and 4 at 16 + 16 = 32, 6 at 40,
    # 5 at 24 + 32 = 56
    assert stream_steps(DONE, 3, 8) == 56
    # a prompt of two ids: needed 27 6 20 3 12 27 8.  1 leaves at 8 (2 in), 0 at 28 and 2 at 8 + 20 = 28 (3, 4 in), 3 at 32 (5 in), 4 at
    # 28 + 12 = 40 (6 in), 6 at 48, 5 at 32 + 28 = 60
    assert stream_steps(DONE, 2, 4, n_prompt=2) == 60
    # lock-step batches with the early stop: each runs its prompt, then the first multiple of the interval that covers its slowest group
    assert lockstep_steps(DONE, 2, 4, 0, 32) == 28 + 20 + 28 + 8
    assert lockstep_steps(DONE, 3, 8, 0, 32) == 32 + 32 + 8
    assert lockstep_steps(DONE, 2, 4, 2, 32) == 30 + 22 + 30 + 10
    assert lockstep_steps([30, 2], 2, 8, 0, 31) == 31                        # never more than n_steps
    assert stream_steps(DONE, 2, 4) < lockstep_steps(DONE, 2, 4, 0, 32) and stream_steps(DONE, 3, 8) < lockstep_steps(DONE, 3, 8, 0, 32)
