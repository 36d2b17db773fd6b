"""Device detokeniser, the parts that need no GPU (include/ymt3.h, device detokeniser):
  1. TaskManager.token_table() says about every id what decode_segment would do with it;
  2. tests/detok_model.py -- the kernels' algorithm in plain Python -- equals the host path on the fuzz families of tests/detok_cases.py
     (notes, confidences, invalid-token count), and those cases cover every merge rule;
  3. the C ABI: the three entry points are declared, listed, exported, and documented with the rules a caller must know."""
import os
import re

import numpy as np
import pytest

import detok_cases as C
import detok_model as M
from yourmt3_amd.task_manager import DRUM_PROGRAM, TOKEN_CLASSES, TaskManager
from yourmt3_amd.vocab import EOS, PAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_MAX_TOKENS = 20000          # the Python model walks lanes one by one: the two full-size cases are left to the GPU test


@pytest.mark.parametrize("task", ["mt3_full_plus", "singing_drum_v1"])
def test_token_table_agrees_with_the_codec(task):
    tm = TaskManager(task)
    table = tm.token_table()
    assert table.shape == (tm.vocab_size,) and table.dtype == np.uint16
    assert (task == "singing_drum_v1") == bool(tm.tokenizer.skip_ids)
    for i in range(tm.vocab_size):
        cls, val = int(table[i]) >> 12, int(table[i]) & 0xFFF
        ev = tm.codec.decode(i)
        if i in (PAD, EOS):
            assert cls == TOKEN_CLASSES["stop"], i
        elif i in tm.tokenizer.skip_ids:
            assert cls == TOKEN_CLASSES["skip"], i
        elif ev.type == "special":
            assert cls == TOKEN_CLASSES["invalid"], i
        else:
            assert (cls, val) == (TOKEN_CLASSES[ev.type], ev.value), i
    assert int(table[tm.codec.size - 1]) >> 12 == TOKEN_CLASSES["drum"] and int(table[-1]) >> 12 == TOKEN_CLASSES["invalid"]


def test_cases_cover_every_merge_rule():
    total = dict.fromkeys(C.KINDS, 0)
    for case in C.cases():
        for k, v in C.coverage(case).items():
            total[k] += v
    print(total)
    assert all(total[k] > 0 for k in C.KINDS), total


@pytest.mark.parametrize("case", [c for c in C.cases() if c["tokens"].size <= MODEL_MAX_TOKENS], ids=lambda c: c["id"])
def test_model_equals_host_path(case):
    tm = C.task_manager(case["task"])
    ref_notes, ref_bad, _ = C.reference(case)
    records, bad = M.detokenize(tm.token_table(), case["tokens"], case["starts"], case["end_sec"], tm.codec.steps_per_second, DRUM_PROGRAM,
                                scores=case["scores"])
    assert bad == ref_bad
    assert C.same_notes(M.to_notes(records), ref_notes) is None, C.same_notes(M.to_notes(records), ref_notes)


def test_model_counts_ids_outside_the_vocabulary_as_invalid():
    tm = TaskManager("mt3_full_plus")
    tokens = np.full((2, 1, 70), np.iinfo(np.int32).min, np.int32)
    segs, ref_bad = tm.detokenize_list_batches([tokens[:, 0]], [0.0, 2.0], return_events=True)
    records, bad = M.detokenize(tm.token_table(), tokens, [0.0, 2.0], 3.0, 100, DRUM_PROGRAM)
    assert records == [] and bad == ref_bad == 140


def test_entry_points_declared_listed_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from yourmt3_amd import _lib
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    lib = _lib.load()
    for name in ("ymt3_detok_create", "ymt3_detok_destroy", "ymt3_detokenize"):
        assert re.search(r"\b" + name + r"\s*\(ymt3_", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct ymt3_detok_s* ymt3_detok;" in header
    assert lib.ymt3_abi_version() == 3 and "#define YMT3_ABI_VERSION 3" in header


def test_header_states_the_callers_obligations():
    header = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    block = header[header.index("/* Device detokeniser"):header.index("ymt3_detokenize(ymt3_handle")]
    text = " ".join(block.split())
    assert "strictly increasing" in text
    assert "capacity >= n_segments * n_channels * n_steps" in text
    assert "YMT3_ERR_ARG" in text and "NULL" in text
