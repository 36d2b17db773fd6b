"""The attention pair against the separate launches (decode.hip, attn_body as dec_attn_pair_kernel and as two dec_attn_kernel launches).

The pair kernel runs its self-attention half at raised wave priority up to the row's signal, and has had the order of its K/V and projection
requests rearranged and measured (profiles/pair_request_order_ab.txt).  Priorities, loads and waits move, no arithmetic does: a default
handle (the pair kernel) and a handle created under YMT3_NO_ATTN_PAIR=1 (the same attn_body as two launches per layer) must give EQUAL ids
and per-step logits (torch.equal).  Flagship dimensions (256 encoder frames), seeded weights.

  1. teacher-forced decode of 400 steps at 1, 5 and 64 rows: n_keys runs from 1 to 400 -- a first block that is partial with every
     sub-block count 1..6, the whole block of 384 keys, and a whole block followed by a tail block;
  2. 8 segments through 5 slots with rows at different positions within one launch (the per-row key count)."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from test_gpu_parity import _model
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.weights import make_weights

pytestmark = pytest.mark.gpu
CFG = YMT3Config(eos_id=-1)          # 256 frames, 1024 positions, no early stop: every row runs all its steps
STEPS = 400
MAX_B = 64


@contextlib.contextmanager
def _env(**kv):
    """the switches are read at ymt3_create: set for the construction only"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def weights():
    return make_weights(CFG, seed=1234)


def _handles(cfg, max_batch, weights):
    """(handle that takes the pair, handle of the separate attention launches); _model's close() fails the test if either fell back from a
    merged kernel"""
    new = _model(cfg, max_batch=max_batch, weights=weights)
    with _env(YMT3_NO_ATTN_PAIR="1"):
        ref = _model(cfg, max_batch=max_batch, weights=weights)
    return new, ref


@pytest.fixture(scope="module")
def pair(weights):
    new, ref = _handles(CFG, MAX_B, weights)
    yield new, ref
    new.close()
    ref.close()


@pytest.fixture(scope="module")
def audio():
    return O.synthetic_audio(MAX_B, CFG)


@pytest.fixture(scope="module")
def enc(pair, audio):
    m = pair[1]
    return m.encode(m.logmel(audio.cuda()))


@pytest.fixture(scope="module")
def forced():
    g = torch.Generator().manual_seed(77)
    return torch.randint(0, CFG.vocab, (MAX_B, 1, STEPS), generator=g, dtype=torch.int32)


# ----------------------------------------------------------------------------- 1. lock-step, teacher-forced
@pytest.mark.parametrize("B", [1, 5, 64])
def test_forced_ids_and_logits_equal_the_separate_launches(pair, enc, forced, B):
    new, ref = pair
    f = forced[:B].cuda()
    t1, l1 = new.decode(enc[:B], STEPS, forced=f, return_logits=True)
    t0, l0 = ref.decode(enc[:B], STEPS, forced=f, return_logits=True)
    assert torch.equal(t1, t0)
    assert torch.equal(l1, l0)
    assert torch.isfinite(l1).all()
    assert new.merged_fallbacks == 0 and ref.merged_fallbacks == 0


# ----------------------------------------------------------------------------- 2. slot mode
def test_slot_mode_rows_at_different_positions(pair, enc, audio, weights):
    n_seg, slots = 8, 5
    toks = pair[1].decode(enc[:n_seg], STEPS).cpu().numpy().reshape(n_seg, STEPS)
    # an EOS that stops the rows after different numbers of steps: a slot is refilled while its neighbours are somewhere else in their rows
    best, key = None, (-1, -1)
    for cand in np.unique(toks):
        first = [int(np.argmax(r == cand)) if (r == cand).any() else STEPS for r in toks]
        k = (len(set(first)), max(first))
        if k > key:
            best, key = int(cand), k
    assert best is not None and key[0] >= 2, "the synthetic decode offers no token that stops rows at different positions"
    new, ref = _handles(dataclasses.replace(CFG, eos_id=best), slots, weights)
    try:
        want, want_s = ref.inference_stream(audio[:n_seg], max_token_length=STEPS, slots=slots, interval=4, return_scores=True)
        got, got_s = new.inference_stream(audio[:n_seg], max_token_length=STEPS, slots=slots, interval=4, return_scores=True)
        stops = sorted({int(np.argmax(r == best)) if (r == best).any() else STEPS for r in want.cpu().numpy().reshape(n_seg, STEPS)})
        print(f"eos={best}: rows stop after {stops} of {STEPS} positions")
        assert len(stops) >= 2
        assert torch.equal(got, want) and torch.equal(got_s, want_s)
        assert new.merged_fallbacks == 0 and ref.merged_fallbacks == 0
    finally:
        new.close()
        ref.close()
