"""The tail of the self-attention stream (decode.hip, `tail` in attn_body).

The stream's last, partly filled block of 384 keys loads and runs only the 64-key sub-blocks in which a wave still has a key, one
straight-line path per count, instead of all six with masks.  A sub-block left out contributed p = 0 everywhere, so the bits stay: a default
handle (attention pair + GEMM chain, the 8-wave kernel inside the pair) and a handle created under YMT3_NO_ATTN_PAIR=1 YMT3_NO_GEMM_CHAIN=1
(the separate launches) must give EQUAL ids and per-step logits (torch.equal), as they did before.  Flagship dimensions, seeded weights.

  1. free-running greedy decode of 770 steps at 1, 5, 17 and 64 rows: n_keys crosses 1, 64, 65, 384, 385, 768 and 769 -- every sub-block
     count from 1 to 6, a first block that is partial, a block boundary and both of its neighbours;
  2. 4 segments through 2 slots, rows at different positions within one launch;
  3. a 770-step decode, then a 100-step decode of another batch on the same handle: keys beyond n_keys are never touched.

(The 2-wave form of the same body is what tests/test_row_space.py and the many-row parity tests run; they pass unchanged.)"""
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
STEPS = 770
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


SEPARATE = dict(YMT3_NO_ATTN_PAIR="1", YMT3_NO_GEMM_CHAIN="1")


@pytest.fixture(scope="module")
def weights():
    return make_weights(CFG, seed=1234)


def _handles(cfg, max_batch, weights):
    """(default handle, handle of the separate launches); _model's close() fails the test if either fell back from a merged kernel"""
    new = _model(cfg, max_batch=max_batch, weights=weights)
    with _env(**SEPARATE):
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


# ----------------------------------------------------------------------------- 1. lock-step, every sub-block count
@pytest.mark.parametrize("B", [1, 5, 17, 64])
def test_free_running_ids_and_logits_equal_the_separate_launches(pair, enc, B):
    new, ref = pair
    t1, l1 = new.decode(enc[:B], STEPS, return_logits=True)
    t0, l0 = ref.decode(enc[:B], STEPS, return_logits=True)
    assert torch.equal(t1, t0)
    assert torch.equal(l1, l0)
    assert torch.isfinite(l1).all()
    assert new.merged_fallbacks == 0 and ref.merged_fallbacks == 0


# ----------------------------------------------------------------------------- 2. slot mode
def test_rows_at_different_positions_within_one_launch(pair, enc, audio, weights):
    n_seg = 4
    toks = pair[1].decode(enc[:n_seg], STEPS).cpu().numpy().reshape(n_seg, STEPS)
    # an EOS that stops the rows after different numbers of steps: a slot is refilled while its neighbour is somewhere else in its row
    best, key = None, (-1, -1)
    for cand in np.unique(toks):
        first = [int(np.argmax(r == cand)) if (r == cand).any() else STEPS for r in toks]
        k = (len(set(first)), max(first))
        if k > key:
            best, key = int(cand), k
    assert best is not None and key[0] >= 2, "the synthetic decode offers no token that stops rows at different positions"
    new, ref = _handles(dataclasses.replace(CFG, eos_id=best), 2, weights)
    try:
        want, want_s = ref.inference_stream(audio[:n_seg], max_token_length=STEPS, slots=2, interval=4, return_scores=True)
        got, got_s = new.inference_stream(audio[:n_seg], max_token_length=STEPS, slots=2, interval=4, return_scores=True)
        stops = sorted({int(np.argmax(r == best)) if (r == best).any() else STEPS for r in want.cpu().numpy().reshape(n_seg, STEPS)})
        print(f"eos={best}: rows stop after {stops} of {STEPS} positions")
        assert len(stops) >= 2
        assert torch.equal(got, want) and torch.equal(got_s, want_s)
        assert new.merged_fallbacks == 0 and ref.merged_fallbacks == 0
    finally:
        new.close()
        ref.close()


# ----------------------------------------------------------------------------- 3. stale cache
def test_a_short_decode_after_a_long_one_reads_no_stale_key(pair, enc, weights):
    new, _ = pair
    new.decode(enc[:5], STEPS)                                   # batch X fills 770 positions of rows 0..4
    t1, l1 = new.decode(enc[32:37], 100, return_logits=True)     # batch Y in the same rows
    fresh = _model(CFG, max_batch=5, weights=weights)
    try:
        t0, l0 = fresh.decode(enc[32:37], 100, return_logits=True)
        assert torch.equal(t1, t0) and torch.equal(l1, l0)
        assert fresh.merged_fallbacks == 0 and new.merged_fallbacks == 0
    finally:
        fresh.close()


# ----------------------------------------------------------------------------- 4. against the masked form
def test_ids_equal_the_masked_form_the_beam_kernels_keep(pair, enc):
    """The beam kernels' self-attention still runs all six sub-blocks of a partly filled block with masks.  A beam call of width 1 through
    them is greedy search: its ids are the greedy call's up to each row's first step whose top-2 margin is below 2e-4 (tests/test_beam.py:
    adding the running log-probability in f32 can merge two logits that close into a tie)."""
    new, _ = pair
    B = 5
    t, l = new.decode(enc[:B], STEPS, return_logits=True)
    tb = new.decode(enc[:B], STEPS, num_beams=1, _force_beam=True)
    t, tb = t.cpu().reshape(B, STEPS), tb.cpu().reshape(B, STEPS)
    top = l.topk(2, -1).values
    low = ((top[..., 0] - top[..., 1]) < 2e-4).cpu().reshape(B, STEPS)
    stops = []
    for g in range(B):
        idx = low[g].nonzero().flatten()
        stop = int(idx[0]) if idx.numel() else STEPS
        stops.append(stop)
        assert torch.equal(tb[g, :stop], t[g, :stop]), g
    print(f"rows compared up to positions {stops} of {STEPS}")
    assert new.merged_fallbacks == 0
