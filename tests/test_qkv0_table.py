"""Layer 0's QKV projection as a per-token table (include/ymt3.h, ymt3_qkv0_table_active; kernels.h, ArgmaxArgs::qkv0).

A default handle gathers layer 0's q / k / v from the table built at construction and launches no layer-0 projection; a handle created
under YMT3_NO_QKV0_TABLE=1 keeps the launch.  Same seed, same weights: ids and per-step logits must be EQUAL (torch.equal), because
the table is written by the projection kernel itself.

  1. lock-step decode at 1, 3, 17, 48, 49 and 64 rows (a ragged row tile, the switch between the kernel's two column-tile forms, the merged regime);
  2. every vocabulary row once, the clamped ids below 0 and above V - 1 included, teacher-forced;
  3. the full cache length, lock-step and through the slot queue with rows at different positions: nothing is written past a (row, head) slab;
  4. prompted, constrained and scored decoding;
  5. the gates: multi-channel, mid-size tiles, a beam call, a stamped handle, the profiled call."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from test_gpu_parity import MC3, SMALL, _model
from yourmt3_amd.constraint import TokenAutomaton

pytestmark = pytest.mark.gpu
STEPS = 24


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


def _handles(cfg, max_batch, **env):
    """(default handle, handle that keeps the launch), both under `env`"""
    with _env(**env):
        tab = _model(cfg, max_batch=max_batch)
    with _env(YMT3_NO_QKV0_TABLE="1", **env):
        ref = _model(cfg, max_batch=max_batch)
    return tab, ref


@pytest.fixture(scope="module")
def pair():
    tab, ref = _handles(SMALL, 64)
    yield tab, ref
    tab.close()
    ref.close()


@pytest.fixture(scope="module")
def audio():
    return O.synthetic_audio(64, SMALL)


@pytest.fixture(scope="module")
def enc(pair, audio):
    m = pair[1]
    return m.encode(m.logmel(audio.cuda()))


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


# ----------------------------------------------------------------------------- 1. lock-step
@pytest.mark.parametrize("B", [1, 3, 17, 48, 49, 64])
def test_lockstep_ids_and_logits_equal_the_launch(pair, enc, B):
    tab, ref = pair
    t1, l1 = tab.decode(enc[:B], STEPS, return_logits=True)
    t0, l0 = ref.decode(enc[:B], STEPS, return_logits=True)
    assert tab.qkv0_table_active and not ref.qkv0_table_active
    assert torch.equal(t1, t0) and torch.equal(l1, l0)
    assert torch.isfinite(l1).all()
    assert tab.merged_fallbacks == 0 and ref.merged_fallbacks == 0
    assert tab.device_bytes - ref.device_bytes == SMALL.vocab * 3 * 512 * 2          # the table is counted


# ----------------------------------------------------------------------------- 2. every vocabulary row
def test_every_vocabulary_row_once(pair, enc):
    tab, ref = pair
    V, L = SMALL.vocab, SMALL.max_decode_len
    rows = V // L
    assert rows * L == V
    forced = torch.arange(V, dtype=torch.int32).reshape(rows, 1, L).clone()
    forced[0, 0, 0] = -5                      # clamped to 0, the id it replaces
    forced[-1, 0, -1] = V + 7                 # clamped to V - 1
    # the id fed after the last step is never read: the second order moves every column, so each id is fed in front of a compared step
    for f in (forced, torch.roll(forced, 1, -1)):
        t1, l1 = tab.decode(enc[:rows], L, forced=f.cuda(), return_logits=True)
        t0, l0 = ref.decode(enc[:rows], L, forced=f.cuda(), return_logits=True)
        assert tab.qkv0_table_active and not ref.qkv0_table_active
        assert torch.equal(l1, l0) and torch.equal(t1, t0)


# ----------------------------------------------------------------------------- 3. full cache length
def test_full_cache_length_lockstep(pair, enc):
    tab, ref = pair
    L = SMALL.max_decode_len
    for B in (3, 5):
        assert torch.equal(tab.decode(enc[:B], L), ref.decode(enc[:B], L))
        assert tab.qkv0_table_active
    # rows are neighbours in the cache: a store past row r's slab would have landed on position 0 of row r + 1 -- decode again
    assert torch.equal(tab.decode(enc[:5], L), ref.decode(enc[:5], L))


def test_full_cache_length_in_the_slot_queue(audio):
    L, n_seg = SMALL.max_decode_len, 5
    free, _ = None, None
    with _env(YMT3_NO_QKV0_TABLE="1"):
        free = _model(dataclasses.replace(SMALL, eos_id=-1), max_batch=n_seg)
    toks = free.inference(audio[:n_seg]).cpu().numpy().reshape(n_seg, L)
    free.close()
    # an EOS that stops some rows early and never occurs in others: those run to the end of the cache while their neighbours,
    # admitted later, sit at other positions
    best, spread = None, -1
    for cand in np.unique(toks):
        first = [int(np.argmax(r == cand)) if (r == cand).any() else L for r in toks]
        if L in first and min(first) < L - 8 and len(set(first)) > spread:
            best, spread = int(cand), len(set(first))
    assert best is not None, "the synthetic decode offers no token that stops some rows early and leaves others running to the end"
    tab, ref = _handles(dataclasses.replace(SMALL, eos_id=best), n_seg)
    want = ref.inference(audio[:n_seg])
    assert not ref.qkv0_table_active
    stops = sorted({int(np.argmax(r == best)) if (r == best).any() else L for r in want.cpu().numpy().reshape(n_seg, L)})
    print(f"eos={best}: rows stop after {stops} of {L} positions")
    assert stops[-1] == L and len(stops) >= 2
    for slots, interval in [(2, 4), (3, 1)]:
        got = tab.inference_stream(audio[:n_seg], slots=slots, interval=interval)
        assert tab.qkv0_table_active
        assert torch.equal(got, want), (slots, interval)
        assert torch.equal(ref.inference_stream(audio[:n_seg], slots=slots, interval=interval), want)
    assert torch.equal(tab.inference(audio[:n_seg]), want) and tab.qkv0_table_active
    tab.close()
    ref.close()


# ----------------------------------------------------------------------------- 4. prompted, constrained, scored
def test_prompted_constrained_and_scored_decoding(pair, enc):
    tab, ref = pair
    V, n = SMALL.vocab, 16
    prompt = torch.tensor([[5, 900, 1535], [0, 77, 1200]], dtype=torch.int32)
    g = np.random.default_rng(3)
    allowed = g.random((3, V)) < 0.5
    allowed[:, :4] = True
    aut = TokenAutomaton(allowed, g.integers(0, 3, (3, V)).astype(np.int32))
    starts = torch.tensor([[1], [2]], dtype=torch.int32)
    out = {}
    for name, m in (("tab", tab), ("ref", ref)):
        c = m.compile_constraint(aut)
        out[name] = [m.decode(enc[:2], n, prompt=prompt, return_logits=True),
                     m.decode(enc[:2], n, return_scores=True, constraint=c, start_states=starts),
                     m.decode(enc[:2], n, prompt=prompt, return_scores=True, constraint=c, start_states=starts),
                     m.decode(enc[:2], n, return_scores=True)]
        assert bool(m.qkv0_table_active) == (name == "tab")
        c.close()
    for a, b in zip(out["tab"], out["ref"]):
        assert _same(a, b)


# ----------------------------------------------------------------------------- 5. gates
def test_multichannel_handles_keep_the_launch():
    tab, ref = _handles(MC3, 2)
    a = O.synthetic_audio(2, MC3)
    t = tab.inference(a, max_token_length=12)
    assert not tab.qkv0_table_active and tab.device_bytes == ref.device_bytes
    assert torch.equal(t, ref.inference(a, max_token_length=12))
    tab.close()
    ref.close()


def test_mid_size_tiles_keep_the_launch(pair, enc):
    tab, ref = _handles(SMALL, 17, YMT3_DEC_GEMM_MID_ROWS="16")
    t17 = tab.decode(enc[:17], STEPS)
    assert not tab.qkv0_table_active
    assert torch.equal(t17, ref.decode(enc[:17], STEPS))
    # below the threshold the same handle gathers, and its ids are the plain handle's
    t3 = tab.decode(enc[:3], STEPS)
    assert tab.qkv0_table_active
    assert torch.equal(t3, pair[1].decode(enc[:3], STEPS))
    tab.close()
    ref.close()


def test_a_beam_call_keeps_the_launch(pair, enc):
    tab, ref = pair
    greedy = tab.decode(enc[:3], STEPS)
    assert tab.qkv0_table_active
    b1 = tab.decode(enc[:3], STEPS, num_beams=2, return_scores=True)
    assert not tab.qkv0_table_active
    assert _same(b1, ref.decode(enc[:3], STEPS, num_beams=2, return_scores=True))
    # and the greedy call after it gathers again, from caches the beam call has written
    assert torch.equal(tab.decode(enc[:3], STEPS), greedy) and tab.qkv0_table_active


def test_a_stamped_handle_keeps_the_launch(pair, enc):
    with _env(YMT3_STAMP="1"):
        m = _model(SMALL, max_batch=3)
    t = m.decode(enc[:3], STEPS)
    assert not m.qkv0_table_active
    assert torch.equal(t, pair[1].decode(enc[:3], STEPS))
    m.close()


def test_the_profiled_call_keeps_the_launch(pair, enc):
    tab, ref = pair
    want = ref.decode(enc[:3], STEPS)
    prof = tab.profile_decode(enc[:3], STEPS, stride=8)
    assert not tab.qkv0_table_active
    assert prof["qkv_cache_gemm"]["launches"] > 0
    assert torch.equal(tab.decode(enc[:3], STEPS), want) and tab.qkv0_table_active
