"""Steps per replayed graph (YMT3_GRAPH_STEPS, read at create) must not change a decode call's results: a call of n_total steps replays
whole G-step graphs and then a one-step tail (runtime.hip: step_graph, replay), and every kernel reads its position from device memory, so
G = 3, G = 1 and the eager launches (YMT3_NO_GRAPH=1) give the same ids bit for bit.  n_total in {2, 3, 7} at G = 3: no G-step graph at
all, exactly one and no tail, two and one tail step."""
import os

import pytest
import torch

from oracle import ymt3_oracle as O
from test_gpu_parity import SMALL, _model

pytestmark = pytest.mark.gpu


def _with_env(env, **kw):
    os.environ.update(env)
    try:
        return _model(SMALL, max_batch=4, **kw)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def handles():
    ms = {"g3": _with_env({"YMT3_GRAPH_STEPS": "3"}), "g1": _with_env({"YMT3_GRAPH_STEPS": "1"}), "eager": _with_env({"YMT3_NO_GRAPH": "1"}),
          "chains2_g3": _with_env({"YMT3_CHAINS": "2", "YMT3_GRAPH_STEPS": "3"})}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def enc(handles):
    m = handles["g1"]
    return m.encode(m.logmel(O.synthetic_audio(4, SMALL, seed=21).cuda()))


@pytest.mark.parametrize("n_total", [2, 3, 7])
def test_graph_steps_do_not_change_the_ids(handles, enc, n_total):
    ref = handles["g1"].decode(enc, n_total).cpu()
    assert ref.shape == (4, 1, n_total)
    assert torch.equal(handles["g3"].decode(enc, n_total).cpu(), ref)
    assert torch.equal(handles["eager"].decode(enc, n_total).cpu(), ref)
    assert all(handles[k].last_decode_steps == n_total for k in ("g3", "g1", "eager"))


def test_graph_steps_with_a_prompt(handles, enc):
    prompt = torch.tensor([3, 5], dtype=torch.int32)          # 2 fed + 5 emitted = 7 steps: two 3-step graphs and one tail step
    ref = handles["g1"].decode(enc, 5, prompt=prompt).cpu()
    assert torch.equal(handles["g3"].decode(enc, 5, prompt=prompt).cpu(), ref)
    assert torch.equal(handles["eager"].decode(enc, 5, prompt=prompt).cpu(), ref)
    assert not torch.equal(ref, handles["g1"].decode(enc, 5).cpu())       # (the prompt is not ignored)


def test_graph_steps_with_beams(handles, enc):
    ref_t, ref_ts, ref_ss = handles["g1"].decode(enc[:2], 7, num_beams=2, return_scores=True)
    t, ts, ss = handles["g3"].decode(enc[:2], 7, num_beams=2, return_scores=True)
    assert torch.equal(t.cpu(), ref_t.cpu()) and torch.equal(ss.cpu(), ref_ss.cpu()) and torch.equal(ts.cpu(), ref_ts.cpu())


def test_graph_steps_with_two_chains(handles, enc):
    ref = handles["g1"].decode(enc, 7).cpu()
    assert torch.equal(handles["chains2_g3"].decode(enc, 7).cpu(), ref)
    assert handles["chains2_g3"].last_decode_chains == 2 and handles["g1"].last_decode_chains == 1
