"""What tests/test_value_space.py rests on, shown from the oracle alone (no GPU): every regime's inputs are finite and leave at
least MIN_SAFE of the steps above the scaled TAU, the constructed cases are what they claim to be (a dead ReLU layer, ties at the
maximum), the checks have teeth (an oracle with the wrong eps misses the `tiny` bound; the derived GEMM bound holds for a plain fp32
matmul), and the host side turns the ids a non-finite row emits into notes without an exception."""
import numpy as np
import pytest
import torch

import value_regimes as VR
from oracle import ymt3_oracle as O

CFG = VR.CFG


@pytest.mark.parametrize("name", VR.REGIMES)
def test_every_regime_is_finite_and_covered_at_its_tau(name):
    case, std = VR.oracle_case(name), VR.oracle_case("std")
    b = VR.bounds(case, std)
    assert case["finite"]
    assert VR.safe_fraction(case, b) >= VR.MIN_SAFE, (VR.safe_fraction(case, b), b)
    # the oracle's own fp32-vs-double difference is far inside the bound it is compared at: the bound leaves room for a second
    # correct implementation, and the regime's values do not make the oracle itself unreliable
    assert case["intrinsic_max"] < 0.5 * b["tol_max"] and case["intrinsic_mean"] < 0.5 * b["tol_mean"], (case["intrinsic_max"], b)
    assert b["tol_max"] >= VR.TOL_MAX and b["tau_std"] >= VR.TAU


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("name", ["std", "tiny"])
def test_ln_eps_cases_are_covered_at_their_tau(name, eps):
    cfg = CFG.with_(ln_eps=eps)
    case = VR.oracle_case(name, cfg)
    b = VR.bounds(case, VR.oracle_case("std", cfg))
    assert case["finite"] and VR.safe_fraction(case, b) >= VR.MIN_SAFE, VR.safe_fraction(case, b)


def test_regime_weights_stay_bf16_exact():
    from yourmt3_amd.weights import is_bf16_tensor
    for name in VR.REGIMES:
        for k, v in VR.regime_weights(CFG, name).items():
            if is_bf16_tensor(k):
                assert torch.equal(v.bfloat16().float(), v), (name, k)
    W, grp = VR.dup_head(CFG, VR.regime_weights(CFG, "std"))
    assert torch.equal(W["dec.lm_head"].bfloat16().float(), W["dec.lm_head"]) and sorted(set(grp.bincount().tolist())) == [30, 36]
    g = VR.regime_weights(CFG, "neg_gain")["dec.1.ln2"]
    assert int((g == 0).sum()) == 13 and int(torch.signbit(g[g == 0]).sum()) == 8 and bool((g <= 0).all())


def test_wrong_eps_fails_the_tiny_bound(monkeypatch):
    """the oracle at eps 1e-5 in place of the HIP result, against the oracle at the config's 1e-6: under `tiny` the error is some
    50 times the bound (under the standard weights it is far inside it: that is why the rest of the suite cannot see eps)"""
    for name, must_fail in (("tiny", True), ("std", False)):
        case = VR.oracle_case(name)
        b = VR.bounds(case, VR.oracle_case("std"))
        _, wrong = O.greedy_decode(case["enc"], case["W"], CFG.with_(ln_eps=1e-5), CFG.max_decode_len, True, forced=case["feed"],
                                   return_logits=True)
        e_max, e_mean = VR.logits_error(wrong, case["logits"], case["std"])
        assert (e_max >= b["tol_max"]) == must_fail, (name, e_max, b["tol_max"])
        if must_fail:
            assert e_max > 10 * b["tol_max"] and e_mean > 10 * b["tol_mean"], (e_max, e_mean)


def test_dead_relu_layer_outputs_exact_zeros(monkeypatch):
    seen = {}
    plain = O.dense_ffn

    def spy(xn, W, p, bf16):
        pre = xn @ W[p + "wi"].T
        out = plain(xn, W, p, bf16)
        s = seen.setdefault(p, [-1e30, 0.0])
        s[0], s[1] = max(s[0], float(pre.max())), max(s[1], float(out.abs().max()))
        return out
    monkeypatch.setattr(O, "dense_ffn", spy)
    case = VR.oracle_case("dead_relu", key="dead_relu_spied")
    dead = f"dec.{VR.DEAD_LAYER}."
    assert seen[dead][0] < -50.0 and seen[dead][1] == 0.0, seen[dead]          # every pre-activation far below 0: output exactly 0
    assert all(v[1] > 0 for p, v in seen.items() if p.startswith("dec.") and p != dead)
    assert case["finite"] and len(set(case["ids"].flatten().tolist())) > 20      # the model still decodes a varied stream


def test_duplicated_head_ties_at_the_maximum():
    cfg = CFG.with_(eos_id=-1)
    W, grp = VR.dup_head(cfg, VR.regime_weights(cfg, "std"))
    case = VR.oracle_case("dup_head", cfg, W=W, key="dup_head")
    lg = case["logits"]
    tied = (lg == lg.amax(-1, keepdim=True)).sum(-1)
    assert float((tied >= 2).float().mean()) >= 0.5, float((tied >= 2).float().mean())
    win = torch.from_numpy(np.argmax(lg.numpy(), -1))
    rel = set()
    for w in win.flatten().tolist():
        cols = (grp == grp[w]).nonzero().flatten().tolist()
        for j in cols[1:]:
            rel |= VR.tie_relations(cols[0], j)
    assert rel >= {"stride", "lanes", "dpp_rows", "waves", "tiles", "first_tile", "last_tile"}, rel
    # distinct rows are told apart at the usual margin often enough
    first = torch.stack([(grp == g).nonzero()[0, 0] for g in range(48)])
    assert float((VR.margin(lg[..., first]) >= VR.bounds(case, VR.oracle_case("std"))["tau"]).float().mean()) >= VR.MIN_SAFE


@pytest.mark.parametrize("kind", VR.GEMM_KINDS)
def test_gemm_bound_holds_for_a_plain_fp32_matmul(kind):
    for M, N, K in ((200, 256, 512), (300, 512, 2048)):
        A, W = VR.gemm_operands(kind, M, N, K)
        ref, bound = VR.gemm_reference_and_bound(A, W)
        got = A.float() @ W.float().T
        assert bool(torch.isfinite(got).all()) and float(((got.double() - ref).abs() / bound).max()) <= 1.0
        if kind == "cancel":
            assert float(ref.abs().max()) < 1.0 and float(bound.min()) > 100.0       # the result is what is left of sums of 1e4
        if kind == "subnormal":
            assert float(A.float().abs()[A.float() != 0].max()) < 2.0 ** -126 and float(ref.abs().max()) > 0


@pytest.mark.parametrize("task", ["mt3_full_plus", "mc13_full_plus_256"])
def test_host_side_survives_the_ids_of_a_non_finite_row(task, tmp_path):
    """a row whose logits were all NaN emits id 0 (PAD) at every step, or under a constraint the lowest allowed id over and over, with
    NaN scores: the note list is empty or short, never an exception, also for ids outside the codec"""
    from yourmt3_amd.midi import write_midi
    from yourmt3_amd.task_manager import TaskManager
    tm = TaskManager(task)
    K, L = tm.num_decoding_channels, 32
    lowest = int(np.argmax(tm.event_automaton()[0].allowed[0]))
    rows = {"pad": np.zeros((1, K, L), np.int32), "lowest_allowed": np.full((1, K, L), lowest, np.int32),
            "beyond_codec": np.full((1, K, L), 2 ** 31 - 1, np.int32), "negative": np.full((1, K, L), -7, np.int32)}
    clean = np.tile(np.arange(3, 3 + L, dtype=np.int32), (1, K, 1))
    for name, bad in rows.items():
        tokens = np.concatenate([clean, bad], 0)
        scores = np.concatenate([np.full((1, K, L), -0.1, np.float32), np.full((1, K, L), np.nan, np.float32)], 0)
        alone = tm.tokens_to_notes([clean], [0.0], 4.0)
        notes = tm.tokens_to_notes([tokens], [0.0, 2.0], 4.0, score_batches=[scores])
        assert len(tm.tokens_to_notes([bad], [0.0], 2.0)) <= 1, name
        assert len(notes) <= len(alone) + 1, name
        write_midi(notes, str(tmp_path / f"{name}.mid"))


@pytest.mark.parametrize("name", ["tiny", "big", "bias40", "crossq8"])
def test_fp8_moe_cases_are_covered_at_their_tau(name):
    """the fp8 MoE cases of test_value_space.py (mixed-norm head): the oracle's own stream leaves at least 0.8 of the steps above
    the fp8 TAU of 0.08 std times the regime's factor -- a cushion over the 0.7 that _moe_case asks of the HIP run"""
    from yourmt3_amd.config import FFN_MOE
    cfg = CFG.with_(dec_ffn=FFN_MOE, moe_fp8=1, eos_id=-1)
    f = VR.bounds(VR.oracle_case(name), VR.oracle_case("std"))["tol_max"] / VR.TOL_MAX
    W = VR.mixed_norm_head(cfg, VR.regime_weights(cfg, name))
    _, enc = VR.oracle_encode(VR.audio(cfg), W, cfg)
    t, lg = O.greedy_decode(enc, W, cfg, cfg.max_decode_len, True, return_logits=True)
    if name == "tiny":
        _, lg = O.greedy_decode(enc, W, cfg, cfg.max_decode_len, True, forced=VR.tiny_feed(t.shape, cfg), return_logits=True)
    assert bool(torch.isfinite(lg).all())
    assert float((VR.margin(lg) / float(lg.std()) >= 0.08 * f).float().mean()) >= 0.8
