"""The model behind tests/test_encoder_kernels.py (tests/enc_kernel_model.py) is right and has teeth -- CPU only:

  * evaluated in fp32 its references ARE the oracle (oracle/ymt3_oracle.py::attention(round_p=True) / rmsnorm, oracle/perceiver_oracle.py::_mha, which
    tests/test_oracle_vs_thirdparty.py pins to HF T5), at that file's tolerance for a norm (1e-6);
  * the fp32 oracle, a correct implementation with another summation order, PASSES the criterion on every case of the GPU tests;
  * at least MIN_STABLE of the elements of every random case are stable under the reference alone, and the exact probes are what they claim:
    P is exactly one-hot on every checked row, and the share of checked rows is asserted;
  * every mutant -- a wrong kernel written as a variant of the reference -- FAILS at least one GPU test's check on that test's own inputs.
"""
import pytest
import torch

import enc_kernel_model as K
from oracle import ymt3_oracle as O
from oracle.perceiver_oracle import _mha

_REF = {}


def _enc_ref(name, make):
    """(inputs, parts, beta, flippable) of one encoder-attention input, computed once"""
    if name not in _REF:
        q, k, v, bo = make()
        _REF[name] = ((q, k, v, bo),) + K.enc_attention_reference(q, k, v, bo)
    return _REF[name]


def _random_ref(case):
    name, T, B, H, fused, qs, bs = case
    return _enc_ref(name, lambda: K.enc_random_case(T, B, H, qs, bs))


# ----------------------------------------------------------------------------- the references are the oracle
@pytest.mark.parametrize("case", K.enc_random_cases()[:12:2] + K.enc_random_cases()[13::4], ids=lambda c: c[0])
def test_attention_reference_in_fp32_is_the_oracle(case):
    name, T, B, H, fused, qs, bs = case
    q, k, v, bo = K.enc_random_case(T, B, H, qs, bs)
    got, _, _ = K.enc_attention_reference(q, k, v, bo, dtype=torch.float32)
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1
    ref = O.attention(K.heads(q).float(), K.heads(k).float(), K.heads(v).float(), bo[:, idx][None], True, round_p=True)
    assert torch.allclose(K.heads(got["out"]), ref, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("case", K.seq_cases()[::3], ids=lambda c: c[0])
def test_sequence_reference_in_fp32_is_the_perceiver_oracle(case):
    name, Tq, Tk, wb, n_seq, inner_n, layout, qs, bs = case
    q, k, v, bo = K.seq_random_case(Tq, Tk, wb, n_seq, qs, bs)
    got, _, _ = K.seq_attention_reference(q, k, v, bo, dtype=torch.float32)
    bias = None
    if wb:
        idx = torch.arange(Tk)[None, :] - torch.arange(Tq)[:, None] + Tk - 1
        bias = bo[:, idx][None]
    ref = _mha(q.float().reshape(n_seq, Tq, -1), k.float().reshape(n_seq, Tk, -1), v.float().reshape(n_seq, Tk, -1), bias, True)
    assert torch.allclose(got["out"].reshape(n_seq, Tq, -1), ref, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("d", K.RMS_D)
def test_rmsnorm_reference_in_fp32_is_the_oracle(d):
    x, gain = K.rmsnorm_case(37, d)
    for eps in (1e-6, 1e-3):
        out, o = K.rmsnorm_model(x, gain, eps, dtype=torch.float32)
        ref = O.rmsnorm(x, gain, eps)
        assert torch.allclose(o, ref, atol=1e-6, rtol=1e-6) and torch.equal(out, O._r(ref, True))


# ----------------------------------------------------------------------------- a correct implementation passes; the cases are stable
@pytest.mark.parametrize("case", K.enc_random_cases(), ids=lambda c: c[0])
def test_encoder_attention_cases_are_stable_and_admit_the_fp32_oracle(case):
    (q, k, v, bo), ref, beta, flip = _random_ref(case)
    own = K.check_bf16(ref["out"], ref["o"], beta)
    assert own["ok"] and own["stable_share"] >= K.MIN_STABLE, own
    got, _, _ = K.enc_attention_reference(q, k, v, bo, dtype=torch.float32)
    rec = K.check_bf16(got["out"], ref["o"], beta)
    assert rec["ok"], rec
    assert float(flip.double().sum(-1).mean()) < 8.0            # flippable keys per row: the bound is not made of flips


def test_encoder_random_cases_cover_every_axis_at_every_T():
    cases = K.enc_random_cases()
    for T in K.ENC_T:
        mine = [c for c in cases if c[1] == T]
        assert {(c[5], c[6]) for c in mine} == set(K.ATTN_REGIMES)
        assert {c[2] for c in mine} == {1, 3} and {c[3] for c in mine} == {1, 8} and {c[4] for c in mine} == {True, False}
    for qs, bs in K.ATTN_REGIMES:
        mine = [c for c in cases if (c[5], c[6]) == (qs, bs)]
        assert {c[2] for c in mine} == {1, 3} and {c[3] for c in mine} == {1, 8} and {c[4] for c in mine} == {True, False}


@pytest.mark.parametrize("case", K.seq_cases(), ids=lambda c: c[0])
def test_sequence_attention_cases_are_stable_and_admit_the_fp32_oracle(case):
    name, Tq, Tk, wb, n_seq, inner_n, layout, qs, bs = case
    q, k, v, bo = K.seq_random_case(Tq, Tk, wb, n_seq, qs, bs)
    ref, beta, _ = K.seq_attention_reference(q, k, v, bo)
    own = K.check_bf16(ref["out"], ref["o"], beta)
    assert own["ok"] and own["stable_share"] >= K.MIN_STABLE, own
    got, _, _ = K.seq_attention_reference(q, k, v, bo, dtype=torch.float32)
    assert K.check_bf16(got["out"], ref["o"], beta)["ok"]
    lay = K.seq_layouts(n_seq, inner_n, Tq, Tk)[layout]
    for st, n_pos, size, at in ((lay["q"], Tq, lay["q_size"], 0), (lay["kv"], Tk, lay["kv_size"] or lay["q_size"], lay["v_at"]), (lay["o"], Tq, lay["o_size"], 0)):
        assert all(s % 8 == 0 for s in st)
        assert int(K.seq_starts(n_seq, inner_n, st).max()) + (n_pos - 1) * st[2] + at + K.SEQ_H * 64 <= size


def test_sequence_cases_cover_the_issue_s_axes():
    cases = K.seq_cases()
    assert {(c[1], c[2], c[3]) for c in cases} == set(K.SEQ_SHAPES)
    for shape in K.SEQ_SHAPES:
        mine = [c for c in cases if (c[1], c[2], c[3]) == shape]
        assert {(c[4], c[5]) for c in mine} == {(1, 1), (1, 3), (5, 1), (5, 3)}
    assert {c[6] for c in cases} == {"temporal", "padded"}
    assert any(c[6] == "temporal" and c[5] == 3 and c[3] for c in cases)          # the temporal transformer's own layout, with its bias


@pytest.mark.parametrize("d", K.RMS_D)
def test_rmsnorm_cases_are_stable_and_admit_the_fp32_oracle(d):
    for M in (5, 4127):
        x, gain = K.rmsnorm_case(M, d)
        for eps in (1e-6, 1e-3):
            out, o = K.rmsnorm_model(x, gain, eps)
            beta = K.rmsnorm_beta(o, d)
            own = K.check_bf16(out, o, beta)
            assert own["ok"] and own["stable_share"] >= K.MIN_STABLE, own
            assert K.check_bf16(K.rmsnorm_model(x, gain, eps, dtype=torch.float32)[0], o, beta)["ok"]


@pytest.mark.parametrize("M,N,K_", K.GEMM_SMALL + K.GEMM_BIG)
def test_gemm_epilogue_cases_are_stable_and_admit_an_fp32_matmul(M, N, K_):
    A, W, bias, resid = K.gemm_case(M, N, K_)
    acc = A.float() @ W.float().T
    o, beta = K.gemm_epilogue_reference(K.EPI_BF16, A, W)
    for relu in (False, True):
        own = K.check_bf16(K.rb(o.clamp(min=0) if relu else o), o, beta, relu=relu)
        assert own["ok"] and own["stable_share"] >= K.MIN_STABLE, own
        assert K.check_bf16((acc.clamp(min=0) if relu else acc).bfloat16(), o, beta, relu=relu)["ok"]
    assert bool((o < -beta).any() and (o > beta).any())                         # the ReLU clamps some columns and passes others
    ref, bound = K.gemm_epilogue_reference(K.EPI_F32, A, W, bias=bias)
    assert K.check_f32(acc + bias, ref, bound)["ok"]
    ref, bound = K.gemm_epilogue_reference(K.EPI_RESID, A, W, resid=resid)
    assert K.check_f32(resid + acc, ref, bound)["ok"]


# ----------------------------------------------------------------------------- the exact probes are what they claim
@pytest.mark.parametrize("T", K.ENC_T)
def test_bias_probe_rows_are_one_hot_and_the_sweep_covers_every_table_index(T):
    n = K.bias_probe_launches(T)
    assert n <= 64
    peaks = torch.cat([K.bias_probe_case(T, j)[4] for j in range(n)])
    assert set(peaks.tolist()) == set(range(2 * T - 1))
    checked = 0
    for j in (range(n) if T <= 128 else (0, n // 2, n - 1)):
        q, k, v, bo, peak, key = K.bias_probe_case(T, j)
        parts = K.attention_model(K.heads(q[:1]), K.heads(k[:1]), K.heads(v[:1]), K.bias_from_table(bo, T, T))
        P, hit = parts["P"][0], key >= 0                                          # (H, T, T), (H, T)
        assert torch.equal(P[hit], torch.nn.functional.one_hot(key[hit], T).double())
        assert torch.equal(parts["out"][0][hit], K.heads(v[:1])[0].double()[torch.nonzero(hit)[:, 0], key[hit]])
        # the other rows are uniform: the closed form the GPU test uses is the reference's
        ref, beta, flip = K.enc_attention_reference(q[:1], k[:1], v[:1], bo)
        uo, ub = K.uniform_row(v[:1])
        miss = ~hit.T[None]                                                       # (1, T, H)
        assert not bool(flip.any())
        assert torch.allclose(ref["o"][miss], uo[:, None].expand(1, T, -1, -1)[miss], rtol=1e-12, atol=0)
        assert torch.allclose(beta[miss], ub[:, None].expand(1, T, -1, -1)[miss], rtol=1e-9, atol=0)
        checked += int(hit.sum())
    assert checked > 0


@pytest.mark.parametrize("T", K.ENC_T)
def test_score_probe_rows_are_one_hot_and_most_rows_are_checked(T):
    q, k, v, bo, key = K.score_probe_case(T)
    ref, beta, _ = K.enc_attention_reference(q, k, v, bo)
    hit = key >= 0                                                                # (B, T, H)
    assert float(hit.double().mean()) >= 0.7, float(hit.double().mean())
    P = ref["P"].transpose(1, 2)                                                  # (B, T, H, T)
    assert torch.equal(P[hit], torch.nn.functional.one_hot(key[hit], T).double())
    b, t, h = torch.nonzero(hit, as_tuple=True)
    assert torch.equal(ref["out"][hit], v.double()[b, key[hit], h])
    assert len(set((key[hit] - t).tolist())) == 63                               # every offset of the window is somebody's winner


@pytest.mark.parametrize("shape", K.SEQ_SHAPES, ids=str)
def test_sequence_score_probe_rows_are_one_hot(shape):
    Tq, Tk, wb = shape
    q, k, v, bo, key = K.seq_score_probe_case(Tq, Tk, 5, wb)
    ref, _, _ = K.seq_attention_reference(q, k, v, bo)
    hit = key >= 0
    assert float(hit.double().mean()) >= (0.7 if wb else 1.0)
    assert torch.equal(ref["P"].transpose(1, 2)[hit], torch.nn.functional.one_hot(key[hit], Tk).double())
    b, t, h = torch.nonzero(hit, as_tuple=True)
    assert torch.equal(ref["out"][hit], v.double()[b, key[hit], h])


# ----------------------------------------------------------------------------- mutants fail
def _enc_inputs():
    """the encoder-attention inputs of the GPU tests, cheapest first: (name, make, winning key per (b, t, h) or None)"""
    for T in (64, 128, 256):
        yield f"score_probe_T{T}", (lambda T=T: K.score_probe_case(T)[:4]), K.score_probe_case(T)[4]
    for T, j in ((64, 0), (64, 3), (128, 9), (256, 17)):
        key = K.bias_probe_case(T, j)[5].T[None].expand(K.BIAS_PROBE_B, -1, -1)
        yield f"bias_probe_T{T}_{j}", (lambda T=T, j=j: K.bias_probe_case(T, j)[:4]), key
    for case in K.enc_random_cases():
        if case[1] <= 256:
            yield case[0], (lambda c=case: K.enc_random_case(c[1], c[2], c[3], c[5], c[6])), None


def _fails(mutant, name, make, key):
    (q, k, v, bo), ref, beta, _ = _enc_ref(name, make)
    got = K.enc_attention_reference(q, k, v, bo, mutant=mutant)[0]["out"]
    if key is not None:
        hit = key >= 0
        b, t, h = torch.nonzero(hit, as_tuple=True)
        if not torch.equal(got[hit], v.double()[b, key[hit], h]):
            return True
    return not K.check_bf16(got, ref["o"], beta)["ok"]


@pytest.mark.parametrize("mutant", ["bias_off_by_one", "bias_next_head", "norm_from_rounded", "trunc_p", "trunc_out", "swap_keys", "swap_v16", "other_group"])
def test_attention_mutant_fails(mutant):
    caught = []
    for name, make, key in _enc_inputs():
        if _fails(mutant, name, make, key):
            caught.append(name)
            if len(caught) >= 3:
                break
    print(mutant, "caught by", caught)
    assert caught, mutant


def test_the_numerics_mutants_fail_on_the_random_cases_alone():
    """the rounding contract (normaliser from the unrounded e, nearest-even P and output) is judged by the criterion, not by the exact probes"""
    for mutant in ("norm_from_rounded", "trunc_p", "trunc_out"):
        caught = [c[0] for c in K.enc_random_cases() if c[1] <= 128 and _fails(mutant, c[0], (lambda c=c: K.enc_random_case(c[1], c[2], c[3], c[5], c[6])), None)]
        assert len(caught) >= 6, (mutant, caught)


@pytest.mark.parametrize("mutant", ["mean_subtracted", "eps_outside"])
def test_rmsnorm_mutant_fails(mutant):
    caught = 0
    for d in K.RMS_D:
        x, gain = K.rmsnorm_case(5, d)
        for eps in (1e-6, 1e-3):
            out, o = K.rmsnorm_model(x, gain, eps)
            caught += not K.check_bf16(K.rmsnorm_model(x, gain, eps, mutant=mutant)[0], o, K.rmsnorm_beta(o, d))["ok"]
    assert caught >= len(K.RMS_D), caught


def test_gemm_epilogue_mutants_fail():
    M, N, K_ = K.GEMM_SMALL[1]
    A, W, bias, resid = K.gemm_case(M, N, K_)
    ref, bound = K.gemm_epilogue_reference(K.EPI_RESID, A, W, resid=resid)
    wrong, _ = K.gemm_epilogue_reference(K.EPI_RESID, A, W, resid=resid, mutant="resid_overwrites")
    assert not K.check_f32(wrong.float(), ref, bound)["ok"]
    twice = ref + K.gemm_reference_and_bound(A, W)[0]                              # the second launch of the GPU test accumulates again
    assert not K.check_f32(ref.float(), twice, bound * 2)["ok"]
    for T, n_seg in ((64, 3), (256, 3)):
        P, Wp, exact = K.permutation_probe(n_seg * T, 1024, 128)
        assert not torch.equal(K.headmajor(exact, T, 8, mutant="swap_h_slab"), K.headmajor(exact, T, 8))


def test_the_criterion_itself():
    o = torch.tensor([1.0, 1.00390625, 1.00390625, -3.0, 0.5, -0.5, 2e-5], dtype=torch.float64)       # 1.00390625 = 1 + 2^-8: a bf16 tie
    beta = torch.full_like(o, 1e-4)
    good = torch.tensor([1.0, 1.0, 1.0078125, -3.0, 0.5, -0.5, 2e-5]).bfloat16()
    rec = K.check_bf16(good, o, beta)
    assert rec["ok"] and rec["unstable"] == 3 and rec["stable_wrong"] == 0
    bad = good.clone()
    bad[0] = 1.0078125                                                          # one ulp off on a stable element
    assert not K.check_bf16(bad, o, beta)["ok"]
    bad = good.clone()
    bad[1] = 1.015625                                                           # two ulps off on an unstable one
    assert not K.check_bf16(bad, o, beta)["ok"]
    relu = K.check_bf16(torch.tensor([1.0, 1.0, 1.0078125, 0.0, 0.5, 0.0, 0.0]).bfloat16(), o, beta, relu=True)
    assert relu["ok"]                                                           # |2e-5| <= beta: 0 is admitted
    assert not K.check_bf16(torch.tensor([1.0, 1.0, 1.0078125, 0.0, 0.0, 0.0, 0.0]).bfloat16(), o, beta, relu=True)["ok"]
    assert not K.check_bf16(torch.tensor([1.0, 1.0, 1.0078125, -3.0, 0.5, 0.0, 0.0]).bfloat16(), o, beta, relu=True)["ok"]
