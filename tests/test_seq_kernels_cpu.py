"""The model behind tests/test_seq_kernels.py (tests/seq_kernel_model.py) is right and has teeth -- CPU only:

  * with the roundings off, its references chained (embed, tile-schedule attention causal and cross, lm head) ARE
    teacher_oracle.teacher_forward(bf16=False): to 1e-9 in float64;
  * with the roundings on and at most 64 keys the attention model IS oracle.attention(round_p=True) in float64, bit for bit; beyond 64 keys
    the global-max arithmetic FAILS the criterion -- the reason the model exists;
  * every random case of the GPU module keeps a stable share >= MIN_STABLE under the reference alone; the same model evaluated in fp32 -- a
    correct implementation in another summation order -- passes with the any-order constant; at 1024 keys the partition-depth constant keeps
    the cap and the any-order constant does not (both sides of the cap, as section 24 of DESIGN.md has them);
  * every wrong-kernel variant FAILS the check of a named GPU test on that test's inputs.
"""
import os
import re

import pytest
import torch

import enc_kernel_model as K
import seq_kernel_model as S
from oracle import ymt3_oracle as O
from teacher_oracle import teacher_forward, teacher_scores
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.weights import make_weights

GPU_MODULE = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_seq_kernels.py")).read()
RANDOM_TEST, SCORE_TEST = "test_attention_random_cases_meet_the_criterion", "test_attention_score_probe_is_exact"
EMBED_TEST, WINNER_TEST, EDGE_TEST = "test_embed_is_exact", "test_lm_head_winner_and_target_placement_are_exact", "test_lm_head_edges_meet_their_bounds"


def test_chained_references_are_the_teacher_oracle_with_the_roundings_off():
    cfg = YMT3Config(segment_samples=8191, max_decode_len=96, n_enc_layers=1, n_dec_layers=1, n_channels=2, eos_id=-1)
    W = {k: v.double() for k, v in make_weights(cfg, seed=1234).items()}
    B, Kc, H, P, n = 2, cfg.n_channels, cfg.n_heads, 2, 70                  # L = 72: two key tiles
    R, L = B * Kc, P + n
    g = torch.Generator().manual_seed(3)
    enc = torch.randn(B, 24, cfg.d_model, generator=g).double()
    tokens = torch.randint(0, cfg.vocab, (B, Kc, n), generator=g, dtype=torch.int32)
    prompt = torch.randint(0, cfg.vocab, (B, Kc, P), generator=g, dtype=torch.int32)
    want = teacher_forward(enc, W, cfg, tokens, prompt, bf16=False)
    assert want.dtype == torch.float64
    ec = dict(n_rows=R, n_steps=n, P=P, L=L, row0=0, V=cfg.vocab, n_channels=Kc, pad_id=cfg.pad_id, embed=W["dec.embed"], chan_embed=W["dec.chan_embed"],
              tokens=tokens.reshape(R, n), prompt=prompt.reshape(R, P))
    h = S.embed_reference(ec, dtype=torch.float64).reshape(R, L, -1)      # (the kernel's one fp32 addition is a rounding point: off here)
    bias = O.decoder_bias_by_distance(W["dec.relbias"], cfg.max_decode_len, cfg)
    ckv = O.cross_kv(enc, W, cfg, False)
    split = lambda x: x.reshape(R, -1, H, 64)
    att = lambda c: S.attention_reference(c, rounding=False)[0]["o"].reshape(R, L, -1)
    p = "dec.0."
    qkv = O.rmsnorm(h, W[p + "ln1"], cfg.ln_eps) @ W[p + "wqkv"].T
    q, k, v = (split(x) for x in qkv.split(cfg.inner, dim=-1))
    h = h + att(dict(causal=True, q=q, k=k, v=v, bias=bias, row0=0, rows_per_kv=1)) @ W[p + "wo"].T
    q = split(O.rmsnorm(h, W[p + "ln2"], cfg.ln_eps) @ W[p + "wq_c"].T)
    kc, vc = (x.transpose(1, 2) for x in ckv[0])                          # (B, T, H, 64): one slab per segment, Kc rows each
    h = h + att(dict(causal=False, q=q, k=kc, v=vc, bias=None, row0=0, rows_per_kv=Kc)) @ W[p + "wo_c"].T
    h = h + O.dense_ffn(O.rmsnorm(h, W[p + "ln3"], cfg.ln_eps), W, p, False)
    xn = O.rmsnorm(h, W["dec.ln_f"], cfg.ln_eps).reshape(R * L, -1)
    ln = torch.tensor([5, 70, 0, 33], dtype=torch.int32)
    ref = S.lm_reference(dict(xn=xn, W=W["dec.lm_head"], tokens=tokens.reshape(R, n), lengths=ln, M=R * L, L=L, P=P, n_steps=n, V=cfg.vocab, row0=0))
    assert bool(ref["written"].all())
    assert float((ref["logits"].reshape(want.shape) - want).abs().max()) < 1e-9
    assert float((ref["scores"].reshape(B, Kc, n) - teacher_scores(want, tokens, ln.reshape(B, Kc))).abs().max()) < 1e-9


@pytest.mark.parametrize("n_keys", [1, 17, 63, 64])
def test_up_to_64_keys_the_tile_schedule_is_the_oracles_attention_bit_for_bit(n_keys):
    g = torch.Generator().manual_seed(n_keys)
    q, k, v = (torch.randn(2, 3, n, 64, generator=g).bfloat16().double() for n in (n_keys, n_keys, n_keys))
    table = torch.randn(3, n_keys + 2, generator=g)
    dist = torch.arange(n_keys)[:, None] - torch.arange(n_keys)[None, :]
    bias = table.double()[:, dist.clamp(min=0)].masked_fill(dist < 0, float("-inf"))[None]
    assert torch.equal(S.attention_tiles(q, k, v, table, True)["out"], O.attention(q, k, v, bias, True, round_p=True))
    assert torch.equal(S.attention_tiles(q, k, v, None, False)["out"], O.attention(q, k, v, None, True, round_p=True))
    assert torch.equal(S.attention_tiles(q, k, v, None, False)["out"], K.attention_model(q, k, v, None)["out"])


BEYOND = [c[0] for c in S.attn_random_cases() if c[2] in (160, 1024) or c[3] == 512]


def test_beyond_64_keys_the_global_max_model_fails_the_criterion():
    """why tests/enc_kernel_model.py::attention_model could not be reused: P rounded against the global maximum differs from the tile schedule
    on stable elements wherever a later tile raises a row's maximum (the uniform cross rows, q = 0, never do)"""
    failed = {}
    for name in BEYOND:
        c = S.attn_random_case(name)
        got = S.attention_reference(c, mutant="p_global_max")[0]["out"]
        rec = S.check_attention(c, got, S.attn_random_reference(name))
        failed[name] = rec["stable_wrong"]
        assert rec["ok"] == (not c["causal"] and "_q0_" in name), (name, rec)
    print(failed)
    assert max(failed.values()) > 1000


@pytest.mark.parametrize("name", [c[0] for c in S.attn_random_cases()])
def test_random_cases_keep_the_cap_and_the_fp32_evaluation_passes(name):
    c = S.attn_random_case(name)
    ref, beta = S.attn_random_reference(name)
    own = S.check_bf16(ref["out"], ref["o"], beta)
    assert own["ok"] and own["stable_share"] >= S.MIN_STABLE, own
    f32 = S.attention_reference(c, dtype=torch.float32)[0]["out"]
    heads = dict(ref, o=K.heads(ref["o"]))
    rec = S.check_bf16(f32, ref["o"], S.attention_beta_any_order(c, heads))
    print(name, own["stable_share"], rec)
    assert rec["ok"], rec


def test_both_sides_of_the_cap_at_1024_keys():
    """why the device is judged with the depth of the kernel's partition: under the reference alone every 1024-key case keeps MIN_STABLE with
    c = 3 n + 4, and the diffuse one falls below it with the any-order c = n_keys + 2 n + 4 (section 24 of DESIGN.md has the same two sides)"""
    depth, any_order = 1.0, 1.0
    for name in [c[0] for c in S.attn_random_cases() if c[2] == 1024]:
        c = S.attn_random_case(name)
        ref, beta = S.attn_random_reference(name)
        depth = min(depth, S.check_bf16(ref["out"], ref["o"], beta)["stable_share"])
        any_order = min(any_order, S.check_bf16(ref["out"], ref["o"], S.attention_beta_any_order(c, dict(ref, o=K.heads(ref["o"]))))["stable_share"])
    print(depth, any_order)
    assert depth >= S.MIN_STABLE > any_order


def test_lm_head_fp32_evaluation_passes_and_the_uniform_row_is_log_v():
    for name, M, L, P, V, row0, wl in S.lm_edge_cases():
        c = S.lm_case(M, L, P, V, row0, wl)
        ref = S.lm_reference(c)
        lg = c["xn"].float() @ c["W"].float().T
        w = ref["written"]
        tok = c["tokens"].long().clamp(0, V - 1)
        sc = torch.full(w.shape, S.SENT)
        full = torch.full(w.shape + (V,), S.SENT)
        n_rows = M // L
        lgr = lg.reshape(n_rows, L, V)[:, P:]
        full[row0:] = lgr
        s = torch.log_softmax(lgr, -1).gather(-1, tok[row0:, :, None])[..., 0]
        if wl:
            s = s.masked_fill(torch.arange(L - P)[None, :] >= c["lengths"][row0:].long().clamp(0, L - P)[:, None], 0.0)
        sc[row0:] = s
        rec = S.check_lm(c, sc, full)
        assert rec["ok"] and rec["past_length_exact"], (name, rec)
    c = S.lm_uniform_case()
    ref = S.lm_reference(c)
    w = ref["written"]
    assert float((ref["scores"][w] + torch.log(torch.tensor(1536.0, dtype=torch.float64))).abs().max()) < 1e-12
    assert float(ref["score_bound"][w].max()) < 1e-4                      # 2^-24 (V / 4 + 3 V / 16 + ...) and the fixed ulps


# ----------------------------------------------------------------------------- sharpness
BIAS_CASE = "causal_L160_k160_q4_b20_R3_H2_row2_rpk1_fused"
SOFT_CASE = "causal_L160_k160_q0.5_b0.5_R2_H1_row0_rpk1_fused"
ATTN_SHARP = {
    "bias_by_key": BIAS_CASE, "bias_off_by_one": BIAS_CASE, "bias_next_head": BIAS_CASE, "bias_next_tile_window": BIAS_CASE, "kv_next_head": BIAS_CASE,
    "row0_ignored": BIAS_CASE, "rows_per_kv_ignored": "cross_L40_k64_q4_b0.5_R2_H2_row12_rpk13_headmajor",
    "keys_beyond_n_keys": S.find_random_case(causal=False, n_keys=65, qs=0.0, bs=0.5),       # uniform rows: 63 zero keys let in halve the output
    "no_rescale": SOFT_CASE, "rescale_num_only": SOFT_CASE, "p_global_max": SOFT_CASE, "norm_from_rounded": SOFT_CASE, "trunc_p": SOFT_CASE,
    "trunc_out": SOFT_CASE, "swap_v16": SOFT_CASE,
    "diag_lt": "causal_L65", "wave_skips_diagonal": "causal_L65",
}


def test_the_sharpness_table_covers_every_variant_and_names_real_tests():
    assert set(ATTN_SHARP) == set(S.ATTN_MUTANTS)
    for t in (RANDOM_TEST, SCORE_TEST, EMBED_TEST, WINNER_TEST, EDGE_TEST):
        assert re.search(rf"^def {t}\(", GPU_MODULE, re.M), t
    names = [c[0] for c in S.attn_random_cases()] + [c[0] for c in S.score_probe_cases()]
    assert all(v in names for v in ATTN_SHARP.values())


@pytest.mark.parametrize("mutant", S.ATTN_MUTANTS)
def test_every_wrong_attention_kernel_fails_a_named_gpu_test(mutant):
    name = ATTN_SHARP[mutant]
    if name.startswith("causal_L65"):                                      # SCORE_TEST
        _, causal, L, nk, n_rows, H, row0, rpk, layout = next(x for x in S.score_probe_cases() if x[0] == name)
        c, key = S.score_probe_case(causal, L, nk, n_rows, H, row0, rpk, layout)
        assert S.check_score_probe(c, key, S.attention_reference(c)[0]["out"].bfloat16())["ok"]
        rec = S.check_score_probe(c, key, S.attention_reference(c, mutant=mutant)[0]["out"].bfloat16())
    else:                                                                  # RANDOM_TEST
        c = S.attn_random_case(name)
        rec = S.check_attention(c, S.attention_reference(c, mutant=mutant)[0]["out"], S.attn_random_reference(name))
    print(mutant, rec)
    assert not rec["ok"], rec


def test_the_probes_value_code_is_injective():
    """no other (slab, key, head) row of a probe's V is bit-equal to the one a row must return: an aliased address could not pass 'bit for bit'"""
    for n_slabs, n_keys, H in ((1, 1024, 64), (5, 1024, 2), (2, 512, 2), (3, 160, 2)):
        rows = S.v_code(n_slabs, n_keys, H).reshape(-1, 64).view(torch.int16)
        assert torch.unique(rows, dim=0).shape[0] == rows.shape[0], (n_slabs, n_keys, H)
    assert float(S.v_code(5, 1024, 64).float().max()) <= 250


def test_the_random_cases_are_the_six_regimes_at_every_size():
    cases = S.attn_random_cases()
    assert len(cases) == 96 and len({c[0] for c in cases}) == 96
    assert {(c[1], c[3], c[9], c[10]) for c in cases} == {(True, L, qs, bs) for L in S.SCORE_CAUSAL_L for qs, bs in K.ATTN_REGIMES} | {
        (False, nk, qs, bs) for nk in S.SCORE_CROSS_KEYS for qs, bs in K.ATTN_REGIMES}


def test_the_exact_probes_are_exact_under_the_reference_and_in_fp32():
    for case in S.score_probe_cases():
        name, causal, L, nk, n_rows, H, row0, rpk, layout = case
        if L == 1024:
            continue                                                        # (the same construction; 1024 keys in float64 cost seconds)
        c, key = S.score_probe_case(causal, L, nk, n_rows, H, row0, rpk, layout)
        for dtype in (torch.float64, torch.float32):
            assert S.check_score_probe(c, key, S.attention_reference(c, dtype=dtype)[0]["out"].bfloat16())["ok"], (name, dtype)
    # the bias probe at a size the CPU affords: every distance the lone peak once
    L, H = 160, 8
    for launch in range(L // H):
        c, key = S.bias_probe_case(launch, L, H)
        got = S.attention_reference(c)[0]["out"].bfloat16()
        rec = S.check_bias_probe(c, key, got)
        assert rec["ok"] and rec["exact"], (launch, rec)
        if launch == 3:
            for mutant in ("bias_by_key", "bias_off_by_one", "bias_next_head", "bias_next_tile_window"):
                assert not S.check_bias_probe(c, key, S.attention_reference(c, mutant=mutant)[0]["out"].bfloat16())["ok"], mutant


@pytest.mark.parametrize("mutant", S.EMBED_MUTANTS)
def test_every_wrong_embed_fails_the_embed_test(mutant):
    oks = []
    for n_rows, n, P, row0, Kc in S.EMBED_CASES:
        c = S.embed_case(n_rows, n, P, row0, Kc)
        assert S.check_embed(c, S.embed_reference(c))["ok"]
        oks.append(S.check_embed(c, S.embed_reference(c, mutant))["ok"])
    assert not all(oks), oks


@pytest.mark.parametrize("mutant", S.LM_MUTANTS)
def test_every_wrong_lm_head_fails_a_named_gpu_test(mutant):
    if mutant in ("lm_j_le_len", "lm_row0_ignored", "lm_j_from_position_0"):          # EDGE_TEST
        oks = []
        for name, M, L, P, V, row0, wl in S.lm_edge_cases():
            c = S.lm_case(M, L, P, V, row0, wl)
            oks.append(S.check_lm(c, S.lm_reference(c, mutant)["scores"].float())["ok"])
        assert not all(oks), oks
    else:                                                                              # WINNER_TEST
        c, want, _ = S.lm_winner_case()
        assert S.check_lm_winner(c, want, S.lm_reference(c)["scores"].float())["ok"]
        assert not S.check_lm_winner(c, want, S.lm_reference(c, mutant)["scores"].float())["ok"]


def test_the_winner_probe_places_the_target_everywhere():
    """every (tile parity, lane quarter, element) = target mod 32, in both 16-row halves of every wave: (flat row / 16) mod 8"""
    c, want, tgt = S.lm_winner_case()
    m = torch.arange(c["M"])
    plain = m < c["M"] // 2
    seen = {(int(g), int(r)) for g, r in zip((m // 16 % 8)[plain], (tgt % 32)[plain])}
    assert seen == {(g, r) for g in range(8) for r in range(32)}
    assert int((want == 0).sum()) >= c["M"] // 2


def test_the_doors_are_in_the_header_and_the_library():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ymt3.h")).read()
    runtime = open(os.path.join(root, "yourmt3_amd", "csrc", "runtime.hip")).read()
    for name, launcher in (("ymt3_test_seq_embed", "launch_seq_embed"), ("ymt3_test_dec_seq_attention", "launch_dec_seq_attention"),
                           ("ymt3_test_seq_lm_head", "launch_seq_lm_head_score")):
        assert re.search(rf"\bint {name}\(", header)
        body = runtime[runtime.index(f'extern "C" int {name}('):]
        body = body[:body.index("\n}\n")]
        assert body.count("LAUNCH(") == 1 and f"LAUNCH({launcher}(" in body and "h->" not in body
        assert runtime.count(name + "(") == 1                             # nothing on the production path calls a door
