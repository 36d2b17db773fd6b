"""tests/select_kernel_model.py without a GPU: the reference agrees with torch on plain inputs, the case builders place what they claim, and
every named case of tests/test_select_kernels.py rejects the mutants it is there for -- a kernel with that defect cannot pass it."""
import numpy as np
import pytest
import torch

import select_kernel_model as S

_CASES = S.greedy_cases()


def test_reference_agrees_with_torch_on_plain_rows():
    rng = np.random.default_rng(0)
    for V in (16, 272, 1536):
        x = rng.normal(0, 3, (7, V)).astype(np.float32)
        lp = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
        for r in range(7):
            i = S.pick(x[r])
            assert i == int(torch.from_numpy(x[r]).argmax())
            assert abs(S.score(x[r], i) - lp[r, i]) < 1e-12 and abs(S.score(x[r], 3) - lp[r, 3]) < 1e-12
        al = rng.random(V) < 0.3
        al[5] = True
        masked = torch.from_numpy(x[0]).double().masked_fill(~torch.from_numpy(al), float("-inf"))
        assert S.pick(x[0], al) == int(masked.argmax())
        assert abs(S.score(x[0], 5, al) - torch.log_softmax(masked, -1)[5].item()) < 1e-12
        assert S.score(x[0], int(np.flatnonzero(~al)[0]), al) == -np.inf


def test_reference_special_values():
    V = 48
    nan, ninf = np.full(V, np.nan, np.float32), np.full(V, -np.inf, np.float32)
    assert S.pick(nan) == 0 and S.pick(ninf) == 0 and np.isnan(S.score(nan, 0)) and np.isnan(S.score(ninf, 0))
    al = np.zeros(V, bool)
    assert S.pick(np.zeros(V, np.float32), al) == V - 1 and S.score(np.zeros(V, np.float32), V - 1, al) == -np.inf
    al[[7, 30]] = True
    assert S.pick(nan, al) == 7 and S.pick(ninf, al) == 7
    x = np.zeros(V, np.float32)
    x[7] = np.nan
    assert S.pick(x, al) == 30 and np.isnan(S.score(x, 30, al))
    x[:] = 1.5
    assert abs(S.score(x, 3) + np.log(V)) < 1e-12 and abs(S.score(x, 7, al) + np.log(2)) < 1e-12


def test_bf16_helpers_agree_with_torch():
    x = np.random.default_rng(1).normal(0, 100, 4096).astype(np.float32)
    t = torch.from_numpy(x).bfloat16()
    assert np.array_equal(S.bf16_bits(x), t.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(S.bf16_f32(S.bf16_bits(x)), t.float().numpy())
    assert S.bf16_bits(np.float32(S.SENT)) == S.SENT_BF16
    al = np.random.default_rng(2).random((3, 1040)) < 0.5
    w = S.allowed_words(al)
    assert w.shape == (3, 33)
    back = ((w[:, np.arange(1040) >> 5] >> (np.arange(1040) & 31).astype(np.uint32)) & 1).astype(bool)
    assert np.array_equal(back, al) and (w[:, 32] >> 16 == 0xffff).all()


@pytest.mark.parametrize("V", S.PLACE_V)
def test_placement_rows_place_what_their_labels_say(V):
    x, labels = S.placement_rows(V)
    kinds = {lab[0] for lab in labels}
    assert kinds == {"single", "tie", "nan_low", "all_nan", "all_ninf"}
    for row, lab in zip(x, labels):
        want = lab[3] if lab[0] == "nan_low" else 0 if lab[0].startswith("all") else lab[2]
        assert S.pick(row) == want, (V, lab)
    assert set(S.place_set(V)) >= {0, V - 1} and all(0 <= i < V for i in S.place_set(V))
    assert all(c.R <= S.MAX_ROWS for c in S.placement_cases(V)) and sum(c.R for c in S.placement_cases(V)) == len(x)


@pytest.mark.parametrize("name", list(_CASES))
def test_case_rejects_its_mutants(name):
    c, kills = _CASES[name]
    ref = S.token_step_ref(c)
    bad, _ = S.compare(c, ref, S.token_step_ref(c))
    assert not bad
    for mut in kills:
        bad, _ = S.compare(c, ref, S.token_step_ref(c, (mut,)))
        assert bad, (name, mut)


def test_every_mutant_is_rejected_by_a_named_case():
    killed = {mut for _, kills in _CASES.values() for mut in kills}
    assert killed == set(S.MUTANTS)


def test_uniform_rows_make_the_score_bound_sharp():
    """one dropped term moves -log n by log(n / (n - 1)) >= 1 / n: more than three times 1e-4 + 1e-5 |ref| at every V the uniform cases use"""
    used = [c.V for name, (c, _) in _CASES.items() if name.startswith("uniform")]
    assert max(used) == 1536
    for V in used:
        assert np.log(V / (V - 1)) > 3 * (S.SCORE_ABS + S.SCORE_REL * np.log(V))


def test_score_comparison_knows_the_special_values():
    ref = np.array([np.nan, -np.inf, 0.0, S.SENT, -1.0])
    assert S.compare_scores(ref, ref.copy())[0]
    for i, v in enumerate([0.0, np.nan, -1e-7, -1.0, -1.0 - 2.2e-4]):
        got = ref.copy()
        got[i] = v
        assert not S.compare_scores(ref, got)[0], i
    got = ref.copy()
    got[4] = -1.0 - 1e-5
    assert S.compare_scores(ref, got)[0]


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("V", [16, 272])
def test_beam_step0_case_has_no_undecided_comparison_and_expands_beam_0_only(W, V):
    from beam_oracle import host_select
    _, run, acc = S.beam_step0_case(2, W, V)
    for g in range(2):
        assert S.undecided(acc[g], W) == 0
        sel = host_select(acc[g], W, -1, False, [], 1, 1.0)
        assert [p for p, _, _ in sel["beams"]] == [0] * W and not sel["entered"] and not sel["done"]
        assert [t for _, t, _ in sel["beams"]] == list(np.argsort(-acc[g, 0])[:W])
        # a kernel that expanded every beam at step 0 (all runs 0) would pick other parents: the case sees it
        sel_all = host_select(acc[g] - run[g][:, None], W, -1, False, [], 1, 1.0)
        assert [p for p, _, _ in sel_all["beams"]] != [0] * W


_SEQ = S.beam_sequences()


@pytest.mark.parametrize("name", list(_SEQ))
def test_beam_sequence_is_decided_shows_its_events_and_rejects_its_mutants(name):
    """under the reference alone: zero undecided comparisons (each is an exact tie or has a float64 margin >= 2e-4), the situations the
    sequence is there for occur, and a select with the named defect leaves another state at some position"""
    p, steps, N, want, kills = _SEQ[name]
    states, ev = S.beam_simulate(p, steps)
    assert ev["undecided"] == 0 and len(states) == p.P + p.ns
    assert all(ev[w] > 0 for w in want), ev
    assert all((st.n_fin == p.W).all() for st in states[-1:])            # the length limit fills every slot
    for mut in kills:
        other, _ = S.beam_simulate(p, steps, (mut,))
        assert any(S.beam_compare(a, b)[0] for a, b in zip(states, other)), (name, mut)


def test_beam_sequences_cover_every_situation_and_mutant():
    seen = {}
    for p, steps, N, want, kills in _SEQ.values():
        for k, v in S.beam_simulate(p, steps)[1].items():
            seen[k] = seen.get(k, 0) + v
    assert all(seen[k] > 0 for k in ("hit_in_w", "hit_outside_w", "displaced", "store_reused", "filled", "done_idle", "tie_across", "dead", "at_limit")), seen
    assert {m for *_, kills in _SEQ.values() for m in kills} == set(S.BEAM_MUTANTS)
    assert {p.W for p, *_ in _SEQ.values()} == {1, 2, 4, 8} and {p.V for p, *_ in _SEQ.values()} >= {16, 272, 1536}
    assert {p.alpha for p, *_ in _SEQ.values()} == {0.0, 1.0, 2.0} and any(N < p.W for p, _, N, *_ in _SEQ.values())


def test_beam_step_reference_follows_the_oracle_search_over_a_sequence():
    """beam_oracle.beam_search over a real decoder's logits, and the step reference driven by the same logits: the same beams (parent, token)
    and runs at every step, the same slots at the end"""
    from beam_oracle import beam_search
    from oracle import ymt3_oracle as O
    from test_oracle_vs_thirdparty import CFG
    from yourmt3_amd.weights import make_weights
    W, ns = 3, 8
    weights = make_weights(CFG, seed=1234)
    _, enc = O.encode(O.synthetic_audio(2, CFG), weights, CFG, bf16=False)
    eos = int(O.greedy_decode(enc, weights, CFG.with_(eos_id=-1), 6, bf16=False)[0, 0, 3])
    cfg = CFG.with_(eos_id=eos)
    got = beam_search(enc, weights, cfg, ns, False, W, W, 1.0, return_logits=True)
    G = got.trace.shape[1]
    p = S.beam_params(G, W, cfg.vocab, ns, eos=eos, pad=cfg.pad_id, alpha=1.0)
    s = S.beam_init_state(p)
    for j in range(got.steps_run):
        o, ev = S.beam_step_ref(s, got.logits[j].reshape(G * W, cfg.vocab).numpy(), p)
        for g in range(G):
            if s.n_fin[g] < W:
                assert np.array_equal(o.parent[g * W:(g + 1) * W], got.trace[j, g, :, 0]) and np.array_equal(o.feed[g * W:(g + 1) * W], got.trace[j, g, :, 1])
                assert np.allclose(o.run[g * W:(g + 1) * W], got.run[j, g], rtol=1e-6, atol=1e-4)
        s = S._as_device(o)
    for g in range(G):
        assert int(s.n_fin[g]) == len(got.fins[g])
        for i, f in enumerate(got.fins[g]):
            assert abs(s.fin_score[g * W + i] - f["score"]) < 1e-4 and s.fin_len[g * W + i] == f["len"] and s.fin_tok[g * W + i] == f["token"]


def test_beam_slot_case_is_decided_and_has_groups_at_different_positions_one_stopped():
    p, n_queue, actions = S.beam_slot_case()
    s = S.beam_slot_empty_state(p)
    seen_stopped_beside_live = False
    for a in actions:
        if a[0] == "start":
            s = S.beam_slot_start_ref(s, p, a[1], a[2])
            continue
        live = [g for g in range(p.G) if not s.finished[g * p.W]]
        seen_stopped_beside_live |= 0 < len(live) < p.G and len({int(s.row_pos[g * p.W]) for g in live}) == len(live)
        o, ev = S.beam_step_ref(s, a[1], p)
        assert ev["undecided"] == 0
        stopped = [g for g in range(p.G) if s.finished[g * p.W]]
        assert all(np.array_equal(o.row_pos[g * p.W:(g + 1) * p.W], s.row_pos[g * p.W:(g + 1) * p.W]) for g in stopped)
        other, _ = S.beam_step_ref(s, a[1], p, ("anc_at_t",))
        assert S.beam_compare(o, other)[0] or not live
        s = S._as_device(o)
    assert seen_stopped_beside_live and (s.n_fin == p.W).all() and (s.finished == 1).all()
