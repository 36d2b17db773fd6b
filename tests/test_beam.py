"""Beam search on the device (include/ymt3.h, beam search) against the host and the CPU oracle.

The search is discrete, so the comparisons go through the debug trace (ymt3_debug_beam_trace), the way the MoE router is tested:
  * selection: from the device's OWN raw logits and its own `run` of the previous step the host recomputes every candidate in float64; the
    device's choices must be the host's wherever every deciding comparison has a margin >= 2e-4 (two scores, each within the 1e-4 the
    token-score tests allow against float64), and within 2e-4 of the cut below that;
  * parity: the device's (parent, token) trace is fed to tests/beam_oracle.py (bf16 emulation); the raw logits of every running beam are
    compared at every step with the decoder's usual bounds, and every device choice must be the oracle's own wherever the oracle's
    deciding margin is >= TAU, else within TAU of its cut.  A wrong parent anywhere in the ancestry-addressed attention is an O(1) error;
  * results: tokens / sequence scores / token scores equal what the host derives from the device's own numbers.
The covered shares are written to beam_parity_report.json under $YMT3_REPORT_DIR (default results/; committed copy:
profiles/beam_parity_report.json)."""
import atexit
import json
import os

import numpy as np
import pytest
import torch

from beam_oracle import NEG, beam_search, host_select
from oracle import ymt3_oracle as O
from test_gpu_parity import MC3, SMALL, TAU, _model
from yourmt3_amd.config import FFN_MOE, YMT3Config
from yourmt3_amd.weights import make_weights

pytestmark = pytest.mark.gpu
MARGIN = 2e-4
_REPORT = {}


def _dump_report():
    if _REPORT:
        try:
            out = os.environ.get("YMT3_REPORT_DIR", "results")
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, "beam_parity_report.json"), "w") as f:
                json.dump(_REPORT, f, indent=1)
        except OSError:
            pass


atexit.register(_dump_report)


def _separate(monkeypatch, hooks=True):
    monkeypatch.setenv("YMT3_NO_ATTN_PAIR", "1")
    monkeypatch.setenv("YMT3_NO_GEMM_CHAIN", "1")
    if hooks:
        monkeypatch.setenv("YMT3_DEBUG_HOOKS", "1")


def _enc(m, cfg, B, seed=0):
    _, enc = O.encode(O.synthetic_audio(B, cfg, seed=seed), m.weights, cfg, True)
    return enc


def _pick_eos(m, cfg, enc, n, which=0):
    """a token the oracle's greedy stream emits within the first ten steps of some rows"""
    g = O.greedy_decode(enc, m.weights, cfg.with_(eos_id=-1), min(n, 12), True)
    ids, counts = torch.unique(g[..., :10], return_counts=True)
    order = sorted(zip(counts.tolist(), ids.tolist()), key=lambda x: (-x[0], x[1]))
    return int(order[which % len(order)][1])


def _run(m, enc, n, W, N=None, alpha=1.0, prompt=None, constraint=None, start_states=None, logits=True):
    """one traced beam call -> dict of host arrays"""
    G = enc.shape[0] * m.cfg.n_channels
    tr, run, lg = m.beam_trace(n, G, W, logits=logits)
    tok, ts, ss = m.decode(enc.bfloat16().cuda(), n, prompt=prompt, return_scores=True, num_beams=W, num_return_sequences=N or W,
                           length_penalty=alpha, constraint=constraint, start_states=start_states, _force_beam=True)
    torch.cuda.synchronize()
    out = dict(tokens=tok.cpu().numpy().reshape(G, N or W, n), ts=ts.cpu().numpy().reshape(G, N or W, n), ss=ss.cpu().numpy().reshape(G, N or W),
               trace=tr.cpu().numpy().astype(np.int64), run=run.cpu().numpy(), logits=lg.cpu().numpy() if lg is not None else None)
    assert m._lib.ymt3_debug_beam_trace(m._handle, None, None, None, 0, 0) == 0
    return out


def _host_follow(cfg, r, n, W, alpha, automaton=None, start_states=None):
    """Follow the device's trace on the host with the device's own raw logits and run values (float64): per step the host's own selection
    (host_select) beside the device's, the decided flags, and the results the host derives (steps 3-7 of the semantics)."""
    G, V = r["trace"].shape[1], cfg.vocab
    allowed = nxt = None
    state = np.zeros((G, W), np.int64)
    if automaton is not None:
        allowed, nxt = automaton.allowed, automaton.next.astype(np.int64)
        if start_states is not None:
            st0 = np.asarray(start_states)
            st0 = np.tile(st0, G // cfg.n_channels) if st0.ndim == 1 else st0.reshape(G)
            state[:] = st0.reshape(G, 1)
    run_prev = np.full((G, W), NEG)
    run_prev[:, 0] = 0.0
    fins = [[] for _ in range(G)]
    hist_tok = np.zeros((G, W, n), np.int64)
    hist_lp = np.zeros((G, W, n))
    steps = decided = 0
    clean = np.ones(G, bool)            # no undecided step of the group involved a finishing candidate
    max_run_err = 0.0
    for j in range(n):
        for g in range(G):
            if len(fins[g]) >= W:
                assert (r["trace"][j, g, :, 0] == np.arange(W)).all() and (r["trace"][j, g, :, 1] == cfg.pad_id).all(), (j, g)
                continue
            lg = torch.from_numpy(r["logits"][j, g]).double()
            assert bool(torch.isfinite(lg).all()), (j, g)
            if allowed is not None:
                lg = lg.masked_fill(~torch.from_numpy(allowed[state[g]]), float("-inf"))
            lp = torch.log_softmax(lg, -1).numpy()
            acc = run_prev[g][:, None] + lp
            at_limit = j + 1 >= n
            sel = host_select(acc, W, cfg.eos_id, at_limit, fins[g], j + 1, alpha)
            # every comparison that decided the step: the order of the 2W + 1 best candidates (the cut included) and of the merged slots
            # the candidates the step consulted: the first W (finishing candidates enter from there) and everything down to the last one that
            # became a running beam; each adjacent comparison among them, and the one that cut the list off behind them, decided something
            key = np.sort(np.where(np.isnan(acc), NEG, acc).reshape(-1))[::-1][:2 * W + 1]
            key = key[np.isfinite(key)]
            chosen = sorted(range(2 * W), key=lambda c: (-sel["kmod"][c], c))[:W]
            last_used = max(max(chosen), W - 1)
            gaps = list(-np.diff(key))[:last_used + 1]
            slot_gaps = []
            if sel["entered"] or any(sel["hit"][:W]):
                sc = sorted([s["score"] for s in sel["fin"]] + [s["score"] for s in fins[g]], reverse=True)
                slot_gaps = [a - b for a, b in zip(sc, sc[1:]) if a != b]
            ok = (min(gaps + slot_gaps) if gaps + slot_gaps else 1.0) >= MARGIN
            # what the finished slots depend on: which hit candidates are among the first W, in which order, and the merged slot order
            hit_w = sel["hit"] + [False]
            if any(gaps[i] < MARGIN and (hit_w[i] or hit_w[i + 1]) for i in range(min(W, len(gaps)))) or any(x < MARGIN for x in slot_gaps):
                clean[g] = False
            steps += 1
            decided += int(ok)
            dev = [(int(p), int(t)) for p, t in r["trace"][j, g]]
            assert all(0 <= p < W and 0 <= t < V for p, t in dev), (j, g, dev)
            forced = host_select(acc, W, cfg.eos_id, at_limit, fins[g], j + 1, alpha, forced=dev)
            if ok:
                assert dev == [(p, t) for p, t, _ in sel["beams"]], (j, g, dev, sel["beams"])
            else:
                cut = sorted(sel["kmod"], reverse=True)[W - 1]
                assert all(rr >= cut - MARGIN for _, _, rr in forced["beams"]), (j, g, forced["beams"], cut)
            for i, (p, t, rr) in enumerate(forced["beams"]):
                got = float(r["run"][j, g, i])
                err = abs(got - rr)
                assert err <= 1e-4 + 1e-5 * abs(rr), (j, g, i, got, rr)
                if rr > NEG / 2:
                    max_run_err = max(max_run_err, err)
            for s in sel["fin"]:
                if "new" in s:
                    s["tokens"] = list(hist_tok[g, s["parent"], :j]) + [s["token"]]
                    del s["new"]
            fins[g] = sel["fin"]
            ht, hl, st = hist_tok[g].copy(), hist_lp[g].copy(), state[g].copy()
            for i, (p, t) in enumerate(dev):
                hist_tok[g, i] = ht[p]
                hist_tok[g, i, j] = t
                if nxt is not None:
                    state[g, i] = nxt[st[p], t]
            run_prev[g] = r["run"][j, g].astype(np.float64)
    return dict(fins=fins, steps=steps, decided=decided, clean=clean, max_run_err=max_run_err)


def _check_results(cfg, r, host, n, W, N, alpha, name):
    """tokens / seq_scores / token_scores against what the host derived, best-first order, PAD after the last token, token scores summing to
    seq_score * len^alpha.  The exact comparison covers the groups in which no comparison that a finished slot depends on (a finishing
    candidate's rank among the first W, the merged slot order) fell below the 2e-4 margin: below it host and device may legitimately
    differ.  The covered share is recorded; every covered group must match exactly, and at most one group of a case may be left out (a
    sub-margin comparison on a finishing candidate is a once-in-hundreds-of-steps event; more than one per case means something else)."""
    G = r["tokens"].shape[0]
    compared = 0
    for g in range(G):
        ss = r["ss"][g]
        assert all(ss[i] >= ss[i + 1] for i in range(N - 1)), (g, ss)
        for k in range(N):
            toks = r["tokens"][g, k]
            ln = n if (cfg.eos_id < 0 or cfg.eos_id not in toks.tolist()) else toks.tolist().index(cfg.eos_id) + 1
            assert (toks[ln:] == cfg.pad_id).all() and (r["ts"][g, k, ln:] == 0).all(), (g, k)
            assert 0 <= toks.min() and toks.max() < cfg.vocab
            assert abs(float(r["ts"][g, k].astype(np.float64).sum()) - float(ss[k]) * ln ** alpha) <= 1e-4 * ln, (g, k)
        if not host["clean"][g]:
            continue
        compared += 1
        assert len(host["fins"][g]) == W
        for k in range(N):
            s = host["fins"][g][k]
            assert r["tokens"][g, k, :s["len"]].tolist() == [int(t) for t in s["tokens"]], (g, k)
            assert (r["tokens"][g, k, s["len"]:] == cfg.pad_id).all()
            assert abs(float(r["ss"][g, k]) - s["score"]) <= 1e-5 * abs(s["score"]) + 1e-7, (g, k, r["ss"][g, k], s["score"])
    _REPORT[name + "_results"] = {"groups": G, "groups_compared_exactly": compared}
    assert compared >= G - 1, (compared, G)


# ----------------------------------------------------------------------------- 4. W = 1 is greedy
@pytest.mark.parametrize("cfg", [SMALL, MC3.with_(max_decode_len=64)], ids=["dense", "mc3"])
def test_beam_width_one_is_greedy_through_the_beam_kernels(cfg, monkeypatch):
    """decode(num_beams=1, _force_beam=True) runs the beam kernels (the private switch of YourMT3.decode); the logits of its one running beam
    are the greedy call's, bit for bit, up to each row's first step whose greedy top-2 margin is below 2e-4 (adding `run` in f32 can merge two
    logits that close into a tie, which resolves to the lower index), and the ids are equal on that range."""
    _separate(monkeypatch)
    cfg = cfg.with_(eos_id=-1)
    B = 3 if cfg.n_channels > 1 else 8                  # 8 rows, 9 with three channels
    n = 64
    m = _model(cfg, max_batch=B)
    enc = _enc(m, cfg, B)
    ref_t, ref_l = m.decode(enc.bfloat16().cuda(), n, return_logits=True)
    ref_t, ref_l = ref_t.cpu().reshape(-1, n), ref_l.cpu().reshape(-1, n, cfg.vocab)
    r = _run(m, enc, n, 1)
    top = ref_l.topk(2, -1).values
    low = (top[..., 0] - top[..., 1]) < MARGIN
    covered = 0
    for g in range(ref_t.shape[0]):
        idx = low[g].nonzero().flatten()
        stop = int(idx[0]) if idx.numel() else n
        covered += stop
        assert np.array_equal(r["logits"][:stop, g, 0], ref_l[g, :stop].numpy()), g
        assert r["tokens"][g, 0, :stop].tolist() == ref_t[g, :stop].tolist(), g
    share = covered / ref_t.numel()
    _REPORT[f"w1_greedy_{cfg.n_channels}ch"] = {"pairs": int(ref_t.numel()), "covered_share": share}
    assert share >= 0.9, share
    m.close()


# ----------------------------------------------------------------------------- 5. selection, 7. results
def _grammar(cfg):
    from yourmt3_amd.task_manager import TaskManager
    tm = TaskManager("mc13_full_plus_256" if cfg.n_channels == 13 else "mt3_full_plus")
    return tm.event_automaton()


SEL_CASES = [
    ("dense_w2_a0", SMALL, 4, 2, 0.0, False, False),
    ("dense_w4_a1", SMALL, 4, 4, 1.0, False, False),
    ("dense_w8_a1_prompt", SMALL, 2, 8, 1.0, True, False),
    ("dense_w4_a0_grammar", SMALL, 4, 4, 0.0, False, True),
    ("mc13_w2_a1", YMT3Config(segment_samples=8191, max_decode_len=32, n_channels=13), 1, 2, 1.0, False, False),
    ("moe_w4_a1", YMT3Config(segment_samples=8191, max_decode_len=64, dec_ffn=FFN_MOE), 2, 4, 1.0, False, False),
]


@pytest.mark.parametrize("name,cfg,B,W,alpha,prompted,grammar", SEL_CASES, ids=[c[0] for c in SEL_CASES])
def test_selection_is_exact_given_the_devices_own_numbers(name, cfg, B, W, alpha, prompted, grammar, monkeypatch):
    _separate(monkeypatch)
    m0 = _Weights(make_weights(cfg, seed=1234))
    enc = _enc(m0, cfg, B)
    eos = _pick_eos(m0, cfg, enc, 12, which=1)
    cfg = cfg.with_(eos_id=eos)
    m = _model(cfg, max_batch=B * W)
    P = 4 if prompted else 0
    n = min(48, cfg.max_decode_len - P)
    prompt = torch.arange(B * cfg.n_channels * P).reshape(B, cfg.n_channels, P) % 50 + 3 if prompted else None
    aut = st = c = None
    if grammar:
        aut, st = _grammar(cfg)
        c = m.compile_constraint(aut)
    r = _run(m, enc, n, W, alpha=alpha, prompt=prompt, constraint=c, start_states=st)
    host = _host_follow(cfg, r, n, W, alpha, automaton=aut, start_states=st)
    share = host["decided"] / max(host["steps"], 1)
    _REPORT[name] = {"steps": host["steps"], "decided_share": share, "max_run_err": host["max_run_err"]}
    print(name, _REPORT[name])
    assert share >= 0.95, share
    _check_results(cfg, r, host, n, W, W, alpha, name)
    # N < W returns the prefix of the N = W result, bit for bit
    tok, ts, ss = m.decode(enc.bfloat16().cuda(), n, prompt=prompt, return_scores=True, num_beams=W, num_return_sequences=1, length_penalty=alpha,
                           constraint=c, start_states=st, _force_beam=True)
    G = B * cfg.n_channels
    assert np.array_equal(tok.cpu().numpy().reshape(G, n), r["tokens"][:, 0])
    assert np.array_equal(ss.cpu().numpy().reshape(G), r["ss"][:, 0]) and np.array_equal(ts.cpu().numpy().reshape(G, n), r["ts"][:, 0])
    m.close()


# ----------------------------------------------------------------------------- 6. parity with the CPU oracle
def _ancestry_stats(trace, W):
    """share of (step, beam) records whose parent is not the beam's own index; the largest number of distinct physical rows in one history"""
    n, G = trace.shape[:2]
    moved = float((trace[..., 0] != np.arange(W)[None, None, :]).mean())
    spans = 0
    for g in range(G):
        hist = [[w] for w in range(W)]                  # physical rows holding each beam's positions
        for j in range(n):
            hist = [hist[int(p)] + [i] for i, p in enumerate(trace[j, g, :, 0])]
            spans = max(spans, max(len(set(h)) for h in hist))
    return moved, spans


PARITY_CASES = [
    ("dense_4x4x64", SMALL, 4, 4, 64, 0, {}),
    ("dense_2x8x128_l1024_prompt", YMT3Config(segment_samples=8191, max_decode_len=1024), 2, 8, 128, 300, {}),
    ("dense_7x4_2wave", SMALL, 7, 4, 48, 0, {"YMT3_SELF_ATTN_2WAVE": "1"}),
    ("mc3_w4", MC3, 2, 4, 32, 0, {}),
    ("mc13_w2", YMT3Config(segment_samples=8191, max_decode_len=32, n_channels=13), 1, 2, 32, 0, {}),
]


@pytest.mark.parametrize("name,cfg,B,W,n,P,env", PARITY_CASES, ids=[c[0] for c in PARITY_CASES])
def test_parity_with_the_cpu_oracle_through_the_devices_trace(name, cfg, B, W, n, P, env, monkeypatch):
    _separate(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(cfg.with_(eos_id=-1), max_batch=B * W)
    enc = _enc(m, cfg, B)
    G, V = B * cfg.n_channels, cfg.vocab
    prompt = (torch.arange(G * P).reshape(B, cfg.n_channels, P) * 7 % 97 + 3) if P else None
    r = _run(m, enc, n, W, alpha=1.0, prompt=prompt)
    moved, spans = _ancestry_stats(r["trace"], W)
    ref = beam_search(enc, m.weights, cfg.with_(eos_id=-1), n, True, W, W, 1.0, prompt=prompt, forced_trace=r["trace"], return_logits=True)
    ref_l = ref.logits.numpy()                           # (n, G, W, V)
    d = np.abs(r["logits"] - ref_l) / float(ref_l.std())          # in units of the logits' std, as the bounds are stated
    rec = {"steps": n * G, "logits_std": float(ref_l.std()), "logits_max_abs": float(d.max()), "logits_mean_abs": float(d.mean()), "parent_moved_share": moved, "max_rows_in_a_history": spans}
    safe = differ = 0
    for j in range(n):
        for g in range(G):
            own = ref.own[j][g]
            km = sorted(own["kmod"], reverse=True)[:W + 1]
            margin = min(a - b for a, b in zip(km, km[1:]))
            dev = [(int(p), int(t)) for p, t in r["trace"][j, g]]
            if margin >= TAU:
                safe += 1
                differ += int(dev != [(p, t) for p, t, _ in own["beams"]])
            else:
                assert all(ref.run[j, g, i] >= km[W - 1] - TAU for i in range(W)), (j, g)
    rec.update(safe_fraction=safe / (n * G), choices_differ_where_safe=differ)
    _REPORT[name] = rec
    print(name, rec)
    assert moved >= 0.25 and spans >= min(3, W), rec         # (a group of W = 2 has two physical rows: a history can span no more)
    assert rec["logits_max_abs"] < 0.06 and rec["logits_mean_abs"] < 6e-3, rec
    assert differ == 0, rec
    m.close()


# ----------------------------------------------------------------------------- 8. properties
def test_beam_properties(monkeypatch):
    _separate(monkeypatch, hooks=False)
    cfg0 = SMALL.with_(eos_id=-1)
    m0 = _model(cfg0, max_batch=16)
    enc = _enc(m0, cfg0, 4)
    e = enc.bfloat16().cuda()
    n, W = 48, 4
    greedy_before = m0.decode(e, n).cpu()
    a = [x.cpu() for x in m0.decode(e, n, return_scores=True, num_beams=W, num_return_sequences=W)]       # eos_id < 0: runs to the limit
    b = [x.cpu() for x in m0.decode(e, n, return_scores=True, num_beams=W, num_return_sequences=W)]
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "two calls give the same bits"
    assert a[0].shape == (4, 1, W, n) and int(a[0].min()) >= 0 and int(a[0].max()) < cfg0.vocab
    assert torch.equal(m0.decode(e, n).cpu(), greedy_before), "a greedy call after a beam call gives its usual bits"
    alone = [x.cpu() for x in m0.decode(e[2:3], n, return_scores=True, num_beams=W, num_return_sequences=W)]
    assert all(torch.equal(x[0], y[2]) for x, y in zip(alone, a)), "a group does not depend on the other groups of the batch"
    # argument errors leave the handle usable
    from yourmt3_amd._lib import YMT3Error
    with pytest.raises((ValueError, YMT3Error)):
        m0.decode(e, n, num_beams=8, num_return_sequences=1)          # 4 x 8 rows > max_batch 16
    with pytest.raises(ValueError):
        m0.decode(e, n, num_beams=4, forced=torch.zeros(4, 1, n, dtype=torch.int32))
    import ctypes
    from yourmt3_amd import _lib
    bad = _lib.BeamParams(9, 1, 1.0)
    tok = torch.empty(4, 1, 1, n, dtype=torch.int32, device="cuda")
    rc = m0._lib.ymt3_decode_beam(m0._handle, ctypes.c_void_p(e.data_ptr()), 4, n, None, 0, ctypes.byref(bad), ctypes.c_void_p(tok.data_ptr()),
                                  None, None, None, None, None)
    assert rc == 1 and b"num_beams" in m0._lib.ymt3_last_error()
    neg = _lib.BeamParams(4, 1, -1.0)
    assert m0._lib.ymt3_decode_beam(m0._handle, ctypes.c_void_p(e.data_ptr()), 4, n, None, 0, ctypes.byref(neg), ctypes.c_void_p(tok.data_ptr()),
                                    None, None, None, None, None) == 1
    rows = _lib.BeamParams(8, 1, 1.0)
    assert m0._lib.ymt3_decode_beam(m0._handle, ctypes.c_void_p(e.data_ptr()), 4, n, None, 0, ctypes.byref(rows), ctypes.c_void_p(tok.data_ptr()),
                                    None, None, None, None, None) == 1
    assert b"max_batch" in m0._lib.ymt3_last_error()
    assert torch.equal(m0.decode(e, n, num_beams=W, num_return_sequences=W).cpu(), a[0])
    # a non-finite segment: its groups return ids in range and NaN scores, the other groups keep their bits
    e_bad = e.clone()
    e_bad[1] = float("nan")
    c = [x.cpu() for x in m0.decode(e_bad, n, return_scores=True, num_beams=W, num_return_sequences=W)]
    assert int(c[0].min()) >= 0 and int(c[0].max()) < cfg0.vocab and bool(torch.isnan(c[2][1]).all())
    for i in (0, 2, 3):
        assert all(torch.equal(x[i], y[i]) for x, y in zip(c, a)), i
    m0.close()


def test_early_stop_with_beams_stops_once_every_group_is_done(monkeypatch):
    """ymt3_set_early_stop with beams: the host stops launching at the first check after every group has filled its W slots, and the
    result is the full-length call's, bit for bit.  The inputs make every group finish at a known step whatever the numerics: a token
    automaton that allows every token for five steps and then only EOS, so at emitted step 5 each beam has one candidate, the EOS (the
    group runs out of candidates: W of the 2W places), both finish, the W = 2 slots are full.  Checked on the CPU oracle first."""
    from yourmt3_amd.constraint import TokenAutomaton
    _separate(monkeypatch, hooks=False)
    n, W, free, interval, eos = 48, 2, 5, 4, 7
    cfg = SMALL.with_(eos_id=eos)
    V = cfg.vocab
    allowed = np.ones((free + 1, V), bool)
    allowed[free] = False
    allowed[free, eos] = True
    allowed[:free, eos] = False                          # (nothing finishes earlier either)
    nxt = np.minimum(np.arange(free + 1)[:, None] + 1, free).repeat(V, 1).astype(np.int32)
    aut = TokenAutomaton(allowed, nxt)
    m = _model(cfg, max_batch=8)
    enc = _enc(m, cfg, 4)
    ref = beam_search(enc, m.weights, cfg, n, True, W, W, 1.0, automaton=aut)
    assert (ref.done_step == free).all() and ref.steps_run == free + 1, ref.done_step
    c = m.compile_constraint(aut)
    e = enc.bfloat16().cuda()
    full = [x.cpu() for x in m.decode(e, n, return_scores=True, num_beams=W, num_return_sequences=W, constraint=c)]
    assert m.last_decode_steps == n
    m.set_early_stop(interval)
    early = [x.cpu() for x in m.decode(e, n, return_scores=True, num_beams=W, num_return_sequences=W, constraint=c)]
    steps = m.last_decode_steps
    m.set_early_stop(0)
    expected = interval * -(-(free + 1) // interval)     # the first host check at or after the step that filled the last group
    _REPORT["early_stop_steps"] = {"launched": steps, "expected": expected, "of": n}
    assert steps == expected and steps < n, (steps, expected)
    assert all(torch.equal(x, y) for x, y in zip(early, full))
    # every hypothesis: five free tokens, then EOS, then PAD
    assert (full[0][..., free] == eos).all() and (full[0][..., free + 1:] == cfg.pad_id).all() and (full[0][..., :free] != eos).all()
    c.close()
    m.close()


class _Weights:
    def __init__(self, w):
        self.weights = w


# ----------------------------------------------------------------------------- 9. end to end
def test_transcribe_with_beams_writes_a_midi_file(tmp_path, monkeypatch):
    from yourmt3_amd.midi import read_midi_notes
    from yourmt3_amd.transcribe import transcribe
    from yourmt3_amd.task_manager import TaskManager

    class Spy(TaskManager):                             # records what transcribe hands to the detokeniser
        def tokens_to_notes(self, batches, start_secs, end_sec=None, score_batches=None):
            self.seen = ([np.array(b) for b in batches], None if score_batches is None else [np.array(b) for b in score_batches])
            return super().tokens_to_notes(batches, start_secs, end_sec=end_sec, score_batches=score_batches)

    m = _model(SMALL, max_batch=8)
    audio = O.synthetic_audio(1, YMT3Config(segment_samples=3 * 8191))[0].numpy()
    spy = Spy("mt3_full_plus")
    path, notes = transcribe(m, audio, task_manager=spy, bsz=2, output_dir=str(tmp_path), max_token_length=32, return_notes=True, num_beams=4,
                             confidence=True, constrained=True)
    data = open(path, "rb").read()
    assert data[:4] == b"MThd"
    back = read_midi_notes(data)
    assert len(back) <= len(notes) and (len(back) > 0) == (len(notes) > 0)
    assert all(nt.confidence is None or 0.0 <= nt.confidence <= 1.0 + 1e-6 for nt in notes)
    # the notes are hypothesis 0's: the same decode by hand, all segments, detokenised the way transcribe does
    tm = TaskManager("mt3_full_plus")
    aut, st = tm.event_automaton(None)
    c = m.compile_constraint(aut)
    segs = m.ingest(torch.from_numpy(audio), SMALL.sample_rate)
    n_samples = m.last_ingest_samples
    tok_b, sc_b = [], []
    for i in range(0, segs.shape[0], 2):
        toks, ts, ss = m.inference(segs[i:i + 2], max_token_length=32, constraint=c, start_states=st, num_beams=4, num_return_sequences=2,
                                   return_scores=True)
        assert toks.shape == (segs[i:i + 2].shape[0], 1, 2, 32) and bool((ss[..., 0] >= ss[..., 1]).all())
        tok_b.append(toks[:, :, 0].cpu().numpy())
        sc_b.append(ts[:, :, 0].cpu().numpy())
    c.close()
    start_secs = [i * SMALL.segment_samples / SMALL.sample_rate for i in range(segs.shape[0])]
    by_hand = tm.tokens_to_notes(tok_b, start_secs, end_sec=n_samples / SMALL.sample_rate, score_batches=sc_b)
    # (random weights may give no complete note in 32 tokens, so the ids and scores that reached the detokeniser are compared themselves)
    assert len(spy.seen[0]) == len(tok_b) and all(np.array_equal(x, y) for x, y in zip(spy.seen[0], tok_b))
    assert all(np.array_equal(x, y) for x, y in zip(spy.seen[1], sc_b))
    assert any((b != SMALL.pad_id).any() for b in tok_b)
    assert by_hand == notes
    assert [nt.confidence for nt in by_hand] == [nt.confidence for nt in notes]
    other = tm.tokens_to_notes([t for t in tok_b], start_secs, end_sec=n_samples / SMALL.sample_rate)
    assert other == notes                               # (ids alone give the same notes: confidences take no part in equality)
    with pytest.raises(ValueError, match="continuous"):
        transcribe(m, audio, bsz=2, output_dir=str(tmp_path), num_beams=4, continuous=True)
    with pytest.raises(ValueError, match="max_batch"):
        transcribe(m, audio, bsz=4, output_dir=str(tmp_path), num_beams=4)
    m.close()
