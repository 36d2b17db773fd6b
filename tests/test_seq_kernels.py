"""The full-sequence scoring pass's kernels one by one (csrc/dec_seq.hip: seq_embed_kernel, dec_seq_attn_kernel<CAUSAL>, seq_lm_head_score_kernel),
through the test doors ymt3_test_seq_embed / _dec_seq_attention / _seq_lm_head of include/ymt3.h, against float64 references of their contracts
(tests/seq_kernel_model.py; tests/test_seq_kernels_cpu.py shows that model right and sharp, and that every random case here keeps its cap under
the reference alone):

  exact probes   a bias table with one peak returns V[t - distance] bit for bit, every distance 0 .. 1023 once; one-hot queries against keys with
                 two hot coordinates return V[target] bit for bit over every tile count, both layouts, rows_per_kv and row0; one-hot lm-head rows
                 give code[target] - 512 exactly with the target in every (tile parity, lane quarter, element), both halves of every wave
  criterion      tests/enc_kernel_model.py's, against the TILE-SCHEDULE reference: a stable element equals the reference bit for bit, the others
                 lie within beta + 1 bf16 ulp; fp32 outputs (logits, scores) within their derived bounds
  guards         every output lies inside sentinels (Guarded); pad columns, unused slabs and rows below row0 of the inputs hold NaN
  state          decode and decode_score after all the door calls give the bits they gave before them (the last test of the module)
Every test records its figures under seq_kernel_* in the parity report.
"""
import ctypes

import pytest
import torch

import seq_kernel_model as S
from test_encoder_kernels import SENT, Guarded, m  # noqa: F401 (m: the encoder module's small handle, one per module)
from test_gpu_parity import _REPORT
from yourmt3_amd import _lib

pytestmark = pytest.mark.gpu
assert SENT == S.SENT
_BEFORE = {}


@pytest.fixture(scope="module", autouse=True)
def _calls_before_the_doors(m):
    """the handle's own decode and decode_score before any door call; the module's last test compares"""
    g = torch.Generator().manual_seed(13)
    enc = torch.randn(2, m.cfg.n_frames, m.cfg.d_model, generator=g).bfloat16()
    ids = torch.randint(0, m.cfg.vocab, (2, m.cfg.n_channels, 40), generator=g, dtype=torch.int32)
    _BEFORE.update(enc=enc, ids=ids, decode=[t.cpu() for t in m.decode(enc, 24, return_logits=True)],
                   score=[t.cpu() for t in m.decode_score(enc, ids, return_logits=True)])
    yield
    _BEFORE.clear()


def _record(name, rec):
    rec = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}
    _REPORT["seq_kernel_" + name] = rec
    print(name, rec)
    return rec


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ----------------------------------------------------------------------------- embed
def _run_embed(m, c):
    dev = m.device
    h = Guarded(m, c["n_rows"] * c["L"] * 512, torch.float32)
    m.test_seq_embed(h=h.view, embed=c["embed"].to(dev), tokens=c["tokens"].to(dev), n_rows=c["n_rows"], n_prompt=c["P"], n_steps=c["n_steps"], V=c["V"],
                     pad_id=c["pad_id"], row0=c["row0"], prompt=c["prompt"].to(dev) if c["P"] else None,
                     chan_embed=c["chan_embed"].to(dev) if c["chan_embed"] is not None else None, n_channels=c["n_channels"])
    return h.read(torch.ones(c["n_rows"] * c["L"] * 512, dtype=torch.bool))


def test_embed_is_exact(m):
    """pad at position 0, the prompt, the shifted tokens, ids clamped at both ends, the channel row of the ABSOLUTE row; n_rows L in {1, 3, 4, 5}
    around the four-waves-per-block edge and one larger; with and without channel embeddings"""
    recs = []
    for n_rows, n, P, row0, Kc in S.EMBED_CASES:
        for chan in (True, False):
            c = S.embed_case(n_rows, n, P, row0, Kc, chan=chan)
            recs.append(S.check_embed(c, _run_embed(m, c)))
    rec = _record("embed", S.join(recs))
    assert rec["ok"], rec


# ----------------------------------------------------------------------------- attention
def _run_attention(m, c, keep=None):
    """one launch -> out (n_rows, L, H, 64) bf16 on the host; `keep`: a dict that holds the layout and its device buffers between launches"""
    keep = {} if keep is None else keep
    if "lay" not in keep:
        keep["lay"] = S.attention_layout(c)
        keep["dev"] = {}
    lay, dev = keep["lay"], keep["dev"]

    def on(name):
        buf, off = lay[name]
        if id(buf) not in dev:
            dev[id(buf)] = buf.flatten().to(m.device)
        return dev[id(buf)][off:]

    n_rows, L, H, _ = c["q"].shape
    out = Guarded(m, lay["out_size"], torch.bfloat16)
    bias = c["bias"].to(m.device).contiguous() if c["causal"] else None
    m.test_dec_seq_attention(causal=c["causal"], q=on("q"), k=on("k"), v=on("v"), out=out.view, n_rows=n_rows, L=L, n_keys=c["k"].shape[1], H=H,
                             row0=c["row0"], rows_per_kv=c["rows_per_kv"], bias=bias, bias_stride=c["bias"].shape[1] if c["causal"] else 0,
                             **lay["strides"])
    return out.read(lay["out_index"].flatten())[lay["out_index"]]


def test_attention_bias_probe_is_exact(m):
    """every distance 0 .. 1023 is the lone peak of some head once (L = 1024, 64 heads per launch, 16 launches): the bias window of every (query
    block, key tile) pair, the diagonal mask, the tile skip and the V address map, exactly; rows before the peak's distance are uniform"""
    recs, keep = [], {}
    uniform = S.uniform_prefix_rows(S.bias_probe_qkv()[2])
    for launch in range(S.BIAS_PROBE_L // S.BIAS_PROBE_H):
        c, key = S.bias_probe_case(launch)
        recs.append(S.check_bias_probe(c, key, _run_attention(m, c, keep), uniform))
    # (the mean of a few integer codes often lies ON a bf16 rounding boundary: the launches whose only uniform rows are the first few
    # positions have a low share of their own, so the share is taken over all the uniform rows of the sweep)
    share = sum(r["stable_share"] * r["elements"] for r in recs) / max(1, sum(r["elements"] for r in recs))
    rec = _record("attn_bias_probe", dict(S.join(recs), stable_share=share, launches=len(recs), exact=all(r["exact"] for r in recs)))
    assert rec["ok"] and rec["exact"] and rec["exact_rows"] == 1024 * 1025 // 2 and rec["stable_share"] >= S.MIN_STABLE, rec


@pytest.mark.parametrize("case", S.score_probe_cases(), ids=lambda c: c[0])
def test_attention_score_probe_is_exact(m, case):
    """the target key -- the newest, key 0, or one spread over every tile -- wins by 256: V[slab, target] bit for bit"""
    name, causal, L, nk, n_rows, H, row0, rpk, layout = case
    c, key = S.score_probe_case(causal, L, nk, n_rows, H, row0, rpk, layout)
    rec = _record("attn_score_probe_" + name, S.check_score_probe(c, key, _run_attention(m, c)))
    assert rec["ok"], rec


@pytest.mark.parametrize("name", [c[0] for c in S.attn_random_cases()])
def test_attention_random_cases_meet_the_criterion(m, name):
    c = S.attn_random_case(name)
    got = _run_attention(m, c)
    rec = _record("attn_" + name, S.check_attention(c, got, S.attn_random_reference(name)))
    assert rec["ok"] and rec["stable_share"] >= S.MIN_STABLE, rec
    assert torch.equal(_bits(got), _bits(_run_attention(m, c))), "the same launch twice gave other bits"


def test_attention_values(m):
    """scores of +-3e4 stay finite and meet the criterion; a NaN query stays in its own (row, position, head); a NaN in V stays in its slab and head"""
    t = torch.arange(130)
    q = (22.0 * torch.where(t % 2 == 0, 1.0, -1.0))[None, :, None, None].expand(2, 130, 1, 64).contiguous().bfloat16()
    k = (22.0 * torch.where(t % 3 == 0, -1.0, 1.0))[None, :, None, None].expand(2, 130, 1, 64).contiguous().bfloat16()
    g = torch.Generator().manual_seed(2)
    c = dict(causal=True, q=q, k=k, v=torch.randn(2, 130, 1, 64, generator=g).bfloat16(), bias=torch.zeros(1, 130), row0=0, rows_per_kv=1, layout="fused")
    got = _run_attention(m, c)
    huge = S.check_attention(c, got)
    assert bool(torch.isfinite(got.float()).all()) and huge["ok"], huge

    c = S.attn_random_case(S.find_random_case(causal=True, L=129, n_rows=2))
    clean = _run_attention(m, c)
    q = c["q"].clone()
    q[1, 77, 0, 5] = float("nan")
    got = _run_attention(m, dict(c, q=q))
    same = torch.ones(clean.shape[:3], dtype=torch.bool)
    same[1, 77, 0] = False
    assert torch.equal(_bits(got)[same], _bits(clean)[same]) and bool(torch.isnan(got[1, 77, 0].float()).all())

    c = S.attn_random_case(S.find_random_case(causal=False, n_keys=64, n_rows=3, row0=2, rpk=3))       # rows 2, 3, 4: slabs 0, 1, 1
    clean = _run_attention(m, c)
    v = c["v"].clone()
    v[0, 5, 0, 9] = float("nan")
    got = _run_attention(m, dict(c, v=v))
    assert torch.equal(_bits(got)[1:], _bits(clean)[1:]) and bool(torch.isnan(got[0, :, 0, 9].float()).all())
    keep = torch.ones(64, dtype=torch.bool)
    keep[9] = False
    assert torch.equal(_bits(got)[0][..., keep], _bits(clean)[0][..., keep])
    _record("attn_values", dict(huge, nan_rows_contained=True))


# ----------------------------------------------------------------------------- lm head
def _run_lm(m, c, with_logits=True):
    """one launch -> (scores (rows, n_steps), logits (rows, n_steps, V) or None), whole regions: SENT where nothing may be written"""
    dev = m.device
    rows, n, V = c["row0"] + c["M"] // c["L"], c["n_steps"], c["V"]
    sc = Guarded(m, rows * n, torch.float32)
    lg = Guarded(m, rows * n * V, torch.float32) if with_logits else None
    m.test_seq_lm_head(xn=c["xn"].to(dev), W=c["W"].to(dev), tokens=c["tokens"].to(dev), scores=sc.view, M=c["M"], L=c["L"], n_prompt=c["P"], n_steps=n,
                       V=V, row0=c["row0"], lengths=c["lengths"].to(dev) if c["lengths"] is not None else None, logits=lg.view if with_logits else None)
    w = torch.zeros(rows, n, dtype=torch.bool)
    w[c["row0"]:] = True
    return sc.read(w).reshape(rows, n), (lg.read(w[..., None].expand(rows, n, V)).reshape(rows, n, V) if with_logits else None)


def test_lm_head_winner_and_target_placement_are_exact(m):
    """one-hot rows against integer codes with one winner of 512 per column: code[target] - 512 exactly, 0 at the winner, the logits W's column;
    the target in every (tile parity, lane quarter, element) position in both 16-row halves of every wave, row0 = 1"""
    c, want, _ = S.lm_winner_case()
    sc, lg = _run_lm(m, c)
    rec = S.check_lm_winner(c, want, sc)
    ref = S.lm_reference(c)
    rec["logits_exact"] = bool(torch.equal(lg.double(), ref["logits"]))
    sc2, _ = _run_lm(m, c, with_logits=False)
    rec["same_bits_without_logits"] = bool(torch.equal(_bits(sc), _bits(sc2)))
    rec = _record("lm_winner", rec)
    assert rec["ok"] and rec["logits_exact"] and rec["same_bits_without_logits"] and rec["zeros"] >= 32, rec


@pytest.mark.parametrize("case", S.lm_edge_cases(), ids=lambda c: c[0])
def test_lm_head_edges_meet_their_bounds(m, case):
    """logits and scores against float64 of the same inputs as error over bound; M around the 16-row halves and the 128-row block, V from one
    tile, with a prompt (nothing written for its positions), lengths below 0 and beyond n_steps (exactly 0.0 past them), row0 != 0, targets out
    of range; without `logits` the scores have the same bits, and a repeat too"""
    name, M, L, P, V, row0, wl = case
    c = S.lm_case(M, L, P, V, row0, wl)
    sc, lg = _run_lm(m, c)
    rec = _record("lm_" + name, S.check_lm(c, sc, lg))
    assert rec["ok"] and rec["past_length_exact"], rec
    sc2, _ = _run_lm(m, c, with_logits=False)
    assert torch.equal(_bits(sc), _bits(sc2)) and torch.equal(_bits(sc), _bits(_run_lm(m, c)[0]))


def test_lm_head_uniform_and_all_minus_inf(m):
    """xn = 0: every logit is 0 and the score -log V within the derived bound; all logits -inf: NaN, as the kernel's comment promises"""
    c = S.lm_uniform_case()
    sc, lg = _run_lm(m, c)
    rec = S.check_lm(c, sc, lg)
    d = dict(c, xn=torch.ones_like(c["xn"]), W=torch.full_like(c["W"], float("-inf")))
    sn, ln = _run_lm(m, d)
    rec["minus_inf_gives_nan"] = bool(torch.isnan(sn[c["row0"]:]).all()) and bool((ln[c["row0"]:] == float("-inf")).all())
    rec = _record("lm_uniform", rec)
    assert rec["ok"] and rec["minus_inf_gives_nan"], rec


# ----------------------------------------------------------------------------- refusals
def _zeros(m, *s, dt=torch.float32):
    return torch.zeros(*s, dtype=dt, device=m.device)


def test_the_doors_refuse(m):
    """the C side's own refusals (YMT3_ERR_ARG), past the wrappers: a raw argument struct per case; every door stays usable"""
    bf, i32 = torch.bfloat16, torch.int32
    R, L, P, V, H = 2, 4, 1, 32, 2
    n = L - P
    e = dict(h=_zeros(m, R * L, 512), embed=_zeros(m, V, 512, dt=bf), chan_embed=_zeros(m, 2, 512, dt=bf), prompt=_zeros(m, R, P, dt=i32),
             tokens=_zeros(m, R, n, dt=i32))
    long_tokens = _zeros(m, R, L, dt=i32)
    ep = {k: v.data_ptr() for k, v in e.items()}

    def emb(**f):
        a = _lib.SeqEmbedArgs(**dict(dict(ep, row0=0, n_rows=R, L=L, n_prompt=P, n_steps=n, V=V, d=512, n_channels=2, pad_id=0), **f))
        return m._lib.ymt3_test_seq_embed(m._handle, ctypes.byref(a), m._stream())

    assert emb() == 0 and emb(chan_embed=None, n_channels=0) == 0 and emb(n_prompt=0, n_steps=L, prompt=None, tokens=long_tokens.data_ptr()) == 0
    bad = [emb(h=None), emb(embed=None), emb(tokens=None), emb(prompt=None), emb(h=ep["h"] + 4), emb(embed=ep["embed"] + 2), emb(tokens=ep["tokens"] + 4),
           emb(prompt=ep["prompt"] + 4), emb(chan_embed=ep["chan_embed"] + 2), emb(row0=-1), emb(n_rows=0), emb(L=L + 1), emb(n_steps=n + 1),
           emb(n_channels=0), emb(n_channels=-1), emb(d=256), emb(V=0), emb(n_steps=0, L=P), m._lib.ymt3_test_seq_embed(m._handle, None, m._stream())]
    assert all(rc != 0 for rc in bad), bad

    inner = H * 64
    a = dict(q=_zeros(m, R * L * inner, dt=bf), k=_zeros(m, R * L * inner, dt=bf), v=_zeros(m, R * L * inner, dt=bf), out=_zeros(m, R * L * inner, dt=bf),
             bias=_zeros(m, H, L))
    ap = {k: v.data_ptr() for k, v in a.items()}

    def att(**f):
        s = _lib.DecSeqAttnArgs(**dict(dict(ap, q_seq=L * inner, kv_seq=L * inner, o_seq=L * inner, ldq=inner, ldkv=inner, ldo=inner, kv_head=64, row0=0,
                                            n_rows=R, L=L, n_keys=L, rows_per_kv=1, H=H, bias_stride=L, causal=1), **f))
        return m._lib.ymt3_test_dec_seq_attention(m._handle, ctypes.byref(s), m._stream())

    cross = dict(causal=0, bias=None, bias_stride=0)
    assert att() == 0 and att(**cross) == 0 and att(ldkv=64, kv_head=L * 64, kv_seq=H * L * 64, **cross) == 0
    bad = [att(q=None), att(k=None), att(v=None), att(out=None), att(bias=None), att(q=ap["q"] + 2), att(k=ap["k"] + 8), att(v=ap["v"] + 4),
           att(out=ap["out"] + 2), att(bias=ap["bias"] + 4), att(row0=-1), att(n_rows=0), att(n_rows=65536), att(H=0), att(H=65536, ldq=65536 * 64),
           att(L=0), att(n_keys=0, **cross), att(rows_per_kv=0), att(bias_stride=L - 1), att(n_keys=L - 1), att(ldq=inner - 8), att(ldo=inner - 8),
           att(ldkv=inner - 8), att(ldkv=56, kv_head=L * 64), att(ldq=inner + 4), att(ldkv=inner + 4), att(ldo=inner + 4), att(kv_head=68),
           att(q_seq=L * inner + 4), att(kv_seq=L * inner + 4), att(o_seq=L * inner + 4), att(q_seq=-8), att(causal=0, bias_stride=0),
           m._lib.ymt3_test_dec_seq_attention(m._handle, None, m._stream())]
    assert all(rc != 0 for rc in bad), bad

    M = R * L
    t = dict(xn=_zeros(m, M, 512, dt=bf), W=_zeros(m, V, 512, dt=bf), tokens=_zeros(m, R, n, dt=i32), lengths=_zeros(m, 4, dt=i32), scores=_zeros(m, R, n),
             logits=_zeros(m, R, n, V))
    tp = {k: v.data_ptr() for k, v in t.items()}

    def lm(**f):
        s = _lib.SeqLmHeadArgs(**dict(dict(tp, M=M, L=L, n_prompt=P, n_steps=n, V=V, d=512, row0=0), **f))
        return m._lib.ymt3_test_seq_lm_head(m._handle, ctypes.byref(s), m._stream())

    assert lm() == 0 and lm(lengths=None, logits=None) == 0
    bad = [lm(xn=None), lm(W=None), lm(tokens=None), lm(scores=None), lm(xn=tp["xn"] + 2), lm(W=tp["W"] + 2), lm(tokens=tp["tokens"] + 4),
           lm(scores=tp["scores"] + 4), lm(lengths=tp["lengths"] + 4), lm(logits=tp["logits"] + 4), lm(row0=-1), lm(M=0), lm(M=M - 1), lm(L=L + 1),
           lm(n_steps=n + 1), lm(n_steps=0, n_prompt=L), lm(n_prompt=-1, n_steps=L + 1), lm(V=0), lm(V=24), lm(d=256),
           m._lib.ymt3_test_seq_lm_head(m._handle, None, m._stream())]
    assert all(rc != 0 for rc in bad), bad
    assert emb() == 0 and att() == 0 and lm() == 0
    torch.cuda.synchronize()


def test_the_wrappers_refuse_geometry_and_extents(m):
    """ValueError before the library is touched: the doors' refusals, and every extent computed from the shape and the strides"""
    bf, i32 = torch.bfloat16, torch.int32
    R, L, P, V, H = 2, 4, 1, 32, 2
    n, inner = L - P, 2 * 64
    e = dict(h=_zeros(m, R * L * 512), embed=_zeros(m, V * 512, dt=bf), tokens=_zeros(m, R * n, dt=i32), prompt=_zeros(m, R * P, dt=i32),
             chan_embed=_zeros(m, 2 * 512, dt=bf), n_rows=R, n_prompt=P, n_steps=n, V=V, pad_id=0, n_channels=2)
    m.test_seq_embed(**e)
    for f in (dict(h=e["h"][1:]), dict(h=e["h"][:-1]), dict(embed=e["embed"][:-1]), dict(tokens=e["tokens"][:-1]), dict(prompt=e["prompt"][:-1]), dict(row0=1),
              dict(chan_embed=e["chan_embed"][:-1]), dict(n_channels=0), dict(L=L + 1), dict(n_rows=0), dict(row0=-1), dict(prompt=None), dict(d=256),
              dict(h=e["h"].double()), dict(tokens=e["tokens"].long()), dict(embed=e["embed"].cpu())):
        with pytest.raises(ValueError):
            m.test_seq_embed(**dict(e, **f))
    z = lambda k: _zeros(m, k, dt=bf)
    a = dict(causal=True, q=z(R * L * inner), k=z(R * L * inner), v=z(R * L * inner), out=z(R * L * inner), bias=_zeros(m, H * L), bias_stride=L, n_rows=R, L=L,
             n_keys=L, H=H, ldq=inner, ldkv=inner, ldo=inner, kv_head=64, q_seq=L * inner, kv_seq=L * inner, o_seq=L * inner)
    m.test_dec_seq_attention(**a)
    for f in (dict(q=a["q"][:-8]), dict(k=a["k"][:-8]), dict(v=a["v"][:-8]), dict(out=a["out"][:-8]), dict(bias=a["bias"][:-1]), dict(row0=1), dict(bias_stride=L - 1),
              dict(bias=None), dict(n_keys=L + 1), dict(ldq=inner - 8), dict(ldo=inner - 8), dict(ldkv=inner - 8), dict(ldkv=inner + 4), dict(kv_head=32),
              dict(q_seq=-8), dict(n_rows=0), dict(n_rows=65536), dict(H=0), dict(rows_per_kv=0), dict(causal=False), dict(row0=-1), dict(q=a["q"].float()),
              dict(o_seq=L * inner + 8), dict(q_seq=L * inner + 8), dict(kv_seq=L * inner + 8)):
        with pytest.raises(ValueError):
            m.test_dec_seq_attention(**dict(a, **f))
    M = R * L
    t = dict(xn=z(M * 512), W=z(V * 512), tokens=_zeros(m, R * n, dt=i32), scores=_zeros(m, R * n), lengths=_zeros(m, R, dt=i32), logits=_zeros(m, R * n * V),
             M=M, L=L, n_prompt=P, n_steps=n, V=V)
    m.test_seq_lm_head(**t)
    for f in (dict(xn=t["xn"][:-8]), dict(W=t["W"][:-8]), dict(tokens=t["tokens"][:-1]), dict(scores=t["scores"][:-1]), dict(lengths=t["lengths"][:-1]),
              dict(logits=t["logits"][:-1]), dict(row0=1), dict(row0=-1), dict(M=M - 1), dict(L=L + 1), dict(n_steps=n + 1), dict(V=24), dict(V=0), dict(d=256),
              dict(scores=t["scores"].double())):
        with pytest.raises(ValueError):
            m.test_seq_lm_head(**dict(t, **f))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the handle's own state (LAST test of the module)
def test_decode_and_decode_score_after_the_doors_give_the_same_bits(m):
    after = [t.cpu() for t in m.decode(_BEFORE["enc"], 24, return_logits=True)]
    score = [t.cpu() for t in m.decode_score(_BEFORE["enc"], _BEFORE["ids"], return_logits=True)]
    for got, want in ((after, _BEFORE["decode"]), (score, _BEFORE["score"])):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
