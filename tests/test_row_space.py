"""Decoder parity along the row axis: every row-count regime of the decode path against the CPU oracle, at a row count that selects it.

The decoder picks its kernels by the number of rows it decodes, R = segments x channels (runtime.hip: launch_step, decode_run).  For one
channel and 8 heads:
  R 1-64      attention pair + GEMM chain (merged), folded self-attention O-projection; MoE: the MoE chain
  R 65-96     separate launches, folded O-projection; the argmax kernel's two-level ticket (more than 64 workgroups, groups of 32)
  R 97-167    no fold: the self-attention O-projection is a launch of its own again
  R 168-256   two concurrent chains of ceil(R/2) and floor(R/2) rows: no fold, no ticket (early stop keeps one chain)
  R 257-511   one chain; the 2-waves-per-(row, head) self-attention (R x 8 > 2048 (row, head) pairs)
  R >= 512    mid-size tile decode GEMMs (64- or 32-row tiles, a ragged last tile); MoE: the combine launch, no fold
  MoE         at most 1536 rows (the pair list is held in LDS): ymt3_create refuses more
Each regime meets the oracle here at the bounds of test_gpu_parity.py (_check_ids: TAU 0.03, logits max 0.06 / mean 6e-3, MIN_SAFE; the
bf16 and fp8 bounds of _moe_case).  A regime is proved by the launch counts of profile_decode (which runs one chain) and by the chain
count of the real call.  The 2-wave attention and the mid tiles have no launch class of their own: they are proved by their bits, as
test_config_space.py proves "mid".  Every check records its errors, safe fraction, R and the regime it proved in the parity report.

The decoder is what is under test, so both sides decode the same bf16 encoder output: segments encoded on the GPU, the oracle fed
enc.float().  The oracle decodes rows independently: it runs once on the largest batch, and every smaller R takes its rows [0, R).

The row-independence contract of the dense decoder: rows [0, R') of a decode of R rows equal a decode of R' rows bit for bit whenever R
and R' fall in the same class -- 1-256, 257-511, >= 512 rows.  Within a class every form computes a row's sums in the same order: the
merged kernels equal the separate launches, the fold gives the same bits either way, two chains equal one chain.  Across a class
boundary the 2-wave self-attention (beyond 2048 (row, head) pairs) and the mid tiles (from 512 rows) sum in another order.
"""
import os
import time

import pytest
import torch

from oracle import ymt3_oracle as O
from test_gpu_parity import MIN_SAFE, TAU, _REPORT, _check_ids, _check_stream_prefix, _margin, _model, _moe_case
from yourmt3_amd.config import FFN_MOE, YMT3Config

pytestmark = pytest.mark.gpu

CFG = YMT3Config(segment_samples=8191, max_decode_len=32, eos_id=-1)           # 64 frames
N = CFG.max_decode_len
ROWS = [1, 15, 16, 17, 33, 63, 64, 65, 96, 97, 167, 168, 169, 255, 256, 257, 511, 512, 513]
MAXB = max(ROWS)
SEED = 19
PER = 2 * CFG.n_dec_layers          # launches of a per-layer class in profile_decode(e, 8, stride=4): two sampled steps


def _regime(R):
    """what the table above says a decode of R rows of one channel runs, with the default knobs"""
    chains = 2 if 168 <= R <= 256 else 1
    return {"merged": R <= 64, "fold": R <= 96 and chains == 1, "chains": chains, "ticket": R > 64 and chains == 1,
            "two_wave_self_attn": R > 256, "mid_tiles": R >= 512}


def _top(R):
    """the largest row count of R's class of equal bits: 1-256, 257-511, >= 512"""
    return 256 if R <= 256 else (511 if R < 512 else MAXB)


def _create(cfg, env, max_batch):
    """a handle created under `env` (the knobs are read at create); the environment is restored"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _model(cfg, max_batch=max_batch)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _launches(m, e):
    return {k: v["launches"] for k, v in m.profile_decode(e, 8, stride=4).items()}


class _Rows:
    """MAXB segments encoded on the GPU, the oracle's free-running stream and logits for all of them, and the handles the tests share"""

    def __init__(self):
        self.m = _model(CFG, max_batch=MAXB)
        self.handles = {}
        self.tops = {}
        self.streams = {}
        self._eos = None
        self.eos_order = {}
        self.audio = O.synthetic_audio(MAXB, CFG, seed=SEED)
        self.e = self.m.encode(self.m.logmel(self.audio.cuda()))
        enc = self.e.float().cpu()
        assert len({r.numpy().tobytes() for r in enc}) == MAXB                # every row decodes a segment of its own
        t0 = time.perf_counter()
        self.ref_t, self.ref_l = O.greedy_decode(enc, self.m.weights, CFG, N, True, return_logits=True)
        secs = time.perf_counter() - t0
        print(f"oracle: {MAXB} rows x {N} steps in {secs:.1f} s")
        self.margin = _margin(self.ref_l)
        streams = len({tuple(r.flatten().tolist()) for r in self.ref_t})
        _REPORT["row_space_oracle"] = {"rows": MAXB, "steps": N, "seconds": round(secs, 1), "distinct_streams": streams}
        assert streams > MAXB // 2                                              # (the rows are not copies of each other)

    def handle(self, key, env, max_batch, cfg=CFG):
        if key not in self.handles:
            self.handles[key] = _create(cfg, env, max_batch)
        return self.handles[key]

    def run(self, R, m=None):
        """rows [0, R) on `m` (default: the shared handle): teacher-forced ids and logits (fed the oracle's stream), free-running ids, and
        the chain count of the call"""
        m = m or self.m
        e = self.e[:R]
        t, lg = m.decode(e, N, forced=self.ref_t[:R].cuda(), return_logits=True)
        chains = m.last_decode_chains
        free = m.decode(e, N)
        assert m.last_decode_chains == chains
        return t.cpu(), lg.cpu(), free.cpu(), chains

    def top(self, R):
        """run() of the largest row count of R's class, computed once"""
        R = _top(R)
        if R not in self.tops:
            self.tops[R] = self.run(R)
        return self.tops[R]

    def class_streams(self, c):
        """free-running ids of all MAXB segments, each decoded in a batch of class c (0: 1-256 rows, 1: 257-511 rows).  Streams of two
        classes differ after a near-tie step (another summation order, other last bits), so a batch is built from streams of its own class."""
        if c not in self.streams:
            if c == 0:
                s = torch.cat([self.m.decode(self.e[i:i + 256], N).cpu() for i in range(0, MAXB, 256)])
            else:
                lo, hi = self.m.decode(self.e[:300], N).cpu(), self.m.decode(self.e[MAXB - 300:], N).cpu()
                s = torch.cat([lo, hi[300 - (MAXB - 300):]])
            self.streams[c] = s[:, 0]
        return self.streams[c]

    @staticmethod
    def _first(streams, cand, within=25):
        """(rows,) the first step < `within` at which each stream emits `cand` (1 << 30: none)"""
        early = streams[:, :within]
        return torch.where(early == cand, torch.arange(within).expand_as(early), 1 << 30).amin(1)

    def eos_pool(self, R):
        """(eos, order) for a batch of R rows.  eos: among the ids that at least 128 of the class-0 streams first emit at steps 1-24, the one
        whose first steps are the most varied (the random-weight model's streams share long prefixes: at step 0 nearly every row emits one
        of two ids).  order: the segments whose stream of R's class first emits it at steps 1-24, round-robin over those steps (so that
        every prefix of the order holds all of them), repeated up to MAXB."""
        if self._eos is None:
            s = self.class_streams(0)
            best = None
            for cand in torch.unique(s[:, :25]).tolist():
                first = self._first(s, cand)
                ok = first >= 1
                score = (len(set(first[ok & (first < 25)].tolist())), int((ok & (first < 25)).sum()))
                if cand != CFG.pad_id and score[1] >= 128 and (best is None or score > best[0]):
                    best = (score, cand)
            assert best is not None and best[0][0] >= 4, "no id that many streams emit early, at different steps"
            self._eos = best[1]
        c = 0 if R <= 256 else 1
        if c not in self.eos_order:
            first = self._first(self.class_streams(c), self._eos)
            steps = sorted(set(first[(first >= 1) & (first < 25)].tolist()))
            groups = [(first == p).nonzero().flatten().tolist() for p in steps]
            order = [g[i] for i in range(max(map(len, groups))) for g in groups if i < len(g)]
            self.eos_order[c] = torch.tensor(order).repeat(-(-MAXB // len(order)))[:MAXB]
        return self._eos, self.eos_order[c]

    def close(self):
        for h in self.handles.values():
            h.close()
        self.m.close()


@pytest.fixture(scope="module")
def rows():
    st = _Rows()
    yield st
    st.close()


# ----------------------------------------------------------------------------- A + B: the dense decoder at every row count
@pytest.mark.parametrize("R", ROWS)
def test_dense_decoder_matches_the_oracle_at_every_row_count(rows, R):
    """A: teacher-forced ids and logits, a free-running stream and the id range against the oracle, and the regime R takes.  B: the
    row-independence contract -- rows [0, R) of the class's largest decode, and a handle created for exactly R rows (the KV-cache pitch is
    maxR-based), give the shared handle's bits."""
    rg = _regime(R)
    t, lg, free, chains = rows.top(R) if R == _top(R) else rows.run(R)
    rec = _check_ids(f"row_space_{R}_rows_teacher_forced", t, rows.ref_t[:R], rows.ref_l[:R], lg)
    _check_stream_prefix(free, rows.ref_t[:R], rows.margin[:R])
    for ids in (t, free):
        assert int(ids.min()) >= 0 and int(ids.max()) < CFG.vocab
    p = _launches(rows.m, rows.e[:R])
    if rg["merged"]:
        assert p["attn_pair"] == PER and p["gemm_chain"] == PER and p["self_attn"] == 0 and p["self_o_gemm"] == 0, p
    else:
        assert p["attn_pair"] == 0 and p["gemm_chain"] == 0 and p["self_attn"] == PER, p
        assert p["self_o_gemm"] == (0 if R <= 96 else PER), p               # (profile_decode runs one chain: the fold up to 96 rows)
    assert p["step_layers"] == 0, p
    assert chains == rg["chains"], (R, chains)
    rec.update(rows=R, regime=rg, launches={k: v for k, v in p.items() if v}, chains=chains)
    top_t, top_l, top_free, _ = rows.top(R)
    assert torch.equal(t, top_t[:R]) and torch.equal(lg, top_l[:R]) and torch.equal(free, top_free[:R])
    x = _model(CFG, max_batch=R)
    x_t, x_l, x_free, x_chains = rows.run(R, x)
    x.close()
    assert x_chains == chains and torch.equal(x_t, t) and torch.equal(x_l, lg) and torch.equal(x_free, free)
    if R in (257, 512):
        # the first row count past a class boundary: its rows [0, R - 1) differ from the (R - 1)-row decode, and equal a handle that takes
        # the new form at R - 1 rows through its knob (at 511 rows the 2-wave attention is already the natural form)
        prev = R - 1
        knob = {"YMT3_SELF_ATTN_2WAVE": "1"} if R == 257 else {"YMT3_DEC_GEMM_MID_ROWS": "1"}
        assert not torch.equal(lg[:prev], rows.top(prev)[1])
        k = _create(CFG, knob, prev)
        k_t, k_l, k_free, _ = rows.run(prev, k)
        k.close()
        assert torch.equal(k_l, lg[:prev]) and torch.equal(k_t, t[:prev]) and torch.equal(k_free, free[:prev])
        rec["proved_by_bits"] = f"rows [0, {prev}) differ from the {prev}-row decode and equal a {prev}-row handle under {knob}"


# ----------------------------------------------------------------------------- C: the options along the row axis
@pytest.mark.parametrize("R", [65, 96, 97, 128, 167, 256])
def test_merged_kernels_up_to_256_rows_are_bit_identical(rows, R):
    """YMT3_MERGED_MAX_ROWS=256: the attention pair and the GEMM chain beyond 64 rows, up to 16 row tiles (at 256 rows with YMT3_CHAINS=1:
    one of two concurrent chains never takes them) -- the default handle's logits and ids, bit for bit"""
    if R == 256:
        m = rows.handle("merged256_one_chain", {"YMT3_MERGED_MAX_ROWS": "256", "YMT3_CHAINS": "1"}, 256)
    else:
        m = rows.handle("merged256", {"YMT3_MERGED_MAX_ROWS": "256"}, 167)
    p = _launches(m, rows.e[:R])
    assert p["attn_pair"] == PER and p["gemm_chain"] == PER and p["self_attn"] == 0 and p["self_o_gemm"] == 0, p
    t, lg, free, chains = rows.run(R, m)
    assert chains == 1 and m.merged_fallbacks == 0
    d_t, d_l, d_free, _ = rows.run(R)
    assert torch.equal(t, d_t) and torch.equal(lg, d_l) and torch.equal(free, d_free)


@pytest.mark.parametrize("R", [168, 169, 255, 256])
def test_one_chain_equals_two_chains_at_their_edges(rows, R):
    """YMT3_CHAINS=1 against the automatic two chains: halves of 84, 85/84, 128/127 and 128 rows"""
    one = rows.handle("one_chain", {"YMT3_CHAINS": "1"}, 256)
    t, lg, free, chains = rows.run(R, one)
    d_t, d_l, d_free, d_chains = rows.run(R)
    assert chains == 1 and d_chains == 2
    assert torch.equal(t, d_t) and torch.equal(lg, d_l) and torch.equal(free, d_free)


@pytest.mark.parametrize("R", [1, 17, 63, 64])
def test_step_kernel_along_the_rows(rows, R):
    """YMT3_STEP_KERNEL=1 (all layers of a step as one launch) against the default, bit for bit"""
    sk = rows.handle("step_kernel", {"YMT3_STEP_KERNEL": "1"}, 64)
    p = _launches(sk, rows.e[:R])
    assert p["step_layers"] == 2 and p["attn_pair"] == 0 and p["gemm_chain"] == 0, p
    t, lg, free, _ = rows.run(R, sk)
    d_t, d_l, d_free, _ = rows.run(R)
    assert torch.equal(t, d_t) and torch.equal(lg, d_l) and torch.equal(free, d_free)
    assert sk.merged_fallbacks == 0


# ----------------------------------------------------------------------------- D: MoE along the row axis
MOE_ROWS = [17, 64, 65, 200, 512, 1536]
MOE_MAXB = max(MOE_ROWS)
MOE_SEED = 23
MOE_BOUNDS = {0: dict(tol_max=0.06, tol_mean=6e-3, tau=TAU, max_deficit=0.01, min_safe=MIN_SAFE),     # test_moe_decoder_ffn_matches_oracle
              1: dict(tol_max=0.08, tol_mean=8e-3, tau=0.08, max_deficit=0.04, min_safe=0.7)}         # test_moe_fp8_expert_gemms_match_oracle


class _Moe:
    """one MoE handle of 1536 rows (router trace hook on), 1536 segments encoded on the GPU, and the ids both sides are fed: the handle's
    own free-running streams, 32 steps of rows [0, 512) and 8 steps of all 1536"""

    def __init__(self, fp8):
        self.cfg = YMT3Config(segment_samples=8191, max_decode_len=32, dec_ffn=FFN_MOE, moe_fp8=fp8, eos_id=-1)
        self.m = _create(self.cfg, {"YMT3_DEBUG_HOOKS": "1"}, MOE_MAXB)
        a = O.synthetic_audio(MOE_MAXB, self.cfg, seed=MOE_SEED)
        self.e = self.m.encode(self.m.logmel(a.cuda()))
        self.feed = {32: self.m.decode(self.e[:512], 32).cpu(), 8: self.m.decode(self.e, 8).cpu()}
        assert torch.equal(self.feed[8][:512], self.feed[32][..., :8])        # (both from 512 rows on: a row's bits do not depend on the batch)
        self.traces = {}


@pytest.fixture(scope="module")
def moe():
    made = {}

    def get(fp8):
        if fp8 not in made:
            made[fp8] = _Moe(fp8)
        return made[fp8]
    yield get
    for st in made.values():
        st.m.close()


@pytest.mark.parametrize("R", MOE_ROWS)
@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_moe_decoder_matches_the_oracle_at_every_row_count(moe, fp8, R, monkeypatch):
    """The router's recorded choices fed to the oracle (_moe_case), at the MoE chain's row counts, the five launches' and from 512 rows on
    the combine launch and mid tiles; the pair counts per expert show the grouped GEMM's edges were met, and the routing of a row does
    not depend on the rest of the batch."""
    st = moe(fp8)
    cfg, m = st.cfg, st.m
    n = 8 if R == MOE_MAXB else 32
    e = st.e[:R]
    p = _launches(m, e)
    if R <= 64:                          # the MoE chain: cross O-projection -> router -> experts -> next QKV / lm_head as one launch
        assert p["attn_pair"] == PER and p["gemm_chain"] == PER and p["cross_o_gemm"] == 0 and p["ffn_wi_gemm"] == 0, p
    else:                                # the five launches
        assert p["attn_pair"] == 0 and p["gemm_chain"] == 0 and p["self_attn"] == PER and p["cross_o_gemm"] == PER, p
        assert p["ffn_wi_gemm"] > 0 and p["ffn_wo_gemm"] > 0, p
    out = {}
    name = f"row_space_moe_{'fp8' if fp8 else 'bf16'}_{R}_rows_routing_teacher_forced"
    _moe_case(cfg, n, monkeypatch=monkeypatch, enc=e.float().cpu(), m=m, feed=st.feed[n][:R], name=name, out=out, **MOE_BOUNDS[fp8])
    assert out["chains"] == 1
    sel = out["trace"]                                                         # (steps, layers, R, 2)
    counts = torch.stack([(sel == x).sum((-2, -1)) for x in range(cfg.n_experts)], -1)          # (steps, layers, experts): (row, slot) pairs
    assert bool((counts.sum(-1) == 2 * R).all())
    ragged = (counts > 16) & (counts % 16 != 0)        # moe_gemm_kernel walks an expert's pairs in chunks of 16: a second chunk, ragged
    out["rec"].update(rows=R, steps=n, chains=out["chains"], launches={k: v for k, v in p.items() if v},
                      regime={"moe_chain": R <= 64, "combine_folded": R < 512, "two_wave_self_attn": R > 256, "mid_tiles": R >= 512},
                      pairs_per_expert={"min": int(counts.min()), "max": int(counts.max()),
                                        "step_layers_with_an_idle_expert": int((counts == 0).any(-1).sum()),
                                        "experts_with_a_ragged_second_chunk": int(ragged.sum())})
    if R == 17:
        assert bool((counts == 0).any())                                       # an expert without a pair
    if R >= 64:
        assert bool(ragged.any())
    # a row's routing does not depend on the rest of the batch: where two row counts of the same class of bits (below 512 rows, from 512
    # on) share rows and steps, their recorded choices agree
    for R2, (n2, s2) in st.traces.items():
        if (R2 >= 512) == (R >= 512):
            k, r = min(n, n2), min(R, R2)
            assert torch.equal(sel[:k, :, :r], s2[:k, :, :r]), (R, R2)
    st.traces[R] = (n, sel)
    if R == 512:
        # the combine launch and the mid tiles, by their bits: rows [0, 200) differ from the 200-row decode and equal a 200-row handle
        # that takes both through YMT3_DEC_GEMM_MID_ROWS=1 (and the 2-wave self-attention of 512 rows through YMT3_SELF_ATTN_2WAVE=1)
        f = st.feed[n][:200].cuda()
        _, d_l = m.decode(st.e[:200], n, forced=f, return_logits=True)
        assert not torch.equal(out["got_l"][:200], d_l.cpu())
        k = _create(cfg, {"YMT3_DEC_GEMM_MID_ROWS": "1", "YMT3_SELF_ATTN_2WAVE": "1"}, 200)
        k_t, k_l = k.decode(st.e[:200], n, forced=f, return_logits=True)
        k.close()
        assert torch.equal(k_l.cpu(), out["got_l"][:200]) and torch.equal(k_t.cpu(), out["got_t"][:200])


@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_moe_handle_beyond_1536_rows_is_refused(fp8):
    from yourmt3_amd._lib import YMT3Error
    cfg = YMT3Config(segment_samples=8191, max_decode_len=32, dec_ffn=FFN_MOE, moe_fp8=fp8, eos_id=-1)
    with pytest.raises(YMT3Error, match=r"ymt3 error 4: .*at most 1536 decoder rows \(got 1537\)"):
        _model(cfg, max_batch=MOE_MAXB + 1)


# ----------------------------------------------------------------------------- E: EOS and early stop through the ticket path
@pytest.mark.parametrize("R", [65, 100, 200, 257])
def test_early_stop_through_the_ticket_path(rows, R):
    """Rows emit the EOS id at different steps.  set_early_stop(4) gives the ids of the call without it and launches up to the first
    multiple of 4 at which every row has finished (n_unfinished, counted by the argmax kernel's last workgroup: beyond 64 rows through the
    two-level ticket); every row is PAD after its EOS.  At 200 rows early stop runs one chain where the plain call runs two."""
    eos, idx = rows.eos_pool(R)
    m = rows.handle("eos", {}, 320, cfg=CFG.with_(eos_id=eos))
    e = rows.e[idx[:R].cuda()]
    free = rows.m.decode(e, N).cpu()                                           # eos_id = -1
    full = m.decode(e, N).cpu()
    full_chains = m.last_decode_chains
    assert m.last_decode_steps == N
    m.set_early_stop(4)
    try:
        early = m.decode(e, N).cpu()
        steps, early_chains = m.last_decode_steps, m.last_decode_chains
    finally:
        m.set_early_stop(0)
    assert torch.equal(early, full)
    assert full_chains == (2 if R == 200 else 1) and early_chains == 1, (full_chains, early_chains)
    first = [int((r == eos).nonzero()[0]) if bool((r == eos).any()) else N for r in full[:, 0]]
    expect = min(N, -(-(max(first) + 1) // 4) * 4)
    _REPORT[f"row_space_early_stop_{R}_rows"] = {"rows": R, "eos": eos, "steps_launched": steps, "expected": expect,
                                                 "distinct_eos_steps": len(set(first)), "chains": [full_chains, early_chains]}
    assert steps == expect < N, (steps, expect, max(first))
    assert len(set(first)) >= 4
    for b in range(R):
        row, ref, f = full[b, 0], free[b, 0], first[b]
        assert torch.equal(row[:f + 1], ref[:f + 1]) and bool((row[f + 1:] == CFG.pad_id).all()), b


# ----------------------------------------------------------------------------- F: continuous batching through many slots
@pytest.mark.parametrize("slots", [65, 100, 257])
def test_continuous_batching_through_many_slots(rows, slots):
    """Slot mode decodes `slots` rows a step: the ticket path at 65 and 100 slots, the 2-wave self-attention at 257.  The lock-step call
    of the same segments (160 or 320: the same class of bits) gives the same ids, bit for bit."""
    n_seg = 160 if slots <= 256 else 320
    eos, idx = rows.eos_pool(n_seg)
    m = rows.handle("eos", {}, 320, cfg=CFG.with_(eos_id=eos))
    a = rows.audio[idx[:n_seg]].cuda()
    lock = m.inference(a)
    got = m.inference_stream(a, slots=slots, interval=4)
    assert torch.equal(got, lock), slots
    stops = {int((r == eos).nonzero()[0]) if bool((r == eos).any()) else N for r in lock.cpu()[:, 0]}
    assert len(stops) >= 4                                                     # rows retire at different steps: slots are refilled
