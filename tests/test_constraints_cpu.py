"""Constrained decoding on the host (include/ymt3.h, constraints): token automata and their builders, the TaskManager's segment
grammar (sound: nothing it allows decodes to an invalid token or a foreign program; complete: it never forbids a well-formed
encoding), the constrained oracle pinned to HF T5 `generate(prefix_allowed_tokens_fn=...)`, and the C header / bindings."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

from oracle import ymt3_oracle as O
from constraint_oracle import constrained_greedy_decode
from test_importer import CFG, _hf, _imported
from yourmt3_amd.constraint import MAX_STATES, TokenAutomaton, allow_only, stack, suppress
from yourmt3_amd.task_manager import DRUM_PROGRAM, MC13_GROUPS, NoteEvent, TaskManager
from yourmt3_amd.vocab import EOS, PAD, UNK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 1536


# ---------------------------------------------------------------- automata
def test_automaton_validation():
    ok = np.ones((2, 8), bool)
    nx = np.zeros((2, 8), np.int32)
    a = TokenAutomaton(ok, nx)
    assert a.n_states == 2 and a.vocab == 8
    empty = ok.copy()
    empty[1] = False
    with pytest.raises(ValueError, match="allows no token"):
        TokenAutomaton(empty, nx)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="next states"):
            TokenAutomaton(ok, np.full((2, 8), bad, np.int32))
    with pytest.raises(ValueError, match="states outside"):
        TokenAutomaton(np.ones((MAX_STATES + 1, 4), bool), np.zeros((MAX_STATES + 1, 4), np.int32))
    with pytest.raises(ValueError):
        TokenAutomaton(ok, np.zeros((2, 9), np.int32))                # shape mismatch
    with pytest.raises(ValueError):
        TokenAutomaton(ok.astype(np.int32), nx)                        # allowed must be bool
    # a wrong vocabulary is refused by stack (and by the model, test_constraints.py)
    with pytest.raises(ValueError, match="vocabulary"):
        stack([a, TokenAutomaton(np.ones((1, 9), bool), np.zeros((1, 9), np.int32))])


def test_bits_walk_and_builders():
    g = np.random.default_rng(0)
    a = TokenAutomaton(g.random((3, 70)) < 0.5, g.integers(0, 3, (3, 70)).astype(np.int32))
    bits = a.bits()
    assert bits.shape == (3, 3) and bits.dtype == np.uint32
    for s in range(3):
        for i in range(70):
            assert bool((bits[s, i // 32] >> (i % 32)) & 1) == a.allowed[s, i]
    assert not (bits[:, 2] >> 6).any()                                # no bits at or beyond the vocabulary
    w = a.walk([5, 69, 200, -3], state=1)
    st = [1]
    for t in (5, 69, 69, 0):                                           # clamped like the device's fed ids
        st.append(int(a.next[st[-1], t]))
    assert w.tolist() == st
    with pytest.raises(ValueError):
        a.walk([1], state=3)
    s = suppress(V, [0, 2, 1000])
    assert s.n_states == 1 and s.allowed.sum() == V - 3 and not s.allowed[0, 1000]
    o = allow_only(V, [7, 9])
    assert o.allowed.sum() == 2 and o.allows(0, 9) and not o.allows(0, 8)
    with pytest.raises(ValueError):
        allow_only(V, [V])
    three = TokenAutomaton(np.ones((3, V), bool), np.tile(np.array([[1], [2], [0]], np.int32), (1, V)))
    big, offs = stack([three, o, three])
    assert offs == [0, 3, 4] and big.n_states == 7
    assert (big.next[3] == 3).all() and big.next[4:7, 0].tolist() == [5, 6, 4]
    assert big.walk([9, 9, 9, 9], offs[2]).tolist() == [4, 5, 6, 4, 5]


# ---------------------------------------------------------------- the segment grammar
GM_NO_ZERO = [1, 24, 33, 40, 73]
PROGRAM_SETS = [("all", None), ("empty", []), ("piano0", [0]), ("drums", [128]), ("singing", [129]), ("gm_subset", GM_NO_ZERO),
                ("mixed", [0, 5, 128, 129])]


def _programs(tm, programs, ch):
    P = set(range(130)) if programs is None else set(programs)
    if tm.num_decoding_channels > 1:
        P &= set(MC13_GROUPS[ch][1])
    return P


def _random_walk(aut, state, rng, n, eos_bias=0.02):
    toks = []
    for _ in range(n):
        ids = np.flatnonzero(aut.allowed[state])
        t = EOS if EOS in ids and rng.random() < eos_bias else int(rng.choice(ids))
        toks.append(t)
        if t == EOS:
            break
        state = int(aut.next[state, t])
    return toks


@pytest.mark.parametrize("task", ["mt3_full_plus", "mc13_full_plus_256", "singing_drum_v1"])
@pytest.mark.parametrize("name,programs", PROGRAM_SETS, ids=[p[0] for p in PROGRAM_SETS])
def test_grammar_soundness(task, name, programs):
    tm = TaskManager(task)
    aut, starts = tm.event_automaton(programs)
    K = tm.num_decoding_channels
    assert starts.shape == (K,) and aut.vocab == V
    never = [PAD, UNK] + list(range(tm.codec.size, V))
    assert not aut.allowed[:, never].any()                               # task tokens included
    rng = np.random.default_rng(zlib.crc32(f"{task}/{name}".encode()))
    for ch in range(K):
        P = _programs(tm, programs, ch)
        for _ in range(40 if K == 1 else 8):
            toks = _random_walk(aut, int(starts[ch]), rng, 120)
            states = aut.walk(toks, int(starts[ch]))
            assert (states >= starts[ch]).all() and (states < starts[ch] + 6).all()    # a channel stays in its own block
            ev, ties, bad = tm.tokenizer.decode_segment(toks, 0.0)
            assert bad == 0, toks
            for e in ev:
                assert e.program in P, (e, P)
                assert not e.is_drum or DRUM_PROGRAM in P
            for p, _ in ties:
                assert p in P and p != DRUM_PROGRAM
        if not P:
            # nothing to transcribe: TIE then EOS is all a channel can say
            tie = tm.codec.range_of("tie")[0]
            assert np.flatnonzero(aut.allowed[starts[ch]]).tolist() == [tie]
            assert np.flatnonzero(aut.allowed[aut.next[starts[ch], tie]]).tolist() == [EOS]


def _random_notes(rng, P, n):
    pitched = sorted(p for p in P if p != DRUM_PROGRAM)
    events, ties = [], []
    for _ in range(n):
        t = round(float(rng.uniform(0, 4.0)), 2)
        if DRUM_PROGRAM in P and (not pitched or rng.random() < 0.3):
            events.append(NoteEvent(t, True, DRUM_PROGRAM, 1, int(rng.integers(0, 128))))
        elif pitched:
            events.append(NoteEvent(t, False, int(rng.choice(pitched)), int(rng.integers(0, 2)), int(rng.integers(0, 128))))
    for _ in range(int(rng.integers(0, 4))):
        if pitched:
            ties.append((int(rng.choice(pitched)), int(rng.integers(0, 128))))
    return events, ties


@pytest.mark.parametrize("task", ["mt3_full_plus", "mc13_full_plus_256", "singing_drum_v1"])
@pytest.mark.parametrize("name,programs", PROGRAM_SETS, ids=[p[0] for p in PROGRAM_SETS])
def test_grammar_completeness(task, name, programs):
    tm = TaskManager(task)
    aut, starts = tm.event_automaton(programs)
    rng = np.random.default_rng(7 + len(name))
    for ch in range(tm.num_decoding_channels):
        P = _programs(tm, programs, ch)
        for _ in range(10):
            events, ties = _random_notes(rng, P, int(rng.integers(0, 12)))
            toks = tm.tokenizer.encode_segment(events, ties, 0.0)
            states = aut.walk(toks, int(starts[ch]))
            for i, t in enumerate(toks):
                assert aut.allows(states[i], t), (i, t, toks)
                if t == EOS:
                    break


def test_grammar_respects_the_task_managers_codec_and_vocab():
    tm = TaskManager(max_shift_steps=100, vocab_size=1024)
    aut, starts = tm.event_automaton([0])
    assert aut.vocab == 1024 and tm.codec.size < 1024
    sh0, sh1 = tm.codec.range_of("shift")
    assert sh1 - sh0 == 100 and aut.allowed[3 + 1, sh0:sh1].all() and not aut.allowed[:, tm.codec.size:].any()
    with pytest.raises(ValueError):
        tm.event_automaton([130])


def test_constrained_oracle_rules():
    """Masking, forced disallowed ids (-inf, the state still moves), EOS freezing, prompt positions."""
    from yourmt3_amd.weights import make_weights
    cfg = CFG.with_(max_decode_len=16, eos_id=1)
    W = make_weights(cfg, 5)
    a = O.synthetic_audio(2, cfg)
    _, enc = O.encode(a, W, cfg, False)
    g = np.random.default_rng(3)
    aut = TokenAutomaton(g.random((3, cfg.vocab)) < 0.3, g.integers(0, 3, (3, cfg.vocab)).astype(np.int32))
    t, s, lg = constrained_greedy_decode(enc, W, cfg, 10, False, aut, start_states=torch.tensor([[1], [2]]))
    for b in range(2):
        st = aut.walk(t[b, 0].tolist(), [1, 2][b])
        eos_seen = False
        for i in range(10):
            if eos_seen:
                assert t[b, 0, i] == cfg.pad_id and s[b, 0, i] == 0.0
                continue
            m = torch.from_numpy(aut.allowed[st[i]])
            row = lg[b, 0, i].masked_fill(~m, float("-inf"))
            assert int(t[b, 0, i]) == int(torch.argmax(row))
            assert abs(float(s[b, 0, i]) - float(torch.log_softmax(row.double(), -1)[t[b, 0, i]])) < 1e-12
            eos_seen = int(t[b, 0, i]) == cfg.eos_id
    forced = torch.from_numpy(g.integers(3, cfg.vocab, (2, 1, 10)).astype(np.int32))
    tf, sf, lf = constrained_greedy_decode(enc, W, cfg, 10, False, aut, forced=forced)
    for b in range(2):
        st = aut.walk(forced[b, 0].tolist(), 0)
        for i in range(10):
            ok = aut.allows(st[i], int(forced[b, 0, i]))
            assert (sf[b, 0, i] == float("-inf")) == (not ok)


# ---------------------------------------------------------------- HF pin
def _hf_setup():
    m = _hf()
    W = _imported(m)
    a = O.synthetic_audio(2, CFG)
    enc = O.encoder_t5(O.input_projection(O.logmel(a, CFG), W, bf16=False), W, CFG, bf16=False)
    return m, W, enc


def _random_automaton(seed, n_states=3, p=0.25):
    g = np.random.default_rng(seed)
    allowed = g.random((n_states, CFG.vocab)) < p
    allowed[:, 0] = False                                      # PAD never (HF pads finished rows; the comparison stops at EOS)
    return TokenAutomaton(allowed, g.integers(0, n_states, (n_states, CFG.vocab)).astype(np.int32))


@pytest.mark.parametrize("prompted", [False, True], ids=["plain", "prompted"])
@pytest.mark.parametrize("kind", ["random3", "grammar"])
def test_constrained_oracle_matches_hf_prefix_allowed_tokens(prompted, kind):
    """fp32 both sides: ids equal, scores within 1e-4 up to EOS (HF compute_transition_scores(normalize_logits=True) over the
    scores its PrefixConstrainedLogitsProcessor produced)."""
    from transformers.modeling_outputs import BaseModelOutput
    m, W, enc = _hf_setup()
    n = 12
    if kind == "grammar":
        aut, starts = TaskManager().event_automaton([0, 5, 128])
        start = [int(starts[0]), int(starts[0])]
    else:
        aut = _random_automaton(11)
        start = [1, 2]
    prompt = torch.tensor([[[599, 598]], [[601, 598]]], dtype=torch.int32) if prompted else None
    toks, scores, _ = constrained_greedy_decode(enc, W, CFG, n, False, aut, start_states=torch.tensor(start)[:, None], prompt=prompt)
    dec_in = torch.full((2, 1), CFG.pad_id, dtype=torch.long)
    if prompt is not None:
        dec_in = torch.cat([dec_in, prompt[:, 0].long()], 1)
    n_in = dec_in.shape[1]

    def allowed_fn(batch_id, input_ids):
        st = aut.walk(input_ids[n_in:].tolist(), start[batch_id])[-1]
        return np.flatnonzero(aut.allowed[st]).tolist()

    with torch.no_grad():
        out = m.generate(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=dec_in, max_new_tokens=n,
                         do_sample=False, num_beams=1, output_scores=True, return_dict_in_generate=True,
                         prefix_allowed_tokens_fn=allowed_fn)
        ref = m.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    ref_tokens = out.sequences[:, n_in:]
    L = ref_tokens.shape[1]
    assert L >= 4
    eos = (ref_tokens == CFG.eos_id).int()
    live = (eos.cumsum(-1) - eos) == 0
    assert torch.equal(toks[:, 0, :L].long()[live], ref_tokens[live])
    d = (scores[:, 0, :L] - ref.double()).abs()[live]
    assert d.max().item() < 1e-4
    # every compared id is allowed where the walk has it
    for b in range(2):
        st = aut.walk(toks[b, 0].tolist(), start[b])
        assert all(aut.allows(st[i], int(toks[b, 0, i])) for i in range(int(live[b].sum())))


# ---------------------------------------------------------------- C header and bindings
NEW = ("ymt3_constraint_create", "ymt3_constraint_destroy", "ymt3_decode_constrained", "ymt3_transcribe_segments_constrained",
       "ymt3_transcribe_stream_constrained")


def test_header_declares_and_lib_binds_the_constrained_entry_points():
    from yourmt3_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ymt3.h")).read()
    for name in NEW:
        assert f" {name}(" in hdr, name
        assert name in _lib.SYMBOLS, name
    assert "#define YMT3_ABI_VERSION 3" in hdr and "Constraints" in hdr


def test_constrained_declarations_compile_as_plain_c(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "con.c"
    src.write_text('#include "ymt3.h"\n'
                   'int main(void) {\n'
                   '  ymt3_constraint c = 0;\n'
                   '  int (*cr)(ymt3_handle, int, int, const uint32_t*, const int32_t*, ymt3_constraint*) = ymt3_constraint_create;\n'
                   '  void (*de)(ymt3_constraint) = ymt3_constraint_destroy;\n'
                   '  int (*d)(ymt3_handle, const void*, int, int, const int32_t*, int, int32_t*, float*, const int32_t*, float*,\n'
                   '           ymt3_constraint, const int32_t*, void*) = ymt3_decode_constrained;\n'
                   '  int (*t)(ymt3_handle, const float*, int, int, const int32_t*, int, int32_t*, float*, ymt3_constraint,\n'
                   '           const int32_t*, void*) = ymt3_transcribe_segments_constrained;\n'
                   '  int (*s)(ymt3_handle, const float*, int, int, const int32_t*, int, int32_t*, float*, int, int, ymt3_constraint,\n'
                   '           const int32_t*, void*) = ymt3_transcribe_stream_constrained;\n'
                   '  (void)c; (void)cr; (void)de; (void)d; (void)t; (void)s; return 0;\n}\n')
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_lib_argtypes_match_the_header():
    """The library (built by build()) carries the symbols with the arities _lib declares."""
    from yourmt3_amd import _lib
    lib = _lib.load()
    assert len(lib.ymt3_decode_constrained.argtypes) == 13
    assert len(lib.ymt3_transcribe_segments_constrained.argtypes) == 11
    assert len(lib.ymt3_transcribe_stream_constrained.argtypes) == 13
    assert len(lib.ymt3_constraint_create.argtypes) == 6
