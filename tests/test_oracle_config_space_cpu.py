"""The CPU oracle against third-party arithmetic at the shapes tests/test_config_space.py runs on the GPU.

test_oracle_vs_thirdparty.py pins the oracle at the default shape only; the GPU config-space tests are only as good as the oracle
at theirs.  Same references and fp32 tolerances: HF `T5ForConditionalGeneration` built from a local config with the same seeded
weights (vocab, d_ff, decoder depth, relative-position tables, pad / EOS ids), `torch.stft` power at n_fft 512, and the HTK
filterbank's support where n_fft 512 leaves a mel filter without a bin.
"""
import pytest
import torch

from oracle import ymt3_oracle as O
from test_oracle_vs_thirdparty import _hf_model
from yourmt3_amd.config import YMT3Config
from yourmt3_amd.tables import derived_tables
from yourmt3_amd.weights import make_weights

BASE = YMT3Config(segment_samples=8191, max_decode_len=32)

HF_SHAPES = [
    ("vocab1040", dict(vocab=1040)),
    ("dff1024", dict(d_ff=1024)),
    ("dec1", dict(n_dec_layers=1)),
    ("dec8", dict(n_dec_layers=8)),
    ("rel16", dict(rel_buckets=16, rel_max_distance=64)),
    ("pad3_eos5", dict(pad_id=3, eos_id=5)),
    ("pad3_eos75", dict(pad_id=3, eos_id=75)),           # emitted at steps 7 and 12: the PAD fill is fed back
]


@pytest.mark.parametrize("name,kw", HF_SHAPES, ids=[s[0] for s in HF_SHAPES])
def test_oracle_matches_hf_t5_at_other_shapes(name, kw):
    """encoder against HF's T5 stack; then every position of a greedy decode against HF's one-shot decoder forward over the
    oracle's own fed ids (decoder_start = pad_id, and the PAD fill after an EOS), fp32 both sides"""
    from transformers.modeling_outputs import BaseModelOutput
    cfg = BASE.with_(**kw)
    W = make_weights(cfg, seed=1234)
    hf = _hf_model(W, cfg)
    a = O.synthetic_audio(2, cfg)
    mel = O.logmel(a, cfg)
    h0 = O.input_projection(mel, W, bf16=False)
    enc = O.encoder_t5(h0, W, cfg, bf16=False)
    with torch.no_grad():
        ref_enc = hf.encoder(inputs_embeds=h0).last_hidden_state
    assert (enc - ref_enc).abs().max().item() < 2e-4
    n = cfg.max_decode_len
    toks, logits = O.greedy_decode(enc, W, cfg, n, bf16=False, return_logits=True)
    dec_in = torch.cat([torch.full((2, 1), cfg.pad_id, dtype=torch.long), toks[:, 0, :-1].long()], 1)
    with torch.no_grad():
        ref = hf(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=dec_in).logits      # (2, n, V)
    assert ref.shape == (2, n, cfg.vocab)
    assert (ref - logits[:, 0]).abs().max().item() < 5e-4
    for b in range(2):                                   # the argmax up to (and including) the first EOS; PAD after it
        row = toks[b, 0].tolist()
        stop = row.index(cfg.eos_id) + 1 if cfg.eos_id in row else n
        assert torch.equal(ref[b, :stop].argmax(-1), toks[b, 0, :stop].long()), b
        assert all(t == cfg.pad_id for t in row[stop:])
    assert len(set(toks[0, 0].tolist())) > 8             # the stream is not a collapsed fixed point
    if name == "pad3_eos75":
        assert all(cfg.eos_id in toks[b, 0].tolist() for b in range(2))


@pytest.mark.parametrize("hop,samples", [(64, 4095), (256, 16383)])
def test_power_spectrogram_matches_torch_stft_at_n_fft_512(hop, samples):
    cfg = YMT3Config(n_fft=512, hop=hop, segment_samples=samples)
    a = O.synthetic_audio(2, cfg)
    st = torch.stft(a, cfg.n_fft, cfg.hop, window=torch.hann_window(cfg.n_fft), center=True,
                    pad_mode="reflect", return_complex=True)
    ref = (st.real ** 2 + st.imag ** 2).transpose(1, 2)
    got = O.power_spectrogram(a, cfg)
    assert got.shape == (2, 64, 257) == ref.shape
    assert (ref - got).abs().max() <= 2e-6 * ref.abs().max()


@pytest.mark.parametrize("n_mels,n_empty", [(64, 0), (128, 1)])
def test_mel_filterbank_support_at_n_fft_512(n_mels, n_empty):
    """257 bins spread over 128 triangles leave the narrowest low one without a bin; the blob's CSR tables say the same"""
    cfg = YMT3Config(n_fft=512, n_mels=n_mels, segment_samples=8191)
    fb = O.mel_filterbank_htk(n_mels, 512, cfg.sample_rate, cfg.f_min, cfg.f_max)
    assert fb.shape == (n_mels, 257)
    assert (fb >= 0).all() and fb.max() <= 1.0
    assert ((fb > 0).sum(0) <= 2).all()
    empty = ((fb > 0).sum(1) == 0).nonzero().flatten()
    assert empty.numel() == n_empty
    t = derived_tables(make_weights(cfg), cfg)
    assert torch.equal((t["fe.mel_len"] == 0).nonzero().flatten(), empty)
    assert torch.equal(t["fe.mel_len"].long(), (fb > 0).sum(1))
    # the oracle's log-mel at an empty filter is the floor, exactly
    mel = O.logmel(O.synthetic_audio(1, cfg), cfg)
    floor = torch.log(torch.tensor(cfg.log_floor, dtype=torch.float32))
    for i in empty.tolist():
        assert torch.equal(mel[..., i], torch.full_like(mel[..., i], floor.item()))
