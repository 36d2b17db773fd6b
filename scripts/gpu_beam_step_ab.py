"""Beam step against the greedy step at the same row count, same box, interleaved (profiles/beam_step_ab.txt).

    python scripts/gpu_beam_step_ab.py separate    # beam (B, W) vs greedy at R = B * W rows, both on the separate launches
    python scripts/gpu_beam_step_ab.py default     # for orientation: one greedy batch of 64 on the default (merged) path
    python scripts/gpu_beam_step_ab.py trace       # one greedy and one beam call at 128 rows (run it under rocprofv3 --kernel-trace --stats
                                                   # to split the step between the attention and the selection kernel)

The greedy path of this build is the parent commit's (every existing kernel's ISA is unchanged), so "greedy at R rows" is the parent's
step.  configs[1] shapes (256 frames, 1024 positions), eos_id = -1 so that every call runs its 1024 steps; a decode call includes the
cross-K/V GEMM of its segments (R for greedy, B for beams).  Three interleaved repetitions per pair; the lines are JSON."""
import json
import os
import sys

mode = sys.argv[1] if len(sys.argv) > 1 else "separate"
if mode != "default":
    os.environ["YMT3_NO_ATTN_PAIR"] = "1"
    os.environ["YMT3_NO_GEMM_CHAIN"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from yourmt3_amd.config import baseline_config
from yourmt3_amd.model import YourMT3

cfg = baseline_config(1).with_(eos_id=-1)
L = cfg.max_decode_len


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def enc_of(n):
    g = torch.Generator().manual_seed(n)
    return torch.randn(n, cfg.n_frames, cfg.d_model, generator=g).bfloat16().cuda()


if mode == "default":
    m = YourMT3(cfg, max_batch=64)
    e = enc_of(64)
    m.decode(e, L)
    ms = [timed(lambda: m.decode(e, L)) for _ in range(3)]
    print(json.dumps({"greedy_default_path_rows": 64, "ms_per_call": [round(x, 1) for x in ms], "us_per_step": round(1e3 * min(ms) / L, 1)}))
    m.close()
elif mode == "trace":
    m = YourMT3(cfg, max_batch=128)
    m.decode(enc_of(128), L)
    m.decode(enc_of(32), L, num_beams=4)
    torch.cuda.synchronize()
    m.close()
else:
    m = YourMT3(cfg, max_batch=256)
    for B, W in ((16, 4), (8, 8), (32, 4), (64, 4)):
        R = B * W
        eg, eb = enc_of(R), enc_of(B)
        m.decode(eg, L)
        m.decode(eb, L, num_beams=W)
        g, b = [], []
        for _ in range(3):
            g.append(timed(lambda: m.decode(eg, L)))
            b.append(timed(lambda: m.decode(eb, L, num_beams=W)))
        print(json.dumps({"B": B, "W": W, "rows": R, "greedy_ms": [round(x, 1) for x in g], "beam_ms": [round(x, 1) for x in b],
                          "greedy_us_per_step": round(1e3 * min(g) / L, 1), "beam_us_per_step": round(1e3 * min(b) / L, 1),
                          "beam_over_greedy": round(min(b) / min(g), 3)}), flush=True)
    m.close()
