"""What the merged decode step's kernels may cost after the self-attention tail got one straight-line path per sub-block count (CPU test:
cross-compiles csrc/*.hip to gfx950 assembly, no GPU needed).

dec_attn_pair_kernel: 512 workgroups of 512 threads are resident at once, two per CU -- at most 128 VGPRs, no spill, no scratch.  The GEMM
chain's two launch forms (next QKV projection / lm_head) run without scratch.  The three kernels of a step -- pair, chain, argmax -- stay
under 64 KB of code together (the instruction cache one CU's workgroups share), counting both chain forms."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asm(tmp_path_factory, name):
    hipcc = next((c for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    from yourmt3_amd import build as B
    out = tmp_path_factory.mktemp("isa") / (name + ".s")
    flags = [f for f in B.FLAGS if f not in ("-fPIC",)]
    cmd = [hipcc] + flags + ["-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "yourmt3_amd", "csrc", name + ".hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return out.read_text()


@pytest.fixture(scope="module")
def decode_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "decode")


@pytest.fixture(scope="module")
def chain_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "dec_chain")


def _meta(asm, pattern):
    """[(mangled name, vgprs, spilled vgprs, scratch bytes, code bytes)] of the kernels whose name matches"""
    out = []
    for name, meta in re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S):
        if not re.search(pattern, name):
            continue
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        body = re.search(r"^" + re.escape(name) + r":.*?; codeLenInByte = (\d+)", asm, re.S | re.M)
        assert body, name
        out.append((name, vgpr, spill, scratch, int(body.group(1))))
    return out


def test_attention_pair_keeps_two_workgroups_per_cu(decode_asm):
    (name, vgpr, spill, scratch, _), = _meta(decode_asm, "dec_attn_pair_kernel")
    assert vgpr <= 128 and spill == 0 and scratch == 0, (vgpr, spill, scratch)


def test_chain_launch_forms_run_without_scratch(chain_asm):
    # dec_chain_kernel<DG_NORM_QKV_CACHE = 0, false> and <DG_NORM_LOGITS = 3, false>
    forms = _meta(chain_asm, r"dec_chain_kernelILi[03]ELb0EE")
    assert len(forms) == 2, [f[0] for f in forms]
    for name, vgpr, spill, scratch, _ in forms:
        assert spill == 0 and scratch == 0, (name, spill, scratch)


def test_a_steps_kernels_stay_under_64_kb_of_code(decode_asm, chain_asm):
    (_, _, _, _, pair), = _meta(decode_asm, "dec_attn_pair_kernel")
    (_, _, _, _, argmax), = _meta(decode_asm, "argmax_embed_kernel")
    chains = [f[4] for f in _meta(chain_asm, r"dec_chain_kernelILi[03]ELb0EE")]
    assert len(chains) == 2
    print(f"code bytes: pair {pair}, chain {chains}, argmax {argmax}")
    assert pair + sum(chains) + argmax < 64 * 1024, (pair, chains, argmax)
