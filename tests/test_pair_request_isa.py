"""What hipcc emits for the attention pair's occupancy and priority (CPU test: cross-compiles csrc/decode.hip to gfx950 assembly, no GPU needed).

dec_attn_pair_kernel, resource fields and instruction order only:
  - two workgroups per CU: <= 128 VGPRs, no spill, no scratch, static LDS + the 64 KB of wo within half a CU's 160 KB;
  - laggard first (decode.hip, attn_body): exactly one `s_setprio 1`, in front of the self-attention stream's first request, and one
    `s_setprio 0` behind the row's arrival and in front of every request of the cross-attention half -- a workgroup that kept its priority
    into pair_wait would poll ahead of the producers it waits for.
(The request order of the cross half's K/V block -- K in front of V -- was built and measured with this work and is not in the tree:
profiles/pair_request_order_ab.txt.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def decode_asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    from yourmt3_amd import build as B
    out = tmp_path_factory.mktemp("isa") / "decode.s"
    flags = [f for f in B.FLAGS if f not in ("-fPIC",)]
    cmd = [hipcc] + flags + ["-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "yourmt3_amd", "csrc", "decode.hip"),
                             "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return out.read_text()


VMEM = re.compile(r"^(global_|buffer_|flat_|scratch_)")


def _kernel_body(asm: str, name: str) -> list:
    m = re.search(r"^(_Z\w*" + name + r"\w*):[^\n]*\n(.*?)\n\s*s_endpgm", asm, re.S | re.M)
    assert m, f"kernel {name} not found in the assembly"
    return [l.strip() for l in m.group(2).splitlines() if l.strip() and not l.strip().startswith(";")]


def test_attention_pair_fits_two_workgroups_per_cu(decode_asm):
    m = re.search(r"\.name:\s+\S*dec_attn_pair_kernel\S*\n(.*?)\.wavefront_size", decode_asm, re.S)
    assert m
    meta = m.group(1)
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    k = re.search(r"\.amdhsa_kernel \S*dec_attn_pair_kernel\S*\n(.*?)\.end_amdhsa_kernel", decode_asm, re.S)
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", k.group(1)).group(1))
    print(f"dec_attn_pair_kernel: {vgpr} VGPRs, {spill} + {sspill} spilled, {scratch} B scratch, {lds} B static LDS")
    assert vgpr <= 128 and spill == 0 and sspill == 0 and scratch == 0, (vgpr, spill, sspill, scratch)
    assert lds + 65536 <= 80 * 1024, lds
    body = _kernel_body(decode_asm, "dec_attn_pair_kernel")
    assert not any(l.startswith("scratch_") for l in body)


def test_self_half_runs_at_raised_priority_up_to_the_signal(decode_asm):
    body = _kernel_body(decode_asm, "dec_attn_pair_kernel")
    prio = [(i, l.split()[1]) for i, l in enumerate(body) if l.startswith("s_setprio")]
    assert [p for _, p in prio] == ["1", "0"], prio
    up, down = prio[0][0], prio[1][0]
    first_kv = next(i for i, l in enumerate(body) if l.startswith("global_load_dwordx4") and l.rstrip().endswith(" nt"))
    assert up < first_kv, "raised in front of the self-attention stream's first request"
    arrival = next(i for i, l in enumerate(body) if l.startswith("global_atomic_add"))
    stores = [i for i, l in enumerate(body) if l.startswith("buffer_store_dwordx4") and " sc1" in l]
    assert len(stores) == 4 and up < stores[0] and stores[-1] < arrival < down
    # back to 0 in front of every request of the cross-attention half and of the poll
    between = [l for l in body[arrival + 1:down] if VMEM.match(l) and not l.startswith("global_store_dwordx2")]
    assert not between, between
    assert not any(l.startswith("s_cbranch") for l in body[:up]), "every wave raises its priority: no conditional branch in front of it"
