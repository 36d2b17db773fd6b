"""The launch table of a decode step: which kernel classes a step launches, in which order, on which grids.

Every decode path turns "one step of rows [row0, row0 + R)" into launches in one host function (csrc/runtime.hip, launch_step).  A handle
created under YMT3_STAMP=1 records the (class, grid) of every stamped launch of the last step it built; this file compares that list, for
every regime the step has, with tests/golden/step_launches.json.  The fixture was recorded from the library of the commit named inside
it (the parent of the change that introduced this test), never from the code under test, so a host-side change cannot move, drop or add
a launch unnoticed.  Results are not compared there: the parity suites hold every regime to the oracle and to each other bit for bit.
The last test holds one pair of switches no other file combines (MoE FFN, separate query projection) to the oracle.

Not covered, on purpose: under YMT3_STAMP the layer-0 QKV table is not built (test_qkv0_table.py holds its launch sequence) and the
separate MoE stages carry no stamp (ymt3_profile_decode's launch counts hold them, test_gpu_parity.py).

Re-recording (only when a change means to move a launch): build the commit to record from into a second library and run
    YMT3_LIB=<that library> PYTHONPATH=. python tests/test_step_launches.py --record <its commit hash>
"""
import json
import os
import sys

import pytest

from oracle import ymt3_oracle as O
from test_gpu_parity import MC3, MIN_SAFE, SMALL, TAU, _model, _moe_case
from test_qkv0_table import _env
from yourmt3_amd.config import FFN_MOE

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "step_launches.json")
STEPS = 4
MOE = SMALL.with_(dec_ffn=FFN_MOE)
MOE_FP8 = SMALL.with_(dec_ffn=FFN_MOE, moe_fp8=1)


def _lockstep(B, **kw):
    return lambda m, a: m.inference(a[:B], max_token_length=STEPS, **kw)


def _stream(**kw):
    return lambda m, a: m.inference_stream(a[:3], max_token_length=STEPS, slots=2, **kw)


# (group, config, max_batch, environment at create, [(case, run)]): one handle per group
GROUPS = [
    # 1 .. 64 rows: attention pair + GEMM chain; 65 and 96: folded O-projection without the pair; 97: the self O-projection launched
    ("rows", SMALL, 97, {}, [("r%d" % r, _lockstep(r)) for r in (1, 5, 64, 65, 96, 97)]),
    ("separate", SMALL, 4, {"YMT3_NO_ATTN_PAIR": "1", "YMT3_NO_GEMM_CHAIN": "1"}, [("r4", _lockstep(4))]),
    ("no_fuseq", SMALL, 4, {"YMT3_NO_FUSEQ": "1"}, [("r4", _lockstep(4))]),
    ("no_fold_o", SMALL, 4, {"YMT3_NO_FOLD_O": "1"}, [("r4", _lockstep(4))]),
    ("step_kernel", SMALL, 4, {"YMT3_STEP_KERNEL": "1"}, [("r4", _lockstep(4))]),
    ("two_chains", SMALL, 4, {"YMT3_CHAINS": "2"}, [("r4", _lockstep(4))]),
    ("moe_bf16", MOE, 4, {}, [("r4", _lockstep(4))]),
    ("moe_bf16_no_chain", MOE, 4, {"YMT3_NO_MOE_CHAIN": "1"}, [("r4", _lockstep(4))]),
    ("moe_bf16_combine_launch", MOE, 4, {"YMT3_MOE_COMBINE_LAUNCH": "1"}, [("r4", _lockstep(4))]),
    ("moe_fp8", MOE_FP8, 4, {}, [("r4", _lockstep(4))]),
    ("moe_fp8_no_chain", MOE_FP8, 4, {"YMT3_NO_MOE_CHAIN": "1"}, [("r4", _lockstep(4))]),
    ("moe_fp8_combine_launch", MOE_FP8, 4, {"YMT3_MOE_COMBINE_LAUNCH": "1"}, [("r4", _lockstep(4))]),
    ("mc3", MC3, 4, {}, [("b2", _lockstep(2))]),
    ("modes", SMALL, 4, {}, [("beam_w2_b2", _lockstep(2, num_beams=2)), ("stream_3_in_2", _stream()),
                             ("stream_beam_w2_3_in_2", _stream(num_beams=2))]),
]


def _tables(group):
    """{case id: [[class name, grid], ...]} of one group: a handle under YMT3_STAMP=1 plus the group's environment, 4 steps per case"""
    name, cfg, max_batch, env, cases = group
    with _env(YMT3_STAMP="1", **env):
        m = _model(cfg, max_batch=max_batch)
    try:
        a = O.synthetic_audio(8, cfg, seed=11)
        a = a.repeat(-(-max_batch // 8), 1)[:max_batch].cuda()
        out = {}
        for case, run in cases:
            run(m, a)
            out[name + "/" + case] = [[r[0], r[1]] for r in m.step_stamps()]
        return out
    finally:
        m.close()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_step_launch_table_is_the_recorded_one(group, golden):
    got = _tables(group)
    for case, rows in got.items():
        print(case, rows)
    for case, rows in got.items():
        assert rows, case
        assert rows == golden["cases"][case], case


def test_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(g[0] + "/" + c[0] for g in GROUPS for c in g[4])
    assert len(golden["recorded_from_commit"]) == 40


def test_moe_separate_query_projection_reads_the_residual_buffer_in_use():
    """MoE decoder with the combine folded into the next QKV projection: that projection moves the residual stream to the other of two
    buffers.  A separate cross-attention query projection (YMT3_NO_FUSEQ=1) launched after it must norm the buffer now in use.  No other
    test runs this pair of switches; the handle is held to the oracle at every step, routing teacher-forced, at the bf16 MoE bounds of
    test_gpu_parity.py::test_moe_decoder_ffn_matches_oracle (logits max 0.06 / mean 6e-3, TAU, router deficit 0.01, MIN_SAFE)."""
    cfg = MOE.with_(max_decode_len=32, eos_id=-1)
    with _env(YMT3_NO_FUSEQ="1", YMT3_DEBUG_HOOKS="1"):
        m = _model(cfg, max_batch=4)
    try:
        _moe_case(cfg, 24, 0.06, 6e-3, TAU, 0.01, None, min_safe=MIN_SAFE, m=m, name="moe_no_fuseq_24_steps_routing_teacher_forced")
    finally:
        m.close()


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record" or len(sys.argv[2]) != 40:
        sys.exit("usage: YMT3_LIB=<library of the commit> python tests/test_step_launches.py --record <40-digit commit hash>")
    cases = {}
    for g in GROUPS:
        cases.update(_tables(g))
    with open(FIXTURE, "w") as f:
        f.write('{\n "recorded_from_commit": "%s",\n "cases": {\n' % sys.argv[2])
        f.write(",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in sorted(cases.items())))
        f.write("\n }\n}\n")
    print("recorded", len(cases), "cases to", FIXTURE)
