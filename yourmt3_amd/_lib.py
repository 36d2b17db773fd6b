"""ctypes binding of the C ABI in include/ymt3.h.  No fallback: if the HIP library is missing
or fails to load, importing a model raises -- the product path never routes through a CPU restatement.
"""
from __future__ import annotations

import ctypes
import os

from .config import CConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YMT3_LIB", os.path.join(_HERE, "libymt3_hip.so"))

# every symbol include/ymt3.h declares (tests/test_cpu_host.py::test_library_builds_loads_and_exports_every_header_symbol checks the header against this list)
SYMBOLS = [
    "ymt3_abi_version", "ymt3_last_error", "ymt3_create", "ymt3_destroy", "ymt3_device_bytes",
    "ymt3_logmel", "ymt3_encode", "ymt3_decode_greedy", "ymt3_transcribe_segments", "ymt3_test_gemm", "ymt3_profile_decode", "ymt3_debug_decode_start", "ymt3_debug_force_stage_abort", "ymt3_set_early_stop", "ymt3_last_decode_steps",
    "ymt3_ingest_plan", "ymt3_ingest", "ymt3_transcribe_stream", "ymt3_debug_step_stamps", "ymt3_debug_kernel_stamps",
    "ymt3_set_abort_recovery", "ymt3_merged_fallbacks", "ymt3_debug_moe_trace", "ymt3_last_decode_chains",
    "ymt3_decode_prompted", "ymt3_transcribe_segments_prompted", "ymt3_transcribe_stream_prompted",
    "ymt3_decode_scored", "ymt3_transcribe_segments_scored", "ymt3_transcribe_stream_scored",
    "ymt3_constraint_create", "ymt3_constraint_destroy", "ymt3_decode_constrained", "ymt3_transcribe_segments_constrained",
    "ymt3_transcribe_stream_constrained",
    "ymt3_decode_beam", "ymt3_transcribe_segments_beam", "ymt3_debug_beam_trace", "ymt3_transcribe_stream_beam",
    "ymt3_score_tokens", "ymt3_transcribe_segments_score",
    "ymt3_qkv0_table_active",
    "ymt3_detok_create", "ymt3_detok_destroy", "ymt3_detokenize",
    "ymt3_tok_create", "ymt3_tok_destroy", "ymt3_tokenize",
    "ymt3_metrics_create", "ymt3_metrics_destroy", "ymt3_note_metrics",
    "ymt3_roll_create", "ymt3_roll_destroy", "ymt3_piano_roll", "ymt3_frame_metrics",
    "ymt3_aligner_create", "ymt3_aligner_destroy", "ymt3_align_notes", "ymt3_warp_notes",
    "ymt3_ingest_stream_create", "ymt3_ingest_stream_destroy", "ymt3_ingest_stream_reset", "ymt3_ingest_stream_plan",
    "ymt3_ingest_stream_push", "ymt3_ingest_stream_finish",
    "ymt3_detok_state_create", "ymt3_detok_state_destroy", "ymt3_detok_state_reset", "ymt3_detok_state_carry",
    "ymt3_detokenize_push", "ymt3_detokenize_finish",
    "ymt3_velocity_create", "ymt3_velocity_destroy", "ymt3_note_velocities",
    "ymt3_beats_create", "ymt3_beats_destroy", "ymt3_track_beats", "ymt3_beat_positions",
    "ymt3_bars_create", "ymt3_bars_destroy", "ymt3_track_bars",
    "ymt3_chords_create", "ymt3_chords_destroy", "ymt3_track_chords",
    "ymt3_sections_create", "ymt3_sections_destroy", "ymt3_track_sections",
    "ymt3_hands_create", "ymt3_hands_destroy", "ymt3_split_hands",
    "ymt3_test_gemm_ex", "ymt3_test_rmsnorm", "ymt3_test_enc_attention", "ymt3_test_seq_attention", "ymt3_test_spec_embed",
    "ymt3_test_dec_gemm", "ymt3_test_dec_attention", "ymt3_test_mc_cross_attention", "ymt3_test_moe_stage",
    "ymt3_test_seq_embed", "ymt3_test_dec_seq_attention", "ymt3_test_seq_lm_head",
    "ymt3_test_token_step", "ymt3_test_beam_step",
]

_lib = None


class BeamParams(ctypes.Structure):
    """ymt3_beam_params of include/ymt3.h."""
    _fields_ = [("num_beams", ctypes.c_int32), ("num_return", ctypes.c_int32), ("length_penalty", ctypes.c_float)]


class TokParams(ctypes.Structure):
    """ymt3_tok_params of include/ymt3.h (TaskManager.tok_params gives the fields)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("shift_base", "pitch_base", "velocity_base", "tie_base", "program_base", "drum_base",
                                              "max_shift_steps", "steps_per_second", "drum_program", "eos_id", "pad_id")]


class MetricsParams(ctypes.Structure):
    """ymt3_metrics_params of include/ymt3.h"""
    _fields_ = [("onset_tol", ctypes.c_double), ("offset_min_tol", ctypes.c_double), ("offset_ratio", ctypes.c_double),
                ("n_programs", ctypes.c_int32), ("drum_program", ctypes.c_int32)]


class RollParams(ctypes.Structure):
    """ymt3_roll_params of include/ymt3.h"""
    _fields_ = [("frames_per_second", ctypes.c_double), ("n_programs", ctypes.c_int32), ("drum_program", ctypes.c_int32)]


class AlignParams(ctypes.Structure):
    """ymt3_align_params of include/ymt3.h"""
    _fields_ = [("frames_per_second", ctypes.c_double), ("n_programs", ctypes.c_int32), ("drum_program", ctypes.c_int32),
                ("band_frames", ctypes.c_int32)]


class VelocityParams(ctypes.Structure):
    """ymt3_velocity_params of include/ymt3.h"""
    _fields_ = [("velocity_per_db", ctypes.c_double), ("peak_db", ctypes.c_double)] + [(n, ctypes.c_int32) for n in (
        "sample_rate", "window_samples", "n_harmonics", "peak_velocity", "min_velocity", "default_velocity", "drum_program")]


class BeatParams(ctypes.Structure):
    """ymt3_beat_params of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_double) for n in ("frames_per_second", "bpm_min", "bpm_max", "bpm_prior", "prior_octaves", "tightness")] + [
        (n, ctypes.c_int32) for n in ("window_frames", "hop_frames", "lag_step_max", "onset_cap", "n_programs", "drum_program")]


class BarParams(ctypes.Structure):
    """ymt3_bar_params of include/ymt3.h"""
    _fields_ = [("frames_per_second", ctypes.c_double), ("n_metres", ctypes.c_int32), ("metres", ctypes.c_int32 * 5)] + [
        (n, ctypes.c_int32) for n in ("near_div", "accent_cap", "w_long", "w_kick", "kick_lo", "kick_hi", "w_accent", "switch_cost", "n_programs",
                                      "drum_program")]


class ChordParams(ctypes.Structure):
    """ymt3_chord_params of include/ymt3.h"""
    _fields_ = [("frames_per_second", ctypes.c_double), ("n_qualities", ctypes.c_int32), ("qualities", ctypes.c_int32 * 8)] + [
        (n, ctypes.c_int32) for n in ("near_div", "bass_div", "w_bass", "w_none", "change_cost", "change_cost_down", "n_programs", "drum_program",
                                      "reserved")]


class SectionParams(ctypes.Structure):
    """ymt3_section_params of include/ymt3.h"""
    _fields_ = [("frames_per_second", ctypes.c_double)] + [
        (n, ctypes.c_int32) for n in ("near_div", "n_programs", "drum_program", "context", "kernel_beats", "min_len", "peak_div", "same_dist", "len_num",
                                      "max_sections")]


class HandParams(ctypes.Structure):
    """ymt3_hand_params of include/ymt3.h"""
    _fields_ = [("frames_per_second", ctypes.c_double)] + [
        (n, ctypes.c_int32) for n in ("slice_frames", "program_lo", "program_hi", "span", "w_span", "cut_min", "w_cut", "w_centre", "middle", "mid_free",
                                      "w_mid", "w_move", "w_switch", "rest_slots", "n_programs", "drum_program")]


class SeqAttnArgs(ctypes.Structure):
    """ymt3_seq_attn_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("q", "k", "v", "out", "bias_off")] + [
        (n, ctypes.c_int32) for n in ("n_seq", "H", "Tq", "Tk", "inner_n")] + [
        (n, ctypes.c_int64) for n in ("q_outer", "q_inner", "q_step", "kv_outer", "kv_inner", "kv_step", "o_outer", "o_inner", "o_step")]


class DecGemmArgs(ctypes.Structure):
    """ymt3_dec_gemm_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("x_f32", "a_bf16", "gain", "W", "out_bf16", "out_f32", "kcache", "vcache", "ssq", "part", "pend_y",
                                               "h_out", "table", "row_pos")] + [
        (n, ctypes.c_int32) for n in ("row0", "R", "N", "K", "H", "L", "ssq_stride", "mid_rows", "step")] + [("eps", ctypes.c_float)]


class DecAttnArgs(ctypes.Structure):
    """ymt3_dec_attn_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("q", "k", "v", "out", "bias", "row_pos", "wq", "x_f32", "gain", "ssq", "ipart", "wo", "opart", "anc")] + [
        (n, ctypes.c_int32) for n in ("self_attn", "step", "n_keys_const", "slab_keys", "rows_per_kv", "row0", "R", "H", "bias_stride", "ssq_stride",
                                      "force_many", "anc_rows", "anc_pitch", "W", "d")] + [("eps", ctypes.c_float)]


class McCrossArgs(ctypes.Structure):
    """ymt3_mc_cross_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("x_f32", "gain", "ssq", "wq", "k", "v", "out")] + [
        (n, ctypes.c_int32) for n in ("row0", "n_seg", "n_channels", "H", "T", "ssq_stride", "d")] + [("eps", ctypes.c_float)]


class MoeArgs(ctypes.Structure):
    """ymt3_moe_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("h", "gain", "ssq", "router", "wi", "wo", "wi_q8", "wo_q8", "wi_s", "wo_s", "xn", "sel", "gate",
                                               "hidden", "y")] + [
        (n, ctypes.c_int32) for n in ("ssq_stride", "fp8", "row0", "R", "E", "top_k", "d_model", "d_ff")] + [("eps", ctypes.c_float)]


class SeqEmbedArgs(ctypes.Structure):
    """ymt3_seq_embed_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("h", "embed", "chan_embed", "prompt", "tokens")] + [
        (n, ctypes.c_int32) for n in ("row0", "n_rows", "L", "n_prompt", "n_steps", "V", "d", "n_channels", "pad_id")]


class DecSeqAttnArgs(ctypes.Structure):
    """ymt3_dec_seq_attn_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("q", "k", "v", "out", "bias")] + [(n, ctypes.c_int64) for n in ("q_seq", "kv_seq", "o_seq")] + [
        (n, ctypes.c_int32) for n in ("ldq", "ldkv", "ldo", "kv_head", "row0", "n_rows", "L", "n_keys", "rows_per_kv", "H", "bias_stride", "causal")]


class SeqLmHeadArgs(ctypes.Structure):
    """ymt3_seq_lm_head_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("xn", "W", "tokens", "lengths", "scores", "logits")] + [
        (n, ctypes.c_int32) for n in ("M", "L", "n_prompt", "n_steps", "V", "d", "row0")]


class TokenStepArgs(ctypes.Structure):
    """ymt3_token_step_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("logits", "h", "embed", "chan_embed", "finished", "ssq", "row_pos", "row_out", "row_prompt", "row_state",
                                               "ticket", "zero_sync", "qkv0", "q0", "kcache0", "vcache0", "tokens_out", "forced", "logits_out",
                                               "scores_out", "prompt", "c_allowed", "c_next", "c_start", "state_out")] + [
        (n, ctypes.c_int64) for n in ("first_out", "first_prompt")] + [
        (n, ctypes.c_int32) for n in ("ssq_stride", "row0", "R", "V", "d", "n_channels", "eos_id", "pad_id", "zero_lines", "H", "L", "step", "step0",
                                      "n_steps", "n_prompt", "c_words", "c_n_states", "keep_shared", "from_", "v0")]


class BeamStepArgs(ctypes.Structure):
    """ymt3_beam_step_args of include/ymt3.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("logits", "h", "embed", "chan_embed", "finished", "ssq", "row_state", "anc", "fed_tok", "fed_lp", "run",
                                               "fin_score", "fin_len", "fin_store", "fin_tok", "fin_lp", "n_fin", "slot_anc", "row_pos", "row_out",
                                               "row_prompt", "prompt", "c_allowed", "c_next", "c_start", "tokens_out", "seq_out", "tok_out",
                                               "state_out")] + [("first_group", ctypes.c_int64)] + [
        (n, ctypes.c_int32) for n in ("ssq_stride", "R", "V", "d", "n_channels", "eos_id", "pad_id", "W", "anc_rows", "anc_pitch", "fed_pitch", "step",
                                      "n_steps", "n_prompt", "c_words", "c_n_states", "keep_shared", "N", "row0")] + [("alpha", ctypes.c_float)]


class YMT3Error(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YMT3Error(
            f"{LIB_PATH} not found: build it with `python -m yourmt3_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
    # The process must hold ONE HIP runtime.  torch ships its own libamdhip64.so (SONAME libamdhip64.so.7)
    # and device pointers / streams are shared with it, so torch has to be loaded first: our NEEDED
    # libamdhip64.so.7 then binds to torch's copy.  Loaded the other way round the process ends up with
    # two runtimes and the second one sees no device.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.ymt3_abi_version.restype = i32
    lib.ymt3_last_error.restype = ctypes.c_char_p
    lib.ymt3_create.argtypes = [ctypes.POINTER(CConfig), vp, sz, i32, ctypes.POINTER(vp)]
    lib.ymt3_create.restype = i32
    lib.ymt3_destroy.argtypes = [vp]
    lib.ymt3_destroy.restype = None
    lib.ymt3_device_bytes.argtypes = [vp]
    lib.ymt3_device_bytes.restype = sz
    lib.ymt3_logmel.argtypes = [vp, vp, i32, vp, vp]
    lib.ymt3_encode.argtypes = [vp, vp, i32, vp, vp]
    lib.ymt3_decode_greedy.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    lib.ymt3_transcribe_segments.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.ymt3_test_gemm.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.ymt3_profile_decode.argtypes = [vp, vp, i32, i32, i32, vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), vp]
    lib.ymt3_profile_decode.restype = i32
    lib.ymt3_debug_decode_start.argtypes = [vp, i32]
    lib.ymt3_debug_decode_start.restype = i32
    lib.ymt3_debug_force_stage_abort.argtypes = [vp]
    lib.ymt3_debug_force_stage_abort.restype = i32
    lib.ymt3_last_decode_steps.argtypes = [vp]
    lib.ymt3_last_decode_steps.restype = i32
    lib.ymt3_set_early_stop.argtypes = [vp, i32]
    lib.ymt3_set_early_stop.restype = i32
    lib.ymt3_ingest_plan.argtypes = [vp, ctypes.c_int64, i32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    lib.ymt3_ingest_plan.restype = i32
    lib.ymt3_ingest.argtypes = [vp, vp, i32, ctypes.c_int64, i32, i32, vp, i32, vp]
    lib.ymt3_ingest.restype = i32
    lib.ymt3_transcribe_stream.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp]
    lib.ymt3_transcribe_stream.restype = i32
    lib.ymt3_decode_prompted.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp]
    lib.ymt3_decode_prompted.restype = i32
    lib.ymt3_transcribe_segments_prompted.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    lib.ymt3_transcribe_segments_prompted.restype = i32
    lib.ymt3_transcribe_stream_prompted.argtypes = [vp, vp, i32, i32, vp, i32, vp, i32, i32, vp]
    lib.ymt3_transcribe_stream_prompted.restype = i32
    lib.ymt3_decode_scored.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.ymt3_decode_scored.restype = i32
    lib.ymt3_transcribe_segments_scored.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp]
    lib.ymt3_transcribe_segments_scored.restype = i32
    lib.ymt3_transcribe_stream_scored.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, i32, i32, vp]
    lib.ymt3_transcribe_stream_scored.restype = i32
    lib.ymt3_constraint_create.argtypes = [vp, i32, i32, vp, vp, ctypes.POINTER(vp)]
    lib.ymt3_constraint_create.restype = i32
    lib.ymt3_constraint_destroy.argtypes = [vp]
    lib.ymt3_constraint_destroy.restype = None
    lib.ymt3_decode_constrained.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ymt3_decode_constrained.restype = i32
    lib.ymt3_transcribe_segments_constrained.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.ymt3_transcribe_segments_constrained.restype = i32
    lib.ymt3_transcribe_stream_constrained.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp]
    lib.ymt3_transcribe_stream_constrained.restype = i32
    lib.ymt3_debug_step_stamps.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int)]
    lib.ymt3_debug_step_stamps.restype = i32
    lib.ymt3_debug_kernel_stamps.argtypes = [vp, i32, vp, i32]
    lib.ymt3_debug_kernel_stamps.restype = i32
    lib.ymt3_set_abort_recovery.argtypes = [vp, i32]
    lib.ymt3_set_abort_recovery.restype = i32
    lib.ymt3_merged_fallbacks.argtypes = [vp]
    lib.ymt3_merged_fallbacks.restype = i32
    lib.ymt3_last_decode_chains.argtypes = [vp]
    lib.ymt3_last_decode_chains.restype = i32
    lib.ymt3_qkv0_table_active.argtypes = [vp]
    lib.ymt3_qkv0_table_active.restype = i32
    lib.ymt3_debug_moe_trace.argtypes = [vp, vp, i32, i32]
    lib.ymt3_debug_moe_trace.restype = i32
    bp = ctypes.POINTER(BeamParams)
    lib.ymt3_decode_beam.argtypes = [vp, vp, i32, i32, vp, i32, bp, vp, vp, vp, vp, vp, vp]
    lib.ymt3_decode_beam.restype = i32
    lib.ymt3_transcribe_segments_beam.argtypes = [vp, vp, i32, i32, vp, i32, bp, vp, vp, vp, vp, vp, vp]
    lib.ymt3_transcribe_segments_beam.restype = i32
    lib.ymt3_transcribe_stream_beam.argtypes = [vp, vp, i32, i32, vp, i32, bp, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.ymt3_transcribe_stream_beam.restype = i32
    lib.ymt3_debug_beam_trace.argtypes = [vp, vp, vp, vp, i32, i32]
    lib.ymt3_debug_beam_trace.restype = i32
    lib.ymt3_score_tokens.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.ymt3_score_tokens.restype = i32
    lib.ymt3_transcribe_segments_score.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp]
    lib.ymt3_transcribe_segments_score.restype = i32
    lib.ymt3_detok_create.argtypes = [vp, vp, i32, i32, i32, i32, i32, ctypes.POINTER(vp)]
    lib.ymt3_detok_create.restype = i32
    lib.ymt3_detok_destroy.argtypes = [vp]
    lib.ymt3_detok_destroy.restype = None
    lib.ymt3_detokenize.argtypes = [vp, vp, vp, vp, i32, i32, ctypes.c_longlong, ctypes.c_longlong, vp, ctypes.c_double, vp, ctypes.c_longlong, vp, vp]
    lib.ymt3_detokenize.restype = i32
    lib.ymt3_tok_create.argtypes = [vp, ctypes.POINTER(TokParams), vp, i32, i32, i32, ctypes.POINTER(vp)]
    lib.ymt3_tok_create.restype = i32
    lib.ymt3_tok_destroy.argtypes = [vp]
    lib.ymt3_tok_destroy.restype = None
    lib.ymt3_tokenize.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, i32, ctypes.c_double, i32, vp, vp, vp]
    lib.ymt3_tokenize.restype = i32
    lib.ymt3_metrics_create.argtypes = [vp, ctypes.POINTER(MetricsParams), ctypes.c_longlong, ctypes.c_longlong, ctypes.POINTER(vp)]
    lib.ymt3_metrics_create.restype = i32
    lib.ymt3_metrics_destroy.argtypes = [vp]
    lib.ymt3_metrics_destroy.restype = None
    lib.ymt3_note_metrics.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, vp, ctypes.c_longlong, vp, vp, vp]
    lib.ymt3_note_metrics.restype = i32
    lib.ymt3_roll_create.argtypes = [vp, ctypes.POINTER(RollParams), ctypes.c_longlong, ctypes.POINTER(vp)]
    lib.ymt3_roll_create.restype = i32
    lib.ymt3_roll_destroy.argtypes = [vp]
    lib.ymt3_roll_destroy.restype = None
    lib.ymt3_piano_roll.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, ctypes.c_longlong, i32, i32, vp, vp]
    lib.ymt3_piano_roll.restype = i32
    lib.ymt3_frame_metrics.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, vp, ctypes.c_longlong, vp, ctypes.c_longlong, vp, vp]
    lib.ymt3_frame_metrics.restype = i32
    lib.ymt3_aligner_create.argtypes = [vp, ctypes.POINTER(AlignParams), ctypes.c_longlong, ctypes.POINTER(vp)]
    lib.ymt3_aligner_create.restype = i32
    lib.ymt3_aligner_destroy.argtypes = [vp]
    lib.ymt3_aligner_destroy.restype = None
    lib.ymt3_align_notes.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, ctypes.c_longlong, vp, ctypes.c_longlong, vp, ctypes.c_longlong, vp, vp, vp, vp]
    lib.ymt3_align_notes.restype = i32
    lib.ymt3_warp_notes.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, vp, ctypes.c_longlong, vp, vp]
    lib.ymt3_warp_notes.restype = i32
    i64 = ctypes.c_int64
    lib.ymt3_ingest_stream_create.argtypes = [vp, i32, i32, i32, i64, ctypes.POINTER(vp)]
    lib.ymt3_ingest_stream_create.restype = i32
    lib.ymt3_ingest_stream_destroy.argtypes = [vp]
    lib.ymt3_ingest_stream_destroy.restype = None
    lib.ymt3_ingest_stream_reset.argtypes = [vp, vp, vp]
    lib.ymt3_ingest_stream_reset.restype = i32
    lib.ymt3_ingest_stream_plan.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_int)]
    lib.ymt3_ingest_stream_plan.restype = i32
    lib.ymt3_ingest_stream_push.argtypes = [vp, vp, vp, i64, vp, i32, ctypes.POINTER(ctypes.c_int), vp]
    lib.ymt3_ingest_stream_push.restype = i32
    lib.ymt3_ingest_stream_finish.argtypes = [vp, vp, vp, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(i64), vp]
    lib.ymt3_ingest_stream_finish.restype = i32
    ll, f64 = ctypes.c_longlong, ctypes.c_double
    lib.ymt3_detok_state_create.argtypes = [vp, vp, i32, ctypes.POINTER(vp)]
    lib.ymt3_detok_state_create.restype = i32
    lib.ymt3_detok_state_destroy.argtypes = [vp]
    lib.ymt3_detok_state_destroy.restype = None
    lib.ymt3_detok_state_reset.argtypes = [vp, vp, vp]
    lib.ymt3_detok_state_reset.restype = i32
    lib.ymt3_detok_state_carry.argtypes = [vp]
    lib.ymt3_detok_state_carry.restype = ll
    lib.ymt3_detokenize_push.argtypes = [vp, vp, vp, vp, vp, i32, i32, ll, ll, vp, f64, vp, ll, vp, vp]
    lib.ymt3_detokenize_push.restype = i32
    lib.ymt3_detokenize_finish.argtypes = [vp, vp, vp, f64, vp, ll, vp, vp]
    lib.ymt3_detokenize_finish.restype = i32
    lib.ymt3_velocity_create.argtypes = [vp, ctypes.POINTER(VelocityParams), ctypes.POINTER(vp)]
    lib.ymt3_velocity_create.restype = i32
    lib.ymt3_velocity_destroy.argtypes = [vp]
    lib.ymt3_velocity_destroy.restype = None
    lib.ymt3_note_velocities.argtypes = [vp, vp, vp, ll, vp, ll, vp, vp, vp, vp, vp, vp]
    lib.ymt3_note_velocities.restype = i32
    lib.ymt3_beats_create.argtypes = [vp, ctypes.POINTER(BeatParams), ll, ctypes.POINTER(vp)]
    lib.ymt3_beats_create.restype = i32
    lib.ymt3_beats_destroy.argtypes = [vp]
    lib.ymt3_beats_destroy.restype = None
    lib.ymt3_track_beats.argtypes = [vp, vp, vp, ll, vp, ll, vp, ll, vp, vp, vp]
    lib.ymt3_track_beats.restype = i32
    lib.ymt3_beat_positions.argtypes = [vp, vp, vp, vp, vp, ll, vp, i32, vp, vp]
    lib.ymt3_beat_positions.restype = i32
    lib.ymt3_bars_create.argtypes = [vp, ctypes.POINTER(BarParams), ll, ll, ctypes.POINTER(vp)]
    lib.ymt3_bars_create.restype = i32
    lib.ymt3_bars_destroy.argtypes = [vp]
    lib.ymt3_bars_destroy.restype = None
    lib.ymt3_track_bars.argtypes = [vp, vp, vp, vp, vp, ll, vp, ll, vp, ll, vp, vp]
    lib.ymt3_track_bars.restype = i32
    lib.ymt3_chords_create.argtypes = [vp, ctypes.POINTER(ChordParams), ll, ll, ctypes.POINTER(vp)]
    lib.ymt3_chords_create.restype = i32
    lib.ymt3_chords_destroy.argtypes = [vp]
    lib.ymt3_chords_destroy.restype = None
    lib.ymt3_track_chords.argtypes = [vp, vp, vp, vp, vp, vp, ll, vp, ll, vp, ll, vp, vp]
    lib.ymt3_track_chords.restype = i32
    lib.ymt3_sections_create.argtypes = [vp, ctypes.POINTER(SectionParams), ll, ll, ctypes.POINTER(vp)]
    lib.ymt3_sections_create.restype = i32
    lib.ymt3_sections_destroy.argtypes = [vp]
    lib.ymt3_sections_destroy.restype = None
    lib.ymt3_track_sections.argtypes = [vp, vp, vp, vp, vp, vp, ll, vp, ll, vp, ll, vp, vp, vp]
    lib.ymt3_track_sections.restype = i32
    lib.ymt3_hands_create.argtypes = [vp, ctypes.POINTER(HandParams), ll, ll, ctypes.POINTER(vp)]
    lib.ymt3_hands_create.restype = i32
    lib.ymt3_hands_destroy.argtypes = [vp]
    lib.ymt3_hands_destroy.restype = None
    lib.ymt3_split_hands.argtypes = [vp, vp, vp, ll, vp, ll, vp, vp, ll, vp, vp]
    lib.ymt3_split_hands.restype = i32
    f32 = ctypes.c_float
    lib.ymt3_test_gemm_ex.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.ymt3_test_gemm_ex.restype = i32
    lib.ymt3_test_rmsnorm.argtypes = [vp, vp, vp, vp, i32, i32, f32, vp]
    lib.ymt3_test_rmsnorm.restype = i32
    lib.ymt3_test_enc_attention.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp]
    lib.ymt3_test_enc_attention.restype = i32
    lib.ymt3_test_seq_attention.argtypes = [vp, ctypes.POINTER(SeqAttnArgs), vp]
    lib.ymt3_test_seq_attention.restype = i32
    lib.ymt3_test_spec_embed.argtypes = [vp, vp, vp, vp, vp, vp, ll, i32, i32, f32, vp]
    lib.ymt3_test_spec_embed.restype = i32
    lib.ymt3_test_dec_gemm.argtypes = [vp, i32, ctypes.POINTER(DecGemmArgs), vp]
    lib.ymt3_test_dec_gemm.restype = i32
    lib.ymt3_test_moe_stage.argtypes = [vp, i32, ctypes.POINTER(MoeArgs), vp]
    lib.ymt3_test_moe_stage.restype = i32
    lib.ymt3_test_dec_attention.argtypes = [vp, ctypes.POINTER(DecAttnArgs), vp]
    lib.ymt3_test_dec_attention.restype = i32
    lib.ymt3_test_mc_cross_attention.argtypes = [vp, ctypes.POINTER(McCrossArgs), vp]
    lib.ymt3_test_mc_cross_attention.restype = i32
    for name, struct in (("ymt3_test_seq_embed", SeqEmbedArgs), ("ymt3_test_dec_seq_attention", DecSeqAttnArgs), ("ymt3_test_seq_lm_head", SeqLmHeadArgs)):
        getattr(lib, name).argtypes = [vp, ctypes.POINTER(struct), vp]
        getattr(lib, name).restype = i32
    for name, struct in (("ymt3_test_token_step", TokenStepArgs), ("ymt3_test_beam_step", BeamStepArgs)):
        getattr(lib, name).argtypes = [vp, i32, ctypes.POINTER(struct), vp]
        getattr(lib, name).restype = i32
    for n in ("ymt3_logmel", "ymt3_encode", "ymt3_decode_greedy", "ymt3_transcribe_segments", "ymt3_test_gemm"):
        getattr(lib, n).restype = i32
    if lib.ymt3_abi_version() != 3:
        raise YMT3Error("libymt3_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise YMT3Error(f"ymt3 error {rc}: {load().ymt3_last_error().decode(errors='replace')}")
