"""ctypes binding of ``libsmoltts_hip.so`` (include/smoltts_hip.h) and the thin Python objects
around it.  PyTorch-ROCm is used only as a container for device memory and streams.

There is no CPU fallback: ``load_library`` raises when the HIP library has not been built, and
every wrapper raises ``SmolttsError`` on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass, replace
from functools import cached_property
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .config import NumericsMode, RQTransformerModelArgs, TokenConfig
from .formats import ENC_OFF, check_container, parse_stream_format
from .seam import segment_flags
from .tsm import out_bound
from . import packing

LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libsmoltts_hip.so"
MAX_LAYERS, MAX_FAST_LAYERS, MIMI_MAX_LAYERS = 64, 16, 16


class SmolttsError(RuntimeError):
    pass


# ------------------------------------------------------------------------------- C structs
class BlockWeights(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("attn_norm", "wqkv", "wo", "ffn_norm", "w13", "w2")]


class LMConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dim", "n_layer", "n_head", "n_kv_head", "inter",
        "fast_dim", "n_fast_layer", "fast_n_head", "fast_n_kv_head", "fast_inter",
        "vocab_size", "codebook_size", "num_codebooks", "n_fast", "duplicate_code_0", "depthwise_wte",
        "has_fast_project_in", "embed_mask_mode", "semantic_start_id", "semantic_end_id", "im_end_id",
        "max_seq_len")] + [("norm_eps", C.c_float), ("weight_format", C.c_int32)]


class LMWeights(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "text_emb", "codebook_emb", "fast_emb", "norm", "head", "fast_norm", "fast_head",
        "fast_head_step_stride", "fast_proj_w", "fast_proj_b", "rope", "fast_rope")] + [
        ("layers", BlockWeights * MAX_LAYERS), ("fast_layers", BlockWeights * MAX_FAST_LAYERS)]


class GemmArgs(C.Structure):
    _fields_ = [
        ("w_dev", C.c_void_p), ("w_is_fp32", C.c_int32), ("x_dev", C.c_void_p), ("ldx", C.c_int64),
        ("x_bstride", C.c_int64), ("rows_per_batch", C.c_int32), ("M", C.c_int32), ("N", C.c_int32),
        ("K", C.c_int32), ("prologue", C.c_int32), ("epilogue", C.c_int32), ("gamma_dev", C.c_void_p),
        ("eps", C.c_float), ("bias_dev", C.c_void_p), ("scale_dev", C.c_void_p), ("resid_dev", C.c_void_p),
        ("ldr", C.c_int64), ("r_bstride", C.c_int64), ("out_dev", C.c_void_p), ("ldo", C.c_int64), ("o_bstride", C.c_int64),
        ("elu_out", C.c_int32), ("raw_out_dev", C.c_void_p), ("raw_bstride", C.c_int64), ("rope_dev", C.c_void_p),
        ("row_pos_dev", C.c_void_p), ("row_slot_dev", C.c_void_p), ("k_cache_dev", C.c_void_p),
        ("v_cache_dev", C.c_void_p), ("n_q_heads", C.c_int32), ("n_kv_heads", C.c_int32), ("cache_len", C.c_int32),
        ("w3_dev", C.c_void_p), ("splitk_ws_dev", C.c_void_p), ("splitk_ws_floats", C.c_int64),
        ("beta_dev", C.c_void_p), ("ln_scratch_dev", C.c_void_p), ("k_cache3_dev", C.c_void_p), ("v_cache3_dev", C.c_void_p),
        ("b3_products", C.c_int32),
    ]


class MimiLayerWeights(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("ln1_w", "ln1_b", "wqkv", "wo", "ls1", "ln2_w", "ln2_b", "fc1", "fc2", "ls2",
                                          "wqkv3", "wo3", "fc13", "fc23")]


class MimiConv(C.Structure):
    _fields_ = [("w", C.c_uint64), ("b", C.c_uint64)] + [(n, C.c_int32) for n in ("cin", "cout", "k", "stride", "transposed")] + [
        ("_pad", C.c_int32), ("w3", C.c_uint64)]


class MimiConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_codebooks", "n_layers", "window", "max_positions")]


class MimiWeights(C.Structure):
    _fields_ = [("rvq_table", C.c_uint64), ("upsample_w", C.c_uint64), ("rope", C.c_uint64),
                ("layers", MimiLayerWeights * MIMI_MAX_LAYERS), ("convs", MimiConv * 14), ("final_w", C.c_uint64)]


class MimiEncConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_codebooks", "n_layers", "window", "max_positions", "extra_right")]


class MimiEncWeights(C.Structure):
    _fields_ = [("conv0_w", C.c_uint64), ("conv0_b", C.c_uint64), ("convs", MimiConv * 13),
                ("layers", MimiLayerWeights * MIMI_MAX_LAYERS), ("rope", C.c_uint64), ("downsample_w", C.c_uint64),
                ("in_proj", C.c_uint64 * 2), ("codebooks_t", C.c_uint64), ("codebooks", C.c_uint64), ("codebook_sq", C.c_uint64)]


class PrefixHeader(C.Structure):
    _fields_ = [("magic", C.c_uint32)] + [(n, C.c_int32) for n in ("n_positions", "n_layer", "n_kv_head", "kv_format", "head_dim")] + [
        ("data_bytes", C.c_uint64)]


PRO_NONE, PRO_RMSNORM, PRO_ELU, PRO_LAYERNORM = 0, 1, 2, 3
KV_FORMATS = {"fp32": 0, "bf16": 1}  # SMOLTTS_KV_*
EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_GELU, EPI_SCALE_RESID, EPI_QKV_ROPE = range(6)

_lib = None

_EXPORTS = [
    "smoltts_last_error", "smoltts_abi_version", "smoltts_engine_create", "smoltts_engine_destroy",
    "smoltts_session_slab_bytes", "smoltts_session_create", "smoltts_session_destroy", "smoltts_lm_prefill",
    "smoltts_lm_decode", "smoltts_session_outputs", "smoltts_mimi_create", "smoltts_mimi_destroy",
    "smoltts_mimi_slab_bytes", "smoltts_mimi_session_create", "smoltts_mimi_session_destroy", "smoltts_mimi_reset",
    "smoltts_mimi_decode_chunk", "smoltts_k_gemm", "smoltts_k_attention", "smoltts_k_embed", "smoltts_k_argmax",
    "smoltts_k_layernorm", "smoltts_k_gemm3", "smoltts_k_x3_pack",
    "smoltts_session_measure_duplicate", "smoltts_session_margin_at", "smoltts_session_drop_graph", "smoltts_session_set_frames_per_graph", "smoltts_engine_fast_qkv_bytes", "smoltts_engine_build_fast_qkv", "smoltts_session_set_option", "smoltts_gemm3_attn_fusable", "smoltts_lm_park_slots", "smoltts_lm_prefill_side", "smoltts_lm_start_slots", "smoltts_session_kv_cache", "smoltts_k_attention_split", "smoltts_k_attention_rows3",
    "smoltts_session_slab_bytes_kv", "smoltts_session_create_kv", "smoltts_k_attention_kv", "smoltts_session_set_sampling", "smoltts_k_sample",
    "smoltts_lm_prefill_chunk", "smoltts_lm_prefill_deferred", "smoltts_mimi_reset_slots", "smoltts_mimi_encoder_create", "smoltts_mimi_encoder_destroy", "smoltts_mimi_encode_frames",
    "smoltts_mimi_encode_workspace_bytes", "smoltts_mimi_encode", "smoltts_mimi_session_set_option",
    "smoltts_resample_design", "smoltts_resampler_bytes", "smoltts_resampler_create", "smoltts_resampler_destroy",
    "smoltts_resampler_out_bytes", "smoltts_resampler_reset_slots", "smoltts_resample_chunk",
    "smoltts_tsm_bytes", "smoltts_tsm_create", "smoltts_tsm_destroy", "smoltts_tsm_out_samples", "smoltts_tsm_reset_slots",
    "smoltts_tsm_chunk", "smoltts_tsm_slot_state",
    "smoltts_flac_bytes", "smoltts_flac_create", "smoltts_flac_destroy", "smoltts_flac_max_blocks", "smoltts_flac_out_bytes",
    "smoltts_flac_reset_slots", "smoltts_flac_chunk",
    "smoltts_seam_bytes", "smoltts_seam_create", "smoltts_seam_destroy", "smoltts_seam_out_samples", "smoltts_seam_reset_slots",
    "smoltts_seam_chunk", "smoltts_seam_slot_state",
    "smoltts_loudness_bytes", "smoltts_loudness_table_doubles", "smoltts_loudness_create", "smoltts_loudness_destroy",
    "smoltts_loudness_reset_slots", "smoltts_loudness_chunk", "smoltts_loudness_measure", "smoltts_loudness_scale",
    "smoltts_loudness_slot_state",
    "smoltts_session_set_slot_sampling", "smoltts_k_sample_rows", "smoltts_session_set_slot_filters", "smoltts_k_sample_rows_filtered",
    "smoltts_prefix_kv_bytes", "smoltts_session_save_prefix", "smoltts_session_install_prefix",
    "smoltts_k_seanet_resblock", "smoltts_k_seanet_last", "smoltts_k_rvq_upsample",
]


def exported_symbols() -> List[str]:
    return list(_EXPORTS)


def load_library(path: Optional[Path] = None):
    """dlopen the in-tree HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    override = os.environ.get("SMOLTTS_LIB")  # tools/ A/B runs: a variant built by `python -m smoltts_amd.build --variant ...`
    if path is None and override:
        print(f"[smoltts_amd] loading the library VARIANT {override} (SMOLTTS_LIB is set): not the product build", file=sys.stderr, flush=True)
    p = Path(path) if path is not None else (Path(override) if override else LIB_PATH)
    if not p.exists():
        raise SmolttsError(
            f"{p} not found: build it with `python -m smoltts_amd.build` (hipcc, gfx950). "
            "smoltts_amd has no CPU fallback.")
    lib = C.CDLL(str(p))
    lib.smoltts_last_error.restype = C.c_char_p
    lib.smoltts_session_slab_bytes.restype = C.c_size_t
    lib.smoltts_session_slab_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.smoltts_mimi_slab_bytes.restype = C.c_size_t
    lib.smoltts_mimi_slab_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.smoltts_session_slab_bytes_kv.restype = C.c_size_t
    lib.smoltts_session_slab_bytes_kv.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.smoltts_session_create_kv.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(C.c_void_p)]
    lib.smoltts_k_attention_kv.argtypes = [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_engine_create.argtypes = [C.POINTER(LMConfig), C.POINTER(LMWeights), C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.smoltts_engine_destroy.argtypes = [C.c_void_p]
    lib.smoltts_engine_destroy.restype = None
    lib.smoltts_session_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.smoltts_session_destroy.argtypes = [C.c_void_p]
    lib.smoltts_session_destroy.restype = None
    lib.smoltts_lm_prefill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.smoltts_lm_decode.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_session_outputs.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4
    lib.smoltts_mimi_create.argtypes = [C.POINTER(MimiConfig), C.POINTER(MimiWeights), C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.smoltts_mimi_destroy.argtypes = [C.c_void_p]
    lib.smoltts_mimi_destroy.restype = None
    lib.smoltts_mimi_session_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.smoltts_mimi_session_destroy.argtypes = [C.c_void_p]
    lib.smoltts_mimi_session_destroy.restype = None
    lib.smoltts_mimi_reset.argtypes = [C.c_void_p, C.c_void_p]
    lib.smoltts_mimi_decode_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    lib.smoltts_k_gemm.argtypes = [C.POINTER(GemmArgs), C.c_void_p]
    lib.smoltts_k_attention.argtypes = [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.smoltts_k_embed.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]
    lib.smoltts_k_argmax.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.smoltts_k_layernorm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    lib.smoltts_k_seanet_resblock.argtypes = [C.c_int32] * 3 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.c_void_p]
    lib.smoltts_k_seanet_last.argtypes = [C.c_int32] * 2 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_float, C.c_void_p, C.c_int64,
                                                                                                      C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_k_rvq_upsample.argtypes = [C.c_void_p, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p] * 6
    lib.smoltts_session_set_sampling.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_uint64]
    lib.smoltts_k_sample.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_float, C.c_uint64, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p]
    lib.smoltts_session_set_slot_sampling.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    lib.smoltts_k_sample_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.smoltts_session_set_slot_filters.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    lib.smoltts_k_sample_rows_filtered.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_void_p]
    lib.smoltts_session_measure_duplicate.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.smoltts_session_margin_at.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.smoltts_session_drop_graph.argtypes = [C.c_void_p]
    lib.smoltts_session_set_frames_per_graph.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_engine_fast_qkv_bytes.argtypes = [C.c_void_p]
    lib.smoltts_engine_fast_qkv_bytes.restype = C.c_size_t
    lib.smoltts_engine_build_fast_qkv.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.smoltts_session_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.smoltts_k_attention_rows3.argtypes = [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]
    lib.smoltts_k_attention_split.argtypes = [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.smoltts_mimi_reset_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_lm_prefill_deferred.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                C.c_int32, C.c_void_p]
    lib.smoltts_lm_prefill_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_void_p]
    lib.smoltts_lm_park_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_lm_prefill_side.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_lm_start_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.smoltts_mimi_encoder_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.smoltts_mimi_encoder_destroy.argtypes = [C.c_void_p]
    lib.smoltts_mimi_encoder_destroy.restype = None
    lib.smoltts_mimi_encode_frames.argtypes = [C.c_int32]
    lib.smoltts_mimi_encode_frames.restype = C.c_int32
    lib.smoltts_mimi_encode_workspace_bytes.argtypes = [C.c_void_p, C.c_int32]
    lib.smoltts_mimi_encode_workspace_bytes.restype = C.c_size_t
    lib.smoltts_mimi_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]
    if hasattr(lib, "smoltts_profile_begin"):  # diagnostic builds only (-DSMOLTTS_DEBUG_HOOKS)
        lib.smoltts_profile_begin.argtypes = [C.c_int32] * 4
        lib.smoltts_profile_end.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    lib.smoltts_mimi_session_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.smoltts_resample_design.argtypes = [C.c_int32, C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 3
    lib.smoltts_resampler_bytes.argtypes = [C.c_int32]
    lib.smoltts_resampler_bytes.restype = C.c_size_t
    lib.smoltts_resampler_out_bytes.argtypes = [C.c_int32]
    lib.smoltts_resampler_out_bytes.restype = C.c_size_t
    lib.smoltts_resampler_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_void_p)]
    lib.smoltts_resampler_destroy.argtypes = [C.c_void_p]
    lib.smoltts_resampler_destroy.restype = None
    lib.smoltts_resampler_reset_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_resample_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_void_p]
    lib.smoltts_tsm_bytes.argtypes = [C.c_int32]
    lib.smoltts_tsm_bytes.restype = C.c_size_t
    lib.smoltts_tsm_out_samples.argtypes = [C.c_int32]
    lib.smoltts_tsm_out_samples.restype = C.c_size_t
    lib.smoltts_tsm_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_void_p)]
    lib.smoltts_tsm_destroy.argtypes = [C.c_void_p]
    lib.smoltts_tsm_destroy.restype = None
    lib.smoltts_tsm_reset_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_tsm_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_void_p]
    lib.smoltts_tsm_slot_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.smoltts_seam_bytes.argtypes = [C.c_int32]
    lib.smoltts_seam_bytes.restype = C.c_size_t
    lib.smoltts_seam_out_samples.argtypes = [C.c_int32, C.c_int32]
    lib.smoltts_seam_out_samples.restype = C.c_size_t
    lib.smoltts_seam_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_void_p)]
    lib.smoltts_seam_destroy.argtypes = [C.c_void_p]
    lib.smoltts_seam_destroy.restype = None
    lib.smoltts_seam_reset_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_seam_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.smoltts_seam_slot_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.smoltts_loudness_bytes.argtypes = [C.c_int32]
    lib.smoltts_loudness_bytes.restype = C.c_size_t
    lib.smoltts_loudness_table_doubles.argtypes = []
    lib.smoltts_loudness_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.smoltts_loudness_destroy.argtypes = [C.c_void_p]
    lib.smoltts_loudness_destroy.restype = None
    lib.smoltts_loudness_reset_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_loudness_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_void_p]
    lib.smoltts_loudness_measure.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.smoltts_loudness_scale.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]
    lib.smoltts_loudness_slot_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.smoltts_flac_bytes.argtypes = [C.c_int32]
    lib.smoltts_flac_bytes.restype = C.c_size_t
    lib.smoltts_flac_max_blocks.argtypes = [C.c_int32]
    lib.smoltts_flac_max_blocks.restype = C.c_int32
    lib.smoltts_flac_out_bytes.argtypes = [C.c_int32]
    lib.smoltts_flac_out_bytes.restype = C.c_size_t
    lib.smoltts_flac_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_void_p)]
    lib.smoltts_flac_destroy.argtypes = [C.c_void_p]
    lib.smoltts_flac_destroy.restype = None
    lib.smoltts_flac_reset_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_flac_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    lib.smoltts_prefix_kv_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.smoltts_prefix_kv_bytes.restype = C.c_size_t
    lib.smoltts_session_save_prefix.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(PrefixHeader), C.c_void_p]
    lib.smoltts_session_install_prefix.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(PrefixHeader), C.POINTER(C.c_int32),
                                                   C.c_int32, C.c_void_p]
    if lib.smoltts_abi_version() != 6:
        raise SmolttsError("libsmoltts_hip.so ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load_library().smoltts_last_error().decode(errors="replace")
        raise SmolttsError(f"{what} failed ({status}): {msg}")


def _require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise SmolttsError("no HIP device visible; smoltts_amd runs on MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


_UPLOAD_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def upload_stream(device: torch.device) -> "torch.cuda.Stream":
    """The side stream of ``upload`` for this device, created (and the pinned allocator warmed) on first use; engines call
    this when they are built so that no request pays for it."""
    up = _UPLOAD_STREAMS.get(device.index)
    if up is None:
        up = _UPLOAD_STREAMS[device.index] = torch.cuda.Stream(device)
        # torch caches pinned blocks per power-of-two size class, and the first block of a class costs a hipHostMalloc (ms):
        # take a few of every class up to 1 MiB now
        warm = [[torch.empty(1 << k, dtype=torch.uint8).pin_memory() for _ in range(4)] for k in range(8, 21)]
        # ... and put one copy and one event through the stream: its hardware queue is only created by the first submission
        with torch.cuda.stream(up):
            warm[0][0].to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(up)
        torch.cuda.current_stream(device).wait_event(ev)
        up.synchronize()
        del warm
    return up


def upload(arrays: Sequence[np.ndarray], device: torch.device) -> List[torch.Tensor]:
    """Host arrays -> device tensors usable on the current stream, without waiting for the work already queued on it.
    A plain ``tensor.to(device)`` from pageable memory is stream-ordered *and* blocks the host, i.e. it waits for everything
    the stream still has to do (a serving loop has a tick of frame graphs pending there); here the copies leave pinned memory on
    a side stream that is otherwise idle, and the current stream merely waits for their event."""
    cur = torch.cuda.current_stream(device)
    up = upload_stream(device)
    outs = []
    with torch.cuda.stream(up):
        for a in arrays:
            t = torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)
            t.record_stream(cur)  # allocated under the side stream, consumed on the current one
            outs.append(t)
        ev = torch.cuda.Event()
        ev.record(up)
    cur.wait_event(ev)
    return outs


def current_stream_ptr() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def dptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


def _alloc_slab(nbytes: int, device, settle: bool = False) -> torch.Tensor:
    """A zeroed, 256-byte aligned slab.  The zero fill is queued on the current stream.  ``settle``: wait for it here -- for a slab
    that a C create call then initialises with plain hipMemcpy / hipMemset / a null-stream kernel, which are not ordered against
    a non-blocking current stream (a serving thread's frame stream with ticks queued) and would otherwise be overwritten by a
    late zero fill."""
    slab = torch.zeros(nbytes + 256, dtype=torch.uint8, device=device)
    if settle:
        torch.cuda.current_stream(device).synchronize()
    shift = (-slab.data_ptr()) % 256
    return slab[shift: shift + nbytes]


# ------------------------------------------------------------------------------- LM engine
def lm_config_struct(cfg: RQTransformerModelArgs, tok: TokenConfig, numerics: NumericsMode, weight_format: int = 0) -> LMConfig:
    c = LMConfig()
    c.dim, c.n_layer, c.n_head, c.n_kv_head, c.inter = cfg.dim, cfg.n_layer, cfg.n_head, cfg.n_local_heads, cfg.intermediate_size
    c.fast_dim, c.n_fast_layer, c.fast_n_head = cfg.fast_dim, cfg.n_fast_layer, cfg.fast_n_head
    c.fast_n_kv_head, c.fast_inter = cfg.fast_n_local_heads, cfg.fast_intermediate_size
    c.vocab_size, c.codebook_size, c.num_codebooks = cfg.vocab_size, cfg.codebook_size, cfg.num_codebooks
    c.n_fast = cfg.max_fast_seqlen
    c.duplicate_code_0 = int(bool(cfg.duplicate_code_0))
    c.depthwise_wte = int(bool(cfg.depthwise_wte))
    c.has_fast_project_in = int(cfg.fast_dim != cfg.dim)
    c.embed_mask_mode = 0 if numerics.embed_mask == "torch" else 1
    c.semantic_start_id = tok.semantic_start_id
    c.semantic_end_id = tok.semantic_end_id if tok.semantic_end_id is not None else tok.semantic_start_id
    c.im_end_id = tok.im_end_id
    c.max_seq_len = cfg.max_seq_len
    c.norm_eps = cfg.norm_eps
    c.weight_format = int(weight_format)
    return c


def _fill_block(dst: BlockWeights, src: Dict[str, int]) -> None:
    for k, v in src.items():
        setattr(dst, k, v)


OPT_QKV_TABLE, OPT_COMMIT_PICKS, OPT_SPLIT_ATTN, OPT_STREAM_W, OPT_FUSE_DEPTH_ATTN, OPT_FUSE_PICK, OPT_FP8_PREFILL = 1, 2, 3, 4, 5, 6, 7  # include/smoltts_hip.h SMOLTTS_OPT_*


class LMEngine:
    """Immutable model on one GPU: packed weight arena + ``SmolttsEngine`` handle."""

    def __init__(self, cfg: RQTransformerModelArgs, state: Dict[str, torch.Tensor], token_config: TokenConfig,
                 numerics: Optional[NumericsMode] = None, arena: Optional[torch.Tensor] = None, offsets=None,
                 weight_format: str = "bf16", fast_qkv_table: Optional[bool] = None):
        """``weight_format="fp8"``: the Linears are stored as e4m3 with per-row scales (half the weight bytes);
        the model computed is exactly ``packing.fp8_reference_state`` of the checkpoint.
        ``fast_qkv_table`` (default on; ``SMOLTTS_QKV_TABLE=0`` switches the default off): build the engine's derived table of
        depth layer-0 q | k | v per fast-embedding row (``smoltts_engine_build_fast_qkv``: 7 launches fewer per frame)."""
        cfg.validate_for_engine()
        self.lib = load_library()
        self.device = _require_gpu()
        upload_stream(self.device)
        self.cfg, self.token_config = cfg, token_config
        self.numerics = numerics or NumericsMode.torch_reference()
        if arena is None:
            arena, offsets = packing.pack_lm(cfg, state, self.numerics, weight_format)
        self.offsets = offsets
        self.weight_format = "fp8" if offsets.get("weight_format", 0) else "bf16"
        self.arena = arena.to(self.device) if arena.device != self.device else arena
        self.c_cfg = lm_config_struct(cfg, token_config, self.numerics, offsets.get("weight_format", 0))
        w = LMWeights()
        for k in ("text_emb", "codebook_emb", "fast_emb", "norm", "head", "fast_norm", "fast_head",
                  "fast_head_step_stride", "fast_proj_w", "fast_proj_b", "rope", "fast_rope"):
            setattr(w, k, offsets[k])
        for i, b in enumerate(offsets["layers"]):
            _fill_block(w.layers[i], b)
        for i, b in enumerate(offsets["fast_layers"]):
            _fill_block(w.fast_layers[i], b)
        self.c_w = w
        h = C.c_void_p()
        check(self.lib.smoltts_engine_create(C.byref(self.c_cfg), C.byref(w), dptr(self.arena), self.arena.numel(), C.byref(h)),
              "smoltts_engine_create")
        self.handle = h
        if fast_qkv_table is None:
            fast_qkv_table = os.environ.get("SMOLTTS_QKV_TABLE", "1") != "0"
        self.fast_qkv = None
        need = self.lib.smoltts_engine_fast_qkv_bytes(self.handle) if fast_qkv_table else 0
        if need:
            self.fast_qkv = _alloc_slab(need, self.device)
            check(self.lib.smoltts_engine_build_fast_qkv(self.handle, dptr(self.fast_qkv), need, current_stream_ptr()),
                  "smoltts_engine_build_fast_qkv")

    @property
    def grid_height(self) -> int:
        return 1 + self.cfg.max_fast_seqlen

    def weight_bytes(self) -> int:
        return int(self.arena.numel())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.smoltts_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LMSession:
    """B utterance slots (KV caches + device-side frame loop state) inside one device slab."""

    def __init__(self, engine: LMEngine, max_batch: int, max_seq: Optional[int] = None, max_rows: int = 4096,
                 max_frames: int = 1025, kv_dtype: str = "fp32"):
        """``kv_dtype="bf16"``: the slow transformer's KV cache holds K (after RoPE) and V rounded to bf16 (half the
        attention stream; the oracle's ``kv_bf16=True`` is the same arithmetic).  Default fp32: K/V exactly as computed."""
        if kv_dtype not in KV_FORMATS:
            raise ValueError(f"kv_dtype must be one of {sorted(KV_FORMATS)}, got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        kvf = KV_FORMATS[kv_dtype]
        self.engine, self.lib = engine, engine.lib
        self.B = max_batch
        self.filtered_slots = set()  # slots whose filter entry on the device is on (set_slot_filters)
        self.max_seq = max_seq or engine.cfg.max_seq_len
        self.max_rows = max(max_rows, max_batch)
        self.max_frames = max_frames
        self.H = engine.grid_height
        need = self.lib.smoltts_session_slab_bytes_kv(engine.handle, self.B, self.max_seq, self.max_rows, self.max_frames, kvf)
        if need == 0:
            raise SmolttsError("smoltts_session_slab_bytes returned 0 (bad sizes)")
        self.slab = _alloc_slab(need, engine.device, settle=True)
        h = C.c_void_p()
        check(self.lib.smoltts_session_create_kv(engine.handle, dptr(self.slab), need, self.B, self.max_seq, self.max_rows,
                                                 self.max_frames, kvf, C.byref(h)), "smoltts_session_create")
        self.handle = h
        ptrs = [C.c_void_p() for _ in range(4)]
        check(self.lib.smoltts_session_outputs(h, *[C.byref(p) for p in ptrs]), "smoltts_session_outputs")
        base = self.slab.data_ptr()

        def view(p, nbytes, dtype, shape):
            o = p.value - base
            return self.slab[o: o + nbytes].view(dtype).view(*shape)

        self.codes = view(ptrs[0], self.B * self.max_frames * self.H * 4, torch.int32, (self.B, self.max_frames, self.H))
        self.n_frames = view(ptrs[1], self.B * 4, torch.int32, (self.B,))
        self.done = view(ptrs[2], self.B * 4, torch.int32, (self.B,))
        self.margin = view(ptrs[3], self.B * 4, torch.float32, (self.B,))
        mp = C.c_void_p()
        check(self.lib.smoltts_session_margin_at(h, C.byref(mp)), "smoltts_session_margin_at")
        self.margin_at = view(mp, self.B * 4, torch.int32, (self.B,))  # frame * 64 + step of each slot's smallest gap
        self._keep = None
        self._keep_prefixes = None
        if os.environ.get("SMOLTTS_COMMIT_PICKS") == "0":  # A/B switches of tools/ (the ids are the same either way)
            self.use_commit_picks(False)
        if os.environ.get("SMOLTTS_SPLIT_ATTN") == "0":
            self.use_split_attention(False)
        if os.environ.get("SMOLTTS_FUSE_DEPTH_ATTN") == "0":
            self.use_fused_depth_attention(False)
        if os.environ.get("SMOLTTS_FUSE_PICK") == "0":
            self.use_fused_pick(False)
        if os.environ.get("SMOLTTS_FP8_PREFILL") == "1":  # (bench.py --fp8-prefill: not the parity path)
            self.use_fp8_prefill(True)
        if os.environ.get("SMOLTTS_STREAM_W") is not None:  # mask of SMOLTTS_STREAM_W_* bits
            check(self.lib.smoltts_session_set_option(self.handle, OPT_STREAM_W, int(os.environ["SMOLTTS_STREAM_W"])), "smoltts_session_set_option")

    def _rows(self, prompts, slots, pos0):
        """Prompt grids -> (grid rows, row slots, row positions on the device, last row per utterance, row count)."""
        cfg = self.engine.cfg
        cols, rslot, rpos, last = [], [], [], []
        n = 0
        for g, sl, p0 in zip(prompts, slots, pos0):
            g = np.asarray(g)
            if g.ndim != 2 or g.shape[0] != self.H or g.shape[1] < 1:
                raise ValueError(f"prompt grid must be ({self.H}, T>=1), got {g.shape}")
            T = g.shape[1]
            if p0 + T + 1 > self.max_seq:
                raise SmolttsError(f"prompt of {p0 + T} tokens does not fit max_seq={self.max_seq}")
            if g[0].min() < 0 or g[0].max() >= cfg.vocab_size or g[1:].min() < 0 or g[1:].max() >= cfg.codebook_size:
                raise ValueError("prompt ids out of range")
            cols.append(np.ascontiguousarray(g.T.astype(np.int32)))
            rslot.append(np.full(T, sl, np.int32))
            rpos.append(np.arange(p0, p0 + T, dtype=np.int32))
            n += T
            last.append(n - 1)
        if n > self.max_rows:
            raise SmolttsError(f"{n} prompt rows exceed the session's max_rows={self.max_rows}")
        grid_d, rslot_d, rpos_d = upload([np.concatenate(cols), np.concatenate(rslot), np.concatenate(rpos)], self.engine.device)
        return grid_d, rslot_d, rpos_d, last, n

    # ---- prompt prefill beside the decode frames (include/smoltts_hip.h at smoltts_lm_park_slots): three steps, the first and the
    #      last on the stream the frames run on, the middle one on any other stream once the first has run
    def side_park(self, prompts: Sequence[np.ndarray], slots: Sequence[int], pos0: Optional[Sequence[int]] = None,
                  prefixes: Optional[Sequence[Optional["PrefixKV"]]] = None):
        """Freeze the (idle) ``slots`` at their new prompts' last positions and upload the prompt rows; -> a handle for the two
        steps that follow.  Call on the frame stream.  ``pos0[b]``: position of the first column of ``prompts[b]`` (default 0;
        the slot parks at ``pos0 + T - 1``).  ``prefixes[b]`` (a ``PrefixKV`` or None): installed into the slot first, in one
        launch for all of them; ``pos0`` then defaults to its ``P``."""
        slots = list(slots)
        if len(slots) != len(prompts) or len(set(slots)) != len(slots):
            raise ValueError("slots must be distinct and match prompts")
        pos0 = self._prefix_pos0(prompts, prefixes, pos0)
        grid_d, rslot_d, rpos_d, last, n = self._rows(prompts, slots, pos0)
        if prefixes is not None and any(p is not None for p in prefixes):
            self.install_prefix([p for p in prefixes if p is not None], [b for b, p in zip(slots, prefixes) if p is not None])
        slots_h = (C.c_int32 * len(slots))(*slots)
        park_h = (C.c_int32 * len(slots))(*[p0 + int(np.asarray(g).shape[1]) - 1 for g, p0 in zip(prompts, pos0)])
        check(self.lib.smoltts_lm_park_slots(self.handle, slots_h, park_h, len(slots), current_stream_ptr()), "smoltts_lm_park_slots")
        parked = torch.cuda.Event()
        parked.record(torch.cuda.current_stream())
        return {"rows": (grid_d, rslot_d, rpos_d), "n": n, "slots": slots, "last": last, "parked": parked, "done": None}

    def side_run(self, h) -> None:
        """The prompts' KV rows, on the CURRENT stream (not the frames' one); the park must have run: the host waits for it here."""
        h["parked"].synchronize()
        grid_d, rslot_d, rpos_d = h["rows"]
        check(self.lib.smoltts_lm_prefill_side(self.handle, dptr(grid_d), dptr(rslot_d), dptr(rpos_d), h["n"], current_stream_ptr()),
              "smoltts_lm_prefill_side")
        h["done"] = torch.cuda.Event()
        h["done"].record(torch.cuda.current_stream())

    def side_start(self, h, stop_on_eos: bool = True) -> None:
        """Arm the slots (their frame 0 comes out of the next decode frame).  Call on the frame stream; waits (host) for the side call."""
        h["done"].synchronize()
        grid_d, _, rpos_d = h["rows"]
        slots_h = (C.c_int32 * len(h["slots"]))(*h["slots"])
        last_h = (C.c_int32 * len(h["slots"]))(*h["last"])
        check(self.lib.smoltts_lm_start_slots(self.handle, dptr(grid_d), dptr(rpos_d), slots_h, last_h, len(h["slots"]), int(stop_on_eos),
                                              current_stream_ptr()), "smoltts_lm_start_slots")
        self._keep = h["rows"]  # alive until the stream has consumed them

    def prefill(self, prompts: Sequence[np.ndarray], slots: Optional[Sequence[int]] = None, stop_on_eos: bool = True,
                pos0: Optional[Sequence[int]] = None, final: bool = True, defer_frame0: bool = False) -> None:
        """prompts: one ``(1 + n_fast, T_b)`` int grid per utterance; emits frame 0 of each slot.

        Chunked prefill: ``pos0[b]`` is the position of the first column of ``prompts[b]`` (its earlier columns
        went through previous calls with ``final=False``, which fill the KV cache only and leave the slot idle).
        ``defer_frame0``: no frame-0 tail here; the next ``decode`` call emits frame 0 as its first frame (serving loop)."""
        slots = list(range(len(prompts))) if slots is None else list(slots)
        if len(slots) != len(prompts) or len(set(slots)) != len(slots):
            raise ValueError("slots must be distinct and match prompts")
        pos0 = [0] * len(prompts) if pos0 is None else list(pos0)
        grid_d, rslot_d, rpos_d, last, n = self._rows(prompts, slots, pos0)
        slots_h = (C.c_int32 * len(slots))(*slots)
        last_h = (C.c_int32 * len(slots))(*last)
        self._keep = (grid_d, rslot_d, rpos_d)  # alive until the stream has consumed them
        if final and defer_frame0:
            check(self.lib.smoltts_lm_prefill_deferred(self.handle, dptr(grid_d), dptr(rslot_d), dptr(rpos_d), n, slots_h, last_h,
                                                       len(slots), int(stop_on_eos), current_stream_ptr()), "smoltts_lm_prefill_deferred")
        elif final:
            check(self.lib.smoltts_lm_prefill(self.handle, dptr(grid_d), dptr(rslot_d), dptr(rpos_d), n, slots_h, last_h,
                                              len(slots), int(stop_on_eos), current_stream_ptr()), "smoltts_lm_prefill")
        else:
            check(self.lib.smoltts_lm_prefill_chunk(self.handle, dptr(grid_d), dptr(rslot_d), dptr(rpos_d), n, slots_h, last_h,
                                                    len(slots), current_stream_ptr()), "smoltts_lm_prefill_chunk")

    def prefill_chunked(self, prompts: Sequence[np.ndarray], slots: Optional[Sequence[int]] = None, stop_on_eos: bool = True,
                        chunk: int = 128, between=None, defer_frame0: bool = False, pos0: Optional[Sequence[int]] = None,
                        prefixes: Optional[Sequence[Optional["PrefixKV"]]] = None) -> None:
        """The same result as ``prefill`` with at most ``chunk`` columns per utterance per call; ``between()`` runs
        after every partial call (e.g. a few decode frames for the slots that are already speaking).  ``pos0[b]``: position
        of the first column of ``prompts[b]`` (default 0).  ``prefixes[b]`` (a ``PrefixKV`` or None): installed into the slot
        first, in one launch for all of them; ``pos0`` then defaults to its ``P``."""
        slots = list(range(len(prompts))) if slots is None else list(slots)
        prompts = [np.asarray(g) for g in prompts]
        start = self._prefix_pos0(prompts, prefixes, pos0)
        if prefixes is not None and any(p is not None for p in prefixes):
            have = [i for i, p in enumerate(prefixes) if p is not None]
            self.install_prefix([prefixes[i] for i in have], [slots[i] for i in have])
            if between is not None and any(g.shape[1] > chunk for g in prompts):
                # a tick may run before these slots' first prefill call: park them behind their prompts, where an idle slot's
                # decode rows may scribble without harm (the installed rows stay as they are)
                slots_h = (C.c_int32 * len(have))(*[slots[i] for i in have])
                park_h = (C.c_int32 * len(have))(*[start[i] + int(prompts[i].shape[1]) - 1 for i in have])
                check(self.lib.smoltts_lm_park_slots(self.handle, slots_h, park_h, len(have), current_stream_ptr()), "smoltts_lm_park_slots")
        done = [0] * len(prompts)
        while True:
            part = [i for i, g in enumerate(prompts) if g.shape[1] - done[i] > chunk]
            if not part:
                break
            self.prefill([prompts[i][:, done[i]: done[i] + chunk] for i in part], [slots[i] for i in part], stop_on_eos,
                         pos0=[start[i] + done[i] for i in part], final=False)
            for i in part:
                done[i] += chunk
            if between is not None:
                between()
        self.prefill([g[:, d:] for g, d in zip(prompts, done)], slots, stop_on_eos, pos0=[p + d for p, d in zip(start, done)], final=True,
                     defer_frame0=defer_frame0)

    # ---- voice prefixes (include/smoltts_hip.h at smoltts_session_save_prefix)
    @staticmethod
    def _prefix_pos0(prompts, prefixes, pos0) -> List[int]:
        if prefixes is not None and len(prefixes) != len(prompts):
            raise ValueError("one prefix (or None) per prompt")
        if pos0 is not None:
            pos0 = [int(p) for p in pos0]
            if len(pos0) != len(prompts):
                raise ValueError("one pos0 per prompt")
            if prefixes is not None and any(p is not None and p0 != p.n_positions for p, p0 in zip(prefixes, pos0)):
                raise ValueError("pos0 of a prompt behind a prefix must be the prefix's length")
            return pos0
        return [0 if prefixes is None or p is None else p.n_positions for p in (prefixes or [None] * len(prompts))]

    def save_prefix(self, slot: int, n_positions: int) -> "PrefixKV":
        """Rows [0, n_positions) of ``slot``'s slow KV cache (as the current stream has written them by then) -> a ``PrefixKV``
        that any session on this engine with the same kv dtype can install."""
        pk = PrefixKV(self.engine, int(n_positions), self.kv_dtype)
        hdr = PrefixHeader()
        check(self.lib.smoltts_session_save_prefix(self.handle, int(slot), int(n_positions), dptr(pk.slab), C.byref(hdr),
                                                   current_stream_ptr()), "smoltts_session_save_prefix")
        pk.header = hdr
        return pk

    def install_prefix(self, prefixes: Sequence["PrefixKV"], slots: Sequence[int]) -> None:
        """Copy ``prefixes[i]`` into rows [0, P_i) of slot ``slots[i]`` on the current stream (one launch per 16 prefixes; nothing
        else of the session changes).  The prompt rows that follow must go in at pos0 = P_i before the slots decode again."""
        slots = [int(b) for b in slots]
        n = len(slots)
        if n != len(prefixes) or n == 0:
            raise ValueError("one slot per prefix, at least one")
        for p in prefixes:
            if p.header is None:
                raise ValueError("prefix has not been saved")
        ptrs = (C.c_void_p * n)(*[dptr(p.slab) for p in prefixes])
        hdrs = (PrefixHeader * n)(*[p.header for p in prefixes])
        check(self.lib.smoltts_session_install_prefix(self.handle, ptrs, hdrs, (C.c_int32 * n)(*slots), n, current_stream_ptr()),
              "smoltts_session_install_prefix")
        self._keep_prefixes = list(prefixes)  # alive until the stream has consumed them (freed slabs go back to torch's cache)

    def set_sampling(self, temp: float = 0.0, fast_temp: float = 0.0, min_p: float = 0.0, seed: int = 0) -> None:
        """temp / fast_temp <= 0: greedy (default). Takes effect from the next frame."""
        check(self.lib.smoltts_session_set_sampling(self.handle, float(temp), float(fast_temp), float(min_p), int(seed) & (2**64 - 1)),
              "smoltts_session_set_sampling")

    def set_slot_sampling(self, slots: Sequence[int], temp: Sequence[float], fast_temp: Sequence[float], min_p: Sequence[float],
                          seed: Sequence[int]) -> None:
        """Per-slot sampling (slot mode, include/smoltts_hip.h): slot ``slots[i]`` samples its slow token at ``temp[i]`` and its
        depth codes at ``fast_temp[i]`` (<= 0: greedy) with the effective cut ``min_p[i]`` and the request key of ``seed[i]``.  The
        first call puts the session in slot mode for good (unlisted slots: greedy).  Queued on the current stream: the picks
        behind it on that stream use the new entries; the host does not wait for the stream."""
        n = len(slots)
        if not (len(temp) == len(fast_temp) == len(min_p) == len(seed) == n):
            raise ValueError("slot sampling: one value per slot in every list")
        check(self.lib.smoltts_session_set_slot_sampling(
            self.handle, (C.c_int32 * max(n, 1))(*[int(b) for b in slots]), n, (C.c_float * max(n, 1))(*[float(t) for t in temp]),
            (C.c_float * max(n, 1))(*[float(t) for t in fast_temp]), (C.c_float * max(n, 1))(*[float(p) for p in min_p]),
            (C.c_uint64 * max(n, 1))(*[int(x) & (2**64 - 1) for x in seed]), current_stream_ptr()), "smoltts_session_set_slot_sampling")

    def set_slot_filters(self, slots: Sequence[int], top_p: Sequence[float], top_k: Sequence[int], penalty: Sequence[float],
                         window: Sequence[int]) -> None:
        """Per-slot filters of the sampled picks (``smoltts_session_set_slot_filters``): slot ``slots[i]`` keeps its ``top_k[i]``
        largest logits (0: off), then the ``top_p[i]`` nucleus (0 or 1: off), after the repetition penalty ``penalty[i]`` (0 or
        1: off) over the ids of its last ``window[i]`` frames.  Queued on the current stream like ``set_slot_sampling``."""
        n = len(slots)
        if not (len(top_p) == len(top_k) == len(penalty) == len(window) == n):
            raise ValueError("slot filters: one value per slot in every list")
        check(self.lib.smoltts_session_set_slot_filters(
            self.handle, (C.c_int32 * max(n, 1))(*[int(b) for b in slots]), n, (C.c_float * max(n, 1))(*[float(p) for p in top_p]),
            (C.c_int32 * max(n, 1))(*[int(k) for k in top_k]), (C.c_float * max(n, 1))(*[float(r) for r in penalty]),
            (C.c_int32 * max(n, 1))(*[int(w) for w in window]), current_stream_ptr()), "smoltts_session_set_slot_filters")
        for b, p, k, r, w in zip(slots, top_p, top_k, penalty, window):
            (self.filtered_slots.add if (0 < p < 1 or k > 0 or (r > 1 and w > 0)) else self.filtered_slots.discard)(int(b))

    def measure_duplicate(self, code: int = -1, n_filter: int = 0) -> None:
        """Measurement aid (this session only): issue every launch of one kernel class twice; -1 switches it off."""
        check(self.lib.smoltts_session_measure_duplicate(self.handle, int(code), int(n_filter)), "smoltts_session_measure_duplicate")

    def decode(self, n_frames: int) -> None:
        check(self.lib.smoltts_lm_decode(self.handle, int(n_frames), current_stream_ptr()), "smoltts_lm_decode")

    def use_qkv_table(self, on: bool) -> None:
        """Depth layer-0 q | k | v from the engine's table (default where it exists) or through the wqkv GEMM (A/B, tests)."""
        check(self.lib.smoltts_session_set_option(self.handle, OPT_QKV_TABLE, 1 if on else 0), "smoltts_session_set_option")

    def use_split_attention(self, on: bool) -> None:
        """Slow attention of few rows with the keys of a (row, kv head) pair on two workgroups (default) or on one."""
        check(self.lib.smoltts_session_set_option(self.handle, OPT_SPLIT_ATTN, 1 if on else 0), "smoltts_session_set_option")

    def use_fused_depth_attention(self, on: bool) -> None:
        """Depth steps 1..: attention over the <= 8-entry cache inside the wo launch (default) or as a launch of its own."""
        check(self.lib.smoltts_session_set_option(self.handle, OPT_FUSE_DEPTH_ATTN, 1 if on else 0), "smoltts_session_set_option")

    def kv_cache(self):
        """(K, V) views of the slow transformer's cache: [n_layer, max_batch, n_kv_head, max_seq, 64] in the session's kv dtype (diagnostics)."""
        k, v, lb = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(self.lib.smoltts_session_kv_cache(self.handle, C.byref(k), C.byref(v), C.byref(lb)), "smoltts_session_kv_cache")
        cfg = self.engine.cfg
        n_layer, kvh = cfg.n_layer, cfg.n_local_heads
        dt = torch.float32 if lb.value == self.B * kvh * self.max_seq * 64 * 4 else torch.bfloat16
        base = self.slab.data_ptr()
        out = []
        for p in (k, v):
            o = p.value - base
            out.append(self.slab[o: o + n_layer * lb.value].view(dt).view(n_layer, self.B, kvh, self.max_seq, 64))
        return out

    def use_fp8_prefill(self, on: bool) -> None:
        """fp8-weight engines: prompt prefills of >= 256 rows on the fp8 x fp8 MFMA (BASELINE configs[4]'s fp8 MFMA prefill).  Faster
        first chunk; the prompt's KV rows carry the activations' fp8 rounding, so ids may leave the reference greedy decode."""
        check(self.lib.smoltts_session_set_option(self.handle, OPT_FP8_PREFILL, 1 if on else 0), "smoltts_session_set_option")

    def use_fused_pick(self, on: bool) -> None:
        """Greedy depth codes picked inside the next step's layer-0 attention + wo launch (default) or by a launch of their own."""
        check(self.lib.smoltts_session_set_option(self.handle, OPT_FUSE_PICK, 1 if on else 0), "smoltts_session_set_option")

    def use_commit_picks(self, on: bool) -> None:
        """The frame's slow token and last depth code picked inside the commit kernel (default) or in launches of their own."""
        check(self.lib.smoltts_session_set_option(self.handle, OPT_COMMIT_PICKS, 1 if on else 0), "smoltts_session_set_option")

    def set_frames_per_graph(self, n: int) -> None:
        """Frames per multi-frame graph (1 = single-frame graphs, 0 = follow the decode calls).  After a prefill and with
        n > 0 the graphs are captured now, on the current stream, instead of inside the first decode call."""
        check(self.lib.smoltts_session_set_frames_per_graph(self.handle, int(n), current_stream_ptr()), "smoltts_session_set_frames_per_graph")

    def fetch(self):
        """Synchronise and return (codes [B, max_frames, H] int32, n_frames [B], done [B], margin [B]) on the host."""
        torch.cuda.current_stream().synchronize()
        return (self.codes.cpu().numpy(), self.n_frames.cpu().numpy(), self.done.cpu().numpy(), self.margin.cpu().numpy())

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize()
            self.lib.smoltts_session_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PrefixKV:
    """The slow KV rows of positions [0, P) of one prompt prefix (a cloned voice's speaker turns), in a slab of its own
    (``LMSession.save_prefix``): any session on the same engine with the same kv dtype installs it into a slot in one copy
    (``LMSession.install_prefix``).  The slab is released with the object."""

    def __init__(self, engine: LMEngine, n_positions: int, kv_dtype: str = "fp32"):
        if kv_dtype not in KV_FORMATS:
            raise ValueError(f"kv_dtype must be one of {sorted(KV_FORMATS)}, got {kv_dtype!r}")
        self.engine, self.n_positions, self.kv_dtype = engine, int(n_positions), kv_dtype
        nbytes = engine.lib.smoltts_prefix_kv_bytes(engine.handle, self.n_positions, KV_FORMATS[kv_dtype])
        if nbytes == 0:
            raise SmolttsError(f"smoltts_prefix_kv_bytes returned 0 (P={n_positions})")
        self.slab = _alloc_slab(nbytes, engine.device)
        self.header: Optional[PrefixHeader] = None  # set by the save (the host copy of the slab's header)

    @property
    def nbytes(self) -> int:
        return int(self.slab.numel())

    def close(self):
        self.slab = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------- Mimi engine
class MimiEngine:
    def __init__(self, state: Optional[Dict[str, torch.Tensor]], num_codebooks: int = 8, window: int = 0,
                 max_positions: int = 4096, arena: Optional[torch.Tensor] = None, offsets=None):
        self.lib = load_library()
        self.device = _require_gpu()
        if arena is None:
            arena, offsets = packing.pack_mimi(state, num_codebooks, max_positions)
        off = offsets
        max_positions = off["max_positions"]
        self.arena = arena.to(self.device)
        self.num_codebooks = num_codebooks
        cfg = MimiConfig(num_codebooks, off["n_layers"], window, max_positions)
        w = MimiWeights()
        w.rvq_table, w.upsample_w, w.rope = off["rvq_table"], off["upsample_w"], off["rope"]
        w.final_w = off["final_w"]
        for i, l in enumerate(off["layers"]):
            for k, v in l.items():
                setattr(w.layers[i], k, v)
        for i, cv in enumerate(off["convs"]):
            for k, v in cv.items():
                setattr(w.convs[i], k, v)
        self.c_cfg, self.c_w = cfg, w
        h = C.c_void_p()
        check(self.lib.smoltts_mimi_create(C.byref(cfg), C.byref(w), dptr(self.arena), self.arena.numel(), C.byref(h)),
              "smoltts_mimi_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.smoltts_mimi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MimiEncoder:
    """PCM -> RVQ codes (``MimiModel.encode``, codec/mimi.py:64-71) for voice-clone prompts.

    ``extra_right=False`` pads like the reference's MLX convs (everything on the left), ``True`` like
    ``transformers.MimiConv1d``; they agree for signals of whole frames (multiples of 1920 samples)."""

    def __init__(self, state: Optional[Dict[str, torch.Tensor]], num_codebooks: int = 8, window: int = 0, max_positions: int = 2048,
                 extra_right: bool = False, arena: Optional[torch.Tensor] = None, offsets=None):
        self.lib = load_library()
        self.device = _require_gpu()
        if arena is None:
            arena, offsets = packing.pack_mimi_encoder(state, num_codebooks, max_positions)
        off = offsets
        self.arena = arena.to(self.device)
        self.num_codebooks = off["num_codebooks"]
        cfg = MimiEncConfig(self.num_codebooks, off["n_layers"], window, off["max_positions"], int(extra_right))
        w = MimiEncWeights()
        for k in ("conv0_w", "conv0_b", "rope", "downsample_w", "codebooks_t", "codebooks", "codebook_sq"):
            setattr(w, k, off[k])
        w.in_proj[0], w.in_proj[1] = off["in_proj"]
        for i, l in enumerate(off["layers"]):
            for k, v in l.items():
                setattr(w.layers[i], k, v)
        for i, cv in enumerate(off["convs"]):
            for k, v in cv.items():
                setattr(w.convs[i], k, v)
        self.c_cfg, self.c_w = cfg, w
        h = C.c_void_p()
        check(self.lib.smoltts_mimi_encoder_create(C.byref(cfg), C.byref(w), dptr(self.arena), self.arena.numel(), C.byref(h)),
              "smoltts_mimi_encoder_create")
        self.handle = h
        self._ws = None

    def frames(self, n_samples: int) -> int:
        return int(self.lib.smoltts_mimi_encode_frames(n_samples))

    def encode(self, pcm, return_aux: bool = False):
        """pcm: 1-D float array/tensor of 24 kHz samples -> int32 device tensor (num_codebooks, frames)
        [, latents (frames, 512), squared-distance gaps (num_codebooks, frames)]."""
        x = torch.as_tensor(pcm, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        n = x.numel()
        if n == 0:
            raise SmolttsError("encode: empty signal")
        need = self.lib.smoltts_mimi_encode_workspace_bytes(self.handle, n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = _alloc_slab(need, self.device)
        F = self.frames(n)
        codes = torch.empty(self.num_codebooks, F, dtype=torch.int32, device=self.device)
        emb = torch.empty(F, 512, dtype=torch.float32, device=self.device) if return_aux else None
        gap = torch.empty(self.num_codebooks, F, dtype=torch.float32, device=self.device) if return_aux else None
        check(self.lib.smoltts_mimi_encode(self.handle, dptr(x), n, dptr(codes), dptr(emb) if return_aux else None,
                                           dptr(gap) if return_aux else None, dptr(self._ws), self._ws.numel(), current_stream_ptr()),
              "smoltts_mimi_encode")
        return (codes, emb, gap) if return_aux else codes

    def close(self):
        if getattr(self, "handle", None):
            self.lib.smoltts_mimi_encoder_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MimiSession:
    """Streaming Mimi decode state for ``max_batch`` slots; ``decode`` consumes frames chunk-wise."""

    SAMPLES_PER_FRAME = 1920
    OPT_STATELESS_UPSAMPLE = 1  # SMOLTTS_MIMI_OPT_STATELESS_UPSAMPLE
    OPT_PRODUCTS = 2  # SMOLTTS_MIMI_OPT_PRODUCTS

    def __init__(self, engine: MimiEngine, max_batch: int, max_chunk_frames: int = 8, stateless_upsample: bool = False,
                 products: int = 6):
        """``products`` = 3: the matrix-core kernels form three of the six bf16x3 products per operand pair (23 % faster chunks at a
        PCM RMS error of 7e-7 instead of 1e-7 against the fp32 oracle: include/smoltts_hip.h, SMOLTTS_MIMI_OPT_PRODUCTS).
        ``stateless_upsample``: every decode call up-samples its frames with no tap overlap carried in from the call before --
        the reference's ``decode_step`` (codec/mimi.py:73-77,101-104); off, chunked decode == batch decode."""
        self.engine, self.lib = engine, engine.lib
        self.B, self.chunk = max_batch, max_chunk_frames
        need = self.lib.smoltts_mimi_slab_bytes(engine.handle, max_batch, max_chunk_frames)
        if need == 0:
            raise SmolttsError("smoltts_mimi_slab_bytes returned 0 (bad sizes)")
        self.slab = _alloc_slab(need, engine.device, settle=True)
        h = C.c_void_p()
        check(self.lib.smoltts_mimi_session_create(engine.handle, dptr(self.slab), need, max_batch, max_chunk_frames, C.byref(h)),
              "smoltts_mimi_session_create")
        self.handle = h
        if stateless_upsample:
            self.set_stateless_upsample(True)
        if products != 6:
            self.set_products(products)

    def set_products(self, n: int) -> None:
        check(self.lib.smoltts_mimi_session_set_option(self.handle, self.OPT_PRODUCTS, int(n)), "smoltts_mimi_session_set_option")

    def set_stateless_upsample(self, on: bool) -> None:
        check(self.lib.smoltts_mimi_session_set_option(self.handle, self.OPT_STATELESS_UPSAMPLE, int(bool(on))),
              "smoltts_mimi_session_set_option")

    def reset(self) -> None:
        check(self.lib.smoltts_mimi_reset(self.handle, current_stream_ptr()), "smoltts_mimi_reset")

    def reset_slots(self, slots: Sequence[int]) -> None:
        """Start new streams in the listed slots; the other slots' streams continue."""
        arr = (C.c_int32 * len(slots))(*slots)
        check(self.lib.smoltts_mimi_reset_slots(self.handle, arr, len(slots), current_stream_ptr()), "smoltts_mimi_reset_slots")

    def decode_chunk(self, codes: torch.Tensor, f0: int, n_frames: int, pcm: torch.Tensor, code_offset: int = 0) -> None:
        """codes: device int32 [batch, F, row] (row >= code_offset + num_codebooks); decodes frames
        [f0, f0+n_frames) of every slot into pcm[:, 1920*f0 : 1920*(f0+n_frames)]."""
        batch, F, row = codes.shape
        assert codes.dtype == torch.int32 and codes.is_contiguous() and pcm.dtype == torch.float32 and pcm.is_contiguous()
        assert batch <= self.B and n_frames <= self.chunk and f0 + n_frames <= F
        cptr = codes.data_ptr() + 4 * f0 * row
        pptr = pcm.data_ptr() + 4 * f0 * self.SAMPLES_PER_FRAME
        check(self.lib.smoltts_mimi_decode_chunk(self.handle, cptr, F * row, row, code_offset, batch, n_frames, pptr,
                                                 pcm.shape[1], current_stream_ptr()), "smoltts_mimi_decode_chunk")

    def decode(self, codes: torch.Tensor, code_offset: int = 0, reset: bool = True) -> torch.Tensor:
        """codes device int32 [batch, F, row] -> pcm [batch, 1920 F] (== MimiModel.decode)."""
        if reset:
            self.reset()
        batch, F, _ = codes.shape
        pcm = torch.empty(batch, F * self.SAMPLES_PER_FRAME, dtype=torch.float32, device=codes.device)
        for f0 in range(0, F, self.chunk):
            self.decode_chunk(codes, f0, min(self.chunk, F - f0), pcm, code_offset)
        return pcm

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize()
            self.lib.smoltts_mimi_session_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------- streamed output formats
def resample_design(out_rate: int):
    """(taps float64 [2 half_len + 1], up, down, half_len) of ``out_rate``: scipy.signal.resample_poly's default filter, designed
    on the host by the library (no device needed).  Raises SmolttsError for an unsupported rate."""
    lib = load_library()
    up, down, half = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.smoltts_resample_design(int(out_rate), None, 0, C.byref(up), C.byref(down), C.byref(half)), "smoltts_resample_design")
    taps = np.zeros(2 * half.value + 1, np.float64)
    check(lib.smoltts_resample_design(int(out_rate), taps.ctypes.data, taps.size, C.byref(up), C.byref(down), C.byref(half)),
          "smoltts_resample_design")
    return taps, up.value, down.value, half.value


class _Stage:
    """What the stages behind the codec share: a slab of ``smoltts_<C_NAME>_bytes(max_batch)`` bytes that the handle of
    ``smoltts_<C_NAME>_create`` lives in, destroyed by ``close`` once the device is idle, and the checks of a ``chunk`` call."""

    C_NAME = ""

    def __init__(self, device: torch.device, max_batch: int):
        self.lib = load_library()
        self.device, self.B = device, max_batch
        need = getattr(self.lib, f"smoltts_{self.C_NAME}_bytes")(max_batch)
        if need == 0:
            raise SmolttsError(f"smoltts_{self.C_NAME}_bytes returned 0 (bad sizes)")
        self.slab = _alloc_slab(need, device, settle=True)
        h = C.c_void_p()
        check(getattr(self.lib, f"smoltts_{self.C_NAME}_create")(dptr(self.slab), need, max_batch, *self._create_args(), C.byref(h)),
              f"smoltts_{self.C_NAME}_create")
        self.handle = h

    def _create_args(self) -> tuple:
        """What the stage's create call takes between ``max_batch`` and the handle."""
        return ()

    @staticmethod
    def _ints(v: Sequence[int]):
        """``v`` as a host int32 array for the C calls."""
        return (C.c_int32 * len(v))(*[int(x) for x in v])

    def _check(self, batch: int, pcm: Optional[torch.Tensor], n_in: int, out: torch.Tensor, dtype, width: int,
               counts: torch.Tensor, per_row: int, *controls: Optional[torch.Tensor]) -> None:
        """``pcm``: device fp32 [>= batch, >= n_in] with unit-stride rows (None: not read); ``out``: contiguous ``dtype``
        [>= batch, >= width]; ``counts``: contiguous int32 of ``per_row`` entries per row; ``controls``: None or contiguous
        device int32 [>= batch]."""
        assert batch <= self.B and out.dtype == dtype and out.is_contiguous() and out.shape[0] >= batch and out.shape[1] >= width
        assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.shape[0] >= batch and counts.numel() >= per_row * batch
        assert pcm is None or (pcm.dtype == torch.float32 and pcm.stride(1) == 1 and pcm.shape[0] >= batch and 0 <= n_in <= pcm.shape[1])
        for t in controls:
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= batch)

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize()
            getattr(self.lib, f"smoltts_{self.C_NAME}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resampler(_Stage):
    """Per-slot conversion of streamed 24 kHz fp32 PCM to ``pcm_<rate>`` int16 / ``ulaw_8000`` bytes on the GPU
    (include/smoltts_hip.h, "Streamed output formats"): one launch per call for every slot, each at its own format.  Slots
    start off; ``reset_slots`` starts a new stream in a slot with its format."""

    C_NAME = "resampler"

    def __init__(self, device: torch.device, max_batch: int, max_in: int):
        super().__init__(device, max_batch)
        self.out_stride = int(self.lib.smoltts_resampler_out_bytes(max_in))
        self.formats = [(24000, 0)] * max_batch  # (rate, SMOLTTS_RESAMPLE_*) per slot

    def reset_slots(self, slots: Sequence[int], formats: Sequence[str]) -> None:
        """Start new streams in ``slots`` with their ``output_format`` (``pcm_24000``: the slot is not converted)."""
        parsed = [parse_stream_format(f) for f in formats]
        check(self.lib.smoltts_resampler_reset_slots(self.handle, self._ints(slots), self._ints([p[0] for p in parsed]),
                                                     self._ints([p[1] for p in parsed]), len(slots), current_stream_ptr()),
              "smoltts_resampler_reset_slots")
        for b, p in zip(slots, parsed):
            self.formats[b] = p

    def new_outputs(self, batch: int, n_in: Optional[int] = None):
        """Device buffers of one call: (bytes uint8 [batch, out_stride], counts int32 [batch, 2]); ``n_in``: size them for calls of
        at most that many input samples instead of ``max_in``."""
        stride = self.out_stride if n_in is None else int(self.lib.smoltts_resampler_out_bytes(n_in))
        return (torch.empty(batch, stride, dtype=torch.uint8, device=self.device),
                torch.empty(batch, 2, dtype=torch.int32, device=self.device))

    def chunk(self, pcm: torch.Tensor, n_in: int, out: torch.Tensor, counts: torch.Tensor, valid: Optional[torch.Tensor] = None) -> None:
        """Convert ``n_in`` samples of every row of ``pcm`` (device fp32 [batch, >= n_in], contiguous rows) on the current stream;
        ``valid``: device int32 [batch], the samples of each row that are real (the rest is not consumed)."""
        batch = pcm.shape[0]
        self._check(batch, pcm, n_in, out, torch.uint8, int(self.lib.smoltts_resampler_out_bytes(n_in)), counts, 2, valid)
        check(self.lib.smoltts_resample_chunk(self.handle, dptr(pcm), pcm.stride(0), batch, n_in, dptr(valid), dptr(out), out.shape[1],
                                              dptr(counts), current_stream_ptr()), "smoltts_resample_chunk")

    def slot_bytes(self, host_out: np.ndarray, host_counts: np.ndarray, b: int, tail: bool = False,
                   enc: Optional[int] = None) -> np.ndarray:
        """Slot ``b``'s samples of a call, copied to the host: int16 for pcm_*, uint8 for ulaw_8000; with the tail if ``tail``.
        ``enc``: the encoding the call ran with, when the slot may have been restarted since (default: its current one)."""
        enc = self.formats[b][1] if enc is None else enc
        n = int(host_counts[b, 0]) + (int(host_counts[b, 1]) if tail else 0)
        width = 1 if enc == 2 else 2
        return host_out[b, : n * width].view(np.uint8 if enc == 2 else np.int16).copy()


# ------------------------------------------------------------------------------- speaking speed
class TimeStretcher(_Stage):
    """Per-slot pitch-preserving time stretch of streamed 24 kHz fp32 PCM on the GPU (include/smoltts_hip.h, "Speaking speed";
    the numpy model is ``tsm.Stretcher``): one launch per call for every slot, each at its own speed.  Slots start off;
    ``reset_slots`` starts a new stream in a slot at its ``speed_q`` (65536: off)."""

    C_NAME = "tsm"

    def out_samples(self, n_in: int) -> int:
        """Output samples per row that a call of ``n_in`` input samples needs."""
        return int(self.lib.smoltts_tsm_out_samples(int(n_in)))

    def reset_slots(self, slots: Sequence[int], speed_q: Sequence[int]) -> None:
        check(self.lib.smoltts_tsm_reset_slots(self.handle, self._ints(slots), self._ints(speed_q), len(slots), current_stream_ptr()),
              "smoltts_tsm_reset_slots")

    def new_outputs(self, batch: int, n_in: int):
        """Device buffers of one call of at most ``n_in`` input samples: (fp32 [batch, out_samples(n_in)], counts int32 [batch])."""
        return (torch.empty(batch, self.out_samples(n_in), dtype=torch.float32, device=self.device),
                torch.empty(batch, dtype=torch.int32, device=self.device))

    def chunk(self, pcm: torch.Tensor, n_in: int, out: torch.Tensor, counts: torch.Tensor, valid: Optional[torch.Tensor] = None,
              last: Optional[torch.Tensor] = None) -> None:
        """Stretch ``n_in`` samples of every row of ``pcm`` (device fp32 [batch, >= n_in], contiguous rows) on the current stream.
        ``valid``: device int32 [batch], the samples of each row that are real; ``last``: device int32 [batch], nonzero where the
        row's stream ends with this call (the slot flushes).  ``counts[b]``: the samples slot b wrote to ``out[b]``."""
        batch = pcm.shape[0]
        self._check(batch, pcm, n_in, out, torch.float32, self.out_samples(n_in), counts, 1, valid, last)
        check(self.lib.smoltts_tsm_chunk(self.handle, dptr(pcm), pcm.stride(0), batch, n_in, dptr(valid), dptr(last), dptr(out),
                                         out.shape[1], dptr(counts), current_stream_ptr()), "smoltts_tsm_chunk")

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s counters (synchronises the current stream): k (next segment), p_prev, n_in, n_out, ended."""
        v = (C.c_int64 * 5)()
        check(self.lib.smoltts_tsm_slot_state(self.handle, int(slot), v, current_stream_ptr()), "smoltts_tsm_slot_state")
        return dict(zip(("k", "p_prev", "n_in", "n_out", "ended"), list(v)))


def _whole_row(stage: _Stage, x: np.ndarray, launch):
    """A whole utterance through slot 0 of ``stage``: ``x`` (host, contiguous) goes up as the device row [1, n] (one zero sample
    when empty), and ``launch(row, n, out, counts)`` queues the stage's call into ``stage.new_outputs(1, n)``.  Waits, and
    returns the output row cut to its count, or for FLAC (counts: frame sizes [1, blocks, 2]) the row's frames."""
    n = int(x.size)
    row = torch.from_numpy(x).to(stage.device)[None] if n else torch.zeros(1, 1, dtype=torch.from_numpy(x).dtype, device=stage.device)
    out, counts = stage.new_outputs(1, n)
    launch(row, n, out, counts)
    if counts.dim() == 1:
        return out[0, :int(counts.cpu()[0])].cpu().numpy()
    return FlacEncoder.slot_frames(out.cpu().numpy(), counts.cpu().numpy(), 0)


def stretch_pcm(pcm: np.ndarray, speed_q: int, device: torch.device) -> np.ndarray:
    """A whole utterance (float32 at 24 kHz) stretched on ``device`` (the model's) in one call with ``last`` set: exactly
    ``tsm.out_length(len(pcm), speed_q)`` samples (``SmolTTS.__call__``).  Waits for the result.  ``speed_q == 65536`` returns
    ``pcm`` untouched."""
    pcm = np.ascontiguousarray(np.asarray(pcm, dtype=np.float32).reshape(-1))
    if speed_q == 65536:
        return pcm
    with torch.cuda.device(device):
        ts = TimeStretcher(device, 1)
        try:
            ts.reset_slots([0], [speed_q])
            return _whole_row(ts, pcm, lambda x, n, out, cnt: ts.chunk(x, n, out, cnt, last=torch.ones(1, dtype=torch.int32, device=device)))
        finally:
            ts.close()


# ------------------------------------------------------------------------------- long texts: the seam between segments
SEAM_FIRST, SEAM_FINAL, SEAM_OFF = 1, 2, 4  # SMOLTTS_SEAM_*


class SeamJoiner(_Stage):
    """Per-slot joining of a long text's segments on the GPU (include/smoltts_hip.h, "Seam"; the numpy model is
    ``seam.SeamState``): one launch per call for every slot.  Slots start off; ``start_segments`` opens a segment in a slot with
    its pause and flags (``SEAM_FIRST`` / ``SEAM_FINAL``; ``SEAM_OFF`` switches the slot off)."""

    C_NAME = "seam"

    def __init__(self, device: torch.device, max_batch: int):
        super().__init__(device, max_batch)
        self.zeros = [0] * max_batch  # zeros the slot's open segment owes at most (its lead and its pause)

    def out_samples(self, n_in: int) -> int:
        """Output samples per row of a call of ``n_in`` input samples, for the segments open now."""
        return int(self.lib.smoltts_seam_out_samples(int(n_in), max(self.zeros)))

    def start_segments(self, slots: Sequence[int], pauses: Sequence[int], flags: Sequence[int],
                       leads: Optional[Sequence[int]] = None) -> None:
        """Open a segment in each of ``slots`` on the current stream: its pause G (samples), flags, and the zeros in front of a
        ``SEAM_FIRST`` segment (``leads``)."""
        n = len(slots)
        if not n:
            return
        leads = leads or [0] * n
        check(self.lib.smoltts_seam_reset_slots(self.handle, self._ints(slots), self._ints(pauses), self._ints(flags), self._ints(leads),
                                                n, current_stream_ptr()), "smoltts_seam_reset_slots")
        for b, p, f, ld in zip(slots, pauses, flags, leads):
            self.zeros[b] = 0 if int(f) & SEAM_OFF else int(p) + (int(ld) if int(f) & SEAM_FIRST else 0)

    def new_outputs(self, batch: int, n_in: int):
        """Device buffers of one call of at most ``n_in`` input samples: (fp32 [batch, out_samples(n_in)], counts int32 [batch])."""
        return (torch.empty(batch, self.out_samples(n_in), dtype=torch.float32, device=self.device),
                torch.empty(batch, dtype=torch.int32, device=self.device))

    def chunk(self, pcm: torch.Tensor, n_in: int, out: torch.Tensor, counts: torch.Tensor, valid: Optional[torch.Tensor] = None,
              seg_end: Optional[torch.Tensor] = None, last: Optional[torch.Tensor] = None) -> None:
        """Join ``n_in`` samples of every row of ``pcm`` (device fp32 [batch, >= n_in], contiguous rows) on the current stream.
        ``valid``: device int32 [batch], the real samples of each row; ``seg_end`` / ``last``: device int32 [batch], nonzero where
        the row's segment / stream ends with this call.  ``counts[b]``: the samples slot b wrote to ``out[b]``."""
        batch = pcm.shape[0]
        self._check(batch, pcm, n_in, out, torch.float32, self.out_samples(n_in), counts, 1, valid, seg_end, last)
        check(self.lib.smoltts_seam_chunk(self.handle, dptr(pcm), pcm.stride(0), batch, n_in, dptr(valid), dptr(seg_end), dptr(last),
                                          max(self.zeros), dptr(out), out.shape[1], dptr(counts), current_stream_ptr()),
              "smoltts_seam_chunk")

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s state (synchronises the current stream): n_in, judged, ec, head, open, lead, pause, flags."""
        v = (C.c_int64 * 8)()
        check(self.lib.smoltts_seam_slot_state(self.handle, int(slot), v, current_stream_ptr()), "smoltts_seam_slot_state")
        return dict(zip(("n_in", "judged", "ec", "head", "open", "lead", "pause", "flags"), list(v)))


def seam_join(segments: Sequence[np.ndarray], pauses: Sequence[int], device: torch.device, lead: int = 0, trail: int = 0,
              joiner: Optional[SeamJoiner] = None) -> np.ndarray:
    """Whole segments (float32 at 24 kHz) joined on ``device`` by the seam rule, one call per segment with its end set: what
    ``seam.join`` computes (``SmolTTS.__call__`` with ``segment``).  ``pauses[k]``: the seam after segment k, in samples.
    ``joiner``: a caller's ``SeamJoiner`` whose slot 0 is used (default: one made for the call).  Waits for the result."""
    segs = [np.ascontiguousarray(np.asarray(s, dtype=np.float32).reshape(-1)) for s in segments]
    if len(pauses) != max(len(segs) - 1, 0):
        raise ValueError("one pause per seam")
    out = []
    with torch.cuda.device(device):
        sj = joiner if joiner is not None else SeamJoiner(device, 1)
        try:
            end = torch.ones(1, dtype=torch.int32, device=device)
            for k, x in enumerate(segs):
                final = k == len(segs) - 1
                sj.start_segments([0], [trail if final else pauses[k]], [segment_flags(k, len(segs))], [lead])
                out.append(_whole_row(sj, x, lambda xd, n, y, cnt: sj.chunk(xd, n, y, cnt, seg_end=end, last=end if final else None)))
        finally:
            if joiner is None:
                sj.close()
    return np.concatenate(out) if out else np.zeros(0, np.float32)


# ------------------------------------------------------------------------------- loudness
class LoudnessNormalizer(_Stage):
    """Per-slot loudness normalisation of streamed 24 kHz fp32 PCM on the GPU (include/smoltts_hip.h, "Loudness"; the numpy
    model is ``loudness.StreamState``): one launch per call for every slot, each towards its own target.  A slot emits exactly
    the samples it reads.  Slots start off; ``reset_slots`` starts a new stream in a slot (target None: off)."""

    C_NAME = "loudness"

    def _create_args(self) -> tuple:
        from .loudness import tables

        self._tables = tables().packed()  # (read by the create call only)
        assert self._tables.size == self.lib.smoltts_loudness_table_doubles()
        return self._tables.ctypes.data, int(self._tables.size)

    def reset_slots(self, slots: Sequence[int], targets: Sequence[Optional[float]],
                    start_gain_db: Optional[Sequence[Optional[float]]] = None) -> None:
        """Start new streams in ``slots`` towards their ``targets`` (LUFS; None: the slot is off) from their first knots
        (``start_gain_db``, default 0 dB)."""
        from .loudness import knot_of_db, target_power

        n = len(slots)
        if not n:
            return
        power = (C.c_double * n)(*[0.0 if t is None else target_power(t) for t in targets])
        knots = self._ints([knot_of_db(g or 0.0) for g in (start_gain_db or [0.0] * n)])
        check(self.lib.smoltts_loudness_reset_slots(self.handle, self._ints(slots), power, knots, n, current_stream_ptr()),
              "smoltts_loudness_reset_slots")

    def new_outputs(self, batch: int, n_in: int):
        """Device buffers of one call of at most ``n_in`` input samples: (fp32 [batch, n_in], counts int32 [batch])."""
        return (torch.empty(batch, max(int(n_in), 1), dtype=torch.float32, device=self.device),
                torch.empty(batch, dtype=torch.int32, device=self.device))

    def chunk(self, pcm: torch.Tensor, n_in: int, out: torch.Tensor, counts: torch.Tensor, valid: Optional[torch.Tensor] = None) -> None:
        """Normalise ``n_in`` samples of every row of ``pcm`` (device fp32 [batch, >= n_in], contiguous rows) on the current
        stream.  ``valid``: device int32 [batch], the real samples of each row.  ``counts[b]``: the samples slot b wrote to
        ``out[b]`` (its valid ones; 0 for a slot that is off)."""
        batch = pcm.shape[0]
        self._check(batch, pcm, n_in, out, torch.float32, n_in, counts, 1, valid)
        check(self.lib.smoltts_loudness_chunk(self.handle, dptr(pcm), pcm.stride(0), batch, n_in, dptr(valid), dptr(out), out.shape[1],
                                              dptr(counts), current_stream_ptr()), "smoltts_loudness_chunk")

    def measure(self, row: torch.Tensor, n: int) -> Tuple[float, float]:
        """(gated mean power, peak) of the whole utterance ``row[:n]`` (device fp32, contiguous); waits for the result."""
        hops = torch.empty(n // 2400 + 1, dtype=torch.float64, device=self.device)
        res = torch.empty(4, dtype=torch.float64, device=self.device)
        check(self.lib.smoltts_loudness_measure(self.handle, dptr(row), int(n), dptr(hops), hops.numel(), dptr(res), current_stream_ptr()),
              "smoltts_loudness_measure")
        p, peak = res.cpu().numpy()[:2]
        return float(p), float(peak)

    def scale(self, row: torch.Tensor, n: int, gain: float, out: torch.Tensor) -> None:
        """``out[:n] = float32(row[:n] * gain)`` on the current stream."""
        check(self.lib.smoltts_loudness_scale(dptr(row), int(n), float(gain), dptr(out), current_stream_ptr()), "smoltts_loudness_scale")

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s state (synchronises the current stream), in the layout of ``loudness.StreamState.state``, with
        ``on`` and ``ptarget``."""
        ints, v = (C.c_int64 * 4)(), np.zeros(19 + 512, np.float64)
        check(self.lib.smoltts_loudness_slot_state(self.handle, int(slot), ints, v.ctypes.data, current_stream_ptr()),
              "smoltts_loudness_slot_state")
        return {"pos": int(ints[0]), "ka": int(ints[1]), "kb": int(ints[2]), "on": int(ints[3]), "peak": np.float32(v[17]),
                "ptarget": float(v[18]), "filter": v[:17].copy(), "ring": v[19:].copy()}


def _loudness_whole(pcm: np.ndarray, device: torch.device, target: Optional[float]):
    """(power, peak, gain, output or None) of a whole utterance on ``device``: measured in one launch, and with a ``target``
    scaled by the blocking rule's gain in a second one."""
    from .loudness import static_gain

    x = np.ascontiguousarray(np.asarray(pcm, dtype=np.float32).reshape(-1))
    with torch.cuda.device(device):
        ln = LoudnessNormalizer(device, 1)
        try:
            seen = {}

            def launch(row, n, out, counts):
                seen["p"], seen["peak"] = ln.measure(row, n) if n else (0.0, 0.0)
                seen["g"] = 1.0 if target is None else static_gain(target, seen["p"], seen["peak"])
                ln.scale(row, n, seen["g"], out)
                counts.fill_(n)

            y = _whole_row(ln, x, launch)
        finally:
            ln.close()
    return seen["p"], seen["peak"], seen["g"], (x if seen["g"] == 1.0 else y)


def measure_loudness(pcm: np.ndarray, device: torch.device) -> Tuple[float, float]:
    """(integrated loudness in LUFS by BS.1770-4, -inf when no block passes the absolute gate or the utterance is shorter than
    400 ms; peak) of a whole utterance (float32 at 24 kHz), measured on ``device``: ``loudness.measure``.  Waits."""
    from .loudness import lufs_of_power

    p, peak, _, _ = _loudness_whole(pcm, device, None)
    return lufs_of_power(p), peak


def loudness_normalize(pcm: np.ndarray, target: float, device: torch.device, with_gain: bool = False):
    """A whole utterance (float32 at 24 kHz) brought to ``target`` LUFS on ``device`` by one gain, capped so that its peak
    stays at -1 dBFS: ``loudness.normalize`` (``SmolTTS.__call__``).  An utterance that measures nothing comes back
    unchanged.  ``with_gain``: -> (samples, the gain applied).  Waits for the result."""
    from .loudness import check_target

    _, _, g, y = _loudness_whole(pcm, device, check_target(target))
    return (y, g) if with_gain else y


# ------------------------------------------------------------------------------- FLAC framing
FLAC_OFF, FLAC_F32, FLAC_S16 = 0, 1, 2  # SMOLTTS_FLAC_*


class FlacEncoder(_Stage):
    """Per-slot FLAC framing of streamed samples on the GPU (include/smoltts_hip.h, "FLAC"; the numpy model is
    ``flac.StreamEncoder``): one launch per call for every slot, each reading fp32 PCM or the resampler's int16 at its own rate.
    Slots start off; ``reset_slots`` starts a new stream in a slot.  The stream header (``flac.stream_header``) is the caller's."""

    C_NAME = "flac"

    def reset_slots(self, slots: Sequence[int], rates: Sequence[int], sources: Sequence[int]) -> None:
        """Start new streams in ``slots`` at their rate and source (``FLAC_F32`` / ``FLAC_S16``; ``FLAC_OFF``: off)."""
        check(self.lib.smoltts_flac_reset_slots(self.handle, self._ints(slots), self._ints(rates), self._ints(sources), len(slots),
                                                current_stream_ptr()), "smoltts_flac_reset_slots")

    def new_outputs(self, batch: int, n_max: int):
        """Device buffers of one call in which a slot reads at most ``n_max`` samples: (bytes uint8 [batch, out_bytes],
        sizes int32 [batch, max_blocks, 2])."""
        blocks = int(self.lib.smoltts_flac_max_blocks(int(n_max)))
        return (torch.empty(batch, int(self.lib.smoltts_flac_out_bytes(int(n_max))), dtype=torch.uint8, device=self.device),
                torch.empty(batch, blocks, 2, dtype=torch.int32, device=self.device))

    def chunk(self, batch: int, out: torch.Tensor, sizes: torch.Tensor, pcm: Optional[torch.Tensor] = None, n_in: int = 0,
              valid: Optional[torch.Tensor] = None, s16: Optional[torch.Tensor] = None, s16_counts: Optional[torch.Tensor] = None,
              last: Optional[torch.Tensor] = None) -> None:
        """Frame the samples of slots [0, batch) on the current stream: F32 slots read ``n_in`` samples of ``pcm`` (device fp32
        [batch, >= n_in]; ``valid``: device int32 [batch], the real ones), S16 slots the resampler's ``s16`` bytes (uint8
        [batch, row]) and ``s16_counts`` (int32 [batch, 2]: finals, tail); ``last`` (device int32 [batch]) nonzero where the
        stream ends with this call.  ``sizes[b, j]``: {offset, bytes} of slot b's frame j in ``out[b]``."""
        self._check(batch, pcm, n_in, out, torch.uint8, 0, sizes, 0, valid, last)
        if s16 is not None:
            assert s16.dtype == torch.uint8 and s16.is_contiguous() and s16_counts is not None and s16_counts.is_contiguous()
        check(self.lib.smoltts_flac_chunk(self.handle, dptr(pcm), pcm.stride(0) if pcm is not None else 0, int(n_in), dptr(valid),
                                          dptr(s16), s16.shape[1] if s16 is not None else 0, dptr(s16_counts), batch, dptr(last),
                                          dptr(out), out.shape[1], dptr(sizes), sizes.shape[1], current_stream_ptr()),
              "smoltts_flac_chunk")

    @staticmethod
    def slot_frames(host_out: np.ndarray, host_sizes: np.ndarray, b: int) -> List[bytes]:
        """Slot ``b``'s frames of a call, in order, from the host copies of ``out`` and ``sizes``."""
        frames = []
        for off, n in host_sizes[b]:
            if n <= 0:
                break
            frames.append(host_out[b, int(off):int(off) + int(n)].tobytes())
        return frames


def flac_encode(samples: np.ndarray, sample_rate: int, device: torch.device) -> bytes:
    """A whole utterance as one FLAC file, framed on ``device`` in one call with ``last`` set: float32 samples are quantised as
    rint(clip(x, -1, 1) * 32767), int16 ones taken as they are.  The STREAMINFO carries the true total, the smallest and largest
    frame and the MD5 of the samples (``SmolTTS.__call__``).  Waits for the result."""
    from . import flac

    x = np.asarray(samples).reshape(-1)
    is_f32 = x.dtype != np.int16
    x = np.ascontiguousarray(x, dtype=np.float32 if is_f32 else np.int16)
    s16 = flac.quantize(x) if is_f32 else x
    with torch.cuda.device(device):
        fe = FlacEncoder(device, 1)
        try:
            fe.reset_slots([0], [sample_rate], [FLAC_F32 if is_f32 else FLAC_S16])
            last = torch.ones(1, dtype=torch.int32, device=device)
            if is_f32:
                frames = _whole_row(fe, x, lambda row, n, out, sizes: fe.chunk(1, out, sizes, pcm=row, n_in=n, last=last))
            else:  # (the int16 row read as the resampler's bytes, all of it final)
                frames = _whole_row(fe, x, lambda row, n, out, sizes: fe.chunk(
                    1, out, sizes, s16=row.view(torch.uint8), s16_counts=torch.tensor([[n, 0]], dtype=torch.int32, device=device), last=last))
        finally:
            fe.close()
    return flac.file_from_frames(frames, s16, sample_rate)


# ------------------------------------------------------------------------------- a stream's stages behind the codec
STAGES = ("seam", "stretch", "resample", "flac")  # the stages every build has had, in launch order
LAUNCH_ORDER = ("seam", "loudness", "stretch", "resample", "flac")  # the stages of a pass, in launch order
FLOAT_STAGES = ("seam", "loudness", "stretch")  # fp32 in, fp32 out: the stages behind read their rows


@dataclass(frozen=True)
class SlotRoute:
    """What a slot's stream goes through behind the codec (``StreamConverter``): its format (rate, SMOLTTS_RESAMPLE_*), its Q16
    speed, FLAC framing, whether it is segmented (``start_segments``), its stream generation in the slot and whether its FLAC
    stream header is still owed.  A restarted slot gets a new record: a pass keeps the records of its run."""
    rate: int = 24000
    enc: int = ENC_OFF
    speed_q: int = 65536
    flac: bool = False
    segmented: bool = False
    gen: int = 0
    head_owed: bool = False
    loudness: Optional[float] = None  # target in LUFS (None: the slot never enters the loudness stage)
    start_gain_db: float = 0.0        # its stream's first knot

    @cached_property
    def stages(self) -> Tuple[str, ...]:
        """The stages the slot goes through, in launch order."""
        on = (self.segmented, self.loudness is not None, self.speed_q != 65536, self.enc != ENC_OFF, self.flac)
        return tuple(s for s, o in zip(LAUNCH_ORDER, on) if o)


class PassPlan(NamedTuple):
    stages: List[str]                 # the stages to launch, in order
    rows: Dict[str, List[int]]        # the live slots each of them serves
    through: Dict[str, List[int]]     # float stage (seam, loudness, stretch) -> the live slots it does not serve that a later stage does
    source: Dict[int, Optional[str]]  # live slot -> the last stage it goes through (None: its codec rows are its output)
    host: List[str]                   # the stages whose outputs are copied to the host: the sources of the live slots
    routes: Dict[int, SlotRoute]      # live slot -> its route when planned


def plan_pass(routes: Dict[int, SlotRoute]) -> PassPlan:
    """The plan of one converter pass over the live slots' routes (``{slot: SlotRoute}``, in slot order); no device involved."""
    rows = {s: [] for s in LAUNCH_ORDER}
    through = {s: [] for s in FLOAT_STAGES}
    source = {}
    for b, r in routes.items():
        path = r.stages
        source[b] = path[-1] if path else None
        for s in path:
            rows[s].append(b)
        for s in through:
            if path and s not in path and LAUNCH_ORDER.index(path[-1]) > LAUNCH_ORDER.index(s):
                through[s].append(b)
    stages = [s for s in LAUNCH_ORDER if rows[s]]
    return PassPlan(stages, {s: rows[s] for s in stages}, {s: through[s] for s in through if rows[s]}, source,
                    [s for s in stages if s in source.values()], routes)


class StreamConverter:
    """What a stream's PCM goes through behind its codec decode, per slot of ``max_batch`` (``SlotRoute``, ``STAGES``): a
    segmented slot (``start_segments``) is joined by the seam stage (``SeamJoiner``), a slot with a speed is time-stretched
    (``TimeStretcher``), a slot with an output format is converted (``Resampler``), and a slot with a FLAC container is framed
    (``FlacEncoder``, from the resampler's int16, or from the float32 at 24 kHz); each stage reads the output of the one in
    front, and the state of the stages behind the seam carries from segment to segment.  Each stage is created the first time
    a slot needs it (``seam``: the seam stage at once).  ``n_in``: codec samples per slot and call."""

    def __init__(self, device: torch.device, max_batch: int, n_in: int, seam: bool = False):
        self.device, self.B, self.n_in = device, max_batch, n_in
        self.rs: Optional[Resampler] = None
        self.ts: Optional[TimeStretcher] = None
        self.fl: Optional[FlacEncoder] = None
        self.sj: Optional[SeamJoiner] = SeamJoiner(device, max_batch) if seam else None
        self.ln: Optional[LoudnessNormalizer] = None
        self.routes = [SlotRoute()] * max_batch
        self._plan: Optional[PassPlan] = None  # the last pass's plan

    def reset_slots(self, slots: Sequence[int], formats: Sequence[Optional[str]], speed_q: Sequence[Optional[int]],
                    containers: Optional[Sequence[Optional[str]]] = None, loudness: Optional[Sequence[Optional[float]]] = None,
                    start_gain_db: Optional[Sequence[Optional[float]]] = None) -> None:
        """Start new streams in ``slots`` on the current stream: ``formats[i]`` an ``output_format`` (None / ``pcm_24000``:
        float32), ``speed_q[i]`` a Q16 speed (None / 65536: none), ``containers[i]`` None or ``"flac"`` (FLAC frames of the
        slot's 16-bit samples at its rate), ``loudness[i]`` a target in LUFS (None: none) reached from ``start_gain_db[i]``.
        A slot with none of them is switched off."""
        if not slots:
            return
        formats = [f or "pcm_24000" for f in formats]
        routes = []
        none = [None] * len(slots)
        for b, f, q, c, lt, sg in zip(slots, formats, speed_q, containers or none, loudness or none, start_gain_db or none):
            rate, enc = parse_stream_format(f)
            flac = check_container(c, f) is not None
            routes.append(SlotRoute(rate, enc, q or 65536, flac, segmented=False, gen=self.routes[b].gen + 1, head_owed=flac,
                                    loudness=lt, start_gain_db=sg or 0.0))
        if self.ln is None and any(r.loudness is not None for r in routes):
            self.ln = LoudnessNormalizer(self.device, self.B)
        if self.ln is not None:
            self.ln.reset_slots(slots, [r.loudness for r in routes], [r.start_gain_db for r in routes])
        if self.rs is None and any(r.enc != ENC_OFF for r in routes):
            self.rs = Resampler(self.device, self.B, out_bound(self.n_in))
        if self.ts is None and any(r.speed_q != 65536 for r in routes):
            self.ts = TimeStretcher(self.device, self.B)
        if self.fl is None and any(r.flac for r in routes):
            self.fl = FlacEncoder(self.device, self.B)
        if self.rs is not None:
            self.rs.reset_slots(slots, formats)
        if self.ts is not None:
            self.ts.reset_slots(slots, [r.speed_q for r in routes])
        if self.fl is not None:
            self.fl.reset_slots(slots, [r.rate for r in routes],
                                [FLAC_OFF if not r.flac else (FLAC_F32 if r.enc == ENC_OFF else FLAC_S16) for r in routes])
        if self.sj is not None:
            self.sj.start_segments(slots, [0] * len(slots), [SEAM_OFF] * len(slots))
        for b, r in zip(slots, routes):
            self.routes[b] = r

    def start_segments(self, slots: Sequence[int], pauses: Sequence[int], flags: Sequence[int],
                       leads: Optional[Sequence[int]] = None) -> None:
        """Open the next segment of the segmented streams in ``slots`` (``SeamJoiner.start_segments``), after ``reset_slots``
        started the streams; the other stages' state is kept."""
        if self.sj is None:
            self.sj = SeamJoiner(self.device, self.B)
        self.sj.start_segments(slots, pauses, flags, leads)
        for b, f in zip(slots, flags):
            self.routes[b] = replace(self.routes[b], segmented=not int(f) & SEAM_OFF)

    def converts(self, b: int) -> bool:
        """Whether slot ``b``'s stream goes through a stage: its chunks are ``StreamPass.chunk``'s, not the codec's float32."""
        return bool(self.routes[b].stages)

    def plan(self, slots: Sequence[int]) -> PassPlan:
        """The plan of a pass over the live ``slots``: the last one again while they and their routes stay the same."""
        p, slots = self._plan, tuple(slots)
        if p is None or tuple(p.routes) != slots or any(self.routes[b] is not r for b, r in p.routes.items()):
            p = self._plan = plan_pass({b: self.routes[b] for b in slots})
        return p

    def ends(self, slots: Sequence[int]):
        """The end markers a pass over ``slots`` needs: (``last``: some slot has a speed, FLAC or segments; ``seg_end``: some
        slot has segments)."""
        stages = self.plan(slots).stages
        return any(s in stages for s in ("seam", "stretch", "flac")), "seam" in stages

    def _through(self, plan: PassPlan, stage: str, out: torch.Tensor, counts: torch.Tensor, pcm: torch.Tensor, n_in: int,
                 valid: torch.Tensor) -> torch.Tensor:
        """After a float stage: its rows of the slots it passes through (``plan.through``) take the ``pcm`` it read, so that the
        stages behind serve all slots in one launch each; returns the valid counts of its rows."""
        plain = plan.through[stage]
        if not plain:
            return counts
        served = np.zeros(out.shape[0], np.int32)
        served[plan.rows[stage]] = 1
        served_d, plain_d = upload([served, np.asarray(plain, np.int64)], self.device)
        out[plain_d, :n_in] = pcm[plain_d]
        return torch.where(served_d != 0, counts, valid)

    def run(self, pcm: torch.Tensor, n_in: int, valid: torch.Tensor, last: Optional[torch.Tensor] = None,
            slots: Optional[Sequence[int]] = None, seg_end: Optional[torch.Tensor] = None) -> Optional["StreamPass"]:
        """Queue the stages for ``n_in`` samples of every row of ``pcm`` (device fp32 [batch, >= n_in]) on the current stream.
        ``valid`` (device int32 [batch]): the samples of each row that are real; ``last`` / ``seg_end`` (device int32 [batch],
        needed as ``ends`` says): nonzero where the row's stream / segment ends with this call.  ``slots``: the live streams
        (default: every slot); the others consume what ``valid`` gives them and are never read.  None when no live slot
        converts: no launch."""
        plan = self.plan(range(self.B) if slots is None else slots)
        if not plan.stages:
            return None
        batch, outs = pcm.shape[0], {}
        if "seam" in plan.stages:  # (each float stage's rows, counts and width are what the stages behind it read)
            out, counts = outs["seam"] = self.sj.new_outputs(batch, n_in)
            self.sj.chunk(pcm, n_in, out, counts, valid=valid, seg_end=seg_end, last=last)
            valid, pcm, n_in = self._through(plan, "seam", out, counts, pcm, n_in, valid), out, out.shape[1]
        if "loudness" in plan.stages:
            out, counts = outs["loudness"] = self.ln.new_outputs(batch, n_in)
            self.ln.chunk(pcm, n_in, out, counts, valid=valid)
            valid, pcm, n_in = self._through(plan, "loudness", out, counts, pcm, n_in, valid), out, out.shape[1]
        if "stretch" in plan.stages:
            out, counts = outs["stretch"] = self.ts.new_outputs(batch, n_in)
            self.ts.chunk(pcm, n_in, out, counts, valid=valid, last=last)
            valid, pcm, n_in = self._through(plan, "stretch", out, counts, pcm, n_in, valid), out, out.shape[1]
        if "resample" in plan.stages:
            out, counts = outs["resample"] = self.rs.new_outputs(batch, n_in)
            self.rs.chunk(pcm, n_in, out, counts, valid=valid)
        if "flac" in plan.stages:
            s16, s16_counts = outs["resample"] if any(plan.routes[b].enc != ENC_OFF for b in plan.rows["flac"]) else (None, None)
            fout, fsizes = outs["flac"] = self.fl.new_outputs(batch, max(n_in, s16.shape[1] // 2 if s16 is not None else 0))
            self.fl.chunk(batch, fout, fsizes, pcm=pcm, n_in=n_in, valid=valid, s16=s16, s16_counts=s16_counts, last=last)
        return StreamPass(self, {s: outs[s] for s in plan.host}, plan)

    def close(self):
        for stage in (self.rs, self.ts, self.fl, self.sj, self.ln):
            if stage is not None:
                stage.close()
        self.rs = self.ts = self.fl = self.sj = self.ln = None


class StreamPass:
    """The outputs of one ``StreamConverter.run``: on the device, then (``to_host``) on the host, read slot by slot (``chunk``).
    It reads each slot by the plan of its run: a slot may have been restarted by the time its chunk is read."""

    def __init__(self, conv: StreamConverter, dev: Dict[str, tuple], plan: PassPlan):
        self.conv, self.rs = conv, conv.rs
        self.dev = dev    # source stage -> its (output, counts) on the device
        self.plan = plan
        self.host = None

    def converts(self, b: int) -> bool:
        """Whether slot ``b`` was converted in the run (its chunk is ``chunk(b, ...)``)."""
        return self.plan.source.get(b) is not None

    def to_host(self, stream) -> None:
        """Queue the host copies on ``stream``; ``chunk`` reads them once ``stream`` has run them."""
        with torch.cuda.stream(stream):
            self.host = {s: tuple(t.to("cpu", non_blocking=True) for t in ts) for s, ts in self.dev.items()}

    def chunk(self, b: int, last: bool) -> np.ndarray:
        """Slot ``b``'s chunk from its source stage: its FLAC frames as uint8 (behind the stream header on the stream's first
        chunk), its converted samples (with the resampler's tail when ``last``), or the stretched / joined float32."""
        route, source = self.plan.routes[b], self.plan.source[b]
        out, counts = (t.numpy() for t in self.host[source])
        if source == "flac":
            from .flac import stream_header

            data = b"".join(FlacEncoder.slot_frames(out, counts, b))
            now = self.conv.routes[b]
            if now.head_owed and now.gen == route.gen:
                self.conv.routes[b] = replace(now, head_owed=False)
                data = stream_header(route.rate) + data
            return np.frombuffer(data, dtype=np.uint8).copy()
        if source == "resample":
            return self.rs.slot_bytes(out, counts, b, tail=last, enc=route.enc)
        return out[b, : int(counts[b])].copy()
