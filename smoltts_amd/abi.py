"""The ctypes binding of ``libsmoltts_hip.so``: every struct, constant and signature of include/smoltts_hip.h that Python uses,
and nothing else.  This is the only module that mirrors the header; tests/test_abi_cpu.py parses the header and holds
``SIGNATURES``, the struct layouts and the constants to it.

There is no CPU fallback: ``load_library`` raises when the HIP library has not been built, and ``check`` raises
``SmolttsError`` on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from pathlib import Path
from typing import List, Optional

LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libsmoltts_hip.so"


class SmolttsError(RuntimeError):
    pass


# ------------------------------------------------------------------------------- constants (the header's names minus SMOLTTS_)
ABI_VERSION = 9
OK, E_INVALID, E_HIP, E_STATE, E_CAPACITY = 0, -1, -2, -3, -4
MAX_LAYERS, MAX_FAST_LAYERS, MIMI_MAX_LAYERS = 64, 16, 16
MAX_ALIGN_HEADS = 16
KV_F32, KV_BF16 = 0, 1
W_BF16, W_FP8 = 0, 1
OPT_QKV_TABLE, OPT_COMMIT_PICKS, OPT_SPLIT_ATTN, OPT_STREAM_W, OPT_FUSE_DEPTH_ATTN, OPT_FUSE_PICK, OPT_FP8_PREFILL = 1, 2, 3, 4, 5, 6, 7
MIMI_OPT_STATELESS_UPSAMPLE, MIMI_OPT_PRODUCTS = 1, 2
PRO_NONE, PRO_RMSNORM, PRO_ELU, PRO_LAYERNORM = 0, 1, 2, 3
EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_GELU, EPI_SCALE_RESID, EPI_QKV_ROPE = range(6)
RESAMPLE_OFF, RESAMPLE_S16, RESAMPLE_ULAW = 0, 1, 2
SEAM_FIRST, SEAM_FINAL, SEAM_OFF = 1, 2, 4
FLAC_OFF, FLAC_F32, FLAC_S16 = 0, 1, 2
FILTER_MAX_WINDOW, FILTER_MAX_PENALTY = 64, 1000.0
LENGTH_MAX_FRAMES = 1 << 30
PREFIX_MAGIC, PREFIX_MAX_INSTALL = 0x58464250, 16

KV_FORMATS = {"fp32": KV_F32, "bf16": KV_BF16}


# ------------------------------------------------------------------------------- C structs (Smoltts<Name> in the header)
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


class SlotSampling(C.Structure):
    _fields_ = [("temp", C.c_float), ("fast_temp", C.c_float), ("min_p", C.c_float), ("reserved", C.c_uint32), ("seed", C.c_uint64)]


class SlotFilters(C.Structure):
    _fields_ = [("top_p", C.c_float), ("top_k", C.c_int32), ("penalty", C.c_float), ("inv_penalty", C.c_float),
                ("window", C.c_int32), ("reserved", C.c_int32 * 3)]


class SlotLength(C.Structure):
    _fields_ = [("min_frames", C.c_int32), ("eos_bias", C.c_float), ("reserved", C.c_int32 * 2)]


class PrefixHeader(C.Structure):
    _fields_ = [("magic", C.c_uint32)] + [(n, C.c_int32) for n in ("n_positions", "n_layer", "n_kv_head", "kv_format", "head_dim")] + [
        ("data_bytes", C.c_uint64)]


class MimiLayerWeights(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("ln1_w", "ln1_b", "wqkv", "wo", "ls1", "ln2_w", "ln2_b", "fc1", "fc2", "ls2",
                                          "wqkv3", "wo3", "fc13", "fc23")]


class MimiConv(C.Structure):
    _fields_ = [("w", C.c_uint64), ("b", C.c_uint64)] + [(n, C.c_int32) for n in ("cin", "cout", "k", "stride", "transposed")] + [
        ("w3", C.c_uint64)]


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


class MimiEncLayout(C.Structure):
    _fields_ = [("T", C.c_int32 * 5), ("extra", C.c_int32 * 4), ("left", C.c_int32 * 4), ("F", C.c_int32), ("ds_extra", C.c_int32),
                ("ds_left", C.c_int32), ("xraw", C.c_uint64 * 4), ("xelu", C.c_uint64 * 4), ("helu", C.c_uint64 * 4),
                ("yelu", C.c_uint64 * 4), ("zelu", C.c_uint64), ("kc", C.c_uint64), ("vc", C.c_uint64), ("layer_stride", C.c_uint64),
                ("ds", C.c_uint64), ("emb", C.c_uint64), ("res", C.c_uint64), ("dots", C.c_uint64), ("total", C.c_uint64)]


class GemmArgs(C.Structure):
    _fields_ = [
        ("w_dev", C.c_void_p), ("w_is_fp32", C.c_int32), ("x_dev", C.c_void_p), ("ldx", C.c_int64), ("x_bstride", C.c_int64),
        ("rows_per_batch", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("prologue", C.c_int32),
        ("epilogue", C.c_int32), ("gamma_dev", C.c_void_p), ("eps", C.c_float), ("bias_dev", C.c_void_p), ("scale_dev", C.c_void_p),
        ("resid_dev", C.c_void_p), ("ldr", C.c_int64), ("r_bstride", C.c_int64), ("out_dev", C.c_void_p), ("ldo", C.c_int64),
        ("o_bstride", C.c_int64), ("elu_out", C.c_int32), ("raw_out_dev", C.c_void_p), ("raw_bstride", C.c_int64),
        ("rope_dev", C.c_void_p), ("row_pos_dev", C.c_void_p), ("row_slot_dev", C.c_void_p), ("k_cache_dev", C.c_void_p),
        ("v_cache_dev", C.c_void_p), ("n_q_heads", C.c_int32), ("n_kv_heads", C.c_int32), ("cache_len", C.c_int32),
        ("w3_dev", C.c_void_p), ("splitk_ws_dev", C.c_void_p), ("splitk_ws_floats", C.c_int64), ("beta_dev", C.c_void_p),
        ("ln_scratch_dev", C.c_void_p), ("k_cache3_dev", C.c_void_p), ("v_cache3_dev", C.c_void_p), ("b3_products", C.c_int32),
    ]


class PickArgs(C.Structure):
    _fields_ = [
        ("cand_dev", C.c_void_p), ("cand_tiles", C.c_int32), ("qkv_table_dev", C.c_void_p), ("rope_dev", C.c_void_p),
        ("emb_dev", C.c_void_p), ("emb_row_offset", C.c_int32), ("ids_dev", C.c_void_p), ("ids_stride", C.c_int32),
        ("margin_dev", C.c_void_p), ("margin_mask_dev", C.c_void_p), ("margin_at_dev", C.c_void_p), ("frames_dev", C.c_void_p),
        ("step", C.c_int32),
    ]


class Gemm3Args(C.Structure):
    _fields_ = [
        ("w_dev", C.c_void_p), ("x3_dev", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("epilogue", C.c_int32),
        ("ssq_in_dev", C.c_void_p), ("eps", C.c_float), ("bias_dev", C.c_void_p), ("resid_dev", C.c_void_p), ("out_dev", C.c_void_p),
        ("ldo", C.c_int64), ("x3_out_dev", C.c_void_p), ("emit_a_dev", C.c_void_p), ("gamma_a_dev", C.c_void_p),
        ("emit_b_dev", C.c_void_p), ("gamma_b_dev", C.c_void_p), ("ssq_out_dev", C.c_void_p), ("rope_dev", C.c_void_p),
        ("row_pos_dev", C.c_void_p), ("row_slot_dev", C.c_void_p), ("k_cache_dev", C.c_void_p), ("v_cache_dev", C.c_void_p),
        ("n_q_heads", C.c_int32), ("n_kv_heads", C.c_int32), ("cache_len", C.c_int32), ("w_format", C.c_int32),
        ("w_scale_dev", C.c_void_p), ("v_x3_dev", C.c_void_p), ("kv_format", C.c_int32), ("w_stream", C.c_int32),
        ("attn_q_dev", C.c_void_p), ("attn_pos", C.c_int32), ("cand_out_dev", C.c_void_p), ("pick", C.POINTER(PickArgs)),
        ("fp8_activations", C.c_int32),
    ]


STRUCTS = (BlockWeights, LMConfig, LMWeights, SlotSampling, SlotFilters, SlotLength, PrefixHeader, MimiLayerWeights, MimiConv, MimiConfig,
           MimiWeights, MimiEncConfig, MimiEncWeights, MimiEncLayout, GemmArgs, PickArgs, Gemm3Args)

# ------------------------------------------------------------------------------- signatures
# name -> (restype, argument kinds).  Kinds: p = opaque handle, device pointer, host array or stream (c_void_p); i = int32_t;
# q = int64_t; z = size_t; Q = uint64_t; f = float; d = double; X* = POINTER(X) for X one of p, i, f, Q or a struct above.
INT, I32, SIZE, STR = C.c_int, C.c_int32, C.c_size_t, C.c_char_p
_KINDS = {"p": C.c_void_p, "i": C.c_int32, "q": C.c_int64, "z": C.c_size_t, "Q": C.c_uint64, "f": C.c_float, "d": C.c_double}

SIGNATURES = {
    "smoltts_last_error": (STR, ""),
    "smoltts_abi_version": (INT, ""),
    "smoltts_engine_create": (INT, "LMConfig* LMWeights* p z p*"),
    "smoltts_engine_destroy": (None, "p"),
    "smoltts_engine_fast_qkv_bytes": (SIZE, "p"),
    "smoltts_engine_build_fast_qkv": (INT, "p p z p"),
    "smoltts_session_slab_bytes": (SIZE, "p i i i i"),
    "smoltts_session_create": (INT, "p p z i i i i p*"),
    "smoltts_session_slab_bytes_kv": (SIZE, "p i i i i i"),
    "smoltts_session_create_kv": (INT, "p p z i i i i i p*"),
    "smoltts_session_destroy": (None, "p"),
    "smoltts_lm_prefill": (INT, "p p p p i p p i i p"),
    "smoltts_lm_prefill_chunk": (INT, "p p p p i p p i p"),
    "smoltts_lm_prefill_deferred": (INT, "p p p p i p p i i p"),
    "smoltts_lm_park_slots": (INT, "p p p i p"),
    "smoltts_lm_prefill_side": (INT, "p p p p i p"),
    "smoltts_lm_start_slots": (INT, "p p p p p i i p"),
    "smoltts_lm_measure_rows": (INT, "p p p p p p i p p"),
    "smoltts_lm_decode": (INT, "p i p"),
    "smoltts_session_set_frames_per_graph": (INT, "p i p"),
    "smoltts_session_set_option": (INT, "p i i"),
    "smoltts_session_set_sampling": (INT, "p f f f Q"),
    "smoltts_session_set_slot_sampling": (INT, "p p i p p p p p"),
    "smoltts_session_set_slot_filters": (INT, "p p i p p p p p"),
    "smoltts_session_set_slot_length": (INT, "p p i p p p"),
    "smoltts_session_set_slot_score": (INT, "p p i p"),
    "smoltts_session_logprobs": (INT, "p p* i*"),
    "smoltts_session_align_bytes": (SIZE, "p i"),
    "smoltts_session_set_align_heads": (INT, "p p p i p z"),
    "smoltts_session_set_slot_align": (INT, "p p i p p p"),
    "smoltts_session_alignment": (INT, "p p* i*"),
    "smoltts_session_graph_form": (INT, "p"),
    "smoltts_session_slow_logits": (INT, "p p* i*"),
    "smoltts_session_outputs": (INT, "p p* p* p* p*"),
    "smoltts_session_kv_cache": (INT, "p p* p* Q*"),
    "smoltts_session_fast_kv_cache": (INT, "p p* p* Q*"),
    "smoltts_session_margin_at": (INT, "p p*"),
    "smoltts_prefix_kv_bytes": (SIZE, "p i i"),
    "smoltts_session_save_prefix": (INT, "p i i p PrefixHeader* p"),
    "smoltts_session_install_prefix": (INT, "p p* PrefixHeader* i* i p"),
    "smoltts_session_measure_duplicate": (INT, "p i i"),
    "smoltts_session_drop_graph": (INT, "p"),
    "smoltts_mimi_create": (INT, "MimiConfig* MimiWeights* p z p*"),
    "smoltts_mimi_destroy": (None, "p"),
    "smoltts_mimi_slab_bytes": (SIZE, "p i i"),
    "smoltts_mimi_session_create": (INT, "p p z i i p*"),
    "smoltts_mimi_session_destroy": (None, "p"),
    "smoltts_mimi_reset": (INT, "p p"),
    "smoltts_mimi_reset_slots": (INT, "p p i p"),
    "smoltts_mimi_session_set_option": (INT, "p i i"),
    "smoltts_mimi_decode_chunk": (INT, "p p q i i i i p q p"),
    "smoltts_mimi_encoder_create": (INT, "MimiEncConfig* MimiEncWeights* p z p*"),
    "smoltts_mimi_encoder_destroy": (None, "p"),
    "smoltts_mimi_encode_frames": (I32, "i"),
    "smoltts_mimi_encode_workspace_bytes": (SIZE, "p i"),
    "smoltts_mimi_encode_layout": (INT, "p i MimiEncLayout*"),
    "smoltts_mimi_encode": (INT, "p p i p p p p z p"),
    "smoltts_resample_design": (INT, "i p i i* i* i*"),
    "smoltts_resampler_bytes": (SIZE, "i"),
    "smoltts_resampler_create": (INT, "p z i p*"),
    "smoltts_resampler_destroy": (None, "p"),
    "smoltts_resampler_out_bytes": (SIZE, "i"),
    "smoltts_resampler_reset_slots": (INT, "p p p p i p"),
    "smoltts_resample_chunk": (INT, "p p q i i p p q p p"),
    "smoltts_tsm_bytes": (SIZE, "i"),
    "smoltts_tsm_create": (INT, "p z i p*"),
    "smoltts_tsm_destroy": (None, "p"),
    "smoltts_tsm_out_samples": (SIZE, "i"),
    "smoltts_tsm_reset_slots": (INT, "p p p i p"),
    "smoltts_tsm_chunk": (INT, "p p q i i p p p q p p"),
    "smoltts_tsm_slot_state": (INT, "p i p p"),
    "smoltts_flac_bytes": (SIZE, "i"),
    "smoltts_flac_create": (INT, "p z i p*"),
    "smoltts_flac_destroy": (None, "p"),
    "smoltts_flac_max_blocks": (I32, "i"),
    "smoltts_flac_out_bytes": (SIZE, "i"),
    "smoltts_flac_reset_slots": (INT, "p p p p i p"),
    "smoltts_flac_chunk": (INT, "p p q i p p q p i p p q p i p"),
    "smoltts_seam_bytes": (SIZE, "i"),
    "smoltts_seam_create": (INT, "p z i p*"),
    "smoltts_seam_destroy": (None, "p"),
    "smoltts_seam_out_samples": (SIZE, "i i"),
    "smoltts_seam_reset_slots": (INT, "p p p p p i p"),
    "smoltts_seam_chunk": (INT, "p p q i i p p p i p q p p"),
    "smoltts_seam_slot_state": (INT, "p i p p"),
    "smoltts_trim_bytes": (SIZE, "i"),
    "smoltts_trim_create": (INT, "p z i p*"),
    "smoltts_trim_destroy": (None, "p"),
    "smoltts_trim_out_samples": (SIZE, "i"),
    "smoltts_trim_reset_slots": (INT, "p p p p p p i p"),
    "smoltts_trim_chunk": (INT, "p p q i i p p p p q p p"),
    "smoltts_trim_slot_state": (INT, "p i p p"),
    "smoltts_loudness_bytes": (SIZE, "i"),
    "smoltts_loudness_table_doubles": (I32, ""),
    "smoltts_loudness_create": (INT, "p z i p i p*"),
    "smoltts_loudness_destroy": (None, "p"),
    "smoltts_loudness_reset_slots": (INT, "p p p p i p"),
    "smoltts_loudness_chunk": (INT, "p p q i i p p q p p"),
    "smoltts_loudness_measure": (INT, "p p i p q p p"),
    "smoltts_loudness_scale": (INT, "p q d p p"),
    "smoltts_loudness_slot_state": (INT, "p i p p p"),
    "smoltts_watermark_bytes": (SIZE, "i"),
    "smoltts_watermark_table_doubles": (I32, ""),
    "smoltts_watermark_create": (INT, "p z i p i p*"),
    "smoltts_watermark_destroy": (None, "p"),
    "smoltts_watermark_reset_slots": (INT, "p p p i p"),
    "smoltts_watermark_chunk": (INT, "p p q i i p p q p p"),
    "smoltts_watermark_embed": (INT, "p p i d p p"),
    "smoltts_watermark_slot_state": (INT, "p i p p p"),
    "smoltts_limiter_bytes": (SIZE, "i"),
    "smoltts_limiter_table_doubles": (I32, ""),
    "smoltts_limiter_create": (INT, "p z i p i p*"),
    "smoltts_limiter_destroy": (None, "p"),
    "smoltts_limiter_out_samples": (SIZE, "i"),
    "smoltts_limiter_reset_slots": (INT, "p p p i p"),
    "smoltts_limiter_chunk": (INT, "p p q i i p p p q p p"),
    "smoltts_limiter_apply": (INT, "p p i d p p p"),
    "smoltts_limiter_slot_state": (INT, "p i p p p"),
    "smoltts_align_fit_bytes": (SIZE, "i i i"),
    "smoltts_align_fit_create": (INT, "p z i i i p*"),
    "smoltts_align_fit_destroy": (None, "p"),
    "smoltts_align_fit_reset_slots": (INT, "p p p p p i p"),
    "smoltts_align_fit_push": (INT, "p p i i p p p"),
    "smoltts_align_fit_outputs": (INT, "p p* p* i*"),
    "smoltts_k_gemm": (INT, "GemmArgs* p"),
    "smoltts_gemm3_attn_fusable": (INT, "i i i"),
    "smoltts_k_gemm3": (INT, "Gemm3Args* p"),
    "smoltts_k_x3_pack": (INT, "p q i i p p p p p p"),
    "smoltts_k_attention": (INT, "p p p p p i i i i i p p p"),
    "smoltts_k_attention_kv": (INT, "p p p p p i i i i i p p i p"),
    "smoltts_k_attention_align": (INT, "p p i p p p p p p i i i i i i p p"),
    "smoltts_k_score_rows": (INT, "p i i q p p p"),
    "smoltts_k_attention_split": (INT, "p p p p p i i i i i p p i p p p"),
    "smoltts_k_attention_rows3": (INT, "p p p p p i i i i i p i p"),
    "smoltts_k_embed": (INT, "p i i p p i i i i i i p p"),
    "smoltts_k_argmax": (INT, "p i i q p i p p"),
    "smoltts_k_sample": (INT, "p i i q f f Q i i p p"),
    "smoltts_k_sample_rows": (INT, "p i i q p p i p p"),
    "smoltts_k_sample_rows_filtered": (INT, "p i i q p p p p p i p p"),
    "smoltts_k_sample_rows_length": (INT, "p i i q p p p p p p i i p p"),
    "smoltts_k_sample_rows_scored": (INT, "p i i q p p p p p p i i p p p"),
    "smoltts_k_layernorm": (INT, "p p p i i f p p"),
    "smoltts_k_seanet_resblock": (INT, "i i i p q p p p p p q i p"),
    "smoltts_k_seanet_last": (INT, "i i p q p p p p p p p f p q p i p"),
    "smoltts_k_rvq_upsample": (INT, "p q i i i i i p p p p p p"),
}
DEBUG_HOOKS = {  # diagnostic builds only (-DSMOLTTS_DEBUG_HOOKS); not in the header
    "smoltts_profile_begin": (INT, "i i i i"),
    "smoltts_profile_end": (INT, "f* i*"),
}


def _argtype(kind: str):
    if kind.endswith("*"):
        return C.POINTER(_KINDS.get(kind[:-1]) or globals()[kind[:-1]])
    return _KINDS[kind]


def _bind(lib, table) -> None:
    for name, (restype, kinds) in table.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, [_argtype(k) for k in kinds.split()]


def exported_symbols() -> List[str]:
    return list(SIGNATURES)


_lib = None


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
    _bind(lib, SIGNATURES)
    if hasattr(lib, "smoltts_profile_begin"):
        _bind(lib, DEBUG_HOOKS)
    if lib.smoltts_abi_version() != ABI_VERSION:
        raise SmolttsError("libsmoltts_hip.so ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load_library().smoltts_last_error().decode(errors="replace")
        raise SmolttsError(f"{what} failed ({status}): {msg}")
