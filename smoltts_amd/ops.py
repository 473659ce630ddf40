"""Operator-level wrappers over the ``smoltts_k_*`` C entry points (device tensors in/out).

These mirror the reference's building blocks one to one so the parity tests read like the
reference modules: ``linear`` = RMSNorm/ELU + nn.Linear + epilogue (modeling/model/rq_transformer.py
:535-613), ``attention`` = scaled_dot_product_attention over a KV cache, ``embed`` =
BaseTransformer.embed, ``argmax`` = greedy sampling, ``layernorm`` = nn.LayerNorm.
All of them run the HIP kernels; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import abi as E
from .abi import Gemm3Args, PickArgs, SlotFilters, SlotLength, SlotSampling
from .device import current_stream_ptr, dptr
from .packing import tile_t16x32, tile_w3


def _k(name: str, *args) -> None:
    """``name(*args, current stream)`` of the library, checked."""
    E.check(getattr(E.load_library(), name)(*args, current_stream_ptr()), name)


def pack_weight(w: torch.Tensor, fp32: bool = False) -> torch.Tensor:
    """Row-major [N, K] (CPU or GPU, any float dtype) -> T16x32 tiles on the current GPU."""
    flat = tile_t16x32(w.detach().float().cpu(), torch.float32 if fp32 else torch.bfloat16)
    return flat.cuda()


def pack_weight_w3(w: torch.Tensor) -> torch.Tensor:
    """Row-major fp32 [N, K] -> bf16x3 piece tiles ("W3", include/smoltts_hip.h) on the current GPU."""
    return tile_w3(w.detach().float().cpu()).view(torch.uint8).cuda()


def linear(x: torch.Tensor, w_tiles: torch.Tensor, N: int, *, w_fp32: bool = False, prologue: int = E.PRO_NONE,
           epilogue: int = E.EPI_STORE, gamma: Optional[torch.Tensor] = None, eps: float = 1e-5,
           bias: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
           resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           M: Optional[int] = None, K: Optional[int] = None, ldx: Optional[int] = None, x_bstride: int = 0,
           rows_per_batch: int = 0, ldo: Optional[int] = None, o_bstride: int = 0, ldr: int = 0, r_bstride: int = 0,
           rope: Optional[torch.Tensor] = None, row_pos: Optional[torch.Tensor] = None,
           row_slot: Optional[torch.Tensor] = None, k_cache: Optional[torch.Tensor] = None,
           v_cache: Optional[torch.Tensor] = None, n_q_heads: int = 0, n_kv_heads: int = 0, cache_len: int = 0,
           elu_out: bool = False, raw_out: Optional[torch.Tensor] = None, raw_bstride: int = 0,
           w3: Optional[torch.Tensor] = None, splitk_ws: Optional[torch.Tensor] = None,
           beta: Optional[torch.Tensor] = None, ln_scratch: Optional[torch.Tensor] = None,
           k_cache3: Optional[torch.Tensor] = None, v_cache3: Optional[torch.Tensor] = None, b3_products: int = 6) -> torch.Tensor:
    """``w3`` (``pack_weight_w3`` of the same fp32 matrix): many-row calls run the bf16x3-split kernel (gemm_b3.hip).
    ``k_cache3`` / ``v_cache3`` (``kv3_cache``): EPI_QKV_ROPE also writes the K / V rows as bf16x3 pieces (``attention_rows3``)."""
    M = x.shape[0] if M is None else M
    K = x.shape[1] if K is None else K
    out_cols = N // 2 if epilogue == E.EPI_SWIGLU else (n_q_heads * 64 if epilogue == E.EPI_QKV_ROPE else N)
    if out is None:
        out = torch.empty(M, out_cols, dtype=torch.float32, device=x.device)
    a = E.GemmArgs()
    a.w_dev, a.w_is_fp32, a.x_dev = dptr(w_tiles), int(w_fp32), dptr(x)
    a.ldx = x.stride(0) if ldx is None else ldx
    a.x_bstride, a.rows_per_batch, a.M, a.N, a.K = x_bstride, rows_per_batch, M, N, K
    a.prologue, a.epilogue, a.gamma_dev, a.eps = prologue, epilogue, dptr(gamma), eps
    a.bias_dev, a.scale_dev, a.resid_dev = dptr(bias), dptr(scale), dptr(resid)
    a.ldr, a.r_bstride = ldr, r_bstride
    a.out_dev = dptr(out)
    a.ldo = (out.stride(0) if out.dim() == 2 else out_cols) if ldo is None else ldo
    a.o_bstride = o_bstride
    a.elu_out, a.raw_out_dev, a.raw_bstride = int(elu_out), dptr(raw_out), raw_bstride
    a.rope_dev, a.row_pos_dev, a.row_slot_dev = dptr(rope), dptr(row_pos), dptr(row_slot)
    a.k_cache_dev, a.v_cache_dev = dptr(k_cache), dptr(v_cache)
    a.n_q_heads, a.n_kv_heads, a.cache_len = n_q_heads, n_kv_heads, cache_len
    a.w3_dev = dptr(w3)
    a.splitk_ws_dev, a.splitk_ws_floats = dptr(splitk_ws), (splitk_ws.numel() if splitk_ws is not None else 0)
    a.beta_dev, a.ln_scratch_dev = dptr(beta), dptr(ln_scratch)
    a.k_cache3_dev, a.v_cache3_dev = dptr(k_cache3), dptr(v_cache3)
    a.b3_products = b3_products
    _k("smoltts_k_gemm", C.byref(a))
    return out


def attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, row_pos: torch.Tensor,
              row_slot: torch.Tensor, n_q_heads: int, window: int = 0, out_x3: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [rows, Hq*64]; caches [slots, KV, cache_len, 64] fp32 or bf16; -> [rows, Hq*64] (and the X3 operand if given)."""
    n_kv, cache_len = k_cache.shape[1], k_cache.shape[2]
    assert k_cache.dtype == v_cache.dtype and k_cache.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty_like(q)
    _k("smoltts_k_attention_kv", dptr(q), dptr(k_cache), dptr(v_cache), dptr(row_pos), dptr(row_slot), q.shape[0], n_q_heads, n_kv,
       cache_len, window, dptr(out), dptr(out_x3), 1 if k_cache.dtype == torch.bfloat16 else 0)
    return out


def attention_align(q: torch.Tensor, k_cache: torch.Tensor, row_pos: torch.Tensor, row_slot: torch.Tensor, row_frame: torch.Tensor,
                    row_mask: torch.Tensor, windows: torch.Tensor, heads, n_q_heads: int, out: torch.Tensor) -> torch.Tensor:
    """Text mass and first moment of the query heads ``heads`` (``smoltts_k_attention_align``): q [rows, Hq*64]; k_cache
    [slots, KV, cache_len, 64] fp32 or bf16; row_pos / row_slot / row_frame / row_mask int32 [rows]; windows int32 [slots, 2];
    ``out`` float32 [slots, max_frames, len(heads), 2] is written in place (rows that write nothing keep what it held)."""
    heads = [int(h) for h in heads]
    slots, n_kv, cache_len = k_cache.shape[0], k_cache.shape[1], k_cache.shape[2]
    assert k_cache.dtype in (torch.float32, torch.bfloat16) and k_cache.is_contiguous() and q.is_contiguous()
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == slots and tuple(out.shape[2:]) == (len(heads), 2)
    assert windows.dtype == torch.int32 and tuple(windows.shape) == (slots, 2) and windows.is_contiguous()
    for t in (row_pos, row_slot, row_frame, row_mask):
        assert t.dtype == torch.int32 and t.numel() == q.shape[0]
    _k("smoltts_k_attention_align", dptr(q), dptr(k_cache), 1 if k_cache.dtype == torch.bfloat16 else 0, dptr(row_pos), dptr(row_slot),
       dptr(row_frame), dptr(row_mask), dptr(windows), (C.c_int32 * max(len(heads), 1))(*heads), len(heads), q.shape[0], n_q_heads, n_kv,
       cache_len, out.shape[1], dptr(out))
    return out


def score_rows(logits: torch.Tensor, targets: torch.Tensor, out: torch.Tensor, n_cols: Optional[int] = None) -> torch.Tensor:
    """The score of a given column per row (``smoltts_k_score_rows``; host model ``sampling.pick_logprob``): logits float32
    [rows, ld] of which the first ``n_cols`` columns (default all) are the row; targets int32 [rows]; ``out`` float32 [rows] is
    written in place (a row whose target lies outside [0, n_cols) keeps what it held)."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    assert targets.dtype == torch.int32 and out.dtype == torch.float32 and targets.numel() == out.numel() == logits.shape[0]
    assert targets.is_contiguous() and out.is_contiguous()
    _k("smoltts_k_score_rows", dptr(logits), logits.shape[0], logits.shape[1] if n_cols is None else int(n_cols), logits.stride(0),
       dptr(targets), dptr(out))
    return out


def kv3_cache(slots: int, n_heads: int, cache_len: int, device="cuda") -> torch.Tensor:
    """A zero-filled bf16x3 piece cache (include/smoltts_hip.h SMOLTTS_KV3_BYTES): uint8 [slots, heads, ceil32(cache_len) * 384]."""
    return torch.zeros(slots, n_heads, (cache_len + 31) // 32 * 32 * 384, dtype=torch.uint8, device=device)


def kv3_decode(cache3: torch.Tensor, cache_len: int, is_v: bool) -> torch.Tensor:
    """The fp32 values [slots, heads, cache_len, 64] a piece cache holds (hi + mid + lo, summed smallest first: exact) -- tests."""
    S, H = cache3.shape[0], cache3.shape[1]
    cl = (cache_len + 31) // 32 * 32
    raw = cache3.cpu().view(torch.bfloat16).float()  # [S, H, cl * 192]
    if not is_v:  # [tile][chunk][piece][lane = 16 q + r][8]: K[16 tile + r][32 chunk + 8 q + j]
        v = raw.view(S, H, cl // 16, 2, 3, 4, 16, 8)
        v = (v[:, :, :, :, 2] + v[:, :, :, :, 1]) + v[:, :, :, :, 0]  # [S, H, tile, chunk, q, r, j]
        return v.permute(0, 1, 2, 5, 3, 4, 6).reshape(S, H, cl, 64)[:, :, :cache_len].contiguous()
    v = raw.view(S, H, cl // 32, 4, 3, 4, 16, 8)  # [pb][dim tile][piece][q][r][j]: V[32 pb + (j < 4 ? 4q + j : 16 + 4q + j - 4)][16 t + r]
    v = (v[:, :, :, :, 2] + v[:, :, :, :, 1]) + v[:, :, :, :, 0]  # [S, H, pb, t, q, r, j]
    v = v.view(S, H, cl // 32, 4, 4, 16, 2, 4)  # j = 4 * half + jj -> position 16 half + 4 q + jj
    return v.permute(0, 1, 2, 6, 4, 7, 3, 5).reshape(S, H, cl, 64)[:, :, :cache_len].contiguous()


def kv3_encode(values: torch.Tensor, is_v: bool) -> torch.Tensor:
    """fp32 [slots, heads, cache_len, 64] -> the piece cache bytes (uint8 [slots, heads, ceil32(cache_len) * 384]); tests."""
    S, H, L, _ = values.shape
    cl = (L + 31) // 32 * 32
    x = torch.zeros(S, H, cl, 64)
    x[:, :, :L] = values.float().cpu()
    hi = x.bfloat16()
    r1 = x - hi.float()
    mid = r1.bfloat16()
    lo = (r1 - mid.float()).bfloat16()
    pieces = torch.stack([hi, mid, lo], 0)  # [3, S, H, cl, 64]
    if not is_v:  # -> [S, H, tile, chunk, piece, q, r, j]
        v = pieces.view(3, S, H, cl // 16, 16, 2, 4, 8).permute(1, 2, 3, 5, 0, 6, 4, 7)
    else:  # position = 32 pb + 16 half + 4 q + jj, dim = 16 t + r -> [S, H, pb, t, piece, q, r, half, jj]
        v = pieces.view(3, S, H, cl // 32, 2, 4, 4, 4, 16).permute(1, 2, 3, 7, 0, 5, 8, 4, 6)
    return v.contiguous().view(torch.uint8).reshape(S, H, cl * 384)


def attention_rows3(q: torch.Tensor, k_cache3: torch.Tensor, v_cache3: torch.Tensor, row_pos: torch.Tensor, row_slot: torch.Tensor,
                    rows_per_slot: int, n_heads: int, cache_len: int, window: int = 0, b3_products: int = 6) -> torch.Tensor:
    """Attention of ``rows_per_slot`` (a multiple of 32) consecutive positions per slot over bf16x3 piece caches (attn_rows3_kernel).
    ``b3_products`` = 3: three products per operand pair (the 2^-16-grade form of a codec session with ``products=3``)."""
    out = torch.empty_like(q)
    _k("smoltts_k_attention_rows3", dptr(q), dptr(k_cache3), dptr(v_cache3), dptr(row_pos), dptr(row_slot), q.shape[0], rows_per_slot,
       n_heads, cache_len, window, dptr(out), b3_products)
    return out


SPLIT_PART_FLOATS, SPLIT_TICKETS = 128 * 2 * (4 * 64 + 8), 128  # csrc/common.h ATT_SPLIT_*


def attention_split(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, row_pos: torch.Tensor, row_slot: torch.Tensor,
                    n_q_heads: int, scratch, window: int = 0, out_x3: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``attention`` with the keys of every (row, kv head) pair on two workgroups (rows x kv heads <= 128, cache_len > 128).
    ``scratch`` = (part fp32 [SPLIT_PART_FLOATS], ticket int32 [SPLIT_TICKETS] zeroed once and then left alone)."""
    n_kv, cache_len = k_cache.shape[1], k_cache.shape[2]
    part, ticket = scratch
    assert part.numel() >= SPLIT_PART_FLOATS and ticket.numel() >= SPLIT_TICKETS and ticket.dtype == torch.int32
    out = torch.empty_like(q)
    _k("smoltts_k_attention_split", dptr(q), dptr(k_cache), dptr(v_cache), dptr(row_pos), dptr(row_slot), q.shape[0], n_q_heads, n_kv,
       cache_len, window, dptr(out), dptr(out_x3), 1 if k_cache.dtype == torch.bfloat16 else 0, dptr(part), dptr(ticket))
    return out


def embed(cols: torch.Tensor, text_emb: torch.Tensor, cb_emb: torch.Tensor, codebook_size: int, cb_first_offset: int = 0,
          mask_mode: int = 0, sem_start: int = 320, sem_end: int = 2367) -> torch.Tensor:
    """cols int32 [rows, 1+n]; bf16 tables; -> fp32 [rows, dim]."""
    rows, dim = cols.shape[0], text_emb.shape[1]
    x = torch.empty(rows, dim, dtype=torch.float32, device=cols.device)
    _k("smoltts_k_embed", dptr(cols), rows, cols.shape[1] - 1, dptr(text_emb), dptr(cb_emb), dim, codebook_size, cb_first_offset,
       mask_mode, sem_start, sem_end, dptr(x))
    return x


def argmax(logits: torch.Tensor, margin: Optional[torch.Tensor] = None) -> torch.Tensor:
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    _k("smoltts_k_argmax", dptr(logits), logits.shape[0], logits.shape[1], logits.stride(0), dptr(ids), 1, dptr(margin))
    return ids


def slot_sampling_table(temp, fast_temp, min_p, seed, device="cuda") -> torch.Tensor:
    """Rows of ``SmolttsSlotSampling`` (temp, fast_temp, min_p, 0, seed: 24 bytes each) as a uint8 device tensor."""
    import numpy as np

    a = np.zeros(len(temp), np.dtype(SlotSampling))
    a["temp"], a["fast_temp"], a["min_p"] = temp, fast_temp, min_p
    a["seed"] = np.array([int(x) & (2**64 - 1) for x in seed], dtype=np.uint64)
    return torch.from_numpy(a.view(np.uint8).copy()).to(device)


def sample_rows(logits: torch.Tensor, table: torch.Tensor, frames: Optional[torch.Tensor] = None, step: int = 0) -> torch.Tensor:
    """``smoltts_k_sample_rows``: row r picked with its own entry ``table`` row r (``slot_sampling_table``) and the request key at
    frame ``frames[r]`` (None: r) and ``step`` (0: the entry's temp; > 0: fast_temp)."""
    if table.dtype != torch.uint8 or table.numel() < C.sizeof(SlotSampling) * logits.shape[0]:
        raise ValueError("table: 24 bytes per row (slot_sampling_table)")
    if frames is not None and (frames.dtype != torch.int32 or frames.numel() < logits.shape[0]):
        raise ValueError("frames: int32, one per row")
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    _k("smoltts_k_sample_rows", dptr(logits), logits.shape[0], logits.shape[1], logits.stride(0), dptr(table), dptr(frames), int(step),
       dptr(ids))
    return ids


def slot_filter_table(top_p, top_k, penalty, window, device="cuda") -> torch.Tensor:
    """Rows of ``SmolttsSlotFilters`` (top_p, top_k, penalty, fp32(1 / penalty), window, 0, 0, 0: 32 bytes each) as a uint8 device
    tensor, normalised as ``smoltts_session_set_slot_filters`` does (top_p >= 1 -> 0; penalty <= 1 or window 0 -> all three 0)."""
    import numpy as np

    a = np.zeros(len(top_p), np.dtype(SlotFilters))
    tp = np.asarray(top_p, np.float32)
    a["top_p"] = np.where(tp < 1, tp, 0)
    a["top_k"] = top_k
    r, w = np.asarray(penalty, np.float32), np.asarray(window, np.int32)
    on = (r > 1) & (w > 0)
    a["penalty"] = np.where(on, r, 0)
    a["inv_penalty"] = np.where(on, np.float32(1.0) / np.where(on, r, np.float32(1.0)), 0).astype(np.float32)
    a["window"] = np.where(on, w, 0)
    return torch.from_numpy(a.view(np.uint8).copy()).to(device)


def sample_rows_filtered(logits: torch.Tensor, table: torch.Tensor, filters: torch.Tensor, history: torch.Tensor, history_len: torch.Tensor,
                         frames: Optional[torch.Tensor] = None, step: int = 0) -> torch.Tensor:
    """``smoltts_k_sample_rows_filtered``: ``sample_rows`` with row r's filters ``filters`` row r (``slot_filter_table``) and its
    explicit history: the first ``min(history_len[r], window)`` ids of ``history[r]`` (int32 [rows, 64], newest first)."""
    R = logits.shape[0]
    if table.dtype != torch.uint8 or table.numel() < C.sizeof(SlotSampling) * R:
        raise ValueError("table: 24 bytes per row (slot_sampling_table)")
    if filters.dtype != torch.uint8 or filters.numel() < C.sizeof(SlotFilters) * R:
        raise ValueError("filters: 32 bytes per row (slot_filter_table)")
    if history.dtype != torch.int32 or tuple(history.shape) != (R, 64) or not history.is_contiguous():
        raise ValueError("history: contiguous int32 [rows, 64]")
    if history_len.dtype != torch.int32 or history_len.numel() < R:
        raise ValueError("history_len: int32, one per row")
    if frames is not None and (frames.dtype != torch.int32 or frames.numel() < R):
        raise ValueError("frames: int32, one per row")
    ids = torch.empty(R, dtype=torch.int32, device=logits.device)
    _k("smoltts_k_sample_rows_filtered", dptr(logits), R, logits.shape[1], logits.stride(0), dptr(table), dptr(filters), dptr(frames),
       dptr(history), dptr(history_len), int(step), dptr(ids))
    return ids


def slot_length_table(min_frames, eos_bias, device="cuda") -> torch.Tensor:
    """Rows of ``SmolttsSlotLength`` (min_frames, eos_bias, 0, 0: 16 bytes each) as a uint8 device tensor."""
    import numpy as np

    a = np.zeros(len(min_frames), np.dtype(SlotLength))
    a["min_frames"] = np.asarray(min_frames, np.int32)
    a["eos_bias"] = np.asarray(eos_bias, np.float32)
    return torch.from_numpy(a.view(np.uint8).copy()).to(device)


def sample_rows_length(logits: torch.Tensor, table: torch.Tensor, length: torch.Tensor, im_end: int, frames: Optional[torch.Tensor] = None,
                       step: int = 0, filters: Optional[torch.Tensor] = None, history: Optional[torch.Tensor] = None,
                       history_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``smoltts_k_sample_rows_length``: ``sample_rows`` (``filters`` None) or ``sample_rows_filtered`` with row r's length entry
    ``length`` row r (``slot_length_table``) acting on column ``im_end`` at step 0, the row's frame counter being ``frames[r]``
    (None: r) -- the pick of ``sampling.length_patch`` of the row."""
    R = logits.shape[0]
    if table.dtype != torch.uint8 or table.numel() < C.sizeof(SlotSampling) * R:
        raise ValueError("table: 24 bytes per row (slot_sampling_table)")
    if length.dtype != torch.uint8 or length.numel() < C.sizeof(SlotLength) * R:
        raise ValueError("length: 16 bytes per row (slot_length_table)")
    if not 0 <= int(im_end) < logits.shape[1]:
        raise ValueError("im_end: a column of the row")
    if frames is not None and (frames.dtype != torch.int32 or frames.numel() < R):
        raise ValueError("frames: int32, one per row")
    if filters is not None:
        if filters.dtype != torch.uint8 or filters.numel() < C.sizeof(SlotFilters) * R:
            raise ValueError("filters: 32 bytes per row (slot_filter_table)")
        if history is None or history.dtype != torch.int32 or tuple(history.shape) != (R, 64) or not history.is_contiguous():
            raise ValueError("history: contiguous int32 [rows, 64]")
        if history_len is None or history_len.dtype != torch.int32 or history_len.numel() < R:
            raise ValueError("history_len: int32, one per row")
    ids = torch.empty(R, dtype=torch.int32, device=logits.device)
    _k("smoltts_k_sample_rows_length", dptr(logits), R, logits.shape[1], logits.stride(0), dptr(table), dptr(filters), dptr(frames),
       dptr(history if filters is not None else None), dptr(history_len if filters is not None else None), dptr(length), int(im_end),
       int(step), dptr(ids))
    return ids


def sample_rows_scored(logits: torch.Tensor, table: torch.Tensor, length: Optional[torch.Tensor] = None, im_end: int = 0,
                       frames: Optional[torch.Tensor] = None, step: int = 0, filters: Optional[torch.Tensor] = None,
                       history: Optional[torch.Tensor] = None, history_len: Optional[torch.Tensor] = None):
    """``smoltts_k_sample_rows_scored``: the ids of ``sample_rows_length`` on the same arguments (``length`` None: of
    ``sample_rows`` / ``sample_rows_filtered``) and, per row, the fp32 log-probability at temperature 1 of that id under the row
    its pick saw (``sampling.pick_logprob``) -> ``(ids, logprobs)``."""
    R = logits.shape[0]
    if table.dtype != torch.uint8 or table.numel() < C.sizeof(SlotSampling) * R:
        raise ValueError("table: 24 bytes per row (slot_sampling_table)")
    if length is not None:
        if length.dtype != torch.uint8 or length.numel() < C.sizeof(SlotLength) * R:
            raise ValueError("length: 16 bytes per row (slot_length_table)")
        if not 0 <= int(im_end) < logits.shape[1]:
            raise ValueError("im_end: a column of the row")
    if frames is not None and (frames.dtype != torch.int32 or frames.numel() < R):
        raise ValueError("frames: int32, one per row")
    if filters is not None:
        if filters.dtype != torch.uint8 or filters.numel() < C.sizeof(SlotFilters) * R:
            raise ValueError("filters: 32 bytes per row (slot_filter_table)")
        if history is None or history.dtype != torch.int32 or tuple(history.shape) != (R, 64) or not history.is_contiguous():
            raise ValueError("history: contiguous int32 [rows, 64]")
        if history_len is None or history_len.dtype != torch.int32 or history_len.numel() < R:
            raise ValueError("history_len: int32, one per row")
    ids = torch.empty(R, dtype=torch.int32, device=logits.device)
    lp = torch.empty(R, dtype=torch.float32, device=logits.device)
    _k("smoltts_k_sample_rows_scored", dptr(logits), R, logits.shape[1], logits.stride(0), dptr(table), dptr(filters), dptr(frames),
       dptr(history if filters is not None else None), dptr(history_len if filters is not None else None), dptr(length), int(im_end),
       int(step), dptr(ids), dptr(lp))
    return ids, lp


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    out = torch.empty_like(x)
    _k("smoltts_k_layernorm", dptr(x), dptr(w), dptr(b), x.shape[0], x.shape[1], eps, dptr(out))
    return out


# ------------------------------------------------------------------------------- fused stages of the Mimi decoder
def seanet_resblock(xbuf: torch.Tensor, T: int, w2_w3: torch.Tensor, b2: torch.Tensor, w3_w3: torch.Tensor, b3: torch.Tensor,
                    out: torch.Tensor, out_lead: int = 0, b3_products: int = 6) -> torch.Tensor:
    """``smoltts_k_seanet_resblock`` (csrc/seanet.hip): ``xbuf`` fp32 [slots, 2 + rows, C] holds two halo rows, then the raw block
    input (rows >= T; only [0, T) are read); ELU(x + conv_k1(ELU(conv_k3(ELU(x))))) of those T rows goes to
    ``out[:, out_lead : out_lead + T]`` (fp32 [slots, out_lead + rows', C]).  ``w2_w3`` / ``w3_w3``: ``pack_weight_w3`` of the
    ``conv_as_gemm`` matrices [C/2, 3C] and [C, C/2]."""
    S, rows, Cn = xbuf.shape
    assert xbuf.dtype == out.dtype == torch.float32 and xbuf.stride(2) == 1 and xbuf.stride(1) == Cn and out.stride(2) == 1 and out.stride(1) == Cn
    assert out.shape[0] == S and out.shape[2] == Cn and 0 < T <= rows - 2 and out_lead + T <= out.shape[1]
    _k("smoltts_k_seanet_resblock", Cn, S, T, xbuf.data_ptr() + 4 * 2 * Cn, xbuf.stride(0), dptr(w2_w3), dptr(b2), dptr(w3_w3), dptr(b3),
       out.data_ptr() + 4 * out_lead * Cn, out.stride(0), b3_products)
    return out


def seanet_last(inbuf: torch.Tensor, T: int, wt_w3: torch.Tensor, bt: torch.Tensor, w2_w3: torch.Tensor, b2: torch.Tensor,
                w3_w3: torch.Tensor, b3: torch.Tensor, final_w: torch.Tensor, final_b: float, slot_pos: torch.Tensor, pcm: torch.Tensor,
                b3_products: int = 6) -> torch.Tensor:
    """``smoltts_k_seanet_last`` (csrc/seanet_last.hip): ``inbuf`` fp32 [slots, 2 + rows, 128] = two halo rows, then ELU(stage-3
    output); the 4 T samples of every slot go to ``pcm[:, : 4 T]`` (fp32 [slots, >= 4 T]).  ``slot_pos`` int32 [slots]: 0 = the slot's
    stream starts with this call (its halo rows must be zero).  Weights: ``pack_weight_w3`` of ``conv_as_gemm`` of the ConvTranspose
    ([256, 256], bias repeated: [256]) and of the block's convs ([32, 192], [64, 32]); ``final_w`` fp32 [3 * 64] tap-major."""
    S, rows, Cn = inbuf.shape
    assert inbuf.dtype == pcm.dtype == torch.float32 and Cn == 128 and inbuf.stride(2) == 1 and inbuf.stride(1) == Cn and pcm.stride(1) == 1
    assert pcm.shape[0] == S and 0 < T <= rows - 2 and 4 * T <= pcm.shape[1] and slot_pos.dtype == torch.int32 and slot_pos.numel() >= S
    assert bt.numel() == 256 and final_w.numel() == 192
    _k("smoltts_k_seanet_last", S, T, inbuf.data_ptr() + 4 * 2 * Cn, inbuf.stride(0), dptr(wt_w3), dptr(bt), dptr(w2_w3), dptr(b2),
       dptr(w3_w3), dptr(b3), dptr(final_w), float(final_b), dptr(pcm), pcm.stride(0), dptr(slot_pos), b3_products)
    return pcm


def rvq_upsample(codes: torch.Tensor, f0: int, n_frames: int, nq: int, table: torch.Tensor, upw: torch.Tensor,
                 carry_in: Optional[torch.Tensor], carry_out: torch.Tensor, code_offset: int = 0) -> torch.Tensor:
    """``smoltts_k_rvq_upsample`` (csrc/mimi_engine.hip): frames [f0, f0 + n_frames) of ``codes`` (int32 [slots, F, row], row >=
    code_offset + nq) -> the decoder transformer's input rows fp32 [slots, 2 n_frames, 512].  ``table`` fp32 [nq, 2048, 512] (codebooks
    with the output projection folded in), ``upw`` fp32 [4, 512]; ``carry_in`` [slots, 512] = the embedding of frame f0 - 1 (None: no
    predecessor), ``carry_out`` receives that of the call's last frame."""
    S, F, row = codes.shape
    assert codes.dtype == torch.int32 and codes.is_contiguous() and 0 <= f0 and n_frames > 0 and f0 + n_frames <= F
    assert tuple(table.shape) == (nq, 2048, 512) and table.is_contiguous() and tuple(upw.shape) == (4, 512) and upw.is_contiguous()
    assert carry_out.numel() >= S * 512 and (carry_in is None or carry_in.numel() >= S * 512)
    tx = torch.empty(S, 2 * n_frames, 512, dtype=torch.float32, device=codes.device)
    _k("smoltts_k_rvq_upsample", codes.data_ptr() + 4 * f0 * row, F * row, row, code_offset, nq, S, n_frames, dptr(table), dptr(upw),
       dptr(carry_in), dptr(carry_out), dptr(tx))
    return tx


# ------------------------------------------------------------------------------- X3 / bf16-MFMA path
def x3_bytes(rows: int, K: int) -> int:
    return (rows + 15) // 16 * 16 * K * 6


def x3_alloc(rows: int, K: int) -> torch.Tensor:
    return torch.zeros(x3_bytes(rows, K), dtype=torch.uint8, device="cuda")


def x3_to_float(buf: torch.Tensor, rows: int, K: int) -> torch.Tensor:
    """Decode an X3 operand buffer back to fp32 [rows, K] on the CPU (tests): hi + mid + lo."""
    R16 = (rows + 15) // 16 * 16
    t = buf.cpu()[: R16 * K * 6].view(torch.bfloat16).view(R16 // 16, K // 32, 3, 4, 16, 8)  # tile, chunk, piece, q, r, j
    f = t.float().sum(dim=2)  # tile, chunk, q, r, j  (exact: the pieces do not overlap)
    return f.permute(0, 3, 1, 2, 4).reshape(R16, K)[:rows].contiguous()


def x3_pack(x: torch.Tensor, gamma_a: Optional[torch.Tensor] = None, gamma_b: Optional[torch.Tensor] = None,
            two: bool = False):
    """fp32 rows on the GPU -> (X3 of x*gamma_a, X3 of x*gamma_b or None, ssq [rows, K/16])."""
    rows, K = x.shape
    a = x3_alloc(rows, K)
    b = x3_alloc(rows, K) if two else None
    ssq = torch.zeros(rows, K // 16, dtype=torch.float32, device=x.device)
    _k("smoltts_k_x3_pack", dptr(x), x.stride(0), rows, K, dptr(a), dptr(gamma_a), dptr(b), dptr(gamma_b), dptr(ssq))
    return a, b, ssq


@dataclass
class Pick:
    """The previous depth step's greedy pick in front of ``linear3``'s attention prologue (``SmolttsPickArgs``).
    ``cand`` [M][tiles][4] from the head GEMM's ``cand_out``; ``table`` fp32 [rows][(Hq + 2 KV) * 64] (q | k | v before RoPE);
    ``rope`` fp32 [pos][32][2]; ``emb`` bf16 [rows][K]; row = id + ``emb_row_offset``; ids land in ``ids[r * ids_stride]``;
    ``margin`` / ``margin_mask`` / ``margin_at`` / ``frames`` / ``step``: the top-2 gap records of ``argmax``."""
    cand: torch.Tensor
    table: torch.Tensor
    rope: torch.Tensor
    emb: torch.Tensor
    ids: torch.Tensor
    ids_stride: int = 1
    emb_row_offset: int = 0
    margin: Optional[torch.Tensor] = None
    margin_mask: Optional[torch.Tensor] = None
    margin_at: Optional[torch.Tensor] = None
    frames: Optional[torch.Tensor] = None
    step: int = 0

    def args(self) -> PickArgs:
        k = PickArgs()
        k.cand_dev, k.cand_tiles = dptr(self.cand), self.cand.shape[1]
        k.qkv_table_dev, k.rope_dev, k.emb_dev, k.emb_row_offset = dptr(self.table), dptr(self.rope), dptr(self.emb), self.emb_row_offset
        k.ids_dev, k.ids_stride = dptr(self.ids), self.ids_stride
        k.margin_dev, k.margin_mask_dev = dptr(self.margin), dptr(self.margin_mask)
        k.margin_at_dev, k.frames_dev, k.step = dptr(self.margin_at), dptr(self.frames), self.step
        return k


def pack_weight_fp8(w: torch.Tensor):
    """Row-major [N, K] -> (e4m3 T16x32 tiles, fp32 row scales) on the current GPU, and the dequantised matrix."""
    from .packing import quantize_fp8_rows

    q, scale = quantize_fp8_rows(w.detach().float().cpu())
    return tile_t16x32(q, torch.float8_e4m3fn).view(torch.uint8).cuda(), scale.cuda(), q.float() * scale[:, None]


def linear3(x3: torch.Tensor, w_tiles: torch.Tensor, M: int, N: int, K: int, *, epilogue: int = E.EPI_STORE,
            ssq_in: Optional[torch.Tensor] = None, eps: float = 1e-5, bias: Optional[torch.Tensor] = None,
            resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, x3_out: Optional[torch.Tensor] = None,
            emit_a: Optional[torch.Tensor] = None, gamma_a: Optional[torch.Tensor] = None,
            emit_b: Optional[torch.Tensor] = None, gamma_b: Optional[torch.Tensor] = None,
            ssq_out: Optional[torch.Tensor] = None, rope=None, row_pos=None, row_slot=None, k_cache=None, v_cache=None,
            n_q_heads: int = 0, n_kv_heads: int = 0, cache_len: int = 0, w_scale: Optional[torch.Tensor] = None,
            v_x3: Optional[torch.Tensor] = None, kv_format: int = 0, w_stream: bool = False,
            attn_q: Optional[torch.Tensor] = None, attn_pos: int = 0, cand_out: Optional[torch.Tensor] = None,
            fp8_activations: bool = False, pick: Optional[Pick] = None):
    """The bf16-MFMA GEMM over an X3 operand; returns the fp32 ``out`` tensor (None for SWIGLU).
    ``w_scale`` given: ``w_tiles`` are e4m3 tiles (``pack_weight_fp8``).
    ``attn_q`` given (EPI_RESID): ``x3`` may be None -- the operand is the attention of ``attn_q`` over keys 0..``attn_pos`` of
    ``k_cache`` / ``v_cache`` (row r = slot r), worked out inside the launch (attn_wo_kernel).
    ``pick`` given (EPI_RESID, ``attn_pos`` >= 1): ``attn_q`` and ``resid`` are not read -- each row's q, newest K / V and residual
    come from the table / embedding rows of its picked id (``Pick``), and the new K / V rows are written to the caches."""
    if out is None and epilogue != E.EPI_SWIGLU:
        cols = n_q_heads * 64 if epilogue == E.EPI_QKV_ROPE else N
        out = torch.zeros(M, cols, dtype=torch.float32, device=w_tiles.device)
    a = Gemm3Args()
    a.w_dev, a.x3_dev, a.M, a.N, a.K, a.epilogue = dptr(w_tiles), dptr(x3), M, N, K, epilogue
    a.ssq_in_dev, a.eps, a.bias_dev, a.resid_dev = dptr(ssq_in), eps, dptr(bias), dptr(resid)
    a.out_dev = dptr(out)
    a.ldo = out.stride(0) if out is not None else 0
    a.x3_out_dev = dptr(x3_out)
    a.emit_a_dev, a.gamma_a_dev, a.emit_b_dev, a.gamma_b_dev = dptr(emit_a), dptr(gamma_a), dptr(emit_b), dptr(gamma_b)
    a.ssq_out_dev = dptr(ssq_out)
    a.rope_dev, a.row_pos_dev, a.row_slot_dev = dptr(rope), dptr(row_pos), dptr(row_slot)
    a.k_cache_dev, a.v_cache_dev = dptr(k_cache), dptr(v_cache)
    a.n_q_heads, a.n_kv_heads, a.cache_len = n_q_heads, n_kv_heads, cache_len
    a.w_format, a.w_scale_dev = (1, dptr(w_scale)) if w_scale is not None else (0, None)
    a.v_x3_dev = dptr(v_x3)
    a.kv_format = int(kv_format)
    a.w_stream = 1 if w_stream else 0
    a.attn_q_dev, a.attn_pos = dptr(attn_q), int(attn_pos)
    a.fp8_activations = 1 if fp8_activations else 0  # fp8 weights, M >= 256: fp8 x fp8 MFMA on the activation's hi piece (not the parity path)
    a.cand_out_dev = dptr(cand_out)  # EPI_STORE: per (row, 16-column tile) (max, first column of it as int bits, runner-up, -)
    pk = pick.args() if pick is not None else None  # (kept alive across the call)
    a.pick = C.pointer(pk) if pk is not None else None
    _k("smoltts_k_gemm3", C.byref(a))
    return out
