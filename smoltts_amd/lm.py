"""The DualAR language model behind the C ABI: ``LMEngine`` (weights), ``LMSession`` (slots, KV caches, the frame loop) and
``PrefixKV`` (a saved prompt prefix)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import packing
from .abi import (KV_FORMATS, MAX_ALIGN_HEADS, OPT_COMMIT_PICKS, OPT_FP8_PREFILL, OPT_FUSE_DEPTH_ATTN, OPT_FUSE_PICK, OPT_QKV_TABLE, OPT_SPLIT_ATTN,
                  OPT_STREAM_W, BlockWeights, LMConfig, LMWeights, PrefixHeader, SmolttsError, check, load_library)
from .config import NumericsMode, RQTransformerModelArgs, TokenConfig
from .device import ClosesOnDel, _alloc_slab, _require_gpu, current_stream_ptr, dptr, upload, upload_stream


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


class LMEngine(ClosesOnDel):
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


class LMSession(ClosesOnDel):
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
        self.length_slots = set()  # slots whose length entry on the device is on (set_slot_length)
        self.scored_slots = set()  # slots whose slow token is scored (set_slot_score)
        self.align_slots = set()  # slots whose alignment window is on (set_slot_align)
        self.align_pairs, self.alignment, self._align_buf = [], None, None  # set_align_heads
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
        lp, stride = C.c_void_p(), C.c_int32()
        check(self.lib.smoltts_session_logprobs(h, C.byref(lp), C.byref(stride)), "smoltts_session_logprobs")
        # [slot][frame]: log-probability of each emitted slow id, written while some slot scores (set_slot_score)
        self.logprobs = view(lp, self.B * stride.value * 4, torch.float32, (self.B, stride.value))
        sl, ld = C.c_void_p(), C.c_int32()
        check(self.lib.smoltts_session_slow_logits(h, C.byref(sl), C.byref(ld)), "smoltts_session_slow_logits")
        self.slow_logits = view(sl, self.B * ld.value * 4, torch.float32, (self.B, ld.value))  # the latest frame's (diagnostic)
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

    def _set_slot_table(self, fn: str, slots: Sequence[int], columns: Sequence[Tuple[type, Callable, Sequence]], mismatch: str,
                        stream: bool = True) -> None:
        """One per-slot table call of the C library: the slot list, its length, one array per ``(ctype, convert, values)`` column and
        (``stream``) the current stream.  ``mismatch``: the ``ValueError`` of lists that are not one value per slot."""
        n = len(slots)
        if any(len(values) != n for _, _, values in columns):
            raise ValueError(mismatch)
        arrays = [(ctype * max(n, 1))(*[convert(x) for x in values]) for ctype, convert, values in [(C.c_int32, int, slots), *columns]]
        check(getattr(self.lib, fn)(self.handle, arrays[0], n, *arrays[1:], *([current_stream_ptr()] if stream else [])), fn)

    def set_slot_sampling(self, slots: Sequence[int], temp: Sequence[float], fast_temp: Sequence[float], min_p: Sequence[float],
                          seed: Sequence[int]) -> None:
        """Per-slot sampling (slot mode, include/smoltts_hip.h): slot ``slots[i]`` samples its slow token at ``temp[i]`` and its
        depth codes at ``fast_temp[i]`` (<= 0: greedy) with the effective cut ``min_p[i]`` and the request key of ``seed[i]``.  The
        first call puts the session in slot mode for good (unlisted slots: greedy).  Queued on the current stream: the picks
        behind it on that stream use the new entries; the host does not wait for the stream."""
        self._set_slot_table("smoltts_session_set_slot_sampling", slots,
                             [(C.c_float, float, temp), (C.c_float, float, fast_temp), (C.c_float, float, min_p),
                              (C.c_uint64, lambda x: int(x) & (2**64 - 1), seed)], "slot sampling: one value per slot in every list")

    def set_slot_filters(self, slots: Sequence[int], top_p: Sequence[float], top_k: Sequence[int], penalty: Sequence[float],
                         window: Sequence[int]) -> None:
        """Per-slot filters of the sampled picks (``smoltts_session_set_slot_filters``): slot ``slots[i]`` keeps its ``top_k[i]``
        largest logits (0: off), then the ``top_p[i]`` nucleus (0 or 1: off), after the repetition penalty ``penalty[i]`` (0 or
        1: off) over the ids of its last ``window[i]`` frames.  Queued on the current stream like ``set_slot_sampling``."""
        self._set_slot_table("smoltts_session_set_slot_filters", slots,
                             [(C.c_float, float, top_p), (C.c_int32, int, top_k), (C.c_float, float, penalty), (C.c_int32, int, window)],
                             "slot filters: one value per slot in every list")
        for b, p, k, r, w in zip(slots, top_p, top_k, penalty, window):
            (self.filtered_slots.add if (0 < p < 1 or k > 0 or (r > 1 and w > 0)) else self.filtered_slots.discard)(int(b))

    def set_slot_length(self, slots: Sequence[int], min_frames: Sequence[int], eos_bias: Sequence[float]) -> None:
        """Per-slot length control of the slow pick (``smoltts_session_set_slot_length``): while slot ``slots[i]`` has emitted fewer
        than ``min_frames[i]`` frames its ``<|im_end|>`` column cannot be picked (0: off), and ``eos_bias[i]`` is added to that
        logit (0: off) -- for greedy and sampled slow tokens alike (``sampling.length_patch``).  Queued on the current stream like
        ``set_slot_sampling``; a new tenant without the option needs an off entry, or it inherits its predecessor's."""
        self._set_slot_table("smoltts_session_set_slot_length", slots, [(C.c_int32, int, min_frames), (C.c_float, float, eos_bias)],
                             "slot length: one value per slot in every list")
        for b, m, x in zip(slots, min_frames, eos_bias):
            (self.length_slots.add if (m > 0 or x != 0) else self.length_slots.discard)(int(b))

    def set_slot_score(self, slots: Sequence[int], on: Sequence[bool]) -> None:
        """Score the slow token of slot ``slots[i]`` where ``on[i]`` (``smoltts_session_set_slot_score``): ``logprobs[slot][f]`` then
        receives, with frame f, the log-probability at temperature 1 of the id the slot emitted (``sampling.pick_logprob``).  Host
        flags only; a new tenant without the option needs an off flag, or the session keeps scoring for nobody."""
        self._set_slot_table("smoltts_session_set_slot_score", slots, [(C.c_int32, lambda x: 1 if x else 0, on)],
                             "slot score: one flag per slot", stream=False)
        for b, x in zip(slots, on):
            (self.scored_slots.add if x else self.scored_slots.discard)(int(b))

    def fetch_logprobs(self) -> np.ndarray:
        """Host copy of ``logprobs`` ([max_batch, max_frames] float32); an entry means something for a frame its slot emitted
        while some slot scored.  Waits for the current stream."""
        return self.logprobs.cpu().numpy()

    # ---- where chosen heads of the slow attention look (include/smoltts_hip.h at smoltts_session_set_align_heads)
    def set_align_heads(self, pairs: Sequence) -> None:
        """Choose the (layer, head) pairs whose text mass and first moment the decode frames measure (at most ``MAX_ALIGN_HEADS``;
        sorted by layer here; empty: off).  The rows live in a buffer of their own, not in the session slab.  Waits for the device."""
        pairs = sorted((int(l), int(h)) for l, h in pairs)
        n = len(pairs)
        if n > MAX_ALIGN_HEADS:
            raise ValueError(f"at most {MAX_ALIGN_HEADS} alignment heads, got {n}")
        torch.cuda.current_stream().synchronize()  # (frames in flight may still write the buffer this call replaces)
        need = self.lib.smoltts_session_align_bytes(self.handle, n) if n else 0
        buf = _alloc_slab(need, self.engine.device, settle=True) if n else None  # (the C call zeroes its table on the null stream)
        check(self.lib.smoltts_session_set_align_heads(
            self.handle, (C.c_int32 * max(n, 1))(*[p[0] for p in pairs]), (C.c_int32 * max(n, 1))(*[p[1] for p in pairs]), n,
            dptr(buf), need), "smoltts_session_set_align_heads")
        self.align_pairs, self._align_buf = pairs, buf
        self.align_slots = set()
        self.alignment = None
        if n:
            p, k = C.c_void_p(), C.c_int32()
            check(self.lib.smoltts_session_alignment(self.handle, C.byref(p), C.byref(k)), "smoltts_session_alignment")
            o = p.value - buf.data_ptr()
            # [slot][frame][pair] = (m, s1); m = -1: not measured
            self.alignment = buf[o: o + self.B * self.max_frames * n * 8].view(torch.float32).view(self.B, self.max_frames, n, 2)

    def set_slot_align(self, slots: Sequence[int], t0: Sequence[int], t1: Sequence[int]) -> None:
        """The text window ``[t0[i], t1[i])`` (prompt positions) of slot ``slots[i]``; ``t1 <= t0`` switches its measurement off.
        The slot's rows are reset to "not measured".  Queued on the current stream like ``set_slot_sampling``; a new tenant
        without the option needs an off entry, or it inherits its predecessor's window."""
        self._set_slot_table("smoltts_session_set_slot_align", slots, [(C.c_int32, int, t0), (C.c_int32, int, t1)],
                             "slot align: one window per slot")
        for b, a, z in zip(slots, t0, t1):
            (self.align_slots.add if z > a else self.align_slots.discard)(int(b))

    def graph_form(self) -> int:
        """The graph form of the next frame launches (``smoltts_session_graph_form``; bit 5: some slot's alignment window is on)."""
        f = self.lib.smoltts_session_graph_form(self.handle)
        if f < 0:
            check(f, "smoltts_session_graph_form")
        return int(f)

    def fetch_alignment(self, slot: int, n_frames: int) -> np.ndarray:
        """Host copy of ``alignment[slot, :n_frames]`` ([n_frames, pairs, 2] float32).  Waits for the current stream."""
        if self.alignment is None:
            raise SmolttsError("no alignment heads are set (set_align_heads)")
        return self.alignment[int(slot), :int(n_frames)].cpu().numpy()

    # ---- forced alignment: prompt rows measured instead of only stored (include/smoltts_hip.h at smoltts_lm_measure_rows)
    def iter_measure_rows(self, grid, slot: int, frame_of_row, targets, chunk: Optional[int] = None):
        """``measure_rows`` as a generator: one ``smoltts_lm_measure_rows`` call of at most ``chunk`` columns is queued per
        ``next()``; the generator's return value is the device tensor of the scores (a serving loop runs its ticks in between)."""
        g = np.asarray(grid)
        if g.ndim != 2 or g.shape[0] != self.H or g.shape[1] < 1:
            raise ValueError(f"grid must be ({self.H}, T>=1), got {g.shape}")
        T, slot = int(g.shape[1]), int(slot)
        frames, tgt = np.asarray(frame_of_row, dtype=np.int32).reshape(-1), np.asarray(targets, dtype=np.int32).reshape(-1)
        if frames.shape[0] != T or tgt.shape[0] != T:
            raise ValueError("measure_rows: one frame index and one target per grid column")
        if not 0 <= slot < self.B:
            raise ValueError(f"measure_rows: slot {slot} outside the session's {self.B}")
        if tgt.max() >= self.engine.cfg.vocab_size:
            raise ValueError("measure_rows: target id outside the vocabulary")
        if frames.max() >= self.max_frames:
            raise SmolttsError(f"measure_rows: frame {int(frames.max())} does not fit max_frames={self.max_frames}")
        if T + 1 > self.max_seq:
            raise SmolttsError(f"grid of {T} columns does not fit max_seq={self.max_seq}")
        chunk = min(T, self.max_rows) if chunk is None else max(1, min(int(chunk), self.max_rows))
        # the idle slot waits behind the rows: what its decode rows write there, nothing measured here reads
        check(self.lib.smoltts_lm_park_slots(self.handle, (C.c_int32 * 1)(slot), (C.c_int32 * 1)(T), 1, current_stream_ptr()),
              "smoltts_lm_park_slots")
        lp = torch.full((T,), float("nan"), dtype=torch.float32, device=self.engine.device)
        keep = [lp]
        # a chunk ends in front of the first scored column, so that the head does not run over the prompt's text columns
        first = int(np.argmax(tgt >= 0)) if bool((tgt >= 0).any()) else T
        starts = list(range(0, first, chunk)) + list(range(first, T, chunk))
        for c0, c1 in zip(starts, starts[1:] + [T]):
            grid_d, rslot_d, rpos_d, _, n = self._rows([g[:, c0:c1]], [slot], [c0])
            fr_d, tg_d = upload([frames[c0:c1], tgt[c0:c1]], self.engine.device)
            scored = bool((tgt[c0:c1] >= 0).any())  # (the head runs only over chunks that hold a target)
            check(self.lib.smoltts_lm_measure_rows(self.handle, dptr(grid_d), dptr(rslot_d), dptr(rpos_d), dptr(fr_d), dptr(tg_d), n,
                                                   lp.data_ptr() + 4 * c0 if scored else None, current_stream_ptr()),
                  "smoltts_lm_measure_rows")
            keep += [grid_d, rslot_d, rpos_d, fr_d, tg_d]
            self._keep = keep  # alive until the stream has consumed them
            if c1 < T:
                yield c1
        return lp

    def measure_rows(self, grid, slot: int, frame_of_row, targets, chunk: Optional[int] = None) -> np.ndarray:
        """Teacher-forced measurement of a whole grid ((1 + n_fast, T), positions 0 .. T-1) in the idle ``slot``: its KV rows are
        written as a chunked prefill writes them, column r measures the chosen heads as frame ``frame_of_row[r]`` of the slot
        (< 0: not measured; read them with ``fetch_alignment`` -- ``set_align_heads`` and the slot's window, ``set_slot_align``,
        come first), and the returned float32 [T] holds the log-probability of slow id ``targets[r]`` under column r's logits
        (``sampling.pick_logprob``; NaN where ``targets[r] < 0``).  At most ``chunk`` columns go through per call of the library
        (default: all that ``max_rows`` allows); the results do not depend on it.  No frame is emitted and the slot stays idle,
        parked behind the grid.  Waits for the current stream."""
        it = self.iter_measure_rows(grid, slot, frame_of_row, targets, chunk)
        while True:
            try:
                next(it)
            except StopIteration as done:
                return done.value.cpu().numpy()

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

    def fast_kv_cache(self):
        """(K, V) views of the depth transformer's cache: [n_fast_layer, max_batch, fast_n_kv_head, n_fast, 64] fp32, K after RoPE;
        entry i of a slot is depth step i of its latest frame (diagnostics)."""
        k, v, lb = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(self.lib.smoltts_session_fast_kv_cache(self.handle, C.byref(k), C.byref(v), C.byref(lb)), "smoltts_session_fast_kv_cache")
        cfg = self.engine.cfg
        n_layer, kvh, n_fast = cfg.n_fast_layer, cfg.fast_n_local_heads, self.H - 1
        if lb.value != self.B * kvh * n_fast * 64 * 4:
            raise SmolttsError(f"smoltts_session_fast_kv_cache: {lb.value} bytes per layer, expected {self.B * kvh * n_fast * 64 * 4}")
        base = self.slab.data_ptr()
        out = []
        for p in (k, v):
            o = p.value - base
            out.append(self.slab[o: o + n_layer * lb.value].view(torch.float32).view(n_layer, self.B, kvh, n_fast, 64))
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


class AlignFitter(ClosesOnDel):
    """The causal fit of streamed character timestamps on the device (include/smoltts_hip.h at "Streamed alignment fit"; the
    model is ``align.StreamFit``): per slot the token starts committed so far.  ``starts`` float64 [B, max_tokens] and
    ``committed`` int32 [B] are views of the fitter's slab; ``push`` is one launch over every slot on the current stream."""

    def __init__(self, device, max_batch: int, max_frames: int, max_tokens: int):
        self.lib = load_library()
        self.B, self.max_frames, self.max_tokens = int(max_batch), int(max_frames), int(max_tokens)
        need = self.lib.smoltts_align_fit_bytes(self.B, self.max_frames, self.max_tokens)
        if need == 0:
            raise SmolttsError("smoltts_align_fit_bytes returned 0 (bad sizes)")
        self.slab = _alloc_slab(need, device, settle=True)
        h = C.c_void_p()
        check(self.lib.smoltts_align_fit_create(dptr(self.slab), need, self.B, self.max_frames, self.max_tokens, C.byref(h)),
              "smoltts_align_fit_create")
        self.handle = h
        sp, cp, mt = C.c_void_p(), C.c_void_p(), C.c_int32()
        check(self.lib.smoltts_align_fit_outputs(h, C.byref(sp), C.byref(cp), C.byref(mt)), "smoltts_align_fit_outputs")
        base = self.slab.data_ptr()
        self.starts = self.slab[sp.value - base: sp.value - base + self.B * self.max_tokens * 8].view(torch.float64).view(self.B, self.max_tokens)
        self.committed = self.slab[cp.value - base: cp.value - base + self.B * 4].view(torch.int32)

    @classmethod
    def for_session(cls, session: "LMSession") -> "AlignFitter":
        return cls(session.engine.device, session.B, session.max_frames, session.max_seq)

    def reset_slots(self, slots: Sequence[int], n_tokens: Sequence[Optional[int]], lag: Sequence[int], cap_frames: Sequence[int]) -> None:
        """Start a stream in ``slots`` (``n_tokens[i]`` None: switch the slot off); ordered on the current stream."""
        n = len(slots)
        if n == 0:
            return
        if not (len(n_tokens) == len(lag) == len(cap_frames) == n):
            raise ValueError("align fit: one entry per slot")
        arr = lambda xs: (C.c_int32 * n)(*[int(x) for x in xs])
        check(self.lib.smoltts_align_fit_reset_slots(self.handle, arr(slots), arr([-1 if t is None else t for t in n_tokens]), arr(lag),
                                                     arr(cap_frames), n, current_stream_ptr()), "smoltts_align_fit_reset_slots")

    def push(self, rows: torch.Tensor, n_frames: torch.Tensor, done: torch.Tensor) -> None:
        """``rows`` float32 [B, max_frames, pairs, 2] (``LMSession.alignment``), the session's frame counters and done flags."""
        if rows.dtype != torch.float32 or rows.dim() != 4 or rows.shape[0] != self.B or rows.shape[1] != self.max_frames or rows.shape[3] != 2 \
                or not rows.is_contiguous():
            raise ValueError(f"align fit: rows must be contiguous float32 [{self.B}, {self.max_frames}, pairs, 2], got {tuple(rows.shape)}")
        for t in (n_frames, done):
            if t.dtype != torch.int32 or t.numel() != self.B or not t.is_contiguous():
                raise ValueError(f"align fit: counters must be contiguous int32 [{self.B}]")
        check(self.lib.smoltts_align_fit_push(self.handle, dptr(rows), int(rows.shape[2]), self.max_frames, dptr(n_frames), dptr(done),
                                              current_stream_ptr()), "smoltts_align_fit_push")

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize()
            self.lib.smoltts_align_fit_destroy(self.handle)
            self.handle = None


class PrefixKV(ClosesOnDel):
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
