"""The Mimi codec behind the C ABI: ``MimiEngine`` / ``MimiSession`` (streaming decode) and ``MimiEncoder`` (voice-clone prompts)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import packing
from .abi import (MIMI_OPT_PRODUCTS, MIMI_OPT_STATELESS_UPSAMPLE, MimiConfig, MimiEncConfig, MimiEncLayout, MimiEncWeights, MimiWeights, SmolttsError, check,
                  load_library)
from .device import ClosesOnDel, _alloc_slab, _require_gpu, current_stream_ptr, dptr


class MimiEngine(ClosesOnDel):
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


class MimiEncoder(ClosesOnDel):
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
        self._last_n, self._last_emb = 0, None

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
        self._last_n, self._last_emb = n, emb
        return (codes, emb, gap) if return_aux else codes

    def layout(self, n_samples: int) -> MimiEncLayout:
        """The map of the workspace an ``encode`` of ``n_samples`` carves (``smoltts_mimi_encode_layout``: rows and byte offsets)."""
        lay = MimiEncLayout()
        check(self.lib.smoltts_mimi_encode_layout(self.handle, int(n_samples), C.byref(lay)), "smoltts_mimi_encode_layout")
        return lay

    def stage_views(self, n_samples: int) -> Dict[str, torch.Tensor]:
        """Named fp32 views into the workspace of the LAST ``encode`` call, which must have been one of ``n_samples`` (tests,
        diagnostics): every buffer of ``SmolttsMimiEncLayout`` whole, halo and padding rows included, as [rows, channels] --
        ``xraw{i}``, ``xelu{i}``, ``helu{i}``, ``yelu{i}`` (i = 0..3), ``zelu``, ``ds``, ``emb``, ``res``, ``dots`` -- and ``kc``,
        ``vc`` as [n_layers, 8, positions, 64].  ``kc`` keeps the kernel's head-dim order (``packing._perm_heads``: the RoPE pair
        (j, j + 32) of the checkpoint sits at (2j, 2j + 1)).  ``emb`` is the tensor ``return_aux`` handed out when the call had it
        (the workspace's own copy stays zero then).  The views alias the workspace: the next ``encode`` overwrites them."""
        lay = self.layout(n_samples)
        if self._ws is None or self._last_n != n_samples or self._ws.numel() < lay.total:
            raise SmolttsError(f"stage_views: the last encode on this encoder was of {self._last_n} samples, not {n_samples}")
        ws = self._ws.view(torch.uint8)

        def view(off: int, rows: int, cols: int) -> torch.Tensor:
            return ws[off: off + 4 * rows * cols].view(torch.float32).view(rows, cols)

        out: Dict[str, torch.Tensor] = {}
        for i, r in enumerate((4, 5, 6, 8)):
            c, t = 64 << i, lay.T[i]
            out[f"xraw{i}"] = view(lay.xraw[i], t, c)
            out[f"xelu{i}"] = view(lay.xelu[i], 2 + t, c)
            out[f"helu{i}"] = view(lay.helu[i], t, c // 2)
            out[f"yelu{i}"] = view(lay.yelu[i], r + lay.extra[i] + t, c)
        t4, nl = lay.T[4], self.c_cfg.n_layers
        out["zelu"] = view(lay.zelu, 2 + t4, 1024)
        for name, off in (("kc", lay.kc), ("vc", lay.vc)):
            if lay.layer_stride != 4 * 8 * t4 * 64:
                raise SmolttsError(f"stage_views: layer stride {lay.layer_stride} bytes, expected {4 * 8 * t4 * 64}")
            out[name] = view(off, nl * 8 * t4, 64).view(nl, 8, t4, 64)
        out["ds"] = view(lay.ds, 2 + lay.ds_extra + t4, 512)
        out["emb"] = self._last_emb if self._last_emb is not None else view(lay.emb, lay.F, 512)
        out["res"] = view(lay.res, lay.F, 256)
        out["dots"] = view(lay.dots, lay.F, 2048)
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.lib.smoltts_mimi_encoder_destroy(self.handle)
            self.handle = None


class MimiSession(ClosesOnDel):
    """Streaming Mimi decode state for ``max_batch`` slots; ``decode`` consumes frames chunk-wise."""

    SAMPLES_PER_FRAME = 1920
    OPT_STATELESS_UPSAMPLE = MIMI_OPT_STATELESS_UPSAMPLE
    OPT_PRODUCTS = MIMI_OPT_PRODUCTS

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
