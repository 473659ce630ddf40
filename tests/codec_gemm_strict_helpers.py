"""The per-element measure of the codec's fp32 / bf16x3 GEMM family behind launch_gemm (csrc/gemm.hip: gemm_kernel, gemm_rows_kernel;
csrc/gemm_b3.hip: gemm_b3_kernel; csrc/gemm_dev.h: splitk_reduce_kernel; csrc/conv_xs.hip: conv_xs_kernel; csrc/conv_ks.hip:
conv_ks_kernel), the mirror of its dispatch and its case matrix.

Shared by tests/test_codec_gemm_strict_gpu.py (every launch form against float64) and tests/test_codec_gemm_strict_cpu.py (the
premises: what the measure rejects, the kernels' own K order, which forms the matrix reaches).  GPU-free at import.

The measure (the rule of tests/gemm3_strict_helpers.py, unchanged).  A case's operand matrix A [M, K] is what the kernel reads: rows
of K values ``ldx`` floats apart (ldx < K: overlapping conv windows over halo-prefixed per-slot buffers).  The float64 reference forms
a = pro(A) -- RMSNorm: fp32(A gamma), the row rsqrt applied after the contraction, exactly the kernel's operand; ELU and LayerNorm: the
float64 function of A (the kernels' fp32 evaluation of it is part of what is judged, as it is part of the fp32 torch evaluation) --
then y = sum a_k w_k (+ bias) and the condition scale s = sum |a_k| |w_k| (+ |bias|), and pushes both through the epilogue
(``epilogue``): RESID s + |r|; SCALE_RESID |sc| s + |r|; ELU out s f'(y) + |f(y)|; GELU s |f'(y)| + |y| (the erf form computes
1 + erf(y / sqrt 2), rounded at 2^-24 absolute, times y / 2: the formula's own scale is |y|, which bounds |f(y)|); RoPE
|cos| s0 + |sin| s1.  Judged: e = |got - ref64| / S per element; max e <= FACTOR E_ref and rms e <= FACTOR R_ref over the whole
output, rms e <= FACTOR R_ref over every 16 x 16 tile; E_ref / R_ref are max / rms of the same quantity for the plain fp32 torch
evaluation alone.  Where S == 0 the output must be exactly 0.  The one allowance is the hardware exponential of elu_rows / elu_hw1 /
elu_hw_xs / elu_hw_ks (ELU_EPS, absolute): on an ELU output ELU_EPS, on an ELU operand ELU_EPS sum_{k: A_k < 0} |w_k| pushed through
the epilogue's slope; it is taken off the error before the ratio.  gemm_kernel uses expm1f and gets none."""
from __future__ import annotations

import functools
import math
import zlib
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from lm_strict_helpers import FACTOR, half_ulp_bf16, rms, two_pieces  # noqa: F401  (FACTOR: the project's rule, no other number)
from mimi_enc_strict_helpers import ELU_EPS

EPS = 1e-5
NONE, RMSNORM, ELU, LAYERNORM = 0, 1, 2, 3                    # SMOLTTS_PRO_* (include/smoltts_hip.h)
STORE, RESID, SWIGLU, GELU, SCALE_RESID, QKV = 0, 1, 2, 3, 4, 5  # SMOLTTS_EPI_*
PRO_NAMES = {NONE: "none", RMSNORM: "rmsnorm", ELU: "elu", LAYERNORM: "layernorm"}
EPI_NAMES = {STORE: "store", RESID: "resid", SWIGLU: "swiglu", GELU: "gelu", SCALE_RESID: "scale_resid", QKV: "qkv"}
ROWS_EPIS = (STORE, RESID, GELU, SCALE_RESID, QKV)
SLOTS = 5        # QKV_ROPE: cache slots; cache_len is sized so that slots x cache_len > M
SENTINEL = 1.5   # prefill of the K / V caches
LEAD = 16        # NaN floats in front of every output buffer


# ------------------------------------------------------------------------------------------------ the launch mirror
class Form(NamedTuple):
    """What launch_gemm launches.  ``kernel``: gemm (gemm_kernel<WF32, MT, U, PRO, EPI>) | rows (gemm_rows_kernel<NTW, EPI>) | b3
    (gemm_b3_kernel<TM, TN, EPI, NP>) | xs (conv_xs_kernel<NTW, MT, RA, EPI, NP>) | ks (conv_ks_kernel<NTW, EPI, NP>); ``targs`` the
    template arguments in that order; ``geo`` the launch-time arguments that select code paths inside the instantiation; ``pre``: the
    stand-alone layernorm_kernel ran first; ``reduce``: the epilogue of the splitk_reduce_kernel<EPI> that follows, or -1."""
    kernel: str
    targs: tuple
    geo: tuple = ()
    pre: bool = False
    reduce: int = -1

    @property
    def instance(self) -> tuple:
        return (self.kernel,) + self.targs

    @property
    def instances(self) -> tuple:
        """Every template instantiation of the six kernels the form launches."""
        return (self.instance,) + ((("reduce", self.reduce),) if self.reduce >= 0 else ())

    @property
    def geometry(self) -> tuple:
        return self.instance + self.geo + (("reduce", self.reduce),)

    def __str__(self) -> str:
        names = {"gemm": "gemm_kernel", "rows": "gemm_rows_kernel", "b3": "gemm_b3_kernel", "xs": "conv_xs_kernel", "ks": "conv_ks_kernel"}
        s = f"{names[self.kernel]}<{', '.join(str(int(t)) for t in self.targs)}>"
        if self.geo:
            s += " " + " ".join(f"{k}={v}" for k, v in self.geo)
        if self.reduce >= 0:
            s += f" + splitk_reduce_kernel<{self.reduce}>"
        return ("layernorm_kernel + " if self.pre else "") + s


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def rows_ntw(ntiles: int) -> int:
    return 2 if ntiles >= 8 else 1


def rows_geometry(M: int, N: int):
    """(NTW, WN, grid) of launch_rows / the rows_grid of launch_gemm_impl."""
    ntiles = _cdiv(N, 16)
    NTW = rows_ntw(ntiles)
    per = _cdiv(ntiles, NTW)
    WN = 4 if per >= 4 else (2 if per >= 2 else 1)
    return NTW, WN, _cdiv(per, WN) * _cdiv(M, 64 * (4 // WN))


def gemm_b3_applies(M: int, N: int, K: int, epi: int) -> bool:
    if M < 256 or N < 64 or N % 4 or K % 32:
        return False
    if _cdiv(M, 64) * _cdiv(N, 64) < 192:
        return False
    return epi in ROWS_EPIS


def linear_ksplit(N: int, K: int, M: int, epi: int, ws_floats: int) -> bool:
    return epi == SCALE_RESID and N == 512 and K == 2048 and ws_floats > 0 and 4 * M * N <= ws_floats


def linear_ntw(N: int, K: int, rpb: int, epi: int) -> int:
    if rpb > 0:
        return N // 128 if (epi == RESID and K <= 256 and N in (256, 512)) else 0
    if epi == QKV and N == 1536:
        return 3
    if epi == SCALE_RESID and N == 512:
        return 1
    if epi == GELU and N == 2048:
        return 4
    return 0


def conv_xs_applies(M, K, N, ldx, rpb, epi, w3, ws_floats, pro_elu, ln, aligned) -> bool:
    if not w3 or not aligned:
        return False
    if ldx >= K and linear_ksplit(N, K, M, epi, ws_floats):
        if pro_elu or ln:
            return False
        T = rpb if rpb > 0 else M
        return M % T == 0 and M // T <= 65535 and _cdiv(T, 32) * (M // T) * 4 >= 256
    if ldx >= K:
        if pro_elu or K > 512 or K % 32 or linear_ntw(N, K, rpb, epi) == 0:
            return False
        if ln and (rpb > 0 or K != 512):
            return False
        if rpb > 0:
            return M % rpb == 0 and M // rpb <= 65535 and _cdiv(rpb, 64) * (M // rpb) >= 256
        return _cdiv(M, 32) * 4 >= 256
    if ln or epi != STORE or rpb <= 0 or M % rpb:
        return False
    if ldx % 32 or ldx > 256 or K % ldx:
        return False
    taps = K // ldx
    if taps < 2 or 64 + taps - 1 > 80 or N not in (128, 640):
        return False
    return _cdiv(rpb, 64) * (M // rpb) >= 256 and M // rpb <= 65535


def ks_ntw(M: int, N: int, rpb: int) -> int:
    ct = N // 16
    tiles = _cdiv(rpb, 64) * (M // rpb)
    for ntw in (4, 2, 1):
        if ct % (8 * ntw) == 0 and tiles * (ct // (8 * ntw)) >= 256:
            return ntw
    return 0


def conv_ks_applies(M, K, N, ldx, rpb, epi, w3, ln, aligned) -> bool:
    if not w3 or epi != STORE or ln:
        return False
    if rpb <= 0 or M % rpb or M // rpb > (1 << 20):
        return False
    if ldx >= K or ldx <= 256 or ldx % 128 or K % ldx or not aligned:
        return False
    taps = K // ldx
    if 64 + taps - 1 > 80 or N % 128:
        return False
    return ks_ntw(M, N, rpb) != 0


def _xs_form(M, K, N, ldx, rpb, epi, ws_floats, NP, pro_elu, ln) -> Form:
    if ldx >= K and linear_ksplit(N, K, M, epi, ws_floats):
        return Form("xs", (4, 2, 32, SCALE_RESID, NP), (("ksplit", 4),), reduce=SCALE_RESID)
    if ldx >= K:
        geo = (("ln", True),) if ln else ()
        if rpb > 0:
            return Form("xs", (2 if N == 256 else 4, 4, 64, RESID, NP), geo)
        ntw = linear_ntw(N, K, rpb, epi)
        if ntw == 3:
            return Form("xs", (3, 2, 32, QKV, NP), geo)
        if ntw == 1:
            return Form("xs", (1, 2, 32, SCALE_RESID, NP), geo)
        return Form("xs", (4, 2, 32, GELU, NP), geo)
    geo = (("taps", True),) + ((("pro_elu", True),) if pro_elu else ())
    return Form("xs", (5 if N == 640 else 1, 4, 80, STORE, NP), geo)


def _b3_form(M, K, N, ldx, rpb, epi, ws_floats, NP, pro_elu, aligned) -> Form:
    """launch_gemm_b3: conv_xs, conv_ks, then the tile choice of launch_b3_epi_np."""
    if conv_xs_applies(M, K, N, ldx, rpb, epi, True, ws_floats, pro_elu, False, aligned):
        return _xs_form(M, K, N, ldx, rpb, epi, ws_floats, NP, pro_elu, False)
    pe = (("pro_elu", True),) if pro_elu else ()
    if conv_ks_applies(M, K, N, ldx, rpb, epi, True, False, aligned):
        ntw = ks_ntw(M, N, rpb)
        return Form("ks", (ntw, STORE, NP), (("nparts", N // 16 // (8 * ntw)),) + pe)
    taps = K // ldx if (ldx < K and ldx % 32 == 0 and K % ldx == 0) else 1
    x_bytes, w_bytes = 4.0 * M * min(ldx, K), 6.0 * N * K

    def blocks(bm, bn):
        return _cdiv(M, bm) * _cdiv(N, bn)

    def geo(bm, bn, ksplit):
        rb, cb = _cdiv(M, bm), _cdiv(N, bn)
        by_rows, by_cols = x_bytes + min(rb, 8) * w_bytes, min(cb, 8) * x_bytes + w_bytes
        return (("ksplit", ksplit), ("taps", taps > 1), ("xcd_cols", int(cb % 8 == 0 and by_cols < by_rows))) + pe

    if ws_floats > 0 and N % 4 == 0 and blocks(64, 64) <= 512 and (K >> 5) >= 48 and 4 * M * N <= ws_floats:
        return Form("b3", (2, 2, epi, NP), geo(64, 64, 4), reduce=epi)
    if blocks(128, 128) >= 512 and N >= 128:
        return Form("b3", (4, 4, epi, NP), geo(128, 128, 1))
    if blocks(128, 64) >= 512 and N < 128:
        return Form("b3", (4, 2, epi, NP), geo(128, 64, 1))
    return Form("b3", (2, 2, epi, NP), geo(64, 64, 1))


# the ST_CASE table of launch_gemm_impl: (w_is_fp32, prologue, epilogue)
ST_CASES = ((False, RMSNORM, QKV), (False, NONE, RESID), (False, RMSNORM, SWIGLU), (False, RMSNORM, STORE), (False, NONE, STORE),
            (True, NONE, QKV), (True, NONE, SCALE_RESID), (True, NONE, GELU), (True, NONE, STORE), (True, NONE, RESID),
            (True, ELU, STORE), (True, ELU, RESID), (True, LAYERNORM, QKV), (True, LAYERNORM, GELU))


def skinny_waves(M: int, K: int) -> int:
    nchunks = K // 32
    nwaves = min(16, max(1, (nchunks + 2) // 3))
    if M > 32 and nwaves > 8:
        nwaves = 8
    return max(nwaves, 1 if M <= 16 else (2 if M <= 32 else 4))  # (the in-kernel LayerNorm prologue: at least 4, see launch_form)


def launch_form(M: int, K: int, N: int, ldx: Optional[int] = None, rows_per_batch: int = 0, prologue: int = NONE, epilogue: int = STORE,
                w_fp32: bool = True, w3: bool = False, ws_floats: int = 0, b3_products: int = 6, ln_scratch: bool = True,
                raw_out: bool = False, aligned: bool = True) -> Form:
    """Mirror of launch_gemm_impl and everything it dispatches to, in the order it takes its branches (the ST_KNOB_INT knobs at their
    defaults: they exist in knobs builds only).  ``aligned``: x_bstride, ldo, o_bstride (and raw_bstride with ``raw_out``) are
    multiples of 4, as every case of the matrix has them.  Raises ValueError where the launch returns SMOLTTS_E_INVALID."""
    ldx = K if ldx is None else ldx
    P, E, rpb = prologue, epilogue, rows_per_batch
    if M <= 0 or N <= 0 or K <= 0 or K % 32 or (N % 4 and N >= 4) or ldx % 4 or (N < 4 and E != STORE):
        raise ValueError("gemm: shape")
    NP = 3 if b3_products == 3 else 6
    _, _, rows_grid = rows_geometry(M, N)
    if P == LAYERNORM:
        if not w_fp32 or rpb != 0:
            raise ValueError("gemm: the LayerNorm prologue needs fp32 weights and one flat row range")
        many_b3 = w3 and gemm_b3_applies(M, N, K, E)
        if many_b3 and conv_xs_applies(M, K, N, ldx, rpb, E, True, ws_floats, False, True, aligned):
            return _xs_form(M, K, N, ldx, rpb, E, ws_floats, NP, False, True)
        many_rows = M >= 1024 and rows_grid >= 192
        if many_b3 or many_rows or M > 16 or K > 512 or E not in (QKV, GELU):  # gemm.hip: the re-route condition
            if not ln_scratch or ldx != K:
                raise ValueError("gemm: LayerNorm prologue: scratch missing or strided rows")
            return launch_form(M, K, N, ldx, rpb, NONE, E, w_fp32, w3, ws_floats, b3_products, ln_scratch, raw_out, aligned)._replace(pre=True)
    if w_fp32 and w3 and P in (NONE, ELU) and gemm_b3_applies(M, N, K, E) and not (E == STORE and N < 4):
        return _b3_form(M, K, N, ldx, rpb, E, ws_floats, NP, P == ELU, aligned)
    if w_fp32 and P == NONE and M >= 1024 and rows_grid >= 192 and E in ROWS_EPIS:
        NTW, WN, _ = rows_geometry(M, N)
        return Form("rows", (NTW, E), (("WN", WN),))
    if (bool(w_fp32), P, E) not in ST_CASES:
        raise ValueError(f"gemm: unsupported combination w_is_fp32={w_fp32} prologue={P} epilogue={E}")
    MT, U = (1, 3) if M <= 16 else ((2, 3) if M <= 32 else (4, 2))
    nwaves, nchunks = skinny_waves(M, K), K // 32
    if P == LAYERNORM:  # the statistics pass of the in-kernel prologue gives a wave at most 4 of the 16 rows
        nwaves = max(nwaves, 4)
    counts = [len(range(w, nchunks, nwaves)) for w in range(nwaves)]
    zero_fill = any(n % U for n in counts)  # a wave whose last round of U chunks is not whole takes the zero-fill arm
    return Form("gemm", (bool(w_fp32), MT, U, P, E), (("nwaves", nwaves), ("zero_fill", zero_fill)))


# ------------------------------------------------------------------------------------------------ the codec's own launches
class Call(NamedTuple):
    what: str
    where: str  # file:line of the launch_gemm call
    M: int
    K: int
    N: int
    ldx: int
    rpb: int
    pro: int
    epi: int
    w3: bool
    ws_floats: int = 0
    raw_out: bool = False
    elu_out: bool = False

    def form(self, b3_products: int = 6) -> Form:
        return launch_form(self.M, self.K, self.N, self.ldx, self.rpb, self.pro, self.epi, True, self.w3, self.ws_floats, b3_products,
                           True, self.raw_out)


D_MODEL, FF = 512, 2048
# mimi_engine.hip: the convs that go through launch_gemm (the resnet block of stage 3 and the whole last stage are kernels of their own)
DEC_C = (512, 1024, 512, 256, 512, 256, 128, 256, 128)   # BUF_C[0..8]
DEC_RPF = (2, 2, 16, 16, 16, 96, 96, 96)                 # BUF_RPF[0..7]: rows per frame entering conv i
DEC_CONVS = ((0, "conv0 k7", 7, 0), (1, "convtr s8", 2, 8), (2, "res1 k3", 3, 0), (3, "res1 k1", 1, 0), (4, "convtr s6", 2, 6),
             (5, "res2 k3", 3, 0), (6, "res2 k1", 1, 0), (7, "convtr s5", 2, 5))  # (i, what, taps, stride of a ConvTranspose)


def transformer_gemms(R: int, Tt: int, w3: bool, ws: bool, last_layer: bool) -> list:
    """run_mimi_transformer (mimi_engine.hip), one layer; fc2 passes rows_per_batch = Tt."""
    e = "mimi_engine.hip"
    return [Call("wqkv", f"{e}:210", R, D_MODEL, 3 * D_MODEL, D_MODEL, 0, LAYERNORM, QKV, w3),
            Call("wo", f"{e}:223", R, D_MODEL, D_MODEL, D_MODEL, 0, NONE, SCALE_RESID, w3),
            Call("fc1", f"{e}:231", R, D_MODEL, FF, D_MODEL, 0, LAYERNORM, GELU, w3),
            Call("fc2" + (" (last layer)" if last_layer else ""), f"{e}:245", R, FF, D_MODEL, FF, Tt, NONE, SCALE_RESID, w3, 4 * R * D_MODEL if ws else 0)]


def codec_gemms(slots: int, frames: int) -> list:
    """Every launch_gemm call of a Mimi decode chunk of ``frames`` frames in ``slots`` slots (mimi_engine.hip; the session's arena
    holds W3 tiles and its split-K workspace has 4 R D floats)."""
    Tt = 2 * frames
    out = transformer_gemms(slots * Tt, Tt, True, True, False)
    for i, what, taps, stride in DEC_CONVS:
        cin, cout, T = DEC_C[i], DEC_C[i + 1], DEC_RPF[i] * frames
        N = stride * cout if stride else cout
        pro = ELU if i in (2, 5) else NONE
        epi = RESID if i in (3, 6) else STORE
        out.append(Call(what, "mimi_engine.hip:476", slots * T, taps * cin, N, cin, T, pro, epi, True, elu_out=not stride))
    return out


ENC_RATIOS = (4, 5, 6, 8)


def encoder_gemms(n_samples: int) -> list:
    """Every launch_gemm call of smoltts_mimi_encode (mimi_encoder.hip; no W3 tiles, no split-K workspace, flat rows)."""
    e, out, T = "mimi_encoder.hip", [], n_samples
    for i, r in enumerate(ENC_RATIOS):
        C, Tn = 64 << i, _cdiv(T, r)
        out.append(Call(f"enc res{i} k3", f"{e}:265", T, 3 * C, C // 2, C, 0, NONE, STORE, False, elu_out=True))
        out.append(Call(f"enc res{i} k1", f"{e}:272", T, C // 2, C, C // 2, 0, NONE, RESID, False, elu_out=True))
        out.append(Call(f"enc strided conv {i}", f"{e}:283", Tn, 2 * r * C, 2 * C, r * C, 0, NONE, STORE, False, 0, i + 1 < len(ENC_RATIOS), True))
        T = Tn
    out.append(Call("enc final k3", f"{e}:290", T, 3 * 1024, D_MODEL, 1024, 0, NONE, STORE, False))
    out += [c._replace(what="enc " + c.what) for c in transformer_gemms(T, T, False, False, True)]
    Fr = _cdiv(T, 2)
    out.append(Call("enc downsample", f"{e}:309", Fr, 4 * D_MODEL, D_MODEL, 2 * D_MODEL, 0, NONE, STORE, False))
    out.append(Call("enc rvq in_proj", f"{e}:316", Fr, D_MODEL, 256, D_MODEL, 0, NONE, STORE, False))
    out.append(Call("enc rvq dots", f"{e}:320", Fr, 256, 2048, 256, 0, NONE, STORE, False))
    return out


CODEC_CHUNKS = ((1, 1), (40, 1), (3, 7), (32, 32), (36, 30))
ENCODER_LENGTHS = (1, 961, 960 + 1920, 1920 * 5 + 333, 1920 * 21 - 1)  # tests/mimi_enc_strict_helpers._LENGTHS


def codec_calls() -> dict:
    """{form: (an example, its Call)} over CODEC_CHUNKS and ENCODER_LENGTHS."""
    forms = {}
    for s, f in CODEC_CHUNKS:
        for c in codec_gemms(s, f):
            forms.setdefault(c.form(), (f"decode {s} x {f}: {c.what} ({c.where}) M={c.M} K={c.K} N={c.N}", c))
    for L in ENCODER_LENGTHS:
        for c in encoder_gemms(L):
            forms.setdefault(c.form(), (f"encode {L}: {c.what} ({c.where}) M={c.M} K={c.K} N={c.N}", c))
    return forms


def codec_forms() -> dict:
    return {f: ex for f, (ex, _) in codec_calls().items()}


# ------------------------------------------------------------------------------------------------ the case matrix
class Case(NamedTuple):
    name: str
    M: int
    K: int
    N: int
    epi: int = STORE
    pro: int = NONE
    w_fp32: bool = True
    w3: bool = False
    ldx: int = 0           # 0: K (Linear rows); < K: conv windows, row m reads the K floats from its row's start
    T: int = 0             # rows_per_batch (rows per slot); 0: one flat row range
    ws: str = ""           # split-K workspace: "" none | "full" 4 M N floats | "small" M N floats (too small: the unsplit form)
    products: int = 6
    bias: bool = True
    elu_out: bool = False
    raw_out: bool = False
    inplace: bool = False  # RESID / SCALE_RESID: resid is out
    kv3: bool = False      # QKV_ROPE: also the bf16x3 piece caches
    planted: bool = False  # a quarter of the operand in [-4, 0) (the ELU arms)
    probe: bool = False    # a long-K probe: run and reported, not part of the asserted matrix

    @property
    def id(self) -> str:
        return self.name

    @property
    def ldx_(self) -> int:
        return self.ldx if self.ldx else self.K

    @property
    def windows(self) -> bool:
        return self.ldx_ < self.K

    @property
    def ws_floats(self) -> int:
        return {"": 0, "full": 4 * self.M * self.N, "small": self.M * self.N}[self.ws]

    def form(self) -> Form:
        return launch_form(self.M, self.K, self.N, self.ldx_, self.T, self.pro, self.epi, self.w_fp32, self.w3, self.ws_floats, self.products,
                           True, self.raw_out)

    @property
    def heads(self) -> tuple:
        """(query heads, kv heads) of a QKV_ROPE case: N = (Hq + 2 Hkv) * 64."""
        t = self.N // 64
        kv = t // 3
        return t - 2 * kv, kv

    @property
    def cache_len(self) -> int:
        return _cdiv(self.M, SLOTS) + 3

    @property
    def hw_exp(self) -> bool:
        """The kernel uses the hardware exponential in its ELU (every kernel but gemm_kernel)."""
        return self.form().kernel != "gemm"

    # ---- layouts (floats): every stride a multiple of 4 unless N < 4
    @property
    def Tt(self) -> int:
        return self.T if self.T else self.M

    @property
    def x_span(self) -> int:
        return (self.Tt - 1) * self.ldx_ + self.K

    @property
    def x_bstride(self) -> int:
        return (self.x_span + 3) // 4 * 4 + 4 if self.T else 0

    @property
    def ldo(self) -> int:
        return self.out_cols + 4 if self.N >= 4 else self.N + 1

    @property
    def out_cols(self) -> int:
        return self.N // 2 if self.epi == SWIGLU else (self.heads[0] * 64 if self.epi == QKV else self.N)

    @property
    def o_bstride(self) -> int:
        return self.Tt * self.ldo + 8 if self.T else 0

    @property
    def raw_bstride(self) -> int:
        return self.Tt * self.ldo + 12 if self.T else 0

    @property
    def ldr(self) -> int:
        return 0 if self.inplace else self.N + 8

    @property
    def r_bstride(self) -> int:
        return 0 if self.inplace or not self.T else self.Tt * self.ldr + 4


def _c(name, M, K, N, **kw) -> Case:
    return Case(name, M, K, N, **kw)


def _cases() -> list:
    out = []
    # ---- gemm_kernel: every ST_CASE row x MT 1 / 2 / 4 (M = 1, 16 | 17, 32 | 33, 100), nwaves 1, 2, 3, 8, 16, the zero-fill arm,
    #      N % 16 in {0, 4, 8, 12}, N < 4, strided / batched rows, the in-kernel LayerNorm at K = 256 and 512
    for (wf, pro, epi) in ST_CASES:
        tag = f"gemm-{'f32' if wf else 'bf16'}-{PRO_NAMES[pro]}-{EPI_NAMES[epi]}"
        n_ok = (lambda n: n % 64 == 0 and n >= 192) if epi == QKV else (lambda n: True)
        shapes = [(1, 32, 16), (16, 128, 20), (17, 288, 24), (32, 768, 28), (33, 128, 48), (100, 768, 16), (17, 1472, 48), (1, 160, 16)]
        if epi == QKV:
            shapes = [(1, 32, 192), (16, 128, 192), (17, 288, 384), (32, 768, 192), (33, 128, 192), (100, 768, 192), (17, 1472, 192)]
        if pro == LAYERNORM:  # the in-kernel prologue holds at M <= 16, K <= 512 (more rows: the stand-alone kernel first, below)
            shapes = [(1, 256, 192 if epi == QKV else 20), (16, 512, 192 if epi == QKV else 48), (7, 32, 192 if epi == QKV else 16),
                      (16, 256, 192 if epi == QKV else 24)]  # (K = 32 and 256 would ask for 1 and 3 waves: fewer than the prologue needs)
        for (M, K, N) in shapes:
            if n_ok(N):
                out.append(_c(f"{tag}-M{M}-K{K}-N{N}", M, K, N, epi=epi, pro=pro, w_fp32=wf, inplace=epi in (RESID, SCALE_RESID) and M == 17,
                              planted=pro == ELU, elu_out=epi in (STORE, RESID) and wf and M in (16, 33)))
    for N in (1, 2, 3):  # the N < 4 tail: plain, with elu_out, with elu_out and raw_out
        out.append(_c(f"gemm-tail-N{N}", 17, 128, N))
        out.append(_c(f"gemm-tail-N{N}-elu", 33, 128, N, elu_out=True, bias=N != 2))
        out.append(_c(f"gemm-tail-N{N}-elu-raw", 5, 96, N, elu_out=True, raw_out=True))
    out.append(_c("gemm-batched-store", 3 * 11, 128, 24, T=11, ldx=136, elu_out=True, raw_out=True))
    out.append(_c("gemm-batched-resid", 2 * 9, 96, 20, T=9, ldx=100, epi=RESID))
    out.append(_c("gemm-batched-scale-resid", 4 * 5, 288, 28, T=5, epi=SCALE_RESID))
    out.append(_c("gemm-windows-flat", 70, 256, 16, ldx=64, raw_out=True, elu_out=True))   # the encoder's strided conv: flat overlapping windows
    out.append(_c("gemm-ln-standalone-M17", 17, 512, 48, pro=LAYERNORM, epi=GELU))         # layernorm_kernel + gemm_kernel
    out.append(_c("gemm-ln-standalone-K544", 8, 544, 192, pro=LAYERNORM, epi=QKV))
    out.append(_c("gemm-qkv-kv3", 33, 128, 192, epi=QKV, kv3=True))
    # ---- gemm_rows_kernel: (NTW, WN) = (1, 1), (1, 2), (1, 4), (2, 4) x the five epilogues, M ragged against 64 * WM
    for N, M in ((16, 48897 + 30), (32, 24449 + 70), (64, 12225 + 40), (128, 12225 + 3)):
        for epi in (STORE, RESID, GELU, SCALE_RESID):
            out.append(_c(f"rows-{EPI_NAMES[epi]}-N{N}", M, 32 if N < 128 else 64, N, epi=epi, inplace=epi == RESID and N == 32,
                          elu_out=epi in (STORE, RESID) and N in (16, 128), raw_out=epi == STORE and N == 128, bias=not (epi == STORE and N == 64)))
    out.append(_c("rows-qkv-N192", 6081 + 20, 32, 192, epi=QKV))
    out.append(_c("rows-qkv-N192-kv3", 6081 + 90, 64, 192, epi=QKV, kv3=True))
    out.append(_c("rows-tail-N3-elu-raw", 48897 + 5, 32, 3, elu_out=True, raw_out=True))
    out.append(_c("rows-batched-N20", 49 * 1000, 32, 20, T=1000, ldx=36, epi=RESID, elu_out=True))
    out.append(_c("rows-ln-standalone", 12225 + 9, 64, 64, pro=LAYERNORM, epi=GELU))      # layernorm_kernel + gemm_rows_kernel
    # ---- gemm_b3_kernel: 2 x 2, 4 x 4, 4 x 2, each with the five epilogues; ragged M and N; xcd_cols; taps; PRO_ELU; split-K
    for epi in ROWS_EPIS:
        e = EPI_NAMES[epi]
        qn = epi == QKV
        out.append(_c(f"b3-22-{e}", 1024 - 13, 32, 768, epi=epi, w3=True, inplace=epi == SCALE_RESID, elu_out=epi == RESID))
        out.append(_c(f"b3-44-{e}", 4096 - 50, 32, 2112 if qn else 2052, epi=epi, w3=True, inplace=epi == RESID))
        if not qn:
            out.append(_c(f"b3-42-{e}", 32768 + 100, 32, 68, epi=epi, w3=True, elu_out=epi == STORE, raw_out=epi == STORE))
    out.append(_c("b3-22-xcd-cols", 1024, 32, 1024, w3=True, bias=False))
    out.append(_c("b3-22-ragged-N", 4100, 64, 132, w3=True, elu_out=True, raw_out=True))   # N % 16 == 4, 65 row blocks
    out.append(_c("b3-42-N64", 65536 + 7, 32, 64, w3=True))
    out.append(_c("b3-22-taps", 41 * 100, 3 * 64, 192, ldx=64, T=100, w3=True))             # conv windows neither conv kernel takes (N = 192)
    out.append(_c("b3-22-pro-elu", 3100, 96, 256, pro=ELU, epi=RESID, w3=True, planted=True))
    out.append(_c("b3-22-pro-elu-taps", 104 * 120, 3 * 128, 64, ldx=128, T=120, pro=ELU, w3=True, planted=True, elu_out=True))
    out.append(_c("b3-splitk-store", 12225 + 37, 1536, 64, w3=True, ws="full"))
    out.append(_c("b3-splitk-gelu", 6200, 1600, 132, epi=GELU, w3=True, ws="full"))
    out.append(_c("b3-splitk-resid", 3100, 1536, 256, epi=RESID, w3=True, ws="full", elu_out=True, inplace=True))
    out.append(_c("b3-splitk-scale-resid", 6200, 1568, 128, epi=SCALE_RESID, w3=True, ws="full"))
    out.append(_c("b3-splitk-qkv", 4200, 1536, 192, epi=QKV, w3=True, ws="full", kv3=True))
    # ---- conv_xs_kernel: the eight launch_xs instantiations
    out.append(_c("xs-conv-N128-taps2", 360 * 17, 2 * 32, 128, ldx=32, T=17, w3=True, elu_out=True, raw_out=True))
    out.append(_c("xs-conv-N128-taps17", 128 * 70, 17 * 32, 128, ldx=32, T=70, w3=True))
    out.append(_c("xs-conv-N128-taps3-c256", 256 * 24, 3 * 256, 128, ldx=256, T=24, w3=True, pro=ELU, planted=True, elu_out=True))
    out.append(_c("xs-conv-N640-taps2-c256", 256 * 9, 2 * 256, 640, ldx=256, T=9, w3=True))
    out.append(_c("xs-conv-N640-taps7-c32", 130 * 65, 7 * 32, 640, ldx=32, T=65, w3=True, bias=False))
    out.append(_c("xs-k1-resid-N256", 512 * 6, 128, 256, T=6, epi=RESID, w3=True, elu_out=True))
    out.append(_c("xs-k1-resid-N512", 128 * 67, 256, 512, T=67, epi=RESID, w3=True, elu_out=True, inplace=True))
    out.append(_c("xs-k1-resid-N512-K32", 512 * 3, 32, 512, T=3, epi=RESID, w3=True))
    out.append(_c("xs-lin-qkv", 2017, 512, 1536, epi=QKV, w3=True, kv3=True))
    out.append(_c("xs-lin-qkv-K32", 2048, 32, 1536, epi=QKV, w3=True))
    out.append(_c("xs-lin-scale-resid", 2030, 512, 512, epi=SCALE_RESID, w3=True, inplace=True))
    out.append(_c("xs-lin-scale-resid-K32", 2017, 32, 512, epi=SCALE_RESID, w3=True))
    out.append(_c("xs-lin-gelu", 2019, 512, 2048, epi=GELU, w3=True))
    out.append(_c("xs-lin-gelu-K32", 2048, 32, 2048, epi=GELU, w3=True))
    out.append(_c("xs-ln-qkv", 2021, 512, 1536, pro=LAYERNORM, epi=QKV, w3=True))
    out.append(_c("xs-ln-gelu", 2017, 512, 2048, pro=LAYERNORM, epi=GELU, w3=True))
    out.append(_c("xs-ksplit-flat", 2029, 2048, 512, epi=SCALE_RESID, w3=True, ws="full"))
    out.append(_c("xs-ksplit-slots", 64 * 32, 2048, 512, T=32, epi=SCALE_RESID, w3=True, ws="full", inplace=True))
    out.append(_c("b3-ln-standalone", 600, 512, 2048, pro=LAYERNORM, epi=GELU, w3=True))   # layernorm_kernel + gemm_b3_kernel
    # ---- conv_ks_kernel: NTW 4 / 2 / 1, nparts 1, 2, 3, 8
    out.append(_c("ks-ntw4-np1", 256 * 8, 2 * 384, 512, ldx=384, T=8, w3=True, elu_out=True, raw_out=True))
    out.append(_c("ks-ntw4-np2", 128 * 9, 3 * 512, 1024, ldx=512, T=9, w3=True, elu_out=True))
    out.append(_c("ks-ntw4-np3", 90 * 5, 2 * 512, 1536, ldx=512, T=5, w3=True))
    out.append(_c("ks-ntw4-np8", 64 * 4, 2 * 384, 4096, ldx=384, T=4, w3=True))
    out.append(_c("ks-ntw2-np1", 200 * 70, 2 * 384, 256, ldx=384, T=70, w3=True, pro=ELU, planted=True, elu_out=True))
    out.append(_c("ks-ntw2-np8", 40 * 30, 2 * 384, 2048, ldx=384, T=30, w3=True, bias=False))
    out.append(_c("ks-ntw1-np1", 256 * 24, 2 * 512, 128, ldx=512, T=24, w3=True))
    out.append(_c("ks-ntw1-np8", 40 * 30, 2 * 384, 1024, ldx=384, T=30, w3=True))
    out.append(_c("ks-ntw2-np3-taps7", 90 * 11, 7 * 384, 768, ldx=384, T=11, w3=True))
    # ---- the three-product forms (b3_products = 3), one per kernel template
    out.append(_c("np3-b3", 1024 - 13, 64, 768, w3=True, products=3))
    out.append(_c("np3-xs-conv", 256 * 9, 2 * 256, 640, ldx=256, T=9, w3=True, products=3))
    out.append(_c("np3-xs-lin", 2019, 512, 2048, epi=GELU, w3=True, products=3))
    out.append(_c("np3-ks", 256 * 8, 2 * 384, 512, ldx=384, T=8, w3=True, products=3))
    out.append(_c("np3-b3-splitk", 3100, 1536, 256, epi=RESID, w3=True, ws="full", products=3))
    # ---- long-K probes at the codec's own longest K per many-row kernel (reported, not asserted)
    # a workspace too small: the unsplit form at K = 1536, held to the bits of the call without a workspace; its one chain of 48 chunks
    # is a long-K case like the ones below
    out.append(_c("probe-b3-K1536-ws-small", 12225 + 37, 1536, 64, w3=True, ws="small", probe=True))
    out.append(_c("probe-b3-K2048", 2048, 2048, 512, epi=SCALE_RESID, w3=True, probe=True))          # fc2 unsplit (no workspace)
    out.append(_c("probe-ks-2x1024", 64 * 4, 2 * 1024, 4096, ldx=1024, T=4, w3=True, probe=True))                  # ConvTranspose 1024 -> 512, stride 8
    out.append(_c("probe-ks-7x512", 32 * 64, 7 * 512, 1024, ldx=512, T=64, w3=True, elu_out=True, probe=True))   # conv0
    out.append(_c("probe-xs-3x256", 32 * 512, 3 * 256, 128, ldx=256, T=512, w3=True, pro=ELU, planted=True, elu_out=True, probe=True))  # res2 k3
    # gemm_rows_kernel: the encoder's strided convs (mimi_encoder.hip:283: flat overlapping windows, ldx = K / 2, ELU out, raw copy but
    # for the last) at the fewest output rows that still go to the many-row kernel -- signals of 6100 * 20, 3040 * 120 and 1553 * 960
    # samples; strided conv 3 has the longest K any codec call gives the kernel
    out.append(_c("probe-rows-enc-conv1-K1280", 6081 + 19, 1280, 256, ldx=640, elu_out=True, raw_out=True, probe=True))
    out.append(_c("probe-rows-enc-conv2-K3072", 3009 + 31, 3072, 512, ldx=1536, elu_out=True, raw_out=True, probe=True))
    out.append(_c("probe-rows-enc-conv3-K8192", 1473 + 80, 8192, 1024, ldx=4096, elu_out=True, probe=True))
    assert all(c.form().kernel == "rows" for c in out[-3:])
    return out


def _codec_cases(have: set) -> list:
    """One case for every form of codec_calls() that no hand-written case launches, at the call's own shape or -- gemm_kernel, where
    only the row-tile class of M and K choose the form -- at fewer rows and one column tile."""
    out = []
    for f, (ex, k) in codec_calls().items():
        if f in have:
            continue
        M, N = k.M, k.N
        if f.kernel == "gemm":
            # (one full row tile where the call has a few rows: torch's own one- and two-row products are the noisier reference)
            M, N = (16 if M <= 16 else min(M, 35)), (192 if k.epi == QKV else 16)
        ws = "full" if k.ws_floats else ""
        T = k.rpb if (k.rpb and M == k.M) else 0
        K, ldx = k.K, (k.ldx if k.ldx != k.K else 0)
        if f.kernel == "gemm":  # ... and at the shortest K of the same form (rows of K values: the form does not look at ldx)
            K = next(kk for kk in range(32, k.K + 1, 32) if launch_form(M, kk, N, None, 0, k.pro, k.epi, True, k.w3, 0, 6, True, k.raw_out) == f)
            ldx = ldx if K == k.K else 0
        c = Case(f"codec-{len(out)}-{k.what.replace(' ', '_')}-M{M}-K{K}-N{N}", M, K, N, epi=k.epi, pro=k.pro, w3=k.w3, ldx=ldx, T=T,
                 ws=ws, elu_out=k.elu_out, raw_out=k.raw_out, planted=k.pro == ELU, inplace=k.epi == SCALE_RESID and k.what.startswith("wo"))
        if c.form() != f:
            c = c._replace(M=k.M, N=k.N, T=k.rpb, name=f"codec-{len(out)}-{k.what.replace(' ', '_')}-M{k.M}-K{k.K}-N{k.N}")
        assert c.form() == f, (ex, str(c.form()), str(f))
        assert c.M * c.K * c.N < 8e9, ex
        have.add(f)
        out.append(c)
    return out


def _np3_cases(cases: list) -> list:
    """The three-product twin of the first prologue-free case of every six-product instantiation that has none yet."""
    have = {c.form().instance for c in cases if c.products == 3}
    out = []
    for c in cases:
        f = c.form()
        if f.kernel in ("b3", "xs", "ks") and c.pro == NONE and c.products == 6 and not c.probe:
            twin = c._replace(name="np3-" + c.name, products=3, raw_out=False)
            if twin.form().instance not in have:
                have.add(twin.form().instance)
                out.append(twin)
    return out


def _all_cases() -> list:
    hand = _cases()
    hand += _codec_cases({c.form() for c in hand if not c.probe})
    return hand + _np3_cases(hand)


CASES = _all_cases()
MATRIX = [c for c in CASES if not c.probe]
PROBES = [c for c in CASES if c.probe]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Built instantiations of the six templates that no argument set of smoltts_k_gemm reaches, with the reason.  (None today: the
# coverage test of tests/test_codec_gemm_strict_cpu.py lists what no case launches and fails on any entry missing here.)
UNREACHED: dict = {}


# ------------------------------------------------------------------------------------------------ inputs and references (CPU)
def bf16r(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def row_offsets(M: int, T: int, ld: int, bstride: int) -> torch.Tensor:
    """row_off of gemm_dev.h for every row: int64 [M]."""
    m = torch.arange(M, dtype=torch.int64)
    if T <= 0:
        return m * ld
    return (m // T) * bstride + (m % T) * ld


@functools.lru_cache(maxsize=6)
def make_inputs(c: Case) -> dict:
    """The case's buffers as the launch gets them (CPU).  Buffer rows of x over logspace(-3, 3) in scale, weight rows over
    logspace(-3, 0); one operand row all zero; NaN wherever the kernel may not read (row padding of Linear rows, gaps between
    slots); ``planted``: a quarter of the operand in [-4, 0)."""
    from smoltts_amd.packing import rope_table

    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}|{c.M}|{c.K}|{c.N}".encode()))
    M, K, N, ldx, Tt = c.M, c.K, c.N, c.ldx_, c.Tt
    B = M // Tt
    assert B * Tt == M
    xo = row_offsets(M, c.T, ldx, c.x_bstride)
    total = int(xo[-1]) + K
    win = xo[:, None] + torch.arange(K)[None]                       # [M, K] float index of every operand value
    # the scale of every operand ROW spans logspace(-3, 3): Linear rows one by one; conv windows overlap, so there a slot's rows
    # share one scale (flat windows: the scale goes up and down along the buffer, a factor 1.5 from row to row) -- a window over rows 10^6 apart in scale is no row of
    # the codec, and the fp32 evaluation of such rows is so heavy-tailed that it breaks the tile rule itself (the CPU test holds
    # every case to that premise)
    if not c.windows:
        rowscale = torch.logspace(-3, 3, M)[torch.randperm(M, generator=g)] if M > 1 else torch.tensor([0.7])
        sv = torch.ones(total)
        sv[win.flatten()] = rowscale.repeat_interleave(K)
    elif c.T:
        slotscale = torch.logspace(-3, 3, B)[torch.randperm(B, generator=g)]
        sv = slotscale[(torch.arange(total) // c.x_bstride).clamp(max=B - 1)]
        rowscale = slotscale.repeat_interleave(Tt)
    else:
        nrows_buf = _cdiv(total, ldx)
        tri = 1 - (torch.arange(nrows_buf) % 64 / 32.0 - 1).abs()  # up and down once every 64 buffer rows, a factor 1.5 from row to row
        sv = (10.0 ** (6 * tri - 3)).repeat_interleave(ldx)[:total]
        rowscale = sv[xo]
    data = torch.randn(total, generator=g) * sv
    if c.planted:
        sel = torch.rand(data.numel(), generator=g) < 0.25
        data = torch.where(sel, -4.0 * torch.rand(data.numel(), generator=g), data)
    # (no zero row under LayerNorm, whose operand is then the bias; none in a residual case of few rows: there the row is the fp32
    # rounding of resid + scale * bias alone, 2^-24-grade against S, and one row in sixteen of it would be a third of R_ref)
    zero_row = (3 * Tt) // 7 if Tt > 1 and c.pro != LAYERNORM and (c.epi not in (RESID, SCALE_RESID) or c.M >= 64) else -1
    if zero_row >= 0:
        data[win[zero_row]] = 0.0
    read = torch.zeros(total, dtype=torch.bool)
    read[win.flatten()] = True
    xbuf = torch.where(read, data, torch.full_like(data, float("nan")))
    A = data[win]
    colscale = torch.logspace(-3, 0, N)[torch.randperm(N, generator=g)] if N > 1 else torch.tensor([0.5])
    if c.epi in (SWIGLU, QKV):  # a gate and its up column share a scale, and so do the two columns of a rotated pair
        colscale = colscale.view(N // 2, 2)[:, :1].expand(N // 2, 2).reshape(N)
    w = torch.randn(N, K, generator=g) * 0.05 * colscale[:, None]
    if not c.w_fp32:
        w = bf16r(w)
    d = dict(xbuf=xbuf, A=A, w=w, zero_row=zero_row)
    if c.pro in (RMSNORM, LAYERNORM):
        d["gamma"] = 1 + 0.2 * torch.randn(K, generator=g)
    if c.pro == LAYERNORM:
        d["beta"] = 0.1 * torch.randn(K, generator=g)
    ymag = colscale[None] * (rowscale[:, None] if c.pro in (NONE, ELU) else torch.ones(M, 1))
    d["bias"] = torch.randn(N, generator=g) * 0.5 * colscale if c.bias else None
    if c.epi in (RESID, SCALE_RESID):
        d["resid"] = torch.randn(M, N, generator=g) * 0.5 * ymag
    if c.epi == SCALE_RESID:
        # layer scales of either sign and 0.5 .. 1 in size: in a column of tiny scale the residual alone would make up the output
        d["scale"] = (0.5 + 0.5 * torch.rand(N, generator=g)) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1).float()
    if c.epi == QKV:
        L = c.cache_len
        pairs = torch.randperm(SLOTS * L, generator=g)[:M]
        slot, pos = (pairs // L).int(), (pairs % L).int()
        if M >= 8:  # rows outside the cache: their q is written (rotated by the table's entry at pos), their K / V are not
            pos[1], pos[M // 2] = -1, -1
            pos[2], pos[M // 3] = L, L
        d["row_slot"], d["row_pos"] = slot, pos
        d["rope_full"] = rope_table(L + 2, 64, 10000.0, bf16=False)  # entry i: position i - 1, so that -1 and L are inside the table
    return d


class Ref(NamedTuple):
    ref64: np.ndarray  # float64 [M, cols]
    S: np.ndarray      # float64 [M, cols], the per-element scale
    ref32: np.ndarray  # float32 [M, cols]
    E_ref: float
    R_ref: float
    extra: Optional[np.ndarray]  # float64 [M, cols]: the absolute allowance of the hardware exponential, or None


def _rope_cs(c: Case, d: dict, dtype):
    """(cos, sin) [M, N / 2] of every column pair: the row's table entry below (Hq + Hkv) * 64, (1, 0) in the V columns."""
    Hq, Hkv = c.heads
    cs = d["rope_full"][d["row_pos"].long() + 1].to(dtype)  # [M, 32, 2]
    cos = torch.ones(c.M, c.N // 2, dtype=dtype)
    sin = torch.zeros(c.M, c.N // 2, dtype=dtype)
    nrot = (Hq + Hkv) * 32
    cos[:, :nrot] = cs[:, :, 0].repeat(1, Hq + Hkv)
    sin[:, :nrot] = cs[:, :, 1].repeat(1, Hq + Hkv)
    return cos, sin


def _elu_scale(out, S):
    """ELU on (value, scale): f, s f'(y) + |f(y)|."""
    f = torch.where(out > 0, out, torch.expm1(out.clamp(max=0)))
    if S is None:
        return f, None
    slope = torch.where(out > 0, torch.ones_like(out), torch.exp(out.clamp(max=0)))
    return f, torch.where(S > 0, S * slope + f.abs(), S), slope


def epilogue(c: Case, d: dict, y: torch.Tensor, s: Optional[torch.Tensor] = None, elu_out: Optional[bool] = None, x: Optional[torch.Tensor] = None):
    """The epilogue in y's dtype (y without bias) -> (result [M, cols], per-element scale S or None, the slope d out / d y that an
    absolute error of y is multiplied with, or None).  ``x``: an absolute allowance on y, pushed through the same slope."""
    dt = y.dtype
    elu_out = c.elu_out if elu_out is None else elu_out
    S = None
    slope = torch.ones_like(y)
    if d["bias"] is not None:
        b = d["bias"].to(dt)[None]
        y = y + b
        if s is not None:
            s = s + b.abs()
    if c.epi in (STORE, RESID):
        out = y
        S = s
        if c.epi == RESID:
            r = d["resid"].to(dt)
            out = r + y
            if s is not None:
                S = s + r.abs()
        if elu_out:
            if S is not None:
                out, S, slope = _elu_scale(out, S)
            else:
                out = F.elu(out)
    elif c.epi == SCALE_RESID:
        r, sc = d["resid"].to(dt), d["scale"].to(dt)[None]
        out = r + sc * y
        slope = sc.abs().expand_as(y)
        if s is not None:
            S = sc.abs() * s + r.abs()
    elif c.epi == GELU:
        out = F.gelu(y)
        if s is not None:
            cdf = 0.5 * (1 + torch.erf(y / math.sqrt(2.0)))
            slope = (cdf + y * torch.exp(-0.5 * y * y) / math.sqrt(2 * math.pi)).abs()
            S = torch.where(s > 0, s * slope + y.abs(), s)
    elif c.epi == SWIGLU:
        gt, up = y[:, 0::2], y[:, 1::2]
        out = F.silu(gt) * up
        if s is not None:
            sg = torch.sigmoid(gt)
            dsilu = sg * (1 + gt * (1 - sg))
            S = dsilu.abs() * s[:, 0::2] * up.abs() + (gt * sg).abs() * s[:, 1::2] + out.abs()
    else:
        cos, sin = _rope_cs(c, d, dt)
        y0, y1 = y[:, 0::2], y[:, 1::2]
        out = torch.stack([y0 * cos - y1 * sin, y1 * cos + y0 * sin], -1).flatten(-2)
        if s is not None:
            s0, s1 = s[:, 0::2], s[:, 1::2]
            S = torch.stack([s0 * cos.abs() + s1 * sin.abs(), s1 * cos.abs() + s0 * sin.abs()], -1).flatten(-2)
            if x is not None:
                x0, x1 = x[:, 0::2], x[:, 1::2]
                x = torch.stack([x0 * cos.abs() + x1 * sin.abs(), x1 * cos.abs() + x0 * sin.abs()], -1).flatten(-2)
                return out, S, x
    if x is not None and c.epi != SWIGLU:
        return out, S, x * slope
    return out, S, None


def rstd(A: torch.Tensor) -> torch.Tensor:
    return torch.rsqrt((A * A).mean(-1, keepdim=True) + EPS)


def operand(c: Case, d: dict, dtype) -> torch.Tensor:
    """pro(A) in ``dtype`` (RMSNorm: fp32(A gamma) in both -- the kernel's operand; the row rsqrt comes after the contraction)."""
    A = d["A"]
    if c.pro == RMSNORM:
        return (A * d["gamma"]).to(dtype)
    if c.pro == ELU:
        return F.elu(A.to(dtype))
    if c.pro == LAYERNORM:
        return F.layer_norm(A.to(dtype), (c.K,), d["gamma"].to(dtype), d["beta"].to(dtype), EPS)
    return A.to(dtype)


def reference32(c: Case, d: dict, elu_out: Optional[bool] = None) -> torch.Tensor:
    """The plain fp32 torch evaluation: fp32 prologue, @ w.T, the epilogue in fp32."""
    y = operand(c, d, torch.float32) @ d["w"].T
    if c.pro == RMSNORM:
        y = y * rstd(d["A"])
    return epilogue(c, d, y, elu_out=elu_out)[0]


def noise(res: np.ndarray, ref64: np.ndarray, S: np.ndarray, extra: Optional[np.ndarray] = None) -> np.ndarray:
    """e = |res - ref64| / S per element, 0 where S == 0."""
    diff = np.abs(res.astype(np.float64) - ref64)
    if extra is not None:
        diff = np.maximum(diff - extra, 0.0)
    return np.divide(diff, S, out=np.zeros_like(diff), where=S > 0)


def _finish(c: Case, d: dict, y, s, allow, elu_out, ref32) -> Ref:
    ref64, S, extra = epilogue(c, d, y, s, elu_out=elu_out, x=allow)
    ref64, S = ref64.numpy(), S.numpy()
    if (c.elu_out if elu_out is None else elu_out) and c.hw_exp:  # the output ELU's own hardware exponential
        extra = (extra if extra is not None else torch.zeros_like(y)) + ELU_EPS
    extra = extra.numpy() if extra is not None else None
    e = noise(ref32, ref64, S)  # (the fp32 torch evaluation uses expm1: no allowance for the reference)
    live = S > 0
    assert live.any() and np.isfinite(ref64).all()
    E_ref, R_ref = float(e[live].max()), rms(e[live])
    assert E_ref > 0.0 and R_ref > 0.0
    return Ref(ref64, S, ref32, E_ref, R_ref, extra)


@functools.lru_cache(maxsize=6)
def reference(c: Case, raw: bool = False) -> Ref:
    """The float64 reference of ``out`` (``raw``: of raw_out, the value before the output ELU)."""
    d = make_inputs(c)
    a, w = operand(c, d, torch.float64), d["w"].double()
    r = rstd(d["A"].double()) if c.pro == RMSNORM else 1.0
    y, s = r * (a @ w.T), r * (a.abs() @ w.abs().T)
    allow = None
    if c.pro == ELU and c.hw_exp:  # |elu_hw(x) - elu(x)| <= ELU_EPS for x < 0
        allow = ELU_EPS * ((d["A"] < 0).double() @ w.abs().T)
    elu_out = False if raw else None
    return _finish(c, d, y, s, allow, elu_out, reference32(c, d, elu_out=elu_out).numpy())


def split3(a: torch.Tensor):
    """fp32 -> the (hi, mid, lo) bf16 pieces as fp32 tensors; hi + mid + lo == a."""
    hi = bf16r(a)
    mid = bf16r(a - hi)
    return hi, mid, bf16r(a - hi - mid)


@functools.lru_cache(maxsize=4)
def reference3(c: Case) -> Ref:
    """The model of a three-product form (b3_products = 3): both operands cut to their hi + mid pieces, the products hi hi, mid hi and
    hi mid kept, in float64; scale and noise unit of the six-product reference."""
    assert c.products == 3 and c.pro == NONE
    d, full = make_inputs(c), reference(c)
    xh, xm, _ = (t.double() for t in split3(d["A"]))
    wh, wm, _ = (t.double() for t in split3(d["w"]))
    y = xh @ wh.T + xm @ wh.T + xh @ wm.T
    ref64 = epilogue(c, d, y)[0].numpy()
    return full._replace(ref64=ref64)


def two_piece_model(c: Case, d: dict) -> np.ndarray:
    """The kernel's arithmetic in fp32 on the CPU with the operand cut to two bf16 pieces: 2^-16-grade, must be rejected."""
    y = two_pieces(operand(c, d, torch.float32)) @ d["w"].T
    if c.pro == RMSNORM:
        y = y * rstd(d["A"])
    return epilogue(c, d, y)[0].numpy()


def one_moved(ref: Ref):
    """ref32 with the element of the smallest S > 0 moved by 2^-16 S -> (result, (row, column))."""
    Sm = np.where(ref.S > 0, ref.S, np.inf)
    m, n = np.unravel_index(int(Sm.argmin()), Sm.shape)
    res = ref.ref32.copy()
    res[m, n] = np.float32(res[m, n] + np.float32(2.0 ** -16 * ref.S[m, n]))
    if res[m, n] == ref.ref32[m, n]:  # (2^-16 S below half an ulp of the value cannot happen: S >= |value| up to rounding)
        res[m, n] = np.nextafter(res[m, n], np.float32(np.inf))
    return res, (int(m), int(n))


# ------------------------------------------------------------------------------------------------ fp32 in the kernels' own K order
def chunk_parts(c: Case) -> list:
    """The K order of the launch: a list of parts (accumulators added in list order), each a list of 32-k chunk numbers in the order
    the part's accumulator takes them."""
    f = c.form()
    nch = c.K // 32
    geo = dict(f.geo)
    if f.kernel == "gemm":  # chunk ch belongs to wave ch % nwaves; the partial tiles are added in wave order
        nw = geo["nwaves"]
        return [list(range(w, nch, nw)) for w in range(nw)]
    if f.kernel == "rows":
        return [list(range(nch))]
    if f.kernel == "b3":
        taps = c.K // c.ldx_ if geo["taps"] else 1
        cpt = nch // taps
        order = [(i % taps) * cpt + i // taps for i in range(nch)]
        ks = geo["ksplit"]
        return [order[nch * s // ks: nch * (s + 1) // ks] for s in range(ks)]
    if f.kernel == "xs":
        ks = geo.get("ksplit", 1)
        return [list(range(s * (nch // ks), (s + 1) * (nch // ks))) for s in range(ks)]
    cpt = c.ldx_ // 32  # ks: (slice, tap, chunk of the slice)
    taps = c.K // c.ldx_
    return [[t * cpt + s * 4 + xc for s in range(cpt // 4) for t in range(taps) for xc in range(4)]]


def kernel_order_model(c: Case, d: dict, rows: slice = slice(None)) -> np.ndarray:
    """An honest fp32 evaluation in the kernel's own order on the CPU, of the output rows ``rows``.  v_mfma_f32_16x16x4_f32
    (gemm_kernel, gemm_rows_kernel: 8 per chunk) is a chain of four fused multiply-adds over k = 8 q + j, q = 0..3, one fp32
    rounding each (modelled as ONE exact 4-product sum it stays at half the noise the kernel shows at K = 1024: 1.25 | 1.11 against
    2.45 | 1.93); v_mfma_f32_16x16x32_bf16 adds four exact sums of 8 products, one fp32 rounding each (the grain of
    tests/gemm3_strict_helpers.py), the piece products smallest first as mfma_b3 issues them.  Prologues in fp32 torch; the
    epilogue in fp32."""
    f = c.form()
    w = d["w"].double()
    a32 = operand(c, d, torch.float32)[rows]
    Mr = a32.shape[0]
    v = torch.zeros(Mr, c.N)
    if f.kernel in ("gemm", "rows"):
        a = a32.double()
        for part in chunk_parts(c):
            acc = torch.zeros(Mr, c.N)
            for ch in part:
                for j in range(8):
                    for q in range(4):
                        k = ch * 32 + 8 * q + j
                        acc = (acc.double() + a[:, k:k + 1] * w[:, k][None]).float()
            v = v + acc
    else:
        xp = [p.double() for p in split3(a32)]
        wp = [p.double() for p in split3(d["w"])]
        pairs = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)) if c.products != 3 else ((1, 0), (0, 1), (0, 0))
        for part in chunk_parts(c):
            acc = torch.zeros(Mr, c.N)
            for ch in part:
                for (wi, xi) in pairs:
                    for k0 in range(ch * 32, ch * 32 + 32, 8):
                        acc = (acc.double() + xp[xi][:, k0:k0 + 8] @ wp[wi][:, k0:k0 + 8].T).float()
            v = v + acc
    if c.pro == RMSNORM:
        v = v * rstd(d["A"])[rows]
    full = {k: (t[rows] if k == "resid" else t) for k, t in d.items()}
    if c.epi == QKV:
        full["row_pos"] = d["row_pos"][rows]
    sub = c._replace(M=Mr)
    return epilogue(sub, full, v)[0].numpy()


def ref_rows(ref: Ref, rows: slice) -> Ref:
    return ref._replace(ref64=ref.ref64[rows], S=ref.S[rows], ref32=ref.ref32[rows], extra=None if ref.extra is None else ref.extra[rows])


# ------------------------------------------------------------------------------------------------ the judge
def output_name(c: Case, n: int, which: str = "out") -> str:
    """Which output holds column n of the judged matrix."""
    if c.epi == QKV:
        Hq, Hkv = c.heads
        return "out" if n < Hq * 64 else ("K row" if n < (Hq + Hkv) * 64 else "V row")
    return which


def judge(c: Case, form: Form, got: np.ndarray, ref: Ref, which: str = "out", allow: bool = True, factor: float = FACTOR):
    """``got`` [M, cols] against ref.ref64 -> (failure messages, worst max ratio, worst rms ratio).  ``allow``: take ref.extra (the
    hardware exponential's absolute allowance) off the error before the ratios are formed."""
    assert got.shape == ref.ref64.shape, (got.shape, ref.ref64.shape)
    msgs = []
    head = f"{c.id} [{form}]"
    if not np.isfinite(got).all():
        m, n = np.argwhere(~np.isfinite(got))[0]
        return [f"{head}: {output_name(c, n, which)} row {m} column {n} is {got[m, n]}"], np.inf, np.inf
    live = ref.S > 0
    dead = ~live & (got != 0)
    if dead.any():  # S == 0: an all-zero operand row without bias or residual
        m, n = np.argwhere(dead)[0]
        msgs.append(f"{head}: {output_name(c, n, which)} row {m} column {n}: got {got[m, n]:.9g} where the scale is 0, exact 0 expected")
    e = noise(got, ref.ref64, ref.S, ref.extra if allow else None)
    m, n = np.unravel_index(int(e.argmax()), e.shape)
    we, wr = float(e[m, n]) / ref.E_ref, rms(e[live]) / ref.R_ref
    where = (f"worst at {output_name(c, n, which)} row {m} column {n} (tile {m // 16}, {n // 16}): got {got[m, n]:.9g}, float64 {ref.ref64[m, n]:.9g}, "
             f"S {ref.S[m, n]:.3e}")
    if we > factor or wr > factor:
        msgs.append(f"{head}: max e {e[m, n]:.3e} = {we:.2f} x E_ref ({ref.E_ref:.3e}), rms e = {wr:.2f} x R_ref ({ref.R_ref:.3e}), "
                    f"bound {factor:g}; {where}")
    M, cols = e.shape  # every 16 x 16 tile on its own
    Mp, Np = (M + 15) // 16 * 16, (cols + 15) // 16 * 16
    e2, cnt = np.zeros((Mp, Np)), np.zeros((Mp, Np))
    e2[:M, :cols], cnt[:M, :cols] = np.square(e), live
    e2 = e2.reshape(Mp // 16, 16, Np // 16, 16).sum((1, 3))
    cnt = cnt.reshape(Mp // 16, 16, Np // 16, 16).sum((1, 3))
    trms = np.sqrt(np.divide(e2, cnt, out=np.zeros_like(e2), where=cnt > 0))
    tm, tn = np.unravel_index(int(trms.argmax()), trms.shape)
    if trms[tm, tn] > factor * ref.R_ref:
        blk = e[tm * 16:tm * 16 + 16, tn * 16:tn * 16 + 16]
        bm, bn = np.unravel_index(int(blk.argmax()), blk.shape)
        m, n = tm * 16 + int(bm), tn * 16 + int(bn)
        msgs.append(f"{head}: tile ({tm}, {tn}) rms e = {trms[tm, tn] / ref.R_ref:.2f} x R_ref ({ref.R_ref:.3e}), bound {factor:g} (whole output: "
                    f"max {we:.2f} x E_ref, rms {wr:.2f} x R_ref); its worst element: {output_name(c, n, which)} row {m} column {n}: got {got[m, n]:.9g}, "
                    f"float64 {ref.ref64[m, n]:.9g}, e = {e[m, n] / ref.E_ref:.2f} x E_ref")
    return msgs, we, wr


# ------------------------------------------------------------------------------------------------ the launch (GPU)
def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def _nan_buffer(M: int, T: int, ld: int, bstride: int, cols: int):
    """(flat NaN buffer with LEAD floats in front and a tail margin, int64 index [M, cols] of every addressed element)."""
    ro = row_offsets(M, T, ld, bstride)
    idx = LEAD + ro[:, None] + torch.arange(cols)[None]
    return torch.full((int(idx.max()) + 1 + LEAD,), float("nan")), idx


def margin_written(buf: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Flat positions outside ``idx`` that no longer hold the NaN they were filled with."""
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    keep[idx.flatten()] = False
    blank = torch.full_like(buf, float("nan"))
    return ((buf.view(torch.int32) != blank.view(torch.int32)) & keep).nonzero().flatten()


def run_case(E, ops, c: Case, d: dict, ws_mode: Optional[str] = None) -> dict:
    """One launch of the case on the GPU -> CPU tensors of everything it wrote: out / raw [M, cols] gathered from NaN-filled buffers,
    ``*_margin`` the margin positions that were written, the caches whole."""
    dev = "cuda"
    M, K, N = c.M, c.K, c.N
    w = d["w"]
    kw = dict(w_fp32=c.w_fp32, prologue=c.pro, epilogue=c.epi, eps=EPS, M=M, K=K, ldx=c.ldx_, x_bstride=c.x_bstride, rows_per_batch=c.T,
              ldo=c.ldo, o_bstride=c.o_bstride, elu_out=c.elu_out, b3_products=c.products)
    if c.w3:
        kw["w3"] = ops.pack_weight_w3(w)
    if d["bias"] is not None:
        kw["bias"] = d["bias"].to(dev)
    if c.pro in (RMSNORM, LAYERNORM):
        kw["gamma"] = d["gamma"].to(dev)
    if c.pro == LAYERNORM:
        kw["beta"] = d["beta"].to(dev)
        kw["ln_scratch"] = torch.full((M, K), float("nan"), device=dev)
    obuf, oidx = _nan_buffer(M, c.T, c.ldo, c.o_bstride, c.out_cols)
    if c.epi in (RESID, SCALE_RESID):
        if c.inplace:
            obuf[oidx] = d["resid"]
        else:
            rbuf, ridx = _nan_buffer(M, c.T, c.ldr, c.r_bstride, N)
            rbuf[ridx] = d["resid"]
            kw.update(resid=rbuf.to(dev)[LEAD:], ldr=c.ldr, r_bstride=c.r_bstride)
    obuf = obuf.to(dev)
    if c.inplace:
        kw["resid"] = obuf[LEAD:]
    if c.epi == SCALE_RESID:
        kw["scale"] = d["scale"].to(dev)
    if c.raw_out:
        rawbuf, rawidx = _nan_buffer(M, c.T, c.ldo, c.raw_bstride, N)
        rawbuf = rawbuf.to(dev)
        kw.update(raw_out=rawbuf[LEAD:], raw_bstride=c.raw_bstride)
    ws_mode = c.ws if ws_mode is None else ws_mode
    if ws_mode:
        kw["splitk_ws"] = torch.full((4 * M * N if ws_mode == "full" else M * N,), float("nan"), device=dev)
    if c.epi == QKV:
        Hq, Hkv = c.heads
        L = c.cache_len
        kc = torch.full((SLOTS, Hkv, L, 64), SENTINEL, device=dev)
        vc = torch.full((SLOTS, Hkv, L, 64), SENTINEL, device=dev)
        rope = d["rope_full"].to(dev)
        kw.update(rope=rope[1:], row_pos=d["row_pos"].to(dev), row_slot=d["row_slot"].to(dev), k_cache=kc, v_cache=vc, n_q_heads=Hq,
                  n_kv_heads=Hkv, cache_len=L)
        if c.kv3:
            kw["k_cache3"], kw["v_cache3"] = ops.kv3_cache(SLOTS, Hkv, L), ops.kv3_cache(SLOTS, Hkv, L)
    ops.linear(d["xbuf"].to(dev), ops.pack_weight(w, fp32=c.w_fp32), N, out=obuf[LEAD:], **kw)
    torch.cuda.synchronize()
    ocpu = obuf.cpu()
    res = {"out": ocpu[oidx], "out_margin": margin_written(ocpu, oidx)}
    if c.raw_out:
        rcpu = rawbuf.cpu()
        res["raw"], res["raw_margin"] = rcpu[rawidx], margin_written(rcpu, rawidx)
    if c.epi == QKV:
        res["k_cache"], res["v_cache"] = kc.cpu(), vc.cpu()
        if c.kv3:
            res["k3"], res["v3"] = ops.kv3_decode(kw["k_cache3"], L, False), ops.kv3_decode(kw["v_cache3"], L, True)
    return res


def same_results(a: dict, b: dict) -> list:
    """Names of the results of two runs that differ in any bit."""
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]
