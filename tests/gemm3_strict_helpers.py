"""The per-element measure of the bf16x3 GEMM (csrc/gemm3.hip: gemm3_kernel, gemm3_rows_kernel) and its case matrix.

Shared by tests/test_gemm3_strict_gpu.py (every launch form against float64) and tests/test_gemm3_strict_cpu.py (the premises:
what the measure rejects, and which launch forms the matrix reaches).  GPU-free at import.

The measure.  For a case the float64 reference is worked out from a = fp32(x gamma), exactly what the X3 operand holds,
r = rsqrt(mean(x^2) + eps) (1 without the RMSNorm prologue), the dot products y = r sum a_k w_k and their condition scales
s = r sum |a_k| |w_k|; both go through the epilogue, which gives ref64 and a per-element scale S (``reference``).  The judged
quantity is e = |got - ref64| / S per element; the reference's own noise is the same quantity for ref32, the plain fp32 torch
evaluation in the oracle's order.  A case pools E_ref = max e(ref32) and R_ref = rms e(ref32) over its whole output and requires
max e(got) <= FACTOR E_ref, rms e(got) <= FACTOR R_ref, and rms e(got) <= FACTOR R_ref in every 16 x 16 tile (``judge``).
The CPU stand-ins that go through the same judge: ``two_piece_model`` and ``one_moved`` (must be rejected) and
``kernel_order_model``, fp32 accumulation in the kernels' own K order (must pass)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from lm_strict_helpers import FACTOR, half_ulp_bf16, rms, two_pieces  # noqa: F401  (FACTOR: the project's rule, no other number)

EPS = 1e-5
STORE, RESID, SWIGLU, QKV = 0, 1, 2, 5  # SMOLTTS_EPI_* (include/smoltts_hip.h)
EPI_NAMES = {STORE: "store", RESID: "resid", SWIGLU: "swiglu", QKV: "qkv"}
SLOTS = 5        # QKV_ROPE: cache slots; cache_len is sized so that slots x cache_len > M
SENTINEL = 1.5   # prefill of the K / V caches (a bf16 value)
U32 = 2.0 ** -24  # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ the launch mirror
class Form(NamedTuple):
    """What launch_gemm3 launches: gemm3_kernel<MT, T, U, EPI, W8, NT, NW> with ``half_rows`` (a launch argument, still part of
    the form) or, kind == "rows", gemm3_rows_kernel<NTW, EPI, W8> (MT = T = U = NW = 0 then)."""
    kind: str
    MT: int
    T: int
    U: int
    NW: int
    half_rows: int
    NTW: int
    epi: int
    w8: bool
    nt: bool

    @property
    def geometry(self) -> tuple:
        return (self.kind, self.MT, self.T, self.U, self.NW, self.half_rows, self.NTW)

    @property
    def instance(self) -> tuple:
        """The template instantiation behind the form, as tests/test_gemm3_strict_cpu.py reads it out of the library."""
        if self.kind == "rows":
            return ("rows", self.NTW, self.epi, self.w8)
        return ("one", self.MT, self.T, self.U, self.epi, self.w8, self.nt, self.NW)

    def __str__(self) -> str:
        tail = f"{EPI_NAMES[self.epi]}{', fp8 weights' if self.w8 else ''}{', streamed weights' if self.nt else ''}"
        if self.kind == "rows":
            return f"gemm3_rows_kernel<NTW={self.NTW}> ({tail})"
        return f"gemm3_kernel<MT={self.MT}, T={self.T}, U={self.U}, NW={self.NW}> half_rows={self.half_rows} ({tail})"


def launch_form(M: int, K: int, N: int, epi: int, w8: bool = False, w_stream: bool = False) -> Form:
    """Mirror of launch3_fmt, launch3_one and launch3_rows (gemm3.hip) without fp8_activations."""
    nchunks, ntiles = K // 32, (N + 15) // 16
    nwaves = min(8, max(1, (nchunks + 2) // 3))
    cpw = (nchunks + nwaves - 1) // nwaves
    if M >= 256:  # launch3_rows
        NTW = 4 if ntiles >= 16 else (2 if ntiles >= 8 else 1)
        row_blocks = (M + 63) // 64
        while NTW > 1 and ((ntiles + 4 * NTW - 1) // (4 * NTW)) * row_blocks < 256:
            NTW >>= 1
        return Form("rows", 0, 0, 0, 0, 0, NTW, epi, w8, False)
    half = 0
    if M > 128:
        MT, T, U, nwaves = 4, 1, 2, max(nwaves, 4)
    else:
        MT = 1
        row_tiles = (M + 15) // 16
        wg_limit = 128 * row_tiles if row_tiles > 2 else 256
        T = 1
        while T < 4 and ((ntiles + T - 1) // T) * row_tiles > wg_limit:
            T += 1
        if T > 1:
            U = 3
        else:
            half = 1 if (M > 8 and ntiles * row_tiles * 2 <= wg_limit) else 0
            U = 12 if cpw > 6 else (6 if cpw > 3 else 3)
    nwaves = max(nwaves, MT * T)  # launch3_one
    NW = nwaves if (MT == 1 and nwaves in (8, 6) and nchunks == nwaves * U and ntiles % T == 0) else 0
    return Form("one", MT, T, U, NW, half, 0, epi, w8, bool(w_stream) and MT == 1)


ENGINE_CONFIGS = ("tiny", "tiny_proj", "smoltts_byte_70m", "smoltts_byte_150m")
ENGINE_MS = tuple(range(1, 256)) + (256, 300, 520, 700, 1024, 2048, 3500)


def engine_gemms(cfg) -> list:
    """(what, epilogue, K, N, streamed?) of every weight GEMM lm_engine.hip sends through launch_gemm3 for a config; streamed?
    says whether some SMOLTTS_STREAM_W_* bit reaches the launch's w_stream (run_block, run_tail, run_slow_layers: the slow blocks
    only at M <= 128; smoltts_engine_build_fast_qkv and the fast_project_in Linear never set it)."""
    out = []

    def block(tag, dim, n_head, n_kv, inter):
        out.append((f"{tag} wqkv", QKV, dim, (n_head + 2 * n_kv) * 64, True))
        out.append((f"{tag} wo", RESID, dim, dim, True))
        out.append((f"{tag} w1|w3", SWIGLU, dim, 2 * inter, True))
        out.append((f"{tag} w2", RESID, inter, dim, True))

    block("slow", cfg.dim, cfg.n_head, cfg.n_local_heads, cfg.intermediate_size)
    out.append(("slow head", STORE, cfg.dim, cfg.vocab_size, True))
    if cfg.fast_dim != cfg.dim:
        out.append(("fast_project_in", STORE, cfg.dim, cfg.fast_dim, False))
    block("depth", cfg.fast_dim, cfg.fast_n_head, cfg.fast_n_local_heads, cfg.fast_intermediate_size)
    out.append(("depth head", STORE, cfg.fast_dim, cfg.codebook_size, True))
    out.append(("fast_qkv table", STORE, cfg.fast_dim, (cfg.fast_n_head + 2 * cfg.fast_n_local_heads) * 64, False))
    return out


def engine_forms() -> dict:
    """{form: an example "config what M=.."} over the named configs, both weight formats, w_stream as the engine can set it
    and every M of ENGINE_MS (the fast_qkv table is built in launches of <= 128 rows)."""
    from smoltts_amd.synthetic import named_config

    forms = {}
    for name in ENGINE_CONFIGS:
        for what, epi, K, N, streamed in engine_gemms(named_config(name)):
            for M in ENGINE_MS:
                if what == "fast_qkv table" and M > 128:
                    continue
                for w8 in (False, True):
                    for ws in ((False, True) if streamed else (False,)):
                        forms.setdefault(launch_form(M, K, N, epi, w8, ws), f"{name} {what} M={M} K={K} N={N}")
    return forms


# ------------------------------------------------------------------------------------------------ the case matrix
class Case(NamedTuple):
    M: int
    K: int
    N: int
    epi: int
    w8: bool = False
    norm: bool = True      # RMSNorm prologue (ssq_in); the engine's RESID launches (wo, w2) have none
    kv_bf16: bool = False  # QKV_ROPE: bf16 K / V caches

    @property
    def id(self) -> str:
        return (f"{EPI_NAMES[self.epi]}-M{self.M}-K{self.K}-N{self.N}" + ("-w8" if self.w8 else "") +
                ("" if self.norm or self.epi == RESID else "-nonorm") + ("-kvbf16" if self.kv_bf16 else ""))

    @property
    def streams(self) -> bool:
        """Decode forms (gemm3_kernel with MT = 1) run with w_stream on and off."""
        return self.M <= 128

    def form(self, w_stream: bool = False) -> Form:
        return launch_form(self.M, self.K, self.N, self.epi, self.w8, w_stream)

    @property
    def heads(self) -> tuple:
        """(query heads, kv heads) of a QKV_ROPE case: N = (Hq + 2 Hkv) * 64."""
        t = self.N // 64
        kv = max(1, t // 5)
        return t - 2 * kv, kv

    @property
    def cache_len(self) -> int:
        return (self.M + SLOTS - 1) // SLOTS + 3


# gemm3_kernel<1, 1, U, .., NW>: general (K = 384, 128), predicate-free with 6 and 8 waves, U = 6 and U = 12; each at whole rows
# (M <= 8) and at half rows (M > 8), M = 16 / 17 / 33: one full tile, one tile + one row, three tiles
T1_SHAPES = [(384, 384), (128, 128), (576, 576), (768, 768), (1536, 576), (3072, 768)]
T1_MS = [1, 8, 9, 16, 17, 33, 128]
SHAPES = [(M, K, N) for (K, N) in T1_SHAPES for M in T1_MS] + [
    # T = 2: general, NW = 6, NW = 8;  T = 3
    (17, 128, 2368), (17, 576, 2368), (1, 768, 6144), (16, 768, 6144), (17, 768, 6144), (100, 768, 6144),
    # MT = 4 (129..255 rows, 64 per workgroup)
    (129, 576, 960), (193, 576, 960), (255, 576, 960), (129, 128, 128), (193, 128, 128), (255, 128, 128),
    # many rows: NTW = 1, 1, 2, 4
    (256, 768, 2368), (257, 1536, 576), (1024, 128, 2048), (700, 768, 6144),
    # column edges of the general form: N no multiple of 64 or of T tiles; the predicate-free shapes with one more tile
    (5, 384, 48), (33, 384, 48), (1, 768, 2368), (33, 768, 2368), (16, 576, 592), (5, 768, 784), (32, 1536, 592), (16, 3072, 784),
    (16, 768, 6160),
]


def allowed(M: int, K: int, N: int, epi: int, w8: bool) -> bool:
    """launch_gemm3_impl's requirements on a shape (the matrix leaves out what the launch refuses)."""
    if w8 and N % 16:
        return False
    if epi == SWIGLU:
        return N % 64 == 0
    if epi == QKV:
        return N % 64 == 0 and N >= 192
    return True


def cases() -> list:
    out, seen = [], set()
    for (M, K, N) in SHAPES:
        for epi in (STORE, RESID, SWIGLU, QKV):
            for w8 in (False, True):
                if not allowed(M, K, N, epi, w8):
                    continue
                c = Case(M, K, N, epi, w8, norm=epi != RESID)
                if c not in seen:
                    seen.add(c)
                    out.append(c)
    # the fast_project_in Linear: STORE with bias and emission, no RMSNorm prologue
    out += [Case(M, 384, 128, STORE, w8, norm=False) for M in (1, 9, 33) for w8 in (False, True)]
    # bf16 K / V caches: one case per kernel (decode whole / half rows, T = 2, MT = 4, many rows)
    out += [Case(M, K, N, QKV, w8, kv_bf16=True) for (M, K, N) in ((1, 576, 576), (17, 768, 768), (17, 576, 2368), (129, 576, 960), (257, 1536, 576))
            for w8 in (False, True)]
    return out


CASES = cases()


# ------------------------------------------------------------------------------------------------ inputs and references (CPU)
def bf16r(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def make_inputs(c: Case) -> dict:
    """Rows of x over logspace(-3, 3) (some with mean(x^2) below eps), one all-zero row, weight rows over logspace(-3, 0)."""
    from smoltts_amd.packing import dequantize_fp8_rows, rope_table

    g = torch.Generator().manual_seed(((c.M * 4099 + c.K) * 4099 + c.N) * 16 + c.epi * 2 + int(c.w8))
    M, K, N = c.M, c.K, c.N
    rowscale = torch.logspace(-3, 3, M)[torch.randperm(M, generator=g)] if M > 1 else torch.tensor([0.7])
    colscale = torch.logspace(-3, 0, N)[torch.randperm(N, generator=g)]
    if c.epi in (SWIGLU, QKV):  # a gate and its up column share a scale, and so do the two columns of a rotated pair
        colscale = colscale.view(N // 2, 2)[:, :1].expand(N // 2, 2).reshape(N)
    x = torch.randn(M, K, generator=g) * rowscale[:, None]
    zero_row = (3 * M) // 7 if M > 1 else -1
    if zero_row >= 0:
        x[zero_row] = 0.0
    w_raw = torch.randn(N, K, generator=g) * 0.05 * colscale[:, None]
    w = dequantize_fp8_rows(w_raw) if c.w8 else bf16r(w_raw)
    d = dict(x=x, w=w, w_raw=w_raw, zero_row=zero_row, gamma=(1 + 0.2 * torch.randn(K, generator=g)) if c.norm else None)
    ymag = colscale[None] * (rowscale[:, None] if not c.norm else torch.ones(M, 1))  # the size of y, up to sqrt(K) 0.05
    if c.epi == STORE:
        d["bias"] = torch.randn(N, generator=g) * 0.5 * colscale
    if c.epi == RESID:
        d["resid"] = torch.randn(M, N, generator=g) * 0.5 * ymag
    if c.epi in (STORE, RESID) and N % 64 == 0:
        d["gamma_a"] = 1 + 0.2 * torch.randn(N, generator=g)
        d["gamma_b"] = 1 + 0.2 * torch.randn(N, generator=g)
    if c.epi == QKV:
        L = c.cache_len
        pairs = torch.randperm(SLOTS * L, generator=g)[:M]
        d["row_slot"], d["row_pos"] = (pairs // L).int(), (pairs % L).int()
        d["rope"] = rope_table(L, 64, 100000.0, bf16=True)
    return d


class Ref(NamedTuple):
    ref64: np.ndarray  # float64 [M, cols]
    S: np.ndarray      # float64 [M, cols], the per-element scale (0 exactly on the all-zero row of a case without bias / resid)
    ref32: np.ndarray  # float32 [M, cols]
    E_ref: float
    R_ref: float


def rstd32(x: torch.Tensor) -> torch.Tensor:
    return torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS)


def _rope_cs(c: Case, d: dict, dtype):
    """(cos, sin) [M, N / 2] of every column pair: the row's table entry below (Hq + Hkv) * 64, (1, 0) in the V columns."""
    Hq, Hkv = c.heads
    cs = d["rope"][d["row_pos"].long()].to(dtype)  # [M, 32, 2]
    cos = torch.ones(c.M, c.N // 2, dtype=dtype)
    sin = torch.zeros(c.M, c.N // 2, dtype=dtype)
    nrot = (Hq + Hkv) * 32
    cos[:, :nrot] = cs[:, :, 0].repeat(1, Hq + Hkv)
    sin[:, :nrot] = cs[:, :, 1].repeat(1, Hq + Hkv)
    return cos, sin


def epilogue(c: Case, d: dict, y: torch.Tensor, s: Optional[torch.Tensor] = None):
    """The epilogue in y's dtype -> result [M, cols]; with the condition scales ``s`` also the per-element scale S."""
    dt = y.dtype
    S = None
    if c.epi == STORE:
        b = d["bias"].to(dt)[None]
        out = y + b
        if s is not None:
            S = s + b.abs()
    elif c.epi == RESID:
        r = d["resid"].to(dt)
        out = r + y
        if s is not None:
            S = s + r.abs()
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
    return out, S


def operand32(c: Case, d: dict) -> torch.Tensor:
    """fp32(x gamma): what the X3 operand holds (tests/test_gemm3_gpu.py::test_x3_pack_roundtrip)."""
    return d["x"] * d["gamma"] if c.norm else d["x"]


def reference32(c: Case, d: dict) -> torch.Tensor:
    """The plain fp32 torch evaluation in the oracle's order: fp32 RMSNorm of x times gamma, @ w.T, the epilogue in fp32."""
    x = d["x"]
    n = x * rstd32(x) * d["gamma"] if c.norm else x
    return epilogue(c, d, n @ d["w"].T)[0]


def noise(res: np.ndarray, ref64: np.ndarray, S: np.ndarray) -> np.ndarray:
    """e = |res - ref64| / S per element, 0 where S == 0 (the all-zero row: held to exact zeros instead)."""
    diff = np.abs(res.astype(np.float64) - ref64)
    return np.divide(diff, S, out=np.zeros_like(diff), where=S > 0)


def reference(c: Case, d: dict) -> Ref:
    x = d["x"].double()
    a = operand32(c, d).double()
    w = d["w"].double()
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS) if c.norm else torch.ones(c.M, 1, dtype=torch.float64)
    y = r * (a @ w.T)
    s = r * (a.abs() @ w.abs().T)
    ref64, S = epilogue(c, d, y, s)
    ref64, S, ref32 = ref64.numpy(), S.numpy(), reference32(c, d).numpy()
    e = noise(ref32, ref64, S)
    live = S > 0
    assert live.any() and np.isfinite(ref64).all()
    E_ref, R_ref = float(e[live].max()), rms(e[live])
    assert E_ref > 0.0 and R_ref > 0.0
    return Ref(ref64, S, ref32, E_ref, R_ref)


def two_piece_model(c: Case, d: dict) -> np.ndarray:
    """The kernel's arithmetic in fp32 on the CPU with the operand cut to two bf16 pieces: 2^-16-grade, must be rejected."""
    y = two_pieces(operand32(c, d)) @ d["w"].T
    if c.norm:
        y = y * rstd32(d["x"])
    return epilogue(c, d, y)[0].numpy()


def split3(a: torch.Tensor):
    """fp32 -> the (hi, mid, lo) bf16 pieces of the X3 operand as fp32 tensors; hi + mid + lo == a."""
    hi = bf16r(a)
    mid = bf16r(a - hi)
    return hi, mid, bf16r(a - hi - mid)


def kernel_waves(c: Case) -> int:
    """K parts of the launch: gemm3_kernel's waves (launch3_fmt / launch3_one), 1 for the many-row kernel (no split-K)."""
    f = c.form()
    if f.kind == "rows":
        return 1
    return max(min(8, max(1, (c.K // 32 + 2) // 3)), 4 if f.MT == 4 else 1, f.MT * f.T)


def kernel_order_model(c: Case, d: dict, grain: int = 8) -> np.ndarray:
    """An honest fp32 evaluation in the kernels' own order, on the CPU (bf16 weights): 32-k chunk ch belongs to K part ch % parts;
    a part adds the hi, mid and lo products of its chunks one MFMA after the other into one fp32 accumulator, the partial tiles are
    added in part order, then the row scale and the epilogue.  One MFMA = exact sums of ``grain`` products, one fp32 rounding
    each: 8 (the 8 k values a lane holds, four such sums per instruction) reproduces the figures measured on the MI355X to the
    digit (tests/test_gemm3_strict_gpu.py); 32 would be the whole instruction as one exact sum."""
    assert not c.w8 and 32 % grain == 0
    w = d["w"].double()
    pieces = [p.double() for p in split3(operand32(c, d))]
    parts, nchunks = kernel_waves(c), c.K // 32
    v = torch.zeros(c.M, c.N)
    for part in range(parts):
        acc = torch.zeros(c.M, c.N)
        for ch in range(part, nchunks, parts):
            for p in pieces:
                for k0 in range(ch * 32, ch * 32 + 32, grain):
                    acc = (acc.double() + p[:, k0:k0 + grain] @ w[:, k0:k0 + grain].T).float()
        v = v + acc
    if c.norm:
        v = v * rstd32(d["x"])
    return epilogue(c, d, v)[0].numpy()


def one_moved(ref: Ref):
    """ref32 with the element of the smallest S > 0 moved by 2^-16 S -> (result, (row, column))."""
    Sm = np.where(ref.S > 0, ref.S, np.inf)
    m, n = np.unravel_index(int(Sm.argmin()), Sm.shape)
    res = ref.ref32.copy()
    res[m, n] = np.float32(res[m, n] + np.float32(2.0 ** -16 * ref.S[m, n]))
    return res, (int(m), int(n))


# ------------------------------------------------------------------------------------------------ the judge
def output_name(c: Case, n: int) -> str:
    """Which epilogue output holds column n of the judged matrix."""
    if c.epi == SWIGLU:
        return "x3_out"
    if c.epi == QKV:
        Hq, Hkv = c.heads
        return "out" if n < Hq * 64 else ("K row" if n < (Hq + Hkv) * 64 else "V row")
    return "out"


def judge(c: Case, form: Form, got: np.ndarray, ref: Ref, extra: Optional[np.ndarray] = None, factor: float = FACTOR):
    """``got`` [M, cols] against ref.ref64 -> (failure messages, worst max ratio, worst rms ratio).  ``extra`` [M, cols]: an
    allowance in units of S on top of the fp32 bound of every element (bf16 cache rows: half a bf16 ulp of ref64), taken off the
    error before the ratios are formed."""
    assert got.shape == ref.ref64.shape, (got.shape, ref.ref64.shape)
    msgs = []
    head = f"{c.id} [{form}]"
    if not np.isfinite(got).all():
        m, n = np.argwhere(~np.isfinite(got))[0]
        return [f"{head}: {output_name(c, n)} row {m} column {n} is {got[m, n]}"], np.inf, np.inf
    diff = np.abs(got.astype(np.float64) - ref.ref64)
    if extra is not None:
        diff = np.maximum(diff - extra, 0.0)
    live = ref.S > 0
    dead = ~live & (got != 0)
    if dead.any():  # S == 0: the all-zero row of a case with neither bias nor residual
        m, n = np.argwhere(dead)[0]
        msgs.append(f"{head}: {output_name(c, n)} row {m} column {n}: got {got[m, n]:.9g} for an all-zero input row, exact 0 expected")
    e = np.divide(diff, ref.S, out=np.zeros_like(diff), where=live)
    m, n = np.unravel_index(int(e.argmax()), e.shape)
    we, wr = float(e[m, n]) / ref.E_ref, rms(e[live]) / ref.R_ref
    where = (f"worst at {output_name(c, n)} row {m} column {n} (tile {m // 16}, {n // 16}): got {got[m, n]:.9g}, float64 {ref.ref64[m, n]:.9g}, "
             f"S {ref.S[m, n]:.3e}")
    if we > factor or wr > factor:
        msgs.append(f"{head}: max e {e[m, n]:.3e} = {we:.2f} x E_ref ({ref.E_ref:.3e}), rms e = {wr:.2f} x R_ref ({ref.R_ref:.3e}), "
                    f"bound {factor:g}; {where}")
    # every 16 x 16 tile on its own
    M, cols = e.shape
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
                    f"max {we:.2f} x E_ref, rms {wr:.2f} x R_ref); its worst element: {output_name(c, n)} row {m} column {n}: got {got[m, n]:.9g}, "
                    f"float64 {ref.ref64[m, n]:.9g}, e = {e[m, n] / ref.E_ref:.2f} x E_ref")
    return msgs, we, wr


# ------------------------------------------------------------------------------------------------ the launch (GPU)
PAD_ROWS, PAD_COLS = 1, 4  # out is allocated one row and four columns too large (ldo = N + 4) and prefilled with NaN


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def run_case(E, ops, c: Case, d: dict, w_stream: bool = False) -> dict:
    """One launch of the case on the GPU -> CPU tensors of everything it wrote (whole buffers, margins and sentinels included)."""
    M, K, N = c.M, c.K, c.N
    dev = "cuda"
    x3, _, ssq = ops.x3_pack(d["x"].to(dev), d["gamma"].to(dev) if c.norm else None)
    if c.w8:
        wt, scale, wdq = ops.pack_weight_fp8(d["w_raw"])
        assert torch.equal(wdq, d["w"])
    else:
        wt, scale = ops.pack_weight(d["w"]), None
    kw = dict(epilogue={STORE: E.EPI_STORE, RESID: E.EPI_RESID, SWIGLU: E.EPI_SWIGLU, QKV: E.EPI_QKV_ROPE}[c.epi],
              ssq_in=ssq if c.norm else None, eps=EPS, w_scale=scale, w_stream=w_stream)
    res = {}
    emits = c.epi in (STORE, RESID) and N % 64 == 0
    if c.epi in (STORE, RESID):
        out = torch.full((M + PAD_ROWS, N + PAD_COLS), float("nan"))
        if c.epi == RESID:
            out[:M, :N] = d["resid"]
        out = out.to(dev)
        if c.epi == STORE:
            kw["bias"] = d["bias"].to(dev)
            if M < 256:
                kw["cand_out"] = cand = torch.full((M + 1, (N + 15) // 16, 4), float("nan"), device=dev)
        else:
            kw["resid"] = out  # in place
        if emits:
            kw["emit_a"], kw["gamma_a"] = ops.x3_alloc(M, N), d["gamma_a"].to(dev)
            kw["ssq_out"] = torch.full((M + 1, N // 16), float("nan"), device=dev)
            if c.epi == RESID:
                kw["emit_b"], kw["gamma_b"] = ops.x3_alloc(M, N), d["gamma_b"].to(dev)
        ops.linear3(x3, wt, M, N, K, out=out, **kw)
        res["out_buf"] = out.cpu()
        R16 = (M + 15) // 16 * 16
        for k in ("emit_a", "emit_b"):
            if k in kw:
                res[k] = ops.x3_to_float(kw[k], R16, N)
        if emits:
            res["ssq_out"] = kw["ssq_out"].cpu()
        if "cand_out" in kw:
            res["cand"] = cand.cpu()
    elif c.epi == SWIGLU:
        hout = ops.x3_alloc(M, N // 2)
        ops.linear3(x3, wt, M, N, K, x3_out=hout, **kw)
        res["x3_out"] = ops.x3_to_float(hout, (M + 15) // 16 * 16, N // 2)
    else:
        Hq, Hkv = c.heads
        L = c.cache_len
        cdt = torch.bfloat16 if c.kv_bf16 else torch.float32
        kc = torch.full((SLOTS, Hkv, L, 64), SENTINEL, dtype=cdt, device=dev)
        vc = torch.full((SLOTS, Hkv, L, 64), SENTINEL, dtype=cdt, device=dev)
        out = torch.full((M + PAD_ROWS, Hq * 64 + PAD_COLS), float("nan"), device=dev)
        ops.linear3(x3, wt, M, N, K, out=out, rope=d["rope"].to(dev), row_pos=d["row_pos"].to(dev), row_slot=d["row_slot"].to(dev),
                    k_cache=kc, v_cache=vc, n_q_heads=Hq, n_kv_heads=Hkv, cache_len=L, kv_format=E.KV_BF16 if c.kv_bf16 else E.KV_F32, **kw)
        res["out_buf"], res["k_cache"], res["v_cache"] = out.cpu(), kc.cpu(), vc.cpu()
    torch.cuda.synchronize()
    return res


def same_results(a: dict, b: dict) -> list:
    """Names of the results of two runs that differ in any bit."""
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]
