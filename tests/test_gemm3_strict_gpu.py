"""The bf16x3 GEMM (csrc/gemm3.hip), per element and per launch form, against float64.

tests/test_gemm3_gpu.py, tests/test_gemm3_rows_gpu.py and tests/test_fp8_gpu.py hold max|got - fp32 torch| / max|ref| < 2e-5: ten
times what a 2^-16-grade kernel needs, normalised by the largest output of the whole matrix (blind to one small column, one
ragged tile edge, one row of a half-row split), and without a case for several launch forms.  Here every form that launch_gemm3
can take for the named configs (tests/gemm3_strict_helpers.py: 18 geometries x epilogue x weight format x w_stream; the CPU
test tests/test_gemm3_strict_cpu.py proves the coverage and that the measure rejects a two-piece operand and one moved element)
runs on inputs over a wide dynamic range and is judged per element:
    e = |got - ref64| / S,   S = the element's condition scale pushed through the epilogue,
    max e <= 4 E_ref,   rms e <= 4 R_ref,   rms e of every 16 x 16 tile <= 4 R_ref,
E_ref / R_ref being max / rms of the same quantity for the plain fp32 torch evaluation (never of the kernel's output); 4 is
lm_strict_helpers.FACTOR.  Beside it: an all-zero input row gives exact zeros; the NaN margin of ``out`` (one row, four columns,
ldo = N + 4) and every cache entry that (row_slot, row_pos) does not address keep their bits; emitted X3 operands, the partial
sums of squares and the tile candidates are held against the kernel's own stored ``out``; bf16 K / V rows are within half a bf16
ulp of float64 plus the fp32 bound; w_stream on and off agree bit for bit.

Measured on the MI355X, all 504 cases under the bound; per geometry, over its epilogues, weight formats and row counts:
worst max e / E_ref, worst rms e / R_ref (bound 4; E_ref 1.8e-8 .. 4.3e-7, R_ref 5.7e-9 .. 2.9e-8)
  gemm3_kernel<MT=1, T=1, U=3,  NW=0>  whole rows 1.64, 1.02   half rows 0.80, 0.72
  gemm3_kernel<MT=1, T=1, U=3,  NW=6>  whole rows 0.93, 0.74   half rows 0.78, 0.55
  gemm3_kernel<MT=1, T=1, U=3,  NW=8>  whole rows 0.69, 0.56   half rows 0.83, 0.55
  gemm3_kernel<MT=1, T=1, U=6,  NW=8>  whole rows 1.04, 0.65   half rows 0.82, 0.68
  gemm3_kernel<MT=1, T=1, U=12, NW=8>  whole rows 1.18, 0.85   half rows 1.12, 0.86
  gemm3_kernel<MT=1, T=2, U=3>  NW=0 0.76, 0.59   NW=6 0.65, 0.55   NW=8 0.85, 0.61
  gemm3_kernel<MT=1, T=3, U=3, NW=8> 0.71, 0.54        gemm3_kernel<MT=4, T=1, U=2> 0.78, 0.55
  gemm3_rows_kernel  NTW=1 3.07, 1.66 (K = 1536: (257, 1536, 576); K = 768: 2.12, 1.17)   NTW=2 0.74, 0.67 (K = 128)
                     NTW=4 2.12, 1.18 (K = 768)
  per epilogue, bf16 / fp8 weights: store 2.61, 1.61 / 2.40, 1.44   resid 2.94, 1.66 / 2.62, 1.49   swiglu 1.79, 1.32 / 1.78, 1.18
                     qkv 3.07, 1.62 / 2.78, 1.45 (each worst in the many-row kernel; gemm3_kernel alone stays below 1.7, 1.1)
so the split-K kernel is as close to float64 as the fp32 CPU evaluation in every form, and nothing needed the factor to rise.

The many-row kernel is the noisier one, and its noise grows with K: it has no split-K, every accumulator takes the 3 K / 32
MFMAs of its tile in ONE chain.  A CPU fp32 model of the kernels' order (gemm3_strict_helpers.kernel_order_model: an MFMA adds
four exact sums of 8 products, one fp32 rounding each) reproduces the measured figures to the digit, both judged against the
same fp32 torch reference on the same host (max, rms; kernel | model | model with the whole MFMA as one exact sum):
  resid (257, 1536, 576)  2.94, 1.66 | 2.94, 1.65 | 1.08, 0.86        store (256, 768, 2368)  2.30, 1.17 | 2.30, 1.17 | 1.21, 0.64
  resid (128, 3072, 768)  0.83, 0.85 | 0.84, 0.85 | 0.53, 0.50 (split-K)    store (1024, 128, 2048)  0.54, 0.67 | 0.54, 0.67 | 0.35, 0.44
Honest fp32 accumulation in a longer chain, then, not a lost piece -- and inside the bound at the shapes above.  It does NOT
stay inside at K = 3072, the w2 GEMM of smoltts_byte_150m in a prefill of >= 256 rows, which is no case of this matrix (the
same kernel form as (257, 1536, 576), no other code path).  Measured there, (256 | 300 | 520, 3072, 768): max e 4.0 .. 5.2 x E_ref
for store / resid / qkv with bf16 weights (fp8 2.8 .. 4.4, swiglu 2.6 .. 3.1), rms e 2.0 .. 2.3 x R_ref; resid (256, 3072, 768):
kernel 4.97, 2.30, model 4.97, 2.29, two-piece operand 7.8, 9.5 -- so there the 2^-16-grade control sits only 4.1 x above the
chain's own noise, and taking the kernel's order as a second reference would pass the kernel without still rejecting the
control by a margin.  What brings that shape under this measure is a shorter chain in gemm3_rows_kernel (partial accumulators,
as gemm3_kernel has), a change of the kernel that this test file leaves alone.  The max figure of the many-row kernel at K = 1536
also moves with the row count (M = 256 of the same shape measured 2.7 .. 3.5, one fp8 QKV_ROPE run 4.6).
"""
import numpy as np
import pytest
import torch

from gemm3_strict_helpers import (CASES, FACTOR, PAD_COLS, PAD_ROWS, QKV, RESID, SENTINEL, STORE, SWIGLU, U32, bits, half_ulp_bf16, judge,
                                  make_inputs, reference, run_case, same_results)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from smoltts_amd import engine

    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def ops(E):
    from smoltts_amd import ops

    return ops


def _of(epi):
    cs = [c for c in CASES if c.epi == epi]
    return pytest.mark.parametrize("c", cs, ids=[c.id for c in cs])


def _launch(E, ops, c, d):
    """The case's launch; decode forms with w_stream on and off, which must agree bit for bit (one of the two is judged)."""
    res = run_case(E, ops, c, d, w_stream=False)
    if c.streams:
        differ = same_results(res, run_case(E, ops, c, d, w_stream=True))
        assert not differ, f"{c.id}: w_stream changes {differ}"
    return res


def _report(c, form, got, ref, extra=None):
    msgs, we, wr = judge(c, form, got, ref, extra)
    print(f"{c.id} [{form}]: max e = {we:.2f} x E_ref ({ref.E_ref:.2e}), rms e = {wr:.2f} x R_ref ({ref.R_ref:.2e}), bound {FACTOR:g}")
    assert not msgs, "\n".join(msgs[:4])


def _margin_kept(c, buf, M, cols):
    """out_buf [M + PAD_ROWS, cols + PAD_COLS] was NaN all over: the margin must still hold the same bits."""
    blank = torch.full_like(buf, float("nan"))
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:M, :cols] = False
    changed = (buf.view(torch.int32) != blank.view(torch.int32)) & keep
    assert not changed.any(), f"{c.id}: the NaN margin of out was written at (row, column) {changed.nonzero()[:8].tolist()}"


def _zero_row(c, d, got, ref):
    z = d["zero_row"]
    if z >= 0:  # exactly the epilogue of zeros: 0, the bias or the residual
        bad = np.flatnonzero(got[z].astype(np.float64) != ref.ref64[z])
        assert bad.size == 0, f"{c.id}: all-zero input row {z}, column {bad[0]}: got {got[z, bad[0]]:.9g}, expected exactly {ref.ref64[z, bad[0]]:.9g}"


def _emitted(c, res, d, out):
    """X3 operands, partial sums of squares and tile candidates against the kernel's own stored out [M, N] (fp32)."""
    M, N = out.shape
    o64 = out.double()
    for k, gk in (("emit_a", "gamma_a"), ("emit_b", "gamma_b")):
        if k in res:
            want = o64 * d[gk].double()[None]
            x3 = res[k]
            err = (x3[:M].double() - want).abs()
            bad = (err > 2.0 ** -23 * want.abs()).nonzero()  # the bound of tests/test_gemm3_gpu.py::test_x3_pack_roundtrip
            assert len(bad) == 0, (f"{c.id}: {k} row {int(bad[0][0])} column {int(bad[0][1])}: {float(x3[tuple(bad[0])]):.9g}, out * gamma = "
                                   f"{float(want[tuple(bad[0])]):.9g}")
            assert not x3[M:].any(), f"{c.id}: {k} rows behind M were written"
    if "ssq_out" in res:
        ssq = res["ssq_out"]
        assert torch.isnan(ssq[M:]).all(), f"{c.id}: ssq_out behind row M was written"
        want = (o64 * o64).view(M, N // 16, 16).sum(-1)
        # the kernel squares 16 fp32 values (one rounding each) and adds them in a tree of depth 4 (two additions in the lane, two
        # across the four lanes of the row): every term passes through at most 5 roundings and all terms are >= 0, so
        # |ssq - sum| <= ((1 + u)^5 - 1) sum <= gamma_5 sum, gamma_5 = 5 u / (1 - 5 u), u = 2^-24 (a fused multiply-add only removes
        # roundings).  Squares of this test's values stay far above the subnormal range.
        g5 = 5 * U32 / (1 - 5 * U32)
        bad = ((ssq[:M].double() - want).abs() > g5 * want).nonzero()
        assert len(bad) == 0, (f"{c.id}: ssq_out row {int(bad[0][0])} group {int(bad[0][1])}: {float(ssq[tuple(bad[0])]):.9g}, sum of squares of out "
                               f"{float(want[tuple(bad[0])]):.9g}")
    if "cand" in res:
        cand = res["cand"]
        assert torch.isnan(cand[M:]).all(), f"{c.id}: cand_out behind row M was written"
        assert N % 16 == 0
        tiles = out.numpy().reshape(M, N // 16, 16)
        first = tiles.argmax(-1)  # numpy: the first of equal columns
        srt = np.sort(tiles, -1)
        got = cand[:M].numpy()
        col = got[..., 1].copy().view(np.int32)
        ok = (got[..., 0] == srt[..., -1]) & (col == first + 16 * np.arange(N // 16)[None]) & (got[..., 2] == srt[..., -2])
        bad = np.argwhere(~ok)
        assert len(bad) == 0, (f"{c.id}: cand_out row {bad[0][0]} tile {bad[0][1]}: (max, column, runner-up) = ({got[tuple(bad[0])][0]:.9g}, "
                               f"{col[tuple(bad[0])]}, {got[tuple(bad[0])][2]:.9g}), out has ({srt[tuple(bad[0])][-1]:.9g}, "
                               f"{first[tuple(bad[0])] + 16 * bad[0][1]}, {srt[tuple(bad[0])][-2]:.9g})")


def _store_or_resid(E, ops, c):
    d = make_inputs(c)
    ref = reference(c, d)
    res = _launch(E, ops, c, d)
    buf = res["out_buf"]
    _margin_kept(c, buf, c.M, c.N)
    out = buf[:c.M, :c.N].contiguous()
    _report(c, c.form(), out.numpy(), ref)
    _zero_row(c, d, out.numpy(), ref)
    _emitted(c, res, d, out)


@_of(STORE)
def test_gemm3_strict_store(E, ops, c):
    """STORE with bias, emit_a / ssq_out (N % 64 == 0) and cand_out (M < 256), with and without the RMSNorm prologue."""
    _store_or_resid(E, ops, c)


@_of(RESID)
def test_gemm3_strict_resid(E, ops, c):
    """RESID in place with emit_a, emit_b and ssq_out (N % 64 == 0)."""
    _store_or_resid(E, ops, c)


@_of(SWIGLU)
def test_gemm3_strict_swiglu(E, ops, c):
    d = make_inputs(c)
    ref = reference(c, d)
    res = _launch(E, ops, c, d)
    x3 = res["x3_out"]
    got = x3[:c.M].numpy()
    _report(c, c.form(), got, ref)
    _zero_row(c, d, got, ref)
    assert not x3[c.M:].any(), f"{c.id}: x3_out rows behind M were written"


@_of(QKV)
def test_gemm3_strict_qkv_rope(E, ops, c):
    """QKV_ROPE with fp32 caches and (kv_bf16 cases) bf16 caches: q, the K rows and the V rows as one [M, N] matrix."""
    d = make_inputs(c)
    ref = reference(c, d)
    res = _launch(E, ops, c, d)
    Hq, Hkv = c.heads
    qd, kd = Hq * 64, Hkv * 64
    _margin_kept(c, res["out_buf"], c.M, qd)
    slot, pos = d["row_slot"].long(), d["row_pos"].long()
    parts = [res["out_buf"][:c.M, :qd]]
    for name in ("k_cache", "v_cache"):
        cache = res[name]
        parts.append(cache[slot, :, pos].float().reshape(c.M, kd))  # [M, Hkv, 64]
        addressed = torch.zeros(cache.shape[0], cache.shape[2], dtype=torch.bool)
        addressed[slot, pos] = True
        blank = torch.full_like(cache, SENTINEL)
        changed = (bits(cache) != bits(blank)).view(*cache.shape, -1).any(-1) & ~addressed[:, None, :, None]
        assert not changed.any(), f"{c.id}: {name} entries no row addresses were written at (slot, head, position, dim) {changed.nonzero()[:8].tolist()}"
    got = torch.cat(parts, 1).numpy()
    extra = None
    if c.kv_bf16:  # a bf16 store of a value within the fp32 bound of ref64 lands within half a bf16 ulp of ref64 more
        extra = np.zeros_like(ref.ref64)
        extra[:, qd:] = half_ulp_bf16(ref.ref64[:, qd:])
    _report(c, c.form(), got, ref, extra)
    _zero_row(c, d, got, ref)
