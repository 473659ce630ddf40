"""The codec's fp32 and bf16x3 GEMM family behind launch_gemm (gemm_kernel, gemm_rows_kernel, gemm_b3_kernel, splitk_reduce_kernel,
conv_xs_kernel, conv_ks_kernel), per element and per launch form, against float64.

tests/test_kernels_gpu.py and tests/test_gemm_b3_gpu.py hold max|got - ref| / max|ref| below 2e-6 .. 3e-5: normwise, blind to one small
column, one ragged tile edge or one row of small scale, at a handful of shapes.  Here every form the dispatch can take
(tests/codec_gemm_strict_helpers.py mirrors launch_gemm_impl, launch_gemm_b3, conv_xs_applies / launch_conv_xs and conv_ks_applies /
ks_ntw; tests/test_codec_gemm_strict_cpu.py holds the mirror to the kernel names in the built code object, proves that every form
the Mimi decode chunk and the Mimi encoder launch has a case, and that the measure rejects a two-piece operand and one moved element)
runs at the smallest shape that reaches it, on buffer rows over 10^-3 .. 10^3 in scale and weight rows over 10^-3 .. 1, one operand
row all zero, a quarter of the operand in [-4, 0) for the ELU prologues, and is judged per element:
    e = |got - ref64| / S,   S = the element's condition scale pushed through the epilogue,
    max e <= 4 E_ref,   rms e <= 4 R_ref,   rms e of every 16 x 16 tile <= 4 R_ref,
E_ref / R_ref being max / rms of the same quantity for the plain fp32 torch evaluation; 4 is lm_strict_helpers.FACTOR.  The one
allowance is the hardware exponential of the many-row kernels' ELU (ELU_EPS, absolute, off the error before the ratio).  Beside it:
where S == 0 the output is exactly 0; every output (out, raw_out, the residual read in place) lies in a NaN-filled buffer with
margins in front, behind, in the ldo - N gap of every row and between the slots, which must keep their bits; raw_out is judged like
out against the value before the ELU; QKV_ROPE runs on unique (slot, pos) pairs with rows at pos = -1 and pos = cache_len, whose q
is written and whose K / V are not, into caches prefilled with a sentinel that every unaddressed entry must keep; the bf16x3 piece
caches decode to the fp32 K / V rows bit for bit; split-K twice gives equal bits, a workspace too small the bits of the call without
one; N < 4 with elu_out and raw_out does what include/smoltts_hip.h says in gemm_kernel and in rows_epilogue alike.  The three-product
forms (b3_products = 3, 2^-16-grade by design) are judged the same way against their own model (operands cut to hi + mid pieces, the
products hi hi, mid hi, hi mid in float64) and must FAIL against float64.

Measured on the MI355X, all 243 matrix cases under the bound (207 forms, all 102 built instantiations of the six templates); worst
max e / E_ref | worst rms e / R_ref per kernel over its cases, bound 4 (E_ref 1.9e-8 .. 3.9e-7, R_ref 8.9e-9 .. 3.2e-8); flat
operands and operands with a planted quarter in [-4, 0) (the ELU prologues) apart where a kernel has both:
  gemm_kernel        143 cases  2.95 | 2.07   per row-tile class: MT = 1 2.95 | 2.07, MT = 2 2.38 | 1.55, MT = 4 1.15 | 1.11
                                              per wave count: 1 2.95 | 1.90, 2 2.71 | 2.07, 3 1.14 | 1.08, 4 1.71 | 1.32, 6 0.91 | 0.87,
                                              8 1.15 | 0.94, 16 1.10 | 0.93 (the figures above 2 are one-row cases at K = 32 and 160)
                                              flat 2.95 | 2.07, planted (PRO_ELU, expm1f: no allowance) 1.43 | 1.25
                                              bf16 weights 2.71 | 1.90, fp32 weights 2.95 | 2.07; in-kernel LayerNorm 1.71 | 1.32
                                              N < 4 tail (plain, elu_out, elu_out + raw_out) 2.38 | 1.69, its raw_out 2.40 | 2.15
  gemm_rows_kernel    21 cases  1.85 | 1.00   (NTW, WN) = (1, 1) 1.85 | 0.87, (1, 2) 1.16 | 1.00, (1, 4) 1.22 | 1.00, (2, 4) 0.95 | 0.97
  gemm_b3_kernel      26 cases  1.20 | 1.31   2 x 2 1.04 | 1.31, 4 x 2 0.52 | 0.84, 4 x 4 0.53 | 0.84, split-K + reduce 1.20 | 1.09;
                                              planted (PRO_ELU, hardware exponential allowed) 1.04 | 0.50
  conv_xs_kernel      18 cases  2.04 | 1.36   conv mode 1.95 | 1.29 (planted 1.75 | 0.73), k1 conv + residual 1.32 | 0.84, Linears
                                              1.70 | 1.16, LayerNorm-fused 2.04 | 1.36, linear_ksplit + reduce 0.74 | 1.02
  conv_ks_kernel      10 cases  3.77 | 2.40   NTW = 4 3.22 | 1.65, NTW = 2 3.03 | 2.40 (7 taps x 384), NTW = 1 3.77 | 1.65;
                                              planted 2.04 | 0.72
  the stand-alone layernorm_kernel in front of gemm_kernel / gemm_rows_kernel / gemm_b3_kernel (6 cases, counted above) 1.22 | 1.31
  three products, against their own model: gemm_b3 0.97 | 0.92 (14 cases), conv_xs 1.33 | 0.98 (8), conv_ks 2.11 | 1.23 (3); the same
  results against float64: 5.9 .. 32.7 | 9.8 .. 33.9, every one over the bound, as asserted.
(test_report_table prints the table per instantiation.)

The long-K probes (test_long_k_probe): one case per many-row kernel at the longest K the codec gives it, every accumulator taking
the whole K in one chain.  Whole output max | rms; then kernel against the CPU fp32 model of the kernel's own order
(tests/codec_gemm_strict_helpers.kernel_order_model) on the 64-row block that holds the kernel's worst element, and that element alone:
  gemm_b3 unsplit, K = 2048 (fc2 without a workspace)          2.26 | 1.67   2.26, 1.69 | 2.11, 1.74   element 2.26 | 2.11
  gemm_b3 unsplit, K = 1536 (workspace too small, N = 64)      5.16 | 1.94   5.16, 1.93 | 4.86, 1.92   element 5.16 | 4.86   OVER
  conv_ks 7 x 512 (conv0), NTW = 1                             3.64 | 1.69   3.64, 2.11 | 3.64, 2.03   element 3.64 | 3.64
  conv_ks 2 x 1024 (ConvTranspose 1024 -> 512), NTW = 4        4.24 | 2.16   4.24, 2.19 | 4.43, 2.15   element 4.24 | 3.92   OVER
  conv_xs 3 x 256 (res2 k3, PRO_ELU)                           1.71 | 0.73   1.71, 1.41 | 1.71, 1.41   element 1.71 | 1.71
  gemm_rows_kernel, the encoder's strided convs (flat windows, ELU out; the first rows at which a signal reaches the kernel):
    conv 1, K = 1280, N = 256, 6100 rows        3.61 | 1.29, raw_out 4.28 | 2.13   3.61, 1.26 | 3.61, 1.26   element 3.61 | 3.61   OVER
    conv 2, K = 3072, N = 512, 3040 rows        4.97 | 1.90, raw_out 5.95 | 2.99   4.97, 1.93 | 4.97, 1.92   element 4.97 | 4.97   OVER
    conv 3, K = 8192, N = 1024, 1553 rows       6.65 | 2.82                        6.65, 2.88 | 6.65, 2.87   element 6.65 | 6.65   OVER
As in gemm3_rows_kernel the noise of a single chain grows with K.  The CPU model reproduces the kernels' figures where they are over
the bound, element for element in the fp32-MFMA kernel (modelled as a chain of four fused multiply-adds per instruction; as one
exact 4-product sum the model stays at half the kernel's noise) and within 8 % in the bf16x3 kernels, so this is honest accumulation
in a long chain, not a lost piece -- but it IS over the project's max bound at shapes the codec launches: the encoder's strided
convs 1..3 on signals long enough for the many-row kernel (from 122 000 samples; the strict encoder test's lengths stay in
gemm_kernel there, whose waves split K), the ConvTranspose 1024 -> 512 of a 32 x 32 decode chunk, and an unsplit gemm_b3 at K = 1536.
The same instantiations pass at the smallest K that reaches them, which is what the matrix holds.  Partial accumulators per K part
(as gemm_kernel and split-K have) would bring these back: a change of the kernels, left to a pull request of its own.

Not in the file: N = 1 through gemm_rows_kernel.  A 16 x 16 tile of a one-column output holds 16 elements, so the tile rule is there
a rule on single elements, tighter than the max rule: at (49097, 32, 1) one element at 2.30 E_ref (inside the max bound; whole output
2.30 | 1.22) put its tile at 4.23 R_ref, and the CPU model gives that kernel's figures to the digit.  The measure, not the kernel,
is short there; the asserted N < 4 case of the many-row kernel is N = 3 with elu_out and raw_out.

What the file found: the in-kernel LayerNorm prologue of gemm_kernel normalised the rows from 4 * nwaves on with whatever the LDS
held when K < 320 asked for fewer than 4 waves (M = 7, K = 32: 10^7 E_ref; the codec's K = 512 has 6 waves) -- launch_gemm_impl now
gives that form at least 4 waves; the N < 4 tail of gemm_kernel ignored elu_out and raw_out, that of rows_epilogue raw_out.
"""
import numpy as np
import pytest
import torch

from codec_gemm_strict_helpers import (FACTOR, MATRIX, PROBES, QKV, SENTINEL, bits, judge, kernel_order_model, make_inputs, noise, ref_rows,
                                       reference, reference3, run_case, same_results)

pytestmark = pytest.mark.gpu
MEASURED = {}  # case name -> (form, max ratio, rms ratio): filled as the cases run, printed by the last test


@pytest.fixture(scope="module")
def E():
    from smoltts_amd import engine

    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def ops(E):
    from smoltts_amd import ops

    return ops


def _margins(c, res):
    for k in ("out", "raw"):
        if k + "_margin" in res:
            w = res[k + "_margin"]
            assert w.numel() == 0, f"{c.id}: the NaN margin of {k} was written at flat positions {w[:8].tolist()} ({w.numel()} in all)"


def _assemble(c, d, res, ref):
    """The judged matrix [M, cols] in float64: out, and for QKV_ROPE the K and V rows gathered from the caches (rows outside the
    cache, which write none, take the reference there); checks the sentinel and the piece caches on the way."""
    out = res["out"].double()
    if c.epi != QKV:
        return out.numpy()
    Hq, Hkv = c.heads
    qd, kd, L = Hq * 64, Hkv * 64, c.cache_len
    slot, pos = d["row_slot"].long(), d["row_pos"].long()
    inside = (pos >= 0) & (pos < L)
    parts = [out]
    for j, name in enumerate(("k_cache", "v_cache")):
        cache = res[name]
        rows = torch.from_numpy(ref.ref64[:, qd + j * kd: qd + (j + 1) * kd]).clone()
        rows[inside] = cache[slot[inside], :, pos[inside]].reshape(-1, kd).double()
        parts.append(rows)
        addressed = torch.zeros(cache.shape[0], cache.shape[2], dtype=torch.bool)
        addressed[slot[inside], pos[inside]] = True
        changed = (cache != SENTINEL).any(-1) & ~addressed[:, None, :]
        assert not changed.any(), f"{c.id}: {name} entries no row addresses were written at (slot, head, position) {changed.nonzero()[:8].tolist()}"
        if c.kv3:
            dec = res["k3" if j == 0 else "v3"]
            want = torch.where(addressed[:, None, :, None], cache, torch.zeros_like(cache))
            same = torch.equal(bits(dec), bits(want))
            assert same, f"{c.id}: the {name[0].upper()} piece cache does not decode to the fp32 rows written (or holds an unaddressed entry)"
    return torch.cat(parts, 1).numpy()


def _run(E, ops, c):
    d = make_inputs(c)
    ref = reference3(c) if c.products == 3 else reference(c)
    form = c.form()
    res = run_case(E, ops, c, d)
    _margins(c, res)
    got = _assemble(c, d, res, ref)
    msgs, we, wr = judge(c, form, got, ref)
    line = f"{c.id} [{form}]: max e = {we:.2f} x E_ref ({ref.E_ref:.2e}), rms e = {wr:.2f} x R_ref ({ref.R_ref:.2e}), bound {FACTOR:g}"
    if c.raw_out:
        rmsgs, rwe, rwr = judge(c, form, res["raw"].double().numpy(), reference(c, raw=True), which="raw")
        line += f"; raw_out {rwe:.2f}, {rwr:.2f}"
        msgs += rmsgs
    if c.products == 3:  # 2^-16-grade by design: within the bound of its own model, outside it against float64
        m64, we64, wr64 = judge(c, form, got, reference(c))
        line += f"; against float64 {we64:.1f}, {wr64:.1f}"
        if not c.probe:
            assert m64 and wr64 > FACTOR, f"{c.id}: the three-product form passes against float64 ({we64:.2f}, {wr64:.2f}): it ran six products?"
    print(line)
    MEASURED[c.id] = (form, we, wr)
    if c.ws == "full":
        differ = same_results(res, run_case(E, ops, c, d))
        assert not differ, f"{c.id}: two split-K runs differ in {differ}"
    if c.ws == "small":
        differ = same_results(res, run_case(E, ops, c, d, ws_mode=""))
        assert not differ, f"{c.id}: a workspace too small changes {differ} against the call without one"
    return msgs, res, ref, d


@pytest.mark.parametrize("c", MATRIX, ids=[c.id for c in MATRIX])
def test_codec_gemm_strict(E, ops, c):
    msgs, *_ = _run(E, ops, c)
    assert not msgs, "\n".join(msgs[:4])


@pytest.mark.parametrize("c", PROBES, ids=[c.id for c in PROBES])
def test_long_k_probe(E, ops, c):
    """One case per many-row kernel at the codec's own longest K (every accumulator takes the whole K in one chain): reported beside
    the CPU fp32 model of the kernel's own order, on the first rows and on the 64-row block that holds the kernel's worst element
    (the model is what tells honest accumulation from a bug), and held only to what is no matter of accumulation: margins and
    finiteness."""
    msgs, res, ref, d = _run(E, ops, c)
    full = res["out"].double().numpy()
    assert np.isfinite(full).all()
    e = noise(full, ref.ref64, ref.S, ref.extra)
    wm, wn = np.unravel_index(int(e.argmax()), e.shape)
    first, worst = slice(0, min(c.M, 160)), slice(wm // 64 * 64, min(c.M, wm // 64 * 64 + 64))
    for what, rows in (("the first rows", first), ("the 64-row block of the worst element", worst)):
        sub = ref_rows(ref, rows)
        model = kernel_order_model(c, d, rows)
        _, kwe, kwr = judge(c, c.form(), full[rows], sub)
        _, mwe, mwr = judge(c, c.form(), model, sub)
        print(f"{c.id}: {what}, rows {rows.start}..{rows.stop}: kernel {kwe:.2f}, {kwr:.2f} | CPU model of its order {mwe:.2f}, {mwr:.2f}")
        if rows is worst:
            em = noise(model, sub.ref64, sub.S, sub.extra)[wm - rows.start, wn] / ref.E_ref
            print(f"{c.id}: the worst element (row {wm}, column {wn}): kernel {e[wm, wn] / ref.E_ref:.2f} x E_ref, model {em:.2f} x E_ref" +
                  (f"; OVER THE BOUND on the whole output: {msgs[0]}" if msgs else ""))


def test_report_table():
    """Worst max | rms ratio per form over the cases that ran in this session (nothing to assert when run alone)."""
    worst = {}
    for cid, (form, we, wr) in MEASURED.items():
        key = str(form._replace(geo=()))
        a, b, n = worst.get(key, (0.0, 0.0, 0))
        worst[key] = (max(a, we), max(b, wr), n + 1)
    for key in sorted(worst):
        a, b, n = worst[key]
        print(f"{key:70s} {n:3d} cases   max {a:.2f}   rms {b:.2f}")
