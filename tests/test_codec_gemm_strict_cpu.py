"""The premises of tests/test_codec_gemm_strict_gpu.py, on the CPU.

1. What the measure rejects.  For every case of the GPU matrix two stand-in results, both computed in fp32 on the CPU, go through
   the judge the GPU results go through: the operand cut to two bf16 pieces (2^-16-grade: what a lost `lo` piece leaves) must break
   the rms bound, and the fp32 reference with ONE element -- the one of the smallest scale S -- moved by 2^-16 S must break the max
   bound, in a message that names that element.  If a control passed for some epilogue, the normaliser S of that epilogue would be
   too generous; the factor is not the thing to change.
2. The other side: honest fp32 accumulation in each kernel's own K order (the wave K-split of gemm_kernel, the single chain of
   gemm_rows_kernel and gemm_b3_kernel, the (slice, tap, chunk) order of conv_ks_kernel, the four parts of split-K), an MFMA modelled
   as exact partial sums with one rounding each, must pass the same judge.
3. Form coverage, from the kernel names in the notes of the built gfx950 code object and nothing else: (a) every form the mirror
   (codec_gemm_strict_helpers.launch_form) predicts for a case is a built instantiation; (b) every built instantiation of the six
   kernel templates is launched by a case or stands in helpers.UNREACHED with its reason; (c) every form the Mimi decode chunk and
   the Mimi encoder can launch (codec_gemms / encoder_gemms at the chunk shapes and signal lengths of the strict tests) is launched by
   a case."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
from codec_gemm_strict_helpers import (CASES, EPI_NAMES, FACTOR, MATRIX, PROBES, UNREACHED, codec_forms, judge, kernel_order_model, make_inputs,
                                       one_moved, output_name, ref_rows, reference, reference3, two_piece_model)

LLVM = Path("/opt/rocm/lib/llvm/bin")
# _ZN7smoltts11gemm_kernelILb<WF32>ELi<MT>ELi<U>ELi<PRO>ELi<EPI>EEEv... and its neighbours
NAMES = {
    "gemm": re.compile(r"7smoltts11gemm_kernelILb([01])ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE"),
    "rows": re.compile(r"gemm_rows_kernelILi(\d+)ELi(\d+)EE"),
    "b3": re.compile(r"gemm_b3_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE"),
    "xs": re.compile(r"conv_xs_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE"),
    "ks": re.compile(r"conv_ks_kernelILi(\d+)ELi(\d+)ELi(\d+)EE"),
    "reduce": re.compile(r"splitk_reduce_kernelILi(\d+)EE"),
}


@pytest.mark.parametrize("c", MATRIX, ids=[c.id for c in MATRIX])
def test_controls_are_rejected(c):
    d = make_inputs(c)
    ref = reference(c)
    form = c.form()
    msgs2, we2, wr2 = judge(c, form, two_piece_model(c, d), ref, allow=False)
    moved, (m, n) = one_moved(ref)
    msgs1, we1, _ = judge(c, form, moved, ref, allow=False)
    print(f"{c.id}: E_ref {ref.E_ref:.3e}, R_ref {ref.R_ref:.3e}; two pieces: rms {wr2:.1f} x R_ref, max {we2:.1f} x E_ref; "
          f"one element moved: max {we1:.1f} x E_ref (bound {FACTOR:g})")
    msgs0, we0, wr0 = judge(c, form, ref.ref32, ref, allow=False)
    assert abs(we0 - 1) < 1e-9 and abs(wr0 - 1) < 1e-9  # the reference's own noise is the unit
    assert not msgs0, f"{c.id}: the fp32 reference breaks the tile rule on its own data: {msgs0[0]}"
    assert wr2 > FACTOR, f"{c.id}: the two-piece model passes the rms bound ({wr2:.2f} x R_ref): S of {EPI_NAMES[c.epi]} is too generous"
    assert any("rms e" in s for s in msgs2)
    assert we1 > FACTOR, f"{c.id}: one element moved by 2^-16 S passes the max bound ({we1:.2f} x E_ref)"
    place = f"{output_name(c, n)} row {m} column {n} (tile {m // 16}, {n // 16})"
    assert any(place in s for s in msgs1), f"{c.id}: the message does not name {place}: {msgs1}"
    if c.products == 3:  # the three-product model itself is 2^-16-grade: against float64 it must fail
        m3, _, wr3 = judge(c, form, reference3(c).ref64.astype("float32"), ref, allow=False)
        print(f"{c.id}: the three-product model against float64: rms {wr3:.1f} x R_ref")
        assert m3 and wr3 > FACTOR


# one case per K order (and the split-K pair of each kernel that has one); the model runs on the first ORDER_ROWS rows
ORDER_ROWS = 160
ORDER_NAMES = ("gemm-f32-none-store-M17-K288-N24", "gemm-f32-none-gelu-M100-K768-N16", "gemm-bf16-rmsnorm-store-M17-K1472-N48",
               "gemm-f32-layernorm-gelu-M16-K512-N48", "gemm-f32-elu-resid-M33-K128-N48", "rows-store-N128", "rows-scale_resid-N32",
               "b3-22-store", "b3-22-taps", "b3-splitk-gelu", "b3-44-resid", "xs-conv-N128-taps17", "xs-lin-scale-resid", "xs-ksplit-flat",
               "ks-ntw4-np2", "ks-ntw2-np3-taps7", "np3-b3")
ORDER_CASES = [c for c in CASES if c.name in ORDER_NAMES or c.probe]
assert len(ORDER_CASES) == len(ORDER_NAMES) + len(PROBES)


@pytest.mark.parametrize("c", ORDER_CASES, ids=[c.id for c in ORDER_CASES])
def test_honest_fp32_in_the_kernel_order(c):
    """Matrix cases: must pass.  The long-K probes: the ratios are printed (tests/test_codec_gemm_strict_gpu.py compares the kernel's
    with them); a probe's model may exceed the bound -- that is what makes a probe no matrix case."""
    d = make_inputs(c)
    rows = slice(0, min(c.M, ORDER_ROWS))
    ref = ref_rows(reference3(c) if c.products == 3 else reference(c), rows)
    msgs, we, wr = judge(c, c.form(), kernel_order_model(c, d, rows), ref)
    print(f"{c.id}: fp32 in the kernel's order, rows {rows.start}..{rows.stop}: max {we:.2f} x E_ref, rms {wr:.2f} x R_ref (bound {FACTOR:g})")
    if not c.probe:
        assert not msgs, "\n".join(msgs)


def built_instances(tmp_path):
    from smoltts_amd.build import LIB, build_library

    build_library()
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", so.name], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(tmp_path.glob("lib.so.*gfx950"))
    assert objs, "no gfx950 code object in the library"
    built = set()
    for o in objs:
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        for kind, rx in NAMES.items():
            for m in rx.finditer(notes):
                g = m.groups()
                built.add((kind, g[0] == "1") + tuple(int(v) for v in g[1:]) if kind == "gemm" else (kind,) + tuple(int(v) for v in g))
    return built


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="ROCm LLVM tools not installed")
def test_every_form_has_a_case_and_every_instantiation_a_form(tmp_path):
    built = built_instances(tmp_path)
    for kind in NAMES:
        assert any(b[0] == kind for b in built), f"no {kind} kernel names in the code object's notes"
    matrix = {}
    for c in MATRIX:
        matrix.setdefault(c.form(), c.id)
    launched = {i for f in matrix for i in f.instances}
    print(f"{len(MATRIX)} cases launch {len(matrix)} forms of {len({f.geometry for f in matrix})} geometries and {len(launched)} of the "
          f"{len(built)} built instantiations")
    # (a)
    absent = {i: cid for f, cid in matrix.items() for i in f.instances if i not in built}
    assert not absent, "instantiations the mirror predicts that the library does not hold: " + "; ".join(f"{i} for {cid}" for i, cid in absent.items())
    # (b)
    idle = sorted(built - launched, key=str)
    print(f"{len(idle)} built instantiations that no matrix case launches (helpers.UNREACHED has {len(UNREACHED)}):")
    for i in idle:
        print("  ", i, "--", UNREACHED.get(i, "NOT LISTED"))
    unlisted = [i for i in idle if i not in UNREACHED]
    assert not unlisted, f"built instantiations without a case and without a reason in UNREACHED: {unlisted}"
    stale = [i for i in UNREACHED if i in launched or i not in built]
    assert not stale, f"UNREACHED lists instantiations that a case launches or that are not built: {stale}"
    # (c)
    codec = codec_forms()
    print(f"the decode chunk and the encoder launch {len(codec)} forms")
    uncovered = {f: ex for f, ex in codec.items() if f not in matrix}
    assert not uncovered, "codec-launchable forms no matrix case launches: " + "; ".join(f"{f}, e.g. {ex}" for f, ex in uncovered.items())
