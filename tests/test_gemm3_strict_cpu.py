"""The premises of tests/test_gemm3_strict_gpu.py, on the CPU.

1. What the measure rejects.  For every case of the GPU matrix two stand-in results, both computed in fp32 on the CPU, go through
   the judge the GPU results go through: the kernel's arithmetic with the operand cut to two bf16 pieces (2^-16-grade: what a lost
   `lo` piece leaves) must break the rms bound, and the fp32 reference with ONE element -- the one of the smallest scale S --
   moved by 2^-16 S must break the max bound, in a message that names that element.  If a control passed for some epilogue, the
   normaliser S of that epilogue would be too generous; the factor is not the thing to change.  The other side: honest fp32
   accumulation of all three pieces in the kernels' own K order (gemm3_strict_helpers.kernel_order_model) must pass.
2. Form coverage.  The helpers mirror launch3_fmt / launch3_one / launch3_rows.  Every form the mirror predicts for a matrix case
   must be an instantiation in the built gfx950 code object (kernel names out of the object's notes, nothing else is read), and
   every form the engine can launch for the named configs -- every slow and depth GEMM with its epilogue, both weight formats, the
   w_stream settings the engine can give it, M = 1..255 and the prefill sizes -- must be launched by at least one matrix case."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
from gemm3_strict_helpers import (CASES, EPI_NAMES, FACTOR, engine_forms, judge, kernel_order_model, kernel_waves, make_inputs, one_moved,
                                  output_name, reference, two_piece_model)

LLVM = Path("/opt/rocm/lib/llvm/bin")
# _ZN7smoltts12gemm3_kernelILi<MT>ELi<T>ELi<U>ELi<EPI>ELb<W8>ELb<NT>ELi<NW>EEEv...
ONE = re.compile(r"gemm3_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)EE")
ROWS = re.compile(r"gemm3_rows_kernelILi(\d+)ELi(\d+)ELb([01])EE")
ROWS_F8 = re.compile(r"gemm3_rows_f8_kernelILi(\d+)ELi(\d+)EE")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_controls_are_rejected(c):
    d = make_inputs(c)
    ref = reference(c, d)
    form = c.form()
    msgs2, we2, wr2 = judge(c, form, two_piece_model(c, d), ref)
    moved, (m, n) = one_moved(ref)
    msgs1, we1, _ = judge(c, form, moved, ref)
    _, we0, wr0 = judge(c, form, ref.ref32, ref)
    print(f"{c.id}: E_ref {ref.E_ref:.3e}, R_ref {ref.R_ref:.3e}; two pieces: rms {wr2:.1f} x R_ref, max {we2:.1f} x E_ref; "
          f"one element moved: max {we1:.1f} x E_ref (bound {FACTOR:g})")
    assert abs(we0 - 1) < 1e-9 and abs(wr0 - 1) < 1e-9  # the reference's own noise is the unit
    assert wr2 > FACTOR, f"{c.id}: the two-piece model passes the rms bound ({wr2:.2f} x R_ref): S of {EPI_NAMES[c.epi]} is too generous"
    assert any("rms e" in s for s in msgs2)
    assert we1 > FACTOR, f"{c.id}: one element moved by 2^-16 S passes the max bound ({we1:.2f} x E_ref)"
    place = f"{output_name(c, n)} row {m} column {n} (tile {m // 16}, {n // 16})"
    assert any(place in s for s in msgs1), f"{c.id}: the message does not name {place}: {msgs1}"


ORDER_CASES = [c for c in CASES if not c.w8 and not c.kv_bf16 and c.M in (17, 129, 256, 257, 1024)]


@pytest.mark.parametrize("c", ORDER_CASES, ids=[c.id for c in ORDER_CASES])
def test_honest_fp32_in_the_kernel_order_meets_the_bound(c):
    """The other side of the controls: all three pieces, fp32 accumulation in the kernel's own order (K parts of the split-K
    kernel, the one long chain of the many-row kernel) must pass the judge that rejects the two-piece operand."""
    d = make_inputs(c)
    ref = reference(c, d)
    msgs, we, wr = judge(c, c.form(), kernel_order_model(c, d), ref)
    print(f"{c.id}: fp32 in the kernel's order ({kernel_waves(c)} K parts): max {we:.2f} x E_ref, rms {wr:.2f} x R_ref (bound {FACTOR:g})")
    assert not msgs, "\n".join(msgs)


def built_instances(tmp_path):
    from smoltts_amd.build import LIB, build_library

    build_library()
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", so.name], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(tmp_path.glob("lib.so.*gfx950"))
    assert objs, "no gfx950 code object in the library"
    one, rows, rows_f8 = set(), set(), set()
    for o in objs:
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        for m in ONE.finditer(notes):
            MT, T, U, epi, w8, nt, NW = m.groups()
            one.add(("one", int(MT), int(T), int(U), int(epi), w8 == "1", nt == "1", int(NW)))
        for m in ROWS.finditer(notes):
            NTW, epi, w8 = m.groups()
            rows.add(("rows", int(NTW), int(epi), w8 == "1"))
        for m in ROWS_F8.finditer(notes):
            rows_f8.add(("rows_f8", int(m.group(1)), int(m.group(2))))
    return one | rows, rows_f8


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="ROCm LLVM tools not installed")
def test_every_engine_form_has_a_case(tmp_path):
    built, built_f8 = built_instances(tmp_path)
    assert built and built_f8, "no gemm3 kernel names in the code object's notes"
    matrix = {}
    for c in CASES:
        for ws in ((False, True) if c.streams else (False,)):
            matrix.setdefault(c.form(ws), c.id)
    engine = engine_forms()
    geometries = {f.geometry for f in engine}
    print(f"{len(CASES)} cases launch {len(matrix)} forms; the engine can launch {len(engine)} forms of {len(geometries)} geometries")
    assert len(geometries) == 18, sorted(geometries)
    absent = {f: cid for f, cid in matrix.items() if f.instance not in built}
    assert not absent, "forms the mirror predicts that the library does not hold: " + "; ".join(f"{f} for {cid}" for f, cid in absent.items())
    uncovered = {f: ex for f, ex in engine.items() if f not in matrix}
    assert not uncovered, "engine-launchable forms no matrix case launches: " + "; ".join(f"{f}, e.g. {ex}" for f, ex in uncovered.items())
    # what the dispatch macros emit and no shape of the matrix reaches: listed, not an error (the fp8 x fp8 kernels among them:
    # fp8_activations is not the parity path)
    idle = sorted(built - {f.instance for f in matrix})
    print(f"{len(idle)} gemm3_kernel / gemm3_rows_kernel instantiations that no matrix case launches:")
    for i in idle:
        print("  ", i)
    print(f"{len(built_f8)} gemm3_rows_f8_kernel instantiations (fp8_activations, out of scope): {sorted(built_f8)}")
