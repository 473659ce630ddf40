"""The attn_wo_kernel instantiations in the built code objects against the variant matrix of tests/attn_wo_helpers.py.

Every form the launch can reach must be one that a case of tests/test_attn_wo_matrix_gpu.py launches (by the helpers' mirror of
launch_attn_wo_g's dispatch), and every form the mirror predicts must exist -- so a new instantiation fails here until a case
covers it, and a change of the dispatch rule that the mirror does not follow fails as well."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
from attn_wo_helpers import CASES, instance, launchable

LLVM = Path("/opt/rocm/lib/llvm/bin")
# _ZN7smoltts14attn_wo_kernelILi<G>ELi<T>ELb<TWO>ELb<W8>ELb<PICK>ELi<NBF>EEEv...
NAME = re.compile(r"attn_wo_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELi(\d+)EE")


def built_instances(tmp_path) -> set:
    from smoltts_amd.build import LIB, build_library

    build_library()
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", so.name], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(tmp_path.glob("lib.so.*gfx950"))
    assert objs, "no gfx950 code object in the library"
    found = set()
    for o in objs:
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        for m in NAME.finditer(notes):
            G, T, two, w8, pick, nbf = m.groups()
            found.add((int(G), int(T), two == "1", w8 == "1", pick == "1", int(nbf)))
    return found


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="ROCm LLVM tools not installed")
def test_every_attn_wo_instantiation_is_in_the_matrix(tmp_path):
    built = built_instances(tmp_path)
    reach = launchable()
    mirrored = {instance(c) for c in CASES}
    assert len(reach) == 160
    assert built == reach, f"instantiated but not launchable: {sorted(built - reach)}; launchable but missing: {sorted(reach - built)}"
    assert not reach - mirrored, f"launchable forms no matrix case reaches: {sorted(reach - mirrored)}"
    assert not mirrored - built, f"forms the mirror predicts that the library does not hold: {sorted(mirrored - built)}"
