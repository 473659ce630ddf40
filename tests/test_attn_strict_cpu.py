"""The premises of tests/test_attn_strict_gpu.py, on the CPU, and the kernel forms it covers.

Premises, on every case's own data (tests/attn_strict_helpers.py): the fp32 reference passes the report by construction; in the
flat regime the 2^-16-grade mutant (K and V cut to two bf16 pieces; over a bf16 cache, q and the softmax weights) exceeds the
factor by RMS ratio in every case and by max ratio in most; in the planted regime the mutant that admits the outside key and the
mutant that drops the inside edge key each exceed it in every case that has such a key, and the failure names the place.  So a
kernel that passes the GPU test is neither 2^-16 grade nor wrong by one key at either edge of any row's range.

Coverage: the attention instantiations in the built gfx950 code objects are exactly the forms ``launchable()`` lists, each is the
``instance()`` of some case, and every form the mirror predicts exists."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from attn_strict_helpers import (BY_FORM, CASES, FACTOR, admit_spans, drop_spans, form, form_id, instance, launchable, make_data, reference, references,
                                 rows3_three_product_model, strict_report)

LLVM = Path("/opt/rocm/lib/llvm/bin")
# _ZN7smoltts11attn_kernelILi<G>ELb<KB>EEEv..., ..attn_split_kernelILi<G>ELb<KB>ELi<NS>EEEv..., ..
NAMES = {"attn_short_kernel": "ii", "attn_kernel": "ib", "attn_split_kernel": "ibi", "attn_prefill_kernel": "ib", "attn_rows3_kernel": "ii"}
ARG = {"i": r"Li(\d+)E", "b": r"Lb([01])E"}

IDS = [c.name for c in CASES]


def _model(c):
    return rows3_three_product_model if c.products == 3 else reference


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_fp32_reference_passes_and_two_piece_arithmetic_does_not(c):
    d = make_data(c, "flat")
    r32, r64 = references(c, "flat")
    fails, worst = strict_report(r32, r32, r64, c, "flat")
    assert not fails and worst == (1.0, 1.0), fails
    if c.products == 3:
        # the three-product form is 2^-16 grade and judged against its own model: that bound in turn rejects fp32-grade arithmetic
        fails, (e, r) = strict_report(reference(c, d, torch.float64).float(), r32, r64, c, "flat")
    else:
        fails, (e, r) = strict_report(reference(c, d, torch.float64, cut=True).float(), r32, r64, c, "flat")
    print(f"{c.name}: the other arithmetic class sits at {e:.1f} x E_ref, {r:.1f} x R_ref")
    assert r > FACTOR and fails, (c.name, e, r)
    assert "query head" in fails[0] and "dim" in fails[0] and "row" in fails[0] and "j_lo" in fails[0], fails[0]


def test_two_piece_arithmetic_exceeds_the_max_bound_in_most_cases():
    over = 0
    for c in CASES:
        if c.products == 3:
            continue
        r32, r64 = references(c, "flat")
        _, (e, _r) = strict_report(reference(c, make_data(c, "flat"), torch.float64, cut=True).float(), r32, r64, c, "flat")
        over += e > FACTOR
    n = sum(c.products != 3 for c in CASES)
    assert over >= 0.9 * n, (over, n)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_a_key_admitted_or_dropped_at_a_range_edge_fails(c):
    d = make_data(c, "planted")
    r32, r64 = references(c, "planted")
    fails, _ = strict_report(r32, r32, r64, c, "planted")
    assert not fails, fails
    assert bool(torch.isfinite(d.v).all()) and bool(torch.isfinite(d.k).all())
    kinds = {p.kind for p in d.plants}
    assert kinds & {"first", "last"} and kinds & {"before", "after"}, (c.name, kinds)  # every case has both sorts of key
    for what, spans in (("admits the outside key", admit_spans(c, d)), ("drops the inside edge key", drop_spans(c, d))):
        mutant = _model(c)(c, d, torch.float64, spans=spans).float()
        fails, (e, r) = strict_report(mutant, r32, r64, c, "planted")
        assert e > FACTOR and r > FACTOR and fails, (c.name, what, e, r)
        # the worst element lies in a row whose range the mutant changed, and the message names it
        m = re.search(r"worst at row (\d+) \(slot \d+, pos (-?\d+), j_lo (\d+)\), query head (\d+), dim (\d+): got ", fails[0])
        assert m and int(m.group(1)) in spans, (what, fails[0])


def test_an_admitted_outside_key_would_take_nearly_all_the_weight():
    """The construction: against its own (row, query head) a planted outside key scores so far above every visible key that its
    float64 softmax weight, were it admitted, is above 0.999 -- also behind the bf16 rounding of a bf16 cache."""
    checked = 0
    for c in CASES:
        d = make_data(c, "planted")
        G = c.Hq // c.Hkv
        for p in [p for p in d.plants if p.kind in ("before", "after")][:40]:
            lo, pos = c.span(p.row)
            q = d.q[p.row, p.head * 64:(p.head + 1) * 64].double()
            Ks = d.k[c.row_slot[p.row], p.head // G].double()
            w = 1.0 / (1.0 + float(torch.exp(Ks[lo:pos + 1] @ q / 8.0 - Ks[p.j] @ q / 8.0).sum()))
            assert w > 0.999, (c.name, p, w)
            checked += 1
    assert checked > 200


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
        for kernel, kinds in NAMES.items():
            for m in re.finditer(rf"\d{kernel}I" + "".join(ARG[k] for k in kinds) + "E", notes):
                found.add((kernel, tuple(int(a) if k == "i" else a == "1" for k, a in zip(kinds, m.groups()))))
    return found


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="ROCm LLVM tools not installed")
def test_every_attention_instantiation_is_reached_by_a_case(tmp_path):
    built = built_instances(tmp_path)
    reach = launchable()
    mirrored = {form(c) for c in CASES}
    ids = lambda s: sorted(form_id(f) for f in s)  # noqa: E731
    assert len(reach) == 28
    assert built == reach, f"instantiated but not launchable: {ids(built - reach)}; launchable but missing: {ids(reach - built)}"
    assert not reach - mirrored, f"launchable forms no case reaches: {ids(reach - mirrored)}"
    assert not mirrored - built, f"forms the mirror predicts that the library does not hold: {ids(mirrored - built)}"
    assert set(BY_FORM) == reach


def test_the_cases_hold_the_shapes_each_kernel_needs():
    """Wave counts and thresholds the case list is meant to reach (the mirror says which launch each case is)."""
    waves = {}
    for c in CASES:
        k, targs, nw = instance(c)
        waves.setdefault((k, targs), set()).add(nw)
    for G in (1, 2, 3, 4):
        assert waves[("attn_kernel", (G, False))] == {4, 16}
        assert waves[("attn_split_kernel", (G, True, 1))] == {4, 16}  # the 4-wave launch of a bf16 cache of 17..64 entries
        for kb in (False, True):
            cs = BY_FORM[("attn_split_kernel", (G, kb, 2))]
            Ls = {sp[1] - sp[0] + 1 for c in cs for sp in (c.span(r) for r in range(c.rows)) if sp}
            assert {511, 512, 513} <= Ls and any(c.window == 250 for c in cs) and any(c.window == 600 for c in cs)
        for un, cl in ((2, 8), (4, 16)):
            cs = BY_FORM[("attn_short_kernel", (G, un))]
            assert all(set(range(cl)) <= set(c.row_pos) for c in cs) and {c.window > 0 for c in cs} == {False, True}
    assert any(c.rows * c.Hq % 4 for cs in BY_FORM.values() for c in cs if instance(c)[0] == "attn_short_kernel")
    for kb in (False, True):
        cs = BY_FORM[("attn_prefill_kernel", (1, kb))]
        assert {c.window for c in cs} == {0, 7, 50} and {c.Hq // c.Hkv for c in cs} == {1, 3, 4} and all(c.rows * c.Hkv >= 1024 for c in cs)
    for fam in ("attn_kernel", "attn_split_kernel", "attn_prefill_kernel"):  # rows with nothing cached: pos = -1 and pos = cache_len
        assert any(-1 in c.row_pos and c.cache_len in c.row_pos for c in CASES if instance(c)[0] == fam), fam
