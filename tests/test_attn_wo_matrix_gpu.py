"""Every launchable attn_wo_kernel<G, T, TWO, W8, PICK, NBF> (gemm3.hip: the depth-step attention inside the wo GEMM) against a
float64 reference, one case per form (tests/attn_wo_helpers.py; tests/test_attn_wo_coverage_cpu.py checks that the cases reach
all of them).  Without PICK the launch must also give the bits of the two launches it replaces (attn_short_kernel -> gemm3_kernel)
and the same bits out of place as in place (resid == out).  With PICK: the ids, the top-2 gap records and the K / V cache rows it
writes at attn_pos.  NaN sits in the cache behind the position and in padding rows / columns of resid / out that nothing may
read or write.  Then the whole matrix once more on a build whose dynamic LDS starts as NaN: the same bytes, or a word of LDS was
read before it was written."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from attn_wo_helpers import (CACHE_LEN, CASES, RESULT_KEYS, attention_ref, differing, pick_reference, rel_err, run_pick, run_plain,
                             same_bits, save_evidence)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HELPERS = Path(__file__).resolve().parent / "attn_wo_helpers.py"


@pytest.fixture(scope="module")
def E():
    from smoltts_amd import engine

    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def ops(E):
    from smoltts_amd import ops

    return ops


def _check_emission(d, out, M, N):
    assert rel_err(d["emit"], out * d["gamma"]) < 1e-6
    assert torch.allclose(d["ssq"].sum(-1), (out * out).sum(-1), rtol=1e-5)


def _padding_untouched(buf, M, N):
    assert torch.isnan(buf[M:]).all() and torch.isnan(buf[:, N:]).all(), "a padding row / column of out was written"


@pytest.mark.parametrize("c", [c for c in CASES if not c.pick], ids=lambda c: c.id)
def test_attn_wo_case(E, ops, c, tmp_path):
    assert E.load_library().smoltts_gemm3_attn_fusable(c.Hq, c.KV, CACHE_LEN) == 1
    M, N = c.M, c.Hq * 64
    d = run_plain(E, ops, c)
    out = d["out"][:M, :N]
    att = attention_ref(d["q"], d["k_cache"], d["v_cache"], c.pos, c.Hq)
    ref = (d["resid"].double() + att.double() @ d["w"].double().T).float()
    assert torch.isfinite(out).all()
    assert rel_err(out, ref) < 2e-5
    _check_emission(d, out, M, N)
    _padding_untouched(d["out"], M, N)
    assert rel_err(d["att_two"], att) < 2e-6

    # out of place: resid untouched, the same bits as in place (padding included)
    r_pad = torch.full_like(d["out"], float("nan"))
    r_pad[:M, :N] = d["resid"]
    assert same_bits(d["resid_after"], r_pad), "the out-of-place launch wrote into resid"
    for a, b in (("out", "out_sep"), ("emit", "emit_sep"), ("ssq", "ssq_sep")):
        if not same_bits(d[a], d[b]):
            f = save_evidence(tmp_path / "attn_wo_inplace_vs_separate.npz", d)
            pytest.fail(f"{a}: in place (resid == out) != out of place; evidence {f}; {differing(d[a], d[b])}")

    # the two launches it replaces: every sum in the same order, so the same bits
    for a, b in (("out", "out_two"), ("emit", "emit_two"), ("ssq", "ssq_two")):
        if not same_bits(d[a], d[b]):
            f = save_evidence(tmp_path / "attn_wo_fused_vs_two_launches.npz", d)
            pytest.fail(f"{a}: fused != two launches; evidence {f}; {differing(d[a], d[b])}")


@pytest.mark.parametrize("c", [c for c in CASES if c.pick], ids=lambda c: c.id)
def test_attn_wo_pick_case(E, ops, c):
    M, N = c.M, c.Hq * 64
    d = run_pick(E, ops, c)
    ref = pick_reference(c, d)
    assert torch.equal(d["ids"][0::2][:M], ref["ids"]), "ids != first argmax of the logits rows"
    assert (d["ids"][1::2] == -7).all(), "an id went to the wrong stride"
    assert same_bits(d["margin"], ref["margin"]) and torch.equal(d["margin_at"], ref["margin_at"]), "top-2 gap records"
    # cache rows at attn_pos from the table (K with RoPE), everything else as it was: below pos, NaN behind it, the spare slot
    assert same_bits(d["k_cache_after"], ref["k_cache"]), f"K cache: {differing(d['k_cache_after'].view(-1, 64), ref['k_cache'].view(-1, 64))}"
    assert same_bits(d["v_cache_after"], ref["v_cache"]), f"V cache: {differing(d['v_cache_after'].view(-1, 64), ref['v_cache'].view(-1, 64))}"
    out = d["out"][:M, :N]
    assert torch.isfinite(out).all()
    assert rel_err(out, ref["out"]) < 2e-5
    _check_emission(d, out, M, N)
    _padding_untouched(d["out"], M, N)


def _dump(lib, out: Path, timeout_s: int = 900):
    env = dict(os.environ)
    env.pop("SMOLTTS_LIB", None)
    if lib is not None:
        env["SMOLTTS_LIB"] = str(lib)
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s), sys.executable, str(HELPERS), str(out)], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, f"matrix run on {lib or 'the product library'}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(out)


def test_lds_poison_build_gives_the_product_bytes(tmp_path):
    """-DSMOLTTS_DBG_LDS_POISON (build.py variant lds_poison): attn_wo_kernel and gemm3_kernel start with all dynamic LDS = quiet NaN.
    Fragments left unwritten on purpose (rows >= M, kv heads that are not there) may only reach product columns nobody stores, and
    the partial tiles / row scales must be written before they are read: then every output byte is the product library's."""
    from smoltts_amd.build import build_library

    variant = build_library(variant="lds_poison")
    build_library()
    prod = _dump(None, tmp_path / "product.npz")
    pois = _dump(variant, tmp_path / "lds_poison.npz")
    want = sum(len(RESULT_KEYS[c.pick]) for c in CASES)
    assert len(prod.files) == want and sorted(prod.files) == sorted(pois.files)
    bad = [k for k in prod.files if prod[k].tobytes() != pois[k].tobytes()]
    assert not bad, f"{len(bad)} results differ with LDS poisoned (case index_result): {bad[:12]}; files {tmp_path}"
