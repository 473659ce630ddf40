"""The premises of tests/test_attn_align_gpu.py, on the CPU, on every case's own data (tests/attn_align_helpers.py).

* The fp32 numpy reference passes the report by construction, and its error against float64 is nonzero for every (case, regime):
  for m under every window that holds a visible key, and for s1 under every window wider than one key.
* The float64 reference meets the planted checks: the dominant keys do dominate, inside and outside each window.
* On the planted data a window shifted by one key, and a softmax without the 1 / 8, each exceed the bound by more than 100 x FACTOR:
  a kernel that passes the GPU test has neither fault at any position.
* The launch that must write nothing, and the window that must give (0, 0), are what the references say they are."""
import numpy as np
import pytest

import attn_align_helpers as H

PARAMS = [(c, regime) for c in H.CASES for regime in H.REGIMES]
IDS = [f"{c.name}-{r}" for c, r in PARAMS]


@pytest.mark.parametrize("c,regime", PARAMS, ids=IDS)
def test_the_fp32_reference_passes_with_nonzero_error_and_the_plants_dominate(c, regime):
    pool, rows, fails = H.Pool(), H.judged_rows(c), []
    for win, plant in H.variants(regime):
        d, r32, r64 = H.references(c, regime, win, plant)
        if win == "empty":
            continue
        if win == "beyond":
            assert not r64.any() and not r32.any()
        pool.add(win, r32, r32, r64, rows)
        if plant:
            assert d.planted, (c.name, win, plant)  # every launch of the list carries dominant keys
            fails += H.planted_checks(c, d, plant, r64, r64, "float64")
    assert not fails, "\n".join(fails)
    f, worst, _ = pool.report(f"{c.name} {regime}")
    assert not f and worst == 1.0, (f, worst)
    for (win, comp), own in pool.own.items():
        e_ref = float(np.abs(np.concatenate(own)).max())
        if win == "beyond" or (win == "first" and comp == 1):
            assert e_ref == 0.0, (win, comp, e_ref)
        else:
            assert e_ref > 0.0, f"{c.name} {regime} window {win} component {comp}: the fp32 reference is exact"


@pytest.mark.parametrize("c", H.CASES, ids=[c.name for c in H.CASES])
def test_a_shifted_window_or_a_missing_scale_exceeds_the_bound_a_hundredfold(c):
    rows = H.judged_rows(c)
    for mutant, kw in (("window shifted by one key", {"shift": 1}), ("window shifted back by one key", {"shift": -1}),
                       ("no 1/8 scale", {"scale": 1.0})):
        worst = {}
        for win, plant in H.variants("planted"):
            if win in ("beyond", "empty") or plant == "pos1":
                continue
            d, r32, r64 = H.references(c, "planted", win, plant)
            bad = H.reference(c, d, np.float32, **kw)
            e_ref = np.abs(r32[rows].astype(np.float64) - r64[rows]).max(axis=(0, 1))  # (m, s1)
            e = np.abs(bad[rows].astype(np.float64) - r64[rows]).max(axis=(0, 1))
            # the component that shows it most (under [0, pos + 1) m is 1 whatever the scores are; under [0, 1) s1 is 0)
            worst[win, plant] = max(e[k] / e_ref[k] for k in (0, 1) if e_ref[k] > 0)
        print(f"{c.name}: {mutant}: (m, s1) off by {min(worst.values()):.3g} .. {max(worst.values()):.3g} x E_ref")
        if "shifted" in mutant:
            # a shift shows where a dominant key sits at the edge it moves across
            edge = ("t0", "after") if kw["shift"] == 1 else ("last", "before")
            seen = [v for (win, plant), v in worst.items() if plant in edge and win != "first"]
            assert seen and min(seen) > 100 * H.FACTOR, (c.name, mutant, worst)
        else:
            assert min(worst.values()) > 100 * H.FACTOR, (c.name, mutant, worst)


def test_the_long_cases_cross_the_lds_staging_limit():
    for c in H.LONG_CASES:
        assert c.cache_len > H.LDS_KEYS and max(c.row_pos) >= H.LDS_KEYS
    assert all(c.cache_len <= H.LDS_KEYS for c in H.CASES)
