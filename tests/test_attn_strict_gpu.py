"""Every launchable form of the attention kernels (csrc/attention.hip) against float64, judged by the fp32 reference's own noise.

One pytest case per kernel form ``launch_attention`` / ``launch_attention_rows3`` can reach (28: tests/attn_strict_helpers.py
``launchable()``, held to the built code objects by tests/test_attn_strict_cpu.py); each runs its cases of the helpers' list in
both data regimes -- flat (q, k, v ~ N(0, 1)) and planted (scores of standard deviation 5, a dominant key per row at an edge of
its visible range or just outside it, V + 1e3 in every entry no row may see).  Per case and regime, pooled over the rows that see
at least two keys, on the CPU
    E_ref = max|fp32 reference - float64 reference|   and   R_ref = RMS of the same difference,
both references plain softmax(q K^T / 8) V over keys [max(0, pos + 1 - window), pos] of the row's slot, and required:
    max|kernel - float64| <= 4 E_ref   and   RMS(kernel - float64) <= 4 R_ref.
The factor 4 is the project's rule for two computations that differ by fp32 rounding (tests/lm_strict_helpers.py FACTOR).  A row
that sees one key must be that V row bit for bit in the per-row kernels and within 4 E_ref in the tile kernels; a row with nothing
cached (pos = -1, pos = cache_len) must be zero; the X3 output must hold the fp32 rows' numbers, and the fp32 rows must not
depend on it.  That the bound rejects 2^-16-grade arithmetic on every case's flat data, and a key admitted or dropped at either
edge of a range on every case's planted data: tests/test_attn_strict_cpu.py.  A failure names the form, case, regime, row, slot,
pos, j_lo, query head and dim of the worst element and both ratios.

attn_rows3_kernel<2, 3> is the 2^-16-grade form by design (three of the six bf16x3 products): both regimes are judged, by the
same rule, against its own model -- the operands of both products cut to hi + mid pieces, the probabilities cut where the kernel
cuts them -- in float64, with E_ref / R_ref from the fp32 run of that model (``rows3_three_product_model``).

The key-split cases share one scratch for the whole module (tickets count up across launches, the records start as NaN).

Measured on the MI355X, worst case of each form: max err / E_ref, rms / R_ref (bound 4), flat regime | planted regime:
  attn_kernel<1,false>               1.27, 1.06 | 0.75, 0.72
  attn_kernel<2,false>               1.09, 0.77 | 1.39, 0.98
  attn_kernel<3,false>               1.17, 0.79 | 0.79, 0.80
  attn_kernel<4,false>               0.89, 0.71 | 0.91, 0.86
  attn_prefill_kernel<1,false>       1.63, 1.30 | 1.97, 1.80
  attn_prefill_kernel<1,true>        1.39, 1.32 | 1.99, 1.77
  attn_rows3_kernel<2,3>             1.34, 1.42 | 1.71, 1.12
  attn_rows3_kernel<2,6>             1.23, 0.90 | 2.34, 1.30
  attn_short_kernel<1,2>             1.00, 0.88 | 0.42, 0.53
  attn_short_kernel<1,4>             0.85, 0.81 | 0.61, 0.75
  attn_short_kernel<2,2>             0.84, 0.83 | 1.13, 0.94
  attn_short_kernel<2,4>             0.74, 0.74 | 0.73, 0.86
  attn_short_kernel<3,2>             0.75, 0.71 | 0.78, 0.83
  attn_short_kernel<3,4>             0.90, 0.82 | 1.06, 0.85
  attn_short_kernel<4,2>             1.00, 0.79 | 0.63, 0.73
  attn_short_kernel<4,4>             0.79, 0.79 | 0.77, 0.82
  attn_split_kernel<1,false,2>       0.42, 0.46 | 0.87, 0.87
  attn_split_kernel<1,true,1>        1.48, 0.87 | 1.01, 1.01
  attn_split_kernel<1,true,2>        0.48, 0.50 | 0.50, 0.70
  attn_split_kernel<2,false,2>       0.52, 0.54 | 0.64, 0.74
  attn_split_kernel<2,true,1>        0.95, 0.74 | 1.00, 0.92
  attn_split_kernel<2,true,2>        0.66, 0.58 | 1.62, 1.06
  attn_split_kernel<3,false,2>       0.51, 0.51 | 1.05, 0.65
  attn_split_kernel<3,true,1>        1.04, 0.83 | 1.01, 0.85
  attn_split_kernel<3,true,2>        0.79, 0.56 | 0.72, 0.71
  attn_split_kernel<4,false,2>       0.87, 0.52 | 0.91, 0.79
  attn_split_kernel<4,true,1>        1.05, 0.87 | 0.86, 0.98
  attn_split_kernel<4,true,2>        0.45, 0.51 | 0.93, 0.76
i.e. every form is as close to float64 as the fp32 CPU reference is (0.42 .. 2.34); the matrix-core kernels sit a little higher than
the per-row ones, as in tests/test_lm_strict_gpu.py.  The hardware exponential (|x| 2^-24 relative on e^x) needed no term of its own.
"""
import pytest
import torch

from attn_strict_helpers import BY_FORM, REGIMES, form_id, launchable, make_data, references, run_case, strict_report

pytestmark = pytest.mark.gpu

FORMS = sorted(launchable(), key=form_id)


@pytest.fixture(scope="module")
def ops():
    from smoltts_amd import engine, ops

    engine.load_library()
    return ops


@pytest.fixture(scope="module")
def scratch(ops):
    part = torch.full((ops.SPLIT_PART_FLOATS,), float("nan"), device="cuda")  # poisoned once: only a launch's own records may be read
    ticket = torch.zeros(ops.SPLIT_TICKETS, dtype=torch.int32, device="cuda")
    yield part, ticket
    assert int((ticket.cpu() % 2).sum()) == 0  # every pair that took tickets took them in twos


@pytest.mark.parametrize("form", FORMS, ids=[form_id(f) for f in FORMS])
def test_form_matches_float64_within_the_fp32_reference_noise(ops, scratch, form):
    fails, worst = [], {r: (0.0, 0.0) for r in REGIMES}
    tickets = scratch[1].cpu()
    for c in BY_FORM[form]:
        for regime in REGIMES:
            got = run_case(ops, c, make_data(c, regime), scratch)
            f, (e, r) = strict_report(got, *references(c, regime), c, regime)
            print(f"{form_id(form)} {c.name} {regime}: max {e:.2f} x E_ref, rms {r:.2f} x R_ref")
            fails += f
            worst[regime] = (max(worst[regime][0], e), max(worst[regime][1], r))
    print(f"WORST {form_id(form):34s} " + " | ".join(f"{worst[r][0]:.2f}, {worst[r][1]:.2f}" for r in REGIMES))
    assert not fails, "\n".join(fails)
    if form[0] == "attn_split_kernel" and form[1][2] == 2:  # rows of 512 keys and more were dealt over two workgroups, the others were not
        took = scratch[1].cpu() - tickets
        assert int(took.sum()) > 0 and int((took % 2).sum()) == 0, took.tolist()
