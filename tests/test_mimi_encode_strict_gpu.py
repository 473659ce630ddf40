"""Mimi encode, per stage, per latent and per code: the HIP chain against the float64 oracle, judged by the fp32 oracle's own noise.

tests/test_mimi_encode_gpu.py holds the latents to 1e-4 of their maximum against the fp32 oracle, 150 to 200 times that oracle's own
distance from float64, and sees nothing between the PCM and the latents.  Here every buffer the chain leaves in its workspace
(``MimiEncoder.stage_views``, mapped by ``smoltts_mimi_encode_layout``) is read back and judged by tests/mimi_enc_strict_helpers.py:
  structure  every halo / padding row bit-zero, the edge rows of the downsample input bit-equal to their neighbour, every ELU copy
             within 6e-8 of the ELU of its raw copy;
  chain      per buffer and per layer's K / V:  max|gpu - float64| <= 4 E_ref  and  RMS <= 4 R_ref,  E_ref / R_ref = the fp32
             oracle's own distance from the float64 oracle (CPU only);
  local      per single op (conv0, the twelve SEANet convs, the downsample): the float64 op applied to the GPU's OWN input buffer
             against the GPU's output buffer, the yardstick fp32 torch on that same input, factor 4 again;
  RVQ        teacher-forced on the GPU's latents along the GPU's codes: every code the float64 argmin, |gap - float64 gap| <=
             8 E_d2(q, f), the final residual within 4 E_ref of the fp32 walk; and the codes equal the float64 oracle's end to end.
No differing code is excused: tests/test_mimi_encode_strict_cpu.py shows, with the reference alone, that every pick of every case
has a float64 gap >= 16 E_d2, and that each bound rejects 2^-16-grade activations, a wrong padding row and a missing window.

The encoder has no bf16x3 weights, so every GEMM is an exact-product fp32 kernel.  Where ``launch_gemm_impl`` sends them:
  L = 1, 961, 2880 (1, 2, 3 positions), 9933 (11 positions, 6 frames): every GEMM on ``launch_mt`` -- MT = 1 up to 16 rows, MT = 2 up
      to 32, MT = 4 with a ragged last tile beyond; the transformer's QKV and fc1 take the in-kernel LayerNorm prologue (M <= 16).
  L = 40319 (42 positions, 21 frames): stage 0's conv k3 (M = 40319, N = 32: 315 workgroups of 128 rows, the last holds 127) and
      conv k1 (N = 64: 630 workgroups of 64 rows, the last holds 63) run on ``launch_rows``; every later GEMM has fewer than 192
      workgroups there (stage 0's strided conv: M = 10080, 158) and stays on ``launch_mt`` at MT = 4; the transformer (M = 42) runs
      the stand-alone LayerNorm; the RVQ GEMMs (M = 21) run at MT = 2.

Measured on the MI355X (bound 4; 8 for a gap).  Chain: worst max err / E_ref, rms / R_ref per group; at L = 40319 E_ref runs from
1.4e-7 (conv0) to 2.0e-6 (K), R_ref from 8e-9 to 3.7e-7.  The cases with the alignment rows on the right in brackets where they differ:
  case       conv0       stage0      stage1      stage2      stage3      K           V           tr          emb
  L = 1      1.08 1.00   1.53 1.26   0.89 0.75   0.58 0.72   0.77 0.58   0.79 0.78   0.90 0.79   0.84 0.74   0.69 0.68
             [same       same        0.67 0.76   0.79 0.75   0.49 0.48   0.85 0.82   0.91 0.87   0.88 0.84   0.85 0.78]
  L = 961    1.46 1.95   0.98 1.05   1.13 1.01   1.03 0.92   0.33 0.37   0.43 0.43   0.42 0.42   0.31 0.39   0.46 0.45
             [same       same        1.12 1.00   0.85 0.92   0.37 0.37   0.41 0.39   0.51 0.37   0.37 0.36   0.34 0.38]
  L = 2880   1.36 1.70   0.97 1.04   1.25 1.00   1.09 1.01   1.01 0.93   0.52 0.39   0.42 0.41   0.35 0.37   0.25 0.38  [emb 0.27 0.37]
  L = 9933   1.12 1.84   1.08 1.05   1.15 1.00   1.13 1.14   1.32 1.21   0.73 0.65   0.78 0.65   0.26 0.63   0.39 0.53
             [same       same        1.27 1.00   1.37 1.14   1.36 1.22   0.64 0.64   0.79 0.64   0.32 0.62   0.44 0.52]
  L = 40319  1.21 1.83   2.81 2.08   1.12 1.04   1.15 1.15   1.63 1.45   1.62 1.40   1.64 1.41   1.51 1.46   1.35 1.44
             [same       same        1.29 1.04   1.35 1.15   1.62 1.44   1.39 1.39   1.67 1.42   1.40 1.46   1.49 1.44]
  window 8   as L = 40319 up to stage3;  K 1.61 1.40   V 1.43 1.41   tr 1.41 1.47   emb 1.34 1.45   [1.46 1.39, 1.56 1.42, 1.42 1.46, 1.42 1.44]
  L = 961 on the workspace L = 40319 left: the figures of L = 961, to the digit, for both padding sides.
Local, worst op per case (max, rms): L = 1 k1_2 1.40, k3_0 1.18; L = 961 conv0 1.27, 1.95 [k3_1 1.60]; L = 2880 k3_1 1.80, conv0 1.70;
  L = 9933 k3_2 1.51 [k3_1 1.80], conv0 1.84; L = 40319 k3_0 3.00, 2.10 (the 128-row ``launch_rows`` kernel at K = 192), s_3 2.06,
  every other op <= 1.62.
RVQ: final residual <= 1.00, 0.92; worst |gap - float64 gap| / E_d2 1.39 (L = 2880; E_d2 between 3e-4 and 5e-3); no code differs from
  the float64 argmin nor from the float64 oracle's end-to-end codes.  Min float64 gap / E_d2 on the GPU's latents: L = 1 3.6e4 [6.4e3],
  L = 961 171 [1.2e4], L = 2880 4.5e3 [275], L = 9933 61 [584], L = 40319 155 [35], window 8 334 [199] (premise on the CPU: >= 16).
Nothing needed a factor to rise, and no kernel or plan fault showed.  The 15 tests take 6 s together, oracles included.
"""
import numpy as np
import pytest
import torch

import mimi_enc_strict_helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def encoders():
    """One packed arena, one ``MimiEncoder`` per (window, extra_right) on demand."""
    from smoltts_amd import packing
    from smoltts_amd.engine import MimiEncoder

    arena, offsets = packing.pack_mimi_encoder(H.state(), 8)
    made = {}

    def get(window, extra_right):
        if (window, extra_right) not in made:
            made[window, extra_right] = MimiEncoder(None, 8, window=window, extra_right=extra_right, arena=arena, offsets=offsets)
        return made[window, extra_right]

    yield get
    for e in made.values():
        e.close()


def _encode_and_judge(label, enc, case):
    pcm = H.case_pcm(case.L)
    codes, emb, gap = enc.encode(pcm, return_aux=True)
    lay = enc.layout(case.L)
    assert lay.total == enc.lib.smoltts_mimi_encode_workspace_bytes(enc.handle, case.L) and lay.F == enc.frames(case.L)
    got = {k: v.cpu().numpy() for k, v in enc.stage_views(case.L).items()}
    assert np.array_equal(got["emb"], emb.cpu().numpy())
    return H.judge_call(label, case, got, pcm, codes.cpu().numpy(), gap.cpu().numpy(), H.layout_of(lay))


@pytest.mark.parametrize("name", list(H.CASES))
def test_encode_per_stage(encoders, name):
    """Every case of the helper's table: one sample; 2 and 3 positions (``ds_extra`` 0 and 1); a remainder at every stage; the long
    signal on ``launch_rows``, with and without a window of 8; each again with the alignment rows behind the data."""
    case = H.CASES[name]
    _encode_and_judge(name, encoders(case.window, case.extra_right), case)


@pytest.mark.parametrize("extra_right", [False, True])
def test_second_call_on_a_used_workspace(encoders, extra_right):
    """The long signal, then L = 961 on the same encoder: the short call's buffers lie inside the bytes the long one filled, and are
    judged like a first call's -- the memset and the plan must not depend on what was there."""
    enc = encoders(0, extra_right)
    long, short = H.Case(1920 * 21 - 1, 0, extra_right), H.Case(961, 0, extra_right)
    enc.encode(H.case_pcm(long.L))
    size = enc._ws.numel()
    _encode_and_judge(f"L = 961 after L = {long.L}, extra_right={extra_right}", enc, short)
    assert enc._ws.numel() == size and enc.layout(short.L).total < size


def test_layout_export_and_stage_views_contract(encoders):
    from smoltts_amd.engine import SmolttsError

    enc = encoders(0, False)
    L = 1920 * 5 + 333
    lay = enc.layout(L)
    offs = [lay.xraw[0], lay.xelu[0], lay.helu[0], lay.yelu[0], lay.xraw[1], lay.xelu[3], lay.yelu[3], lay.zelu, lay.kc, lay.vc, lay.ds,
            lay.emb, lay.res, lay.dots, lay.total]
    assert lay.xraw[0] == 0 and offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    assert lay.vc - lay.kc == enc.c_cfg.n_layers * lay.layer_stride == enc.c_cfg.n_layers * 8 * lay.T[4] * 64 * 4
    assert lay.total - lay.dots >= 4 * lay.F * 2048 + 8 * lay.T[4]
    with pytest.raises(SmolttsError):
        enc.layout(0)
    enc.encode(H.case_pcm(L))
    with pytest.raises(SmolttsError, match="last encode"):
        enc.stage_views(L + 1)
    v = enc.stage_views(L)
    assert v["emb"].shape == (lay.F, 512) and float(v["emb"].abs().max()) > 0  # (no return_aux: the workspace's own latents)
