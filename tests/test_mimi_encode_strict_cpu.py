"""What makes the bounds of tests/test_mimi_encode_strict_gpu.py meaningful, on the CPU alone: the float64 oracle and its
``stages``, the RVQ premise of every GPU case, and controls -- CPU computations standing in for the engine -- that the judges of
tests/mimi_enc_strict_helpers.py must reject: 2^-16-grade activations at every stage, a flipped padding side, one padding row more
or fewer at one stage, a missing window, one planted 1e-5 element.

Measured (weights seed 5, ``synthetic_pcm`` seed 4), min over the picks of float64 gap / E_d2 with the fp32 oracle's latents (the
premise asks >= 16), alignment rows on the left, then on the right:
  L = 1: 3.7e4, 6.3e3   L = 961: 165, 1.1e4   L = 2880: 6.0e3, 221   L = 9933: 63, 454   L = 40319: 158, 40   window 8: 274, 191
Rounding control (activations cut to two bf16 pieces; bound 4), smallest rms ratio of the chain / of the local ops per case:
  L = 1: 7.4 (zelu) / 6.1 (s_3)   L = 961: 8.3 (helu3) / 7.1 (s_2)   L = 9933: 9.0 (emb) / 7.5 (downsample), on the right 8.7 / 7.5
  L = 40319, window 8: 9.3 (K7) / 7.7 (k1_3);   conv0 reaches 28;   residual walk (max, rms) between 5.9, 9.1 and 20.1, 20.8.
A flipped padding side or one padding row more or fewer: 1e6 x E_ref at the first wrong buffer; window 8 against 0: 1e5 x on the latents.
"""
import numpy as np
import pytest
import torch

import mimi_enc_strict_helpers as H


def _stand_in(case, orc, lay=None):
    """The view set, codes, gaps and final residual an engine would leave if it computed what ``orc`` computes."""
    lay = lay or H.py_layout(case.L, case.extra_right)
    pcm = H.case_pcm(case.L)
    s = orc.stages(torch.from_numpy(pcm)[None, None])
    got = dict(H.views_from_stages(s, lay, case.extra_right))
    e = s["emb"].transpose(1, 2)
    codes = orc.rvq_encode(e)
    w = orc.rvq_walk(e, codes)
    got["res"] = w["after"][0, -1].numpy()
    return got, pcm, codes[0].numpy(), w["gap"][0].numpy(), lay


def test_float64_oracle_keeps_the_fp32_default_and_stages_compose():
    """``stages`` ends in ``embeddings`` bit for bit (fp32 and float64), the float64 oracle is the fp32 one's weights upcast (its
    latents within 2e-6), and the walk along an oracle's own codes reproduces them."""
    from oracle.mimi_oracle import MimiEncodeOracle

    case = H.CASES["ragged"]
    pcm = torch.from_numpy(H.case_pcm(case.L))[None, None]
    o32, o64 = H.oracles(case.window, case.extra_right)
    for o in (o32, o64):
        s = o.stages(pcm)
        emb = o.embeddings(pcm)
        assert emb.dtype == o.dt and torch.equal(s["emb"].transpose(1, 2), emb)
        assert torch.equal(s["seanet"].transpose(1, 2), o.seanet(pcm.to(o.dt)))
        codes = o.rvq_encode(emb)
        w = o.rvq_walk(emb, codes)
        assert torch.equal(w["argmin"], codes) and float(w["gap"].min()) > 0
        assert torch.equal(w["before"][:, 2] - o.codebook(2)[codes[0, 2]], w["after"][:, 2])
        # the single ops are the chain's: conv k3 of stage 1 on ELU(x1), the downsample on the transformer's output
        assert torch.equal(torch.nn.functional.elu(o.conv(torch.nn.functional.elu(s["x1"].transpose(1, 2)), "4.block.1")), s["h1"].transpose(1, 2))
        assert torch.equal(o.downsample(s["tr"].transpose(1, 2)), emb)
    d = (o32.embeddings(pcm).double() - o64.embeddings(pcm)).abs().max()
    assert 0 < float(d) < 2e-6, float(d)
    for k, v in o64.st.items():
        assert v.dtype == torch.float64 and torch.equal(v, H.state()[k].float().double()), k
    assert torch.equal(o64.codebook(3), o32.codebook(3).double())
    assert torch.equal(MimiEncodeOracle(H.state(), 8, act=lambda x: x).embeddings(pcm), o32.embeddings(pcm))


@pytest.mark.parametrize("name", list(H.CASES))
def test_layout_restatement(name):
    """``py_layout`` (the oracle's padding rule) against the lengths the oracle's convs really produce."""
    case = H.CASES[name]
    lay = H.py_layout(case.L, case.extra_right)
    v32 = H.references(case)[0]
    assert tuple(v32[f"xraw{i}"].shape[0] for i in range(4)) + (v32["zelu"].shape[0] - 2,) == lay.T
    assert v32["emb"].shape[0] == lay.F == -(-case.L // 1920)
    if name.startswith("ragged"):
        assert all(e > 0 for e in lay.extra), lay  # a stride-alignment remainder at every stage
    if name.startswith("two_pos"):
        assert lay.T[4] == 2 and lay.ds_extra == 0
    if name.startswith("three_pos"):
        assert lay.T[4] == 3 and lay.ds_extra == 1


@pytest.mark.parametrize("name", list(H.CASES))
def test_rvq_premise_and_the_fp32_oracle_passes_every_judge(name):
    """With the fp32 oracle standing in for the engine: every judge passes (all chain ratios are 1 by construction), and every pick's
    float64 gap is >= 16 E_d2(q, f) -- the premise under which the GPU tests allow no differing code."""
    case = H.CASES[name]
    got, pcm, codes, gap, lay = _stand_in(case, H.oracles(case.window, case.extra_right)[0])
    msgs, ratios = H.judge_call(f"{name} (fp32 oracle)", case, got, pcm, codes, gap, lay)
    assert ratios["rvq"]["premise"] >= H.PREMISE, f"{name}: min float64 gap / E_d2 = {ratios['rvq']['premise']:.1f}"
    assert all(abs(e - 1) < 1e-12 and abs(r - 1) < 1e-12 for _, e, r in ratios["chain"].values())


@pytest.mark.parametrize("name", ["one", "two_pos", "ragged", "ragged_right", "long_w8"])
def test_bounds_reject_two_piece_activations(name):
    """The rounding control: an fp32 oracle whose conv and Linear activations are cut to two bf16 pieces (2^-16-grade) must violate
    the chain RMS bound at every stage and layer, the local bound at every single-op stage and the residual walk's."""
    from oracle.mimi_oracle import MimiEncodeOracle

    case = H.CASES[name]
    ctrl = MimiEncodeOracle(H.state(), 8, window=case.window, extra_right=case.extra_right, act=H.two_pieces)
    got, pcm, codes, gap, lay = _stand_in(case, ctrl)
    msgs, ratios = H.judge_call(f"{name} (two-piece activations)", case, got, pcm, codes, gap, lay, expect_ok=False)
    for stage, (_, e, r) in ratios["chain"].items():
        assert r > H.FACTOR, f"{name}: the chain RMS bound lets two-piece activations through at {stage}: {r:.2f}"
    for op, (e, r) in ratios["local"].items():
        assert r > H.FACTOR, f"{name}: the local RMS bound lets two-piece activations through at {op}: {e:.2f}, {r:.2f}"
    assert min(ratios["rvq"]["res"]) > H.FACTOR, ratios["rvq"]["res"]
    print(f"{name}: smallest chain rms ratio {min((r, s) for s, (_, _, r) in ratios['chain'].items())}, smallest local rms ratio "
          f"{min((r, s) for s, (_, r) in ratios['local'].items())}, residual walk {ratios['rvq']['res']}")


def test_flipped_padding_side_is_named():
    """``extra_right`` flipped at a ragged length: the data up to y0 is the same (stride-1 convs have no alignment rows), the first
    strided conv's output is the first wrong buffer, and locally exactly the strided convs and the downsample fail."""
    case = H.CASES["ragged"]
    lay = H.py_layout(case.L, False)
    got, pcm, codes, gap, _ = _stand_in(case, H.oracles(case.window, True)[0], lay)
    v32, v64, _, _ = H.references(case)
    cf, cr = H.chain_report(got, v32, v64, lay)
    assert cf and cf[0].stage == "xraw1" and cf[0].max_ratio > 1e3, cf[:1]
    assert {f.stage for f in cf} == {k for k in cr if k not in ("xraw0", "xelu0", "helu0", "yelu0")}
    lf, lr = H.local_report(got, pcm, lay, *H.oracles(case.window, False))
    assert [f.stage for f in lf] == ["s_0", "s_1", "s_2", "s_3", "downsample"] and min(f.max_ratio for f in lf) > 1e3, lf
    print("flipped padding side: first chain failure", cf[0].msg, "\n  local:", {f.stage: round(f.max_ratio) for f in lf})


@pytest.mark.parametrize("delta", [1, -1])
def test_one_padding_row_more_or_fewer_is_named(delta):
    """Stage 2's strided conv reading one zero row more (or fewer) in front of its data: x3 is the first wrong buffer, and locally
    only that conv fails -- every other op is consistent with its own input."""
    import torch.nn.functional as F
    from oracle.mimi_oracle import MimiEncodeOracle

    case = H.CASES["ragged"]

    class OffByOne(MimiEncodeOracle):
        def conv(self, x, key, stride=1):
            if key != "9":  # encoder.layers.9: the strided conv of stage 2 (ratio 6)
                return super().conv(x, key, stride)
            shifted = F.pad(x, (1, 0))[..., :-1] if delta > 0 else F.pad(x[..., 1:], (0, 1))
            return super().conv(shifted, key, stride)

    got, pcm, codes, gap, lay = _stand_in(case, OffByOne(H.state(), 8, window=case.window))
    v32, v64, _, _ = H.references(case)
    cf, cr = H.chain_report(got, v32, v64, lay)
    assert cf and cf[0].stage == "xraw3" and cf[0].max_ratio > 1e3, cf[:1]
    lf, lr = H.local_report(got, pcm, lay, *H.oracles(case.window, False))
    assert [f.stage for f in lf] == ["s_2"] and lf[0].max_ratio > 1e3 and lf[0].rms_ratio > 1e3, lf
    assert not H.structure_report(got, lay, False)
    print(f"padding rows {delta:+d} at stage 2: chain {cf[0].msg}\n  local {lf[0].msg}")


def test_structure_judge_sees_one_bit():
    case = H.CASES["ragged_right"]
    got, pcm, codes, gap, lay = _stand_in(case, H.oracles(case.window, True)[0])
    assert not H.structure_report(got, lay, True)
    for name, row in (("xelu2", 1), ("zelu", 0), ("yelu1", lay.left[1] - 1), ("yelu3", lay.left[3] + lay.T[3])):
        bad = dict(got); bad[name] = got[name].copy(); bad[name][row, 5] = 1e-30
        msgs = H.structure_report(bad, lay, True)
        assert len(msgs) == 1 and f"{name} " in msgs[0] and f"row {row} " in msgs[0] and "channel 5" in msgs[0], msgs
    bad = dict(got); bad["ds"] = got["ds"].copy(); bad["ds"][-1, 7] = np.nextafter(bad["ds"][-1, 7], np.float32(9))
    msgs = H.structure_report(bad, lay, True)
    assert len(msgs) == 1 and "ds edge row" in msgs[0] and "channel 7" in msgs[0], msgs
    bad = dict(got); bad["xelu1"] = got["xelu1"].copy(); bad["xelu1"][2 + 17, 3] += 2e-7
    msgs = H.structure_report(bad, lay, True)
    assert len(msgs) == 1 and "xelu1 row 17 " in msgs[0] and "channel 3" in msgs[0], msgs


def test_window_is_reached():
    """``window = 8`` against ``window = 0`` over 42 positions: layer 0's K / V are the same, every later buffer moves by far more
    than the bound, so an engine that ignored the window cannot pass the ``long_w8`` case."""
    case = H.CASES["long_w8"]
    got, pcm, codes, gap, lay = _stand_in(case, H.oracles(0, False)[0])
    v32, v64, _, _ = H.references(case)
    cf, cr = H.chain_report(got, v32, v64, lay)
    assert cf and cf[0].stage == "K1" and {f.stage for f in cf} >= {"ds", "emb"} | {f"K{l}" for l in range(1, 8)}, [f.stage for f in cf]
    _, e, r = cr["emb"]
    assert e > 100 * H.FACTOR and r > 100 * H.FACTOR, (e, r)
    print(f"window 8 vs 0: emb max err {e:.0f} x E_ref, rms {r:.0f} x R_ref; first failure {cf[0].msg}")


def test_helper_names_a_planted_element():
    """One element of one buffer moved by 1e-5: exactly one chain failure, naming the stage, the row and the channel; the local judge
    names it as the output of its op; a wrong code, a wrong gap and a residual element off by 1e-4 are each named."""
    case = H.CASES["ragged"]
    o32, o64 = H.oracles(case.window, case.extra_right)
    good, pcm, codes, gap, lay = _stand_in(case, o32)
    v32, v64, _, _ = H.references(case)
    for name, row, ch in (("helu1", 2483, 63), ("yelu2", 130, 7), ("xraw3", 64, 500), ("kc", 5, 77), ("emb", 3, 11)):
        got = dict(good)
        got[name] = good[name].copy()
        if name == "kc":
            got[name][4, ch // 64, row, ch % 64] += 1e-5
        else:
            H.data_rows(name, got[name], lay)[row, ch] += 1e-5
        cf, _ = H.chain_report(got, v32, v64, lay)
        want = "K4" if name == "kc" else name
        assert len(cf) == 1 and (cf[0].stage, cf[0].row, cf[0].channel) == (want, row, ch), cf
        assert f"{want} row {row} of" in cf[0].msg and f"row mod 64 = {row % 64}" in cf[0].msg and f"channel {ch}" in cf[0].msg
        assert ("LAST row" in cf[0].msg) == (name == "helu1")
    got = dict(good); got["helu1"] = good["helu1"].copy(); got["helu1"][2483, 63] += 1e-5
    lf, _ = H.local_report(got, pcm, lay, o32, o64)
    assert lf and (lf[0].stage, lf[0].row, lf[0].channel) == ("k3_1", 2483, 63) and {f.stage for f in lf} == {"k3_1", "k1_1"}, lf
    # RVQ: a code that is not the argmin, a gap off by 16 E_d2, a residual element off by 1e-4
    c2 = codes.copy(); c2[3, 2] = (c2[3, 2] + 1) % 2048
    msgs, _ = H.rvq_report(good["emb"], c2, None, None, o32, o64)
    assert msgs[0].startswith("rvq: codebook 3, frame 2: code ") and all(", frame 2:" in m and int(m[14]) >= 3 for m in msgs), msgs
    c2 = codes.copy(); c2[7, 5] = (c2[7, 5] + 1) % 2048  # (the walk follows the given codes: only a last codebook leaves the rest alone)
    msgs, _ = H.rvq_report(good["emb"], c2, None, None, o32, o64)
    assert len(msgs) == 1 and msgs[0].startswith(f"rvq: codebook 7, frame 5: code {c2[7, 5]}, float64 argmin {codes[7, 5]},"), msgs
    w64 = o64.rvq_walk(torch.from_numpy(good["emb"].T.copy())[None], torch.from_numpy(codes)[None])
    g2 = w64["gap"][0].numpy().copy(); g2[6, 4] += 16 * H.e_d2(o32, w64)[6, 4]
    r2 = good["res"].copy(); r2[1, 200] += 1e-4  # (residual elements reach 20 and E_ref 1e-5: 1e-5 is inside its bound)
    msgs, _ = H.rvq_report(good["emb"], codes, g2, r2, o32, o64)
    assert len(msgs) == 2 and msgs[0].startswith("rvq gap: codebook 6, frame 4:") and "res row 1 of 6" in msgs[1] and "channel 200" in msgs[1], msgs
