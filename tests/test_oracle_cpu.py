"""CPU suite: the oracle against the committed golden vectors (which were produced against the
reference's own RQTransformer.forward / against transformers.MimiModel), plus its self-consistency."""
import numpy as np
import pytest
import torch


def _lm(cfgname, seed):
    from oracle.lm_oracle import LMOracle, OracleLMConfig
    from smoltts_amd.synthetic import named_config, state_fingerprint, synthetic_lm_state

    cfg = named_config(cfgname)
    state = synthetic_lm_state(cfg, seed=seed)
    return cfg, state, LMOracle(OracleLMConfig.from_dict(cfg.__dict__), state), state_fingerprint(state)


@pytest.mark.parametrize("name", ["tiny", "tiny_nodup", "tiny_proj", "70m"])
def test_lm_oracle_reproduces_goldens(name, golden_dir):
    g = np.load(golden_dir / f"lm_{name}.npz")
    cfg, state, orc, fp = _lm(str(g["config_name"]), int(g["seed"]))
    assert abs(fp - float(g["fingerprint"])) <= 1e-6 * abs(fp)
    n = len(g["texts"])
    logs = orc.generate([torch.from_numpy(g[f"prompt_{b}"]) for b in range(n)], max_frames=int(g["frames"]), stop_on_eos=False)
    for b in range(n):
        assert np.array_equal(logs[b].as_tensor().numpy(), g[f"grid_{b}"])
        # the reference forward's own logits at three positions (teacher-forced on the golden grid)
        full = torch.cat([torch.from_numpy(g[f"prompt_{b}"]).long(), torch.from_numpy(g[f"grid_{b}"]).long()], dim=1)
        tok, cb = orc.teacher_forced(full)
        rows = g[f"ref_rows_{b}"].tolist()
        assert np.allclose(tok[rows].numpy(), g[f"ref_token_logits_{b}"], atol=5e-5)
        assert np.allclose(cb[rows][:, :, :64].numpy(), g[f"ref_codebook_logits_{b}"], atol=2e-6)


def test_lm_oracle_batch_invariance_and_eos():
    """Batched decode == one-by-one decode; stop rule: the <|im_end|> frame is emitted, then nothing."""
    from oracle.lm_oracle import LMOracle, OracleLMConfig
    from smoltts_amd.prompt import PromptEncoder
    from smoltts_amd.synthetic import named_config, synthetic_lm_state
    from smoltts_amd.tokenizer import load_tokenizer

    cfg = named_config("tiny")
    state = synthetic_lm_state(cfg, seed=5)
    pe = PromptEncoder(load_tokenizer(), 320)
    prompts = [torch.from_numpy(pe.build_prompt(t, "heart")) for t in ("abc", "a longer second prompt", "x")]
    ocfg = OracleLMConfig.from_dict(cfg.__dict__)
    batched = LMOracle(ocfg, state).generate(prompts, max_frames=6, stop_on_eos=False)
    for b, p in enumerate(prompts):
        single = LMOracle(ocfg, state).generate([p], max_frames=6, stop_on_eos=False)[0]
        assert single.grid == batched[b].grid
    eos = batched[1].grid[2][0]
    ocfg2 = OracleLMConfig.from_dict({**cfg.__dict__, "im_end_id": eos})
    logs = LMOracle(ocfg2, state).generate(prompts, max_frames=6, stop_on_eos=True)
    first = next(f for f in range(6) if batched[1].grid[f][0] == eos)
    assert len(logs[1].grid) == first + 1 and logs[1].grid == batched[1].grid[: first + 1]


def test_lm_oracle_mlx_mode_differs_only_by_documented_quirks():
    from oracle.lm_oracle import LMOracle, OracleLMConfig, rope_table
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    state = synthetic_lm_state(cfg, seed=1)
    ocfg = OracleLMConfig.from_dict(cfg.__dict__)
    a, b = LMOracle(ocfg, state, "torch", True), LMOracle(ocfg, state, "mlx", False)
    cols = torch.tensor([[72] + [0] * 8, [320 + 5] + [5, 1, 2, 3, 4, 5, 6, 7], [400] + [0, 9, 9, 9, 9, 9, 9, 9]])
    ea, eb = a.embed(cols), b.embed(cols)
    assert torch.equal(ea[0], eb[0]) and torch.equal(ea[1], eb[1])  # text row / ordinary audio row agree
    assert not torch.equal(ea[2], eb[2])  # code0 == 0 on a semantic row: torch zeroes the code sum, MLX keeps it
    t_bf, t_ex = rope_table(64, 64, 1e5, True), rope_table(64, 64, 1e5, False)
    assert float((t_bf - t_ex).abs().max()) < 4e-3 and not torch.equal(t_bf, t_ex)


def test_mimi_oracle_matches_hf_goldens_and_live_model(golden_dir):
    from oracle.mimi_oracle import MimiDecodeOracle
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    g = np.load(golden_dir / "mimi_hf.npz")
    st = synthetic_mimi_state(seed=int(g["seed"]))
    fp = float(sum(float(v.double().abs().sum()) for v in st.values()))
    assert abs(fp - float(g["fingerprint"])) <= 1e-9 * fp
    codes = torch.from_numpy(g["codes"]).long()
    out = MimiDecodeOracle(st, window=250).decode(codes).numpy()
    assert out.shape == g["pcm"].shape
    assert float(np.sqrt(np.mean((out - g["pcm"]) ** 2))) < 1e-6
    # window = 0 (MLX behaviour) is identical while the context is shorter than 250 positions
    assert np.array_equal(MimiDecodeOracle(st, window=0).decode(codes).numpy(), out)
    transformers = pytest.importorskip("transformers")
    m = transformers.MimiModel(transformers.MimiConfig()).eval()
    m.load_state_dict(st, strict=False)
    codes2 = torch.randint(0, 2048, (1, 8, 9), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref = m.decode(codes2)[0].numpy()
    assert float(np.sqrt(np.mean((MimiDecodeOracle(st, window=250).decode(codes2).numpy() - ref) ** 2))) < 1e-6


def test_mimi_oracle_is_causal():
    from oracle.mimi_oracle import MimiDecodeOracle
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    orc = MimiDecodeOracle(synthetic_mimi_state(seed=1))
    codes = torch.randint(0, 2048, (1, 8, 7), generator=torch.Generator().manual_seed(0))
    full, prefix = orc.decode(codes), orc.decode(codes[:, :, :3])
    assert float((full[..., : 3 * 1920] - prefix).abs().max()) < 1e-5


def test_mimi_oracle_per_call_upsample_is_the_reference_stream():
    """``decode(codes, upsample_call_frames=c)``: what a stream of ``decode_step`` calls of c frames yields in the reference
    (codec/mimi.py:73-77: ``self.upsample`` sees the call's frames only; conv.py:273-282: full transposed conv, k - stride = 2 rows
    trimmed on the right).  Checked against that definition written out per frame, and against the properties that follow from it."""
    import torch.nn.functional as F

    from oracle.mimi_oracle import MimiDecodeOracle
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    st = synthetic_mimi_state(seed=2)
    orc = MimiDecodeOracle(st)
    codes = torch.randint(0, 2048, (2, 8, 6), generator=torch.Generator().manual_seed(5))
    batch = orc.decode(codes)
    # one call over the whole utterance (or more): the batch decode, bit for bit
    assert torch.equal(orc.decode(codes, upsample_call_frames=6), batch) and torch.equal(orc.decode(codes, upsample_call_frames=64), batch)
    # c = 1, from the definition: rows (2f, 2f + 1) = e[f] * w[:, 0], e[f] * w[:, 1]; taps 2, 3 fall into the trimmed rows
    e = orc.rvq_decode(codes.long())  # B, 512, F
    w = st["upsample.conv.weight"]  # 512, 1, 4
    rows = []
    for f in range(6):
        y = F.conv_transpose1d(e[:, :, f:f + 1], w, None, stride=2, groups=512)  # B, 512, 4
        rows.append(y[:, :, :2])
        assert torch.allclose(y[:, :, 0], e[:, :, f] * w[:, 0, 0]) and torch.allclose(y[:, :, 1], e[:, :, f] * w[:, 0, 1])
    up1 = torch.cat(rows, dim=2)
    ref1 = orc.seanet(orc.transformer(up1.transpose(1, 2)).transpose(1, 2))
    one = orc.decode(codes, upsample_call_frames=1)
    assert torch.allclose(one, ref1, atol=1e-6)
    # the first call has nothing to lose; later calls differ from the batch decode (the reference's defect)
    two = orc.decode(codes, upsample_call_frames=2)
    assert float((two[..., : 2 * 1920] - batch[..., : 2 * 1920]).abs().max()) < 1e-5
    assert float((two[..., 2 * 1920:] - batch[..., 2 * 1920:]).abs().max()) > 1e-3
    assert float((one[..., 1920:] - batch[..., 1920:]).abs().max()) > 1e-3


def _rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


@pytest.mark.parametrize("seed,B,F,code_seed", [(3, 2, 9, 209), (0, 2, 33, 11), (4, 1, 20, 9)])
def test_mimi_oracle_float64_and_float32_agree(seed, B, F, code_seed):
    """``MimiDecodeOracle(dtype=torch.float64)`` against the default: the fp32 oracle's own rounding noise on a signal of RMS
    0.2 - 0.4.  Measured RMS 7.6e-8 .. 8.7e-8 and max-abs 3.4e-7 .. 3.8e-7 (these three cases); asserted with a factor of 4
    head-room.  This is the yardstick of tests/test_mimi_strict_gpu.py: an error of the HIP path is judged by this size."""
    from oracle.mimi_oracle import MimiDecodeOracle
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    st = synthetic_mimi_state(seed=seed)
    codes = torch.randint(0, 2048, (B, 8, F), generator=torch.Generator().manual_seed(code_seed))
    o32, o64 = MimiDecodeOracle(st).decode(codes), MimiDecodeOracle(st, dtype=torch.float64).decode(codes)
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64 and o32.shape == o64.shape == (B, 1, 1920 * F)
    d = (o32.double() - o64).numpy()
    print(f"seed {seed}, {B} x {F} frames: fp32 vs float64 oracle rms {_rms(d):.3e}, max {np.abs(d).max():.3e}, signal rms {_rms(o64.numpy()):.3f}")
    assert _rms(d) <= 4 * 8.7e-8 and float(np.abs(d).max()) <= 4 * 3.8e-7
    assert _rms(d) > 1e-9  # (the switch really changes the arithmetic)
    # every intermediate is float64, not only the result
    inter = MimiDecodeOracle(st, dtype=torch.float64).intermediates(codes[:, :, :2])
    assert all(v.dtype == torch.float64 for v in inter.values())


@pytest.mark.parametrize("name", ["mimi_hf", "mimi_hf_long"])
def test_mimi_float64_oracle_reproduces_hf_goldens(name, golden_dir):
    """The float64 oracle against the third-party vectors (PCM of ``transformers.MimiModel.decode``, computed in fp32).  The
    vectors carry their producer's own fp32 rounding, R = RMS(fp32 oracle - float64 oracle) ~ 8e-8 for the same codes, so that is
    how close a float64 computation can come: asserted RMS <= 4 R (the project's factor for two computations that differ by
    fp32 rounding) and, like the fp32 oracle, < 1e-6.  Measured: mimi_hf fp32 7.48e-8 / float64 8.03e-8 (max-abs 3.58e-7 /
    3.17e-7), mimi_hf_long 7.74e-8 / 8.32e-8 (3.58e-7 / 4.25e-7): the fp32 oracle lands 7 % closer in RMS, because it shares
    rounding steps with the fp32 model that made the vectors -- so 'float64 at least as close as fp32' cannot be asserted
    literally; both distances are the vectors' own noise and are printed."""
    from oracle.mimi_oracle import MimiDecodeOracle
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    g = np.load(golden_dir / f"{name}.npz")
    st = synthetic_mimi_state(seed=int(g["seed"]))
    codes = torch.from_numpy(g["codes"]).long()
    window = int(g["window"]) if "window" in g.files else 250
    o32 = MimiDecodeOracle(st, window=window).decode(codes).numpy()
    o64 = MimiDecodeOracle(st, window=window, dtype=torch.float64).decode(codes).numpy()
    want = g["pcm"].reshape(o32.shape)
    e32, e64, own = _rms(o32 - want), _rms(o64 - want), _rms(o32 - o64)
    print(f"{name}: rms vs the stored PCM: fp32 oracle {e32:.3e}, float64 oracle {e64:.3e}; fp32 vs float64 oracle {own:.3e}; "
          f"max-abs {np.abs(o32 - want).max():.3e} / {np.abs(o64 - want).max():.3e}")
    assert e32 < 1e-6 and e64 < 1e-6
    assert e64 <= 4 * own and float(np.abs(o64 - want).max()) <= 4 * float(np.abs(o32 - o64).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_mimi_oracle_seanet_stages_compose_to_seanet(dtype):
    """``seanet_stages``: same arithmetic as ``seanet`` (its "pcm" is bit-identical), channel-last stage outputs of the shapes the
    engine's buffers have, each stage recomputable from the one before it; ``intermediates`` keeps its keys and gains them."""
    import torch.nn.functional as F

    from oracle.mimi_oracle import MimiDecodeOracle
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    st = synthetic_mimi_state(seed=2)
    orc = MimiDecodeOracle(st, dtype=dtype)
    codes = torch.randint(0, 2048, (2, 8, 3), generator=torch.Generator().manual_seed(4))
    inter = orc.intermediates(codes)
    assert {"rvq", "upsample", "transformer", "pcm"} <= set(inter)
    x = inter["transformer"].transpose(1, 2)  # (B, 512, 2 F)
    stages = orc.seanet_stages(x)
    assert list(stages) == ["conv0", "convtr1", "res1", "convtr2", "res2", "convtr3", "res3", "convtr4", "res4", "pcm"]
    assert torch.equal(stages["pcm"], orc.seanet(x)) and torch.equal(stages["pcm"], orc.decode(codes))
    T, ch = 6, 1024
    assert tuple(stages["conv0"].shape) == (2, T, ch)
    for i, r in enumerate((8, 6, 5, 4), 1):
        T, ch = T * r, ch // 2
        assert tuple(stages[f"convtr{i}"].shape) == tuple(stages[f"res{i}"].shape) == (2, T, ch)
        assert torch.equal(inter[f"res{i}"], stages[f"res{i}"])
        # the block, written out once more from the module's definition: y = x + conv_k1(ELU(conv_k3(ELU(x)))), causal
        li = 3 * i
        xin = stages[f"convtr{i}"].transpose(1, 2)
        w1, b1 = orc.st[f"decoder.layers.{li}.block.1.conv.weight"], orc.st[f"decoder.layers.{li}.block.1.conv.bias"]
        w3, b3 = orc.st[f"decoder.layers.{li}.block.3.conv.weight"], orc.st[f"decoder.layers.{li}.block.3.conv.bias"]
        y = xin + F.conv1d(F.elu(F.conv1d(F.pad(F.elu(xin), (2, 0)), w1, b1)), w3, b3)
        assert torch.equal(y.transpose(1, 2), stages[f"res{i}"])
    assert tuple(stages["pcm"].shape) == (2, 1, 1920 * 3)
    w, b = orc.st["decoder.layers.14.conv.weight"], orc.st["decoder.layers.14.conv.bias"]
    assert torch.equal(F.conv1d(F.pad(F.elu(stages["res4"].transpose(1, 2)), (2, 0)), w, b), stages["pcm"])


def test_mimi_oracle_window_250_is_reached_by_140_frames():
    """The sliding window changes the signal once a stream is longer than 250 positions: 140 frames = 280 positions.  The strict
    GPU test decodes this case (tests/mimi_strict_helpers.window_case); here: its ``window = 250`` oracle differs from
    ``window = 0`` by more than 1e-3 RMS over the last 15 frames (and not at all over the first 125), so that test cannot pass by
    ignoring the window.  (Plain synthetic weights: 7e-5 for every seed tried -- hence the case's louder attention.)"""
    from mimi_strict_helpers import rms, window_case
    from oracle.mimi_oracle import MimiDecodeOracle

    st, codes = window_case()
    w250 = MimiDecodeOracle(st, window=250, dtype=torch.float64).decode(codes)[0, 0].numpy()
    w0 = MimiDecodeOracle(st, window=0, dtype=torch.float64).decode(codes)[0, 0].numpy()
    tail = rms(w250[-15 * 1920:] - w0[-15 * 1920:])
    print(f"window 250 vs 0, 140 frames: rms difference over the last 15 frames {tail:.3e}, over the first 125 {rms(w250[:125 * 1920] - w0[:125 * 1920]):.3e}")
    assert tail > 1e-3 and np.array_equal(w250[: 125 * 1920], w0[: 125 * 1920])


def test_lm_float64_oracle_generates_the_golden_ids(golden_dir):
    """``LMOracle(dtype=torch.float64)``, free-running on the tiny golden prompts: the same ids as the fp32 oracle and the golden
    grids (whose gaps, >= 2e-5, are far above fp32 noise), with every cache and logit in float64.  That the fp32 default is
    bit-identical to before the switch existed is what ``test_lm_oracle_reproduces_goldens`` pins."""
    from oracle.lm_oracle import LMOracle, OracleLMConfig

    g = np.load(golden_dir / "lm_tiny.npz")
    cfg, state, o32, _ = _lm(str(g["config_name"]), int(g["seed"]))
    o64 = LMOracle(OracleLMConfig.from_dict(cfg.__dict__), state, dtype=torch.float64)
    n, frames = len(g["texts"]), int(g["frames"])
    prompts = [torch.from_numpy(g[f"prompt_{b}"]) for b in range(n)]
    l32, l64 = o32.generate(prompts, max_frames=frames, stop_on_eos=False), o64.generate(prompts, max_frames=frames, stop_on_eos=False)
    for b in range(n):
        assert l64[b].grid == l32[b].grid and np.array_equal(l64[b].as_tensor().numpy(), g[f"grid_{b}"])
        assert l64[b].min_margin == pytest.approx(l32[b].min_margin, rel=0.05, abs=2e-6)
    assert all(t.dtype == torch.float64 for t in o64.K + o64.V) and all(t.dtype == torch.float32 for t in o32.K + o32.V)
    tok, cb = o64.teacher_forced(torch.cat([prompts[0].long(), l64[0].as_tensor()], dim=1))
    assert tok.dtype == cb.dtype == o64.tf_K.dtype == o64.tf_V.dtype == torch.float64
    assert o64.rope.dtype == torch.float64 and torch.equal(o64.rope.float(), o32.rope)  # the table is an input: the fp32 oracle's values, upcast
    assert torch.equal(o64.E_text.float(), o32.E_text)


@pytest.mark.parametrize("case", ["CASE2", "CASE4"])
def test_lm_strict_bound_rejects_two_piece_activations(case):
    """The yardstick of tests/test_lm_strict_gpu.py has teeth.  A third CPU computation differs from the fp32 oracle only in that
    every weight GEMM's activation operand is cut to two bf16 pieces (2^-16-grade, the kind of error a dropped term of the bf16
    split gives); at the shapes of that suite's cases 2 and 4 it must VIOLATE  RMS(x - float64) <= 4 R_ref  at every layer: for K
    and for V, for every slot, for its prompt rows and its decode rows apart -- every unit the GPU test judges.
    Measured rms / R_ref of the control (bound 4), smallest .. largest over those units: case 2 (tiny) layer 0 5.9 .. 9.1, layer 1
    7.1 .. 10.4; case 4 (70m) layer 0 7.6 .. 8.1, layers 1 - 9 6.7 .. 10.2.  (Its max err / E_ref is 2.0 .. 12.7: one element's
    luck, which is why the control is judged by RMS.)  No layer lets it through, so the per-segment RMS is not too loose."""
    import lm_strict_helpers as H

    name, Ts, n = getattr(H, case)
    cfg, _, o32, o64, o2 = H.make_oracles(name, 3, block_cls=H._two_piece_block())
    gen = torch.Generator().manual_seed(7)
    lo_hi = {}
    for b, T in enumerate(Ts):
        grid = H.random_grid(cfg, T + n, gen)
        r = H.teacher_refs(o32, o64, grid)
        (k2, v2, _, _), _, _ = H.teacher_kv(o2, grid)
        # the fp32 oracle itself passes its own yardstick trivially (ratio 1); the control must fail it everywhere
        for which, got, r32, r64 in (("K", k2, r.K32, r.K64), ("V", v2, r.V32, r.V64)):
            fails, worst = H.strict_kv_report(got, r32, r64, T, b, which)
            units = {(f.layer, f.segment) for f in fails if f.rms_ratio > H.FACTOR}
            assert units == {(l, s) for l in range(cfg.n_layer) for s in ("prompt", "decode")}, \
                f"{name} slot {b} {which}: the two-piece control passes the RMS bound at (layer, segment) " \
                f"{sorted({(l, s) for l in range(cfg.n_layer) for s in ('prompt', 'decode')} - units)}"
            for f in fails:
                a = lo_hi.setdefault(f.layer, [f.rms_ratio, f.rms_ratio])
                a[0], a[1] = min(a[0], f.rms_ratio), max(a[1], f.rms_ratio)
            assert not H.strict_kv_report(r32, r32, r64, T, b, which)[0]
    print(f"{name}: two-piece control, rms / R_ref per layer (min .. max over slots, K / V, segments): " +
          ", ".join(f"{l}: {a[0]:.1f} .. {a[1]:.1f}" for l, a in sorted(lo_hi.items())))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lm_oracle_kv_bf16_exposes_rounded_and_unrounded(dtype):
    """``teacher_forced`` of a ``kv_bf16`` oracle: ``tf_K`` / ``tf_V`` (what the cache holds) are the bf16 rounding of ``tf_K_raw`` /
    ``tf_V_raw``, [n_layer, S, n_kv, 64] in the oracle's dtype; without ``kv_bf16`` the two are the same values."""
    import lm_strict_helpers as H
    from oracle.lm_oracle import LMOracle, OracleLMConfig

    cfg, state, _, _ = _lm("tiny", 3)
    grid = torch.from_numpy(H.random_grid(cfg, 21, torch.Generator().manual_seed(1))).long()
    ocfg = OracleLMConfig.from_dict(cfg.__dict__)
    orc = LMOracle(ocfg, state, kv_bf16=True, dtype=dtype)
    orc.teacher_forced(grid)
    for cached, raw in ((orc.tf_K, orc.tf_K_raw), (orc.tf_V, orc.tf_V_raw)):
        assert cached.dtype == raw.dtype == dtype and tuple(cached.shape) == tuple(raw.shape) == (cfg.n_layer, 21, cfg.n_local_heads, 64)
        assert torch.equal(cached, raw.bfloat16().to(dtype)) and not torch.equal(cached, raw)
    assert torch.equal(orc.K[1][0], orc.tf_K[1]) and torch.equal(orc.V[0][0], orc.tf_V[0])
    plain = LMOracle(ocfg, state, dtype=dtype)
    plain.teacher_forced(grid)
    assert torch.equal(plain.tf_K, plain.tf_K_raw) and torch.equal(plain.tf_V, plain.tf_V_raw)
    assert torch.equal(plain.tf_K_raw[0], orc.tf_K_raw[0])  # layer 0 depends on no cached value


def test_lm_strict_helper_names_the_wrong_element():
    """``strict_kv_report`` on synthetic arrays: 1e-5 added to one element of one layer's K is reported as exactly that layer, slot,
    position, kv head and dimension, on the prompt side and on the decode side; the clean copy passes."""
    import lm_strict_helpers as H

    rng = np.random.default_rng(0)
    n_layer, T, n, kv = 3, 19, 5, 2
    ref64 = rng.standard_normal((n_layer, T + n, kv, 64))
    ref32 = ref64 + rng.standard_normal(ref64.shape) * 3e-7   # the fp32 oracle's own noise
    clean = (ref64 + rng.standard_normal(ref64.shape) * 3e-7).astype(np.float32)
    assert not H.strict_kv_report(clean, ref32, ref64, T, 4, "K")[0]
    for pos, seg in ((7, "prompt"), (T + 2, "decode")):
        bad = clean.copy()
        bad[1, pos, 1, 33] += 1e-5
        fails, worst = H.strict_kv_report(bad, ref32, ref64, T, 4, "K")
        assert len(fails) == 1
        f = fails[0]
        assert (f.which, f.layer, f.slot, f.segment, f.pos, f.head, f.dim) == ("K", 1, 4, seg, pos, 1, 33)
        assert f.max_ratio > H.FACTOR and worst[seg][0] == f.max_ratio
        assert f"K layer 1 slot 4 {seg} rows" in f.msg and f"position {pos} " in f.msg and "kv head 1, dim 33" in f.msg
    # the half-ulp of the bf16 cache test (8 significant bits: ulp(1.0) = 2^-7), at and between powers of two
    assert H.half_ulp_bf16(np.array([1.0, 1.5, 2.0, -0.75, 0.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0]
    x = np.array([0.3, -1.7, 100.0])
    assert (np.abs(torch.tensor(x).bfloat16().double().numpy() - x) <= H.half_ulp_bf16(x)).all()


@pytest.mark.parametrize("case", ["CASE2", "CASE150"])
def test_lm_strict_bound_rejects_two_piece_activations_on_the_fp8_model(case):
    """The same control as above on ``packing.fp8_reference_state``, the model an fp8 engine computes (dequantised e4m3 Linears, an
    explicit head): both oracles and the two-piece control run on it, at the shapes of tests/test_lm_strict_gpu.py's tiny fp8 case
    and of its 150m cases (12 / 4 heads, dim 768).  The control must violate the RMS bound at every layer and segment, for K and V
    and every slot.  Measured rms / R_ref of the control (bound 4), smallest .. largest over those units: tiny 6.4 .. 9.9; 150m 5.7 .. 18.3."""
    import lm_strict_helpers as H

    name, Ts, n = getattr(H, case)
    cfg, _, o32, o64, o2 = H.make_oracles(name, 3, block_cls=H._two_piece_block(), fp8=True)
    assert not o32.cfg.tie_word_embeddings and o64.cfg.tie_word_embeddings is False  # (the reference state's explicit head)
    gen = torch.Generator().manual_seed(7)
    lo, hi = np.inf, 0.0
    every = {(l, s) for l in range(cfg.n_layer) for s in ("prompt", "decode")}
    for b, T in enumerate(Ts):
        grid = H.random_grid(cfg, T + n, gen)
        r = H.teacher_refs(o32, o64, grid)
        (k2, v2, _, _), _, _ = H.teacher_kv(o2, grid)
        for which, got, r32, r64 in (("K", k2, r.K32, r.K64), ("V", v2, r.V32, r.V64)):
            fails, _ = H.strict_kv_report(got, r32, r64, T, b, which)
            units = {(f.layer, f.segment) for f in fails if f.rms_ratio > H.FACTOR}
            assert units == every, f"{name} fp8 slot {b} {which}: the two-piece control passes the RMS bound at {sorted(every - units)}"
            lo, hi = min([lo] + [f.rms_ratio for f in fails]), max([hi] + [f.rms_ratio for f in fails])
            assert not H.strict_kv_report(r32, r32, r64, T, b, which)[0]
    print(f"{name} on the fp8 reference state: two-piece control, rms / R_ref over every unit: {lo:.1f} .. {hi:.1f}")


def _depth_control(name, fp8, n_layer, Ts=None, seed=3):
    """Two-piece control on the DEPTH layers only (the slow stack is the fp32 oracle's): per slot of ``Ts`` a random grid of T +
    DEPTH_FRAMES columns, the depth rows of its frames judged by ``strict_depth_report`` -> (config, {(which, layer): [rms ratio per
    slot]}, {(which, layer): [max ratio per slot]})."""
    import lm_strict_helpers as H

    cfg, _, o32, o64, o2 = H.make_oracles(name, seed, fast_block_cls=H._two_piece_block(), fp8=fp8, n_layer=n_layer)
    gen = torch.Generator().manual_seed(7)
    rr, mm = {}, {}
    for b, T in enumerate(Ts or H.DEPTH_TS[name]):
        grid = H.random_grid(cfg, T + H.DEPTH_FRAMES, gen)
        r = H.teacher_refs(o32, o64, grid)
        H.teacher_kv(o2, grid)
        k2, v2 = H.depth_kv(o2)
        assert np.array_equal(o2.tf_K.double().numpy(), r.K32)  # the control's slow stack is untouched
        for which, got, r32, r64 in (("K", k2, r.fK32, r.fK64), ("V", v2, r.fV32, r.fV64)):
            got, r32, r64 = (H.depth_refs(a, T, H.DEPTH_FRAMES) for a in (got, r32, r64))
            fails, _ = H.strict_depth_report(got, r32, r64, b, which)
            assert not H.strict_depth_report(r32, r32, r64, b, which)[0]  # the fp32 oracle passes its own yardstick (ratio 1)
            seen = {f.layer: f for f in fails}
            for l in range(cfg.n_fast_layer):
                # a unit that passed has no Failure: measure it again with a factor nothing passes
                f = seen.get(l) or [x for x in H.strict_depth_report(got, r32, r64, b, which, factor=0.0)[0] if x.layer == l][0]
                rr.setdefault((which, l), []).append(f.rms_ratio)
                mm.setdefault((which, l), []).append(f.max_ratio)
    return cfg, rr, mm


@pytest.mark.parametrize("name,fp8,n_layer", [("tiny", False, None), ("tiny_nodup", True, None), ("smoltts_byte_70m", False, 1),
                                              ("smoltts_byte_150m", True, 1)])
def test_lm_depth_bound_rejects_two_piece_activations(name, fp8, n_layer):
    """The yardstick of tests/test_lm_depth_strict_gpu.py has teeth: a CPU computation whose depth-layer GEMMs see their activation
    cut to two bf16 pieces (2^-16-grade; the slow stack stays the fp32 oracle's) must VIOLATE  RMS(x - float64) <= 4 R_ref  at every
    depth layer, for K and for V, for every slot, at the configs and prompt lengths of that file, pooled as it pools (4 frames x
    n_fast steps).  Measured rms / R_ref of the control (bound 4), smallest .. largest over the (slot, depth layer, K / V) units: tiny
    5.3 .. 7.5, tiny_nodup fp8 5.4 .. 6.7, 70m with one slow layer 5.6 .. 6.8, 150m fp8 with one slow layer 6.1 .. 6.5.  (Its max err /
    E_ref is 2.6 .. 9.8: the max criterion rests on one element of 8-row frames and need not reject the control; it is not asserted.)"""
    cfg, rr, mm = _depth_control(name, fp8, n_layer)
    assert set(rr) == {(w, l) for w in "KV" for l in range(cfg.n_fast_layer)}
    allr = [x for v in rr.values() for x in v]
    print(f"{name}{' fp8' if fp8 else ''}{' one slow layer' if n_layer else ''}: depth two-piece control, rms / R_ref {min(allr):.1f} .. "
          f"{max(allr):.1f}; max err / E_ref {min(x for v in mm.values() for x in v):.1f} .. {max(x for v in mm.values() for x in v):.1f}")
    for (which, l), v in sorted(rr.items()):
        assert min(v) > 4.0, f"{name}: the depth two-piece control passes the RMS bound at depth layer {l} {which} (slot {int(np.argmin(v))}: {min(v):.2f})"


@pytest.mark.parametrize("name,fp8", [("smoltts_byte_70m", False), ("smoltts_byte_150m", True)])
def test_lm_depth_control_is_drowned_by_the_full_slow_stack(name, fp8):
    """Why tests/test_lm_depth_strict_gpu.py runs its real-size cases with ONE slow layer.  The depth rows inherit the slow stack's
    fp32 noise through the hidden state they start from; R_ref contains it, the depth chain's own error does not grow with it.
    With the full 10-layer stack the depth two-piece control's rms / R_ref is only 3.7 .. 5.3 at 70m (mean 4.3) and 3.9 .. 4.8 at 150m
    fp8 (mean 4.4) -- part of it under the bound of 4, so a 2^-16-grade depth kernel could pass -- against 5.9 .. 6.4 (mean 6.2) and
    5.7 .. 6.4 (mean 6.1) with one slow layer (``dataclasses.replace(cfg, n_layer=1)``: the
    depth transformer keeps its true dimensions).  Asserted: only that the full stack's ratio is the smaller one (mean over the
    units, and the smallest unit); the one-layer ratio's own bar is the test above."""
    Ts = (3, 5, 7)
    _, full, _ = _depth_control(name, fp8, None, Ts)
    _, one, _ = _depth_control(name, fp8, 1, Ts)
    f, o = [x for v in full.values() for x in v], [x for v in one.values() for x in v]
    print(f"{name}{' fp8' if fp8 else ''}: depth two-piece control rms / R_ref, full stack {min(f):.1f} .. {max(f):.1f} (mean {np.mean(f):.1f}), "
          f"one slow layer {min(o):.1f} .. {max(o):.1f} (mean {np.mean(o):.1f})")
    assert np.mean(f) < np.mean(o) and min(f) < min(o)


def test_lm_depth_helper_names_the_wrong_element():
    """``strict_depth_report`` on synthetic arrays: 1e-5 added to one element of one depth layer's V is reported as exactly that layer,
    slot, frame, step, kv head and dimension, with the value got and the float64 value; the clean copy passes.  ``depth_refs`` takes
    frame f from position T - 1 + f and refuses a grid without the column that frame's depth pass reads."""
    import lm_strict_helpers as H

    rng = np.random.default_rng(1)
    n_layer, frames, n_fast, kv = 4, 4, 8, 3
    ref64 = rng.standard_normal((n_layer, frames, n_fast, kv, 64))
    ref32 = ref64 + rng.standard_normal(ref64.shape) * 3e-7
    clean = (ref64 + rng.standard_normal(ref64.shape) * 3e-7).astype(np.float32)
    fails, (we, wr) = H.strict_depth_report(clean, ref32, ref64, 2, "V")
    assert not fails and 0.0 < wr < 2.0 and we < H.FACTOR
    bad = clean.copy()
    bad[2, 3, 5, 1, 17] += 1e-5
    fails, (we, wr) = H.strict_depth_report(bad, ref32, ref64, 2, "V")
    assert len(fails) == 1
    f = fails[0]
    assert (f.which, f.layer, f.slot, f.frame, f.step, f.head, f.dim) == ("V", 2, 2, 3, 5, 1, 17) and f.max_ratio > H.FACTOR and we == f.max_ratio
    assert "depth V layer 2 slot 2" in f.msg and "frame 3, step 5, kv head 1, dim 17" in f.msg
    assert f"got {bad[2, 3, 5, 1, 17]:.9g}, float64 {ref64[2, 3, 5, 1, 17]:.9g}" in f.msg
    with pytest.raises(AssertionError):
        H.strict_depth_report(clean, ref64, ref64, 2, "V")  # e_ref == 0: a reference without noise of its own judges nothing
    S, T = 9, 6
    tf = np.arange(n_layer * S, dtype=np.float64).reshape(n_layer, S, 1, 1, 1) * np.ones((1, 1, n_fast, kv, 64))
    assert H.depth_refs(tf, T, 3)[1, :, 0, 0, 0].tolist() == [S + 5.0, S + 6.0, S + 7.0]
    with pytest.raises(AssertionError):
        H.depth_refs(tf, T, 4)  # frame 3's depth pass reads column 9 of a 9-column grid: the zero-padded one
    cache = rng.standard_normal((n_layer, 5, kv, n_fast, 64)).astype(np.float32)
    assert H.slot_depth_rows(cache, 3).shape == (n_layer, n_fast, kv, 64) and H.slot_depth_rows(cache, 3)[1, 6, 2, 9] == cache[1, 3, 2, 6, 9]


@pytest.mark.parametrize("name,dtype", [("tiny", torch.float32), ("tiny_nodup", torch.float32), ("tiny_proj", torch.float64)])
def test_lm_oracle_depth_rows_leave_the_logits_unchanged(name, dtype):
    """``teacher_forced`` leaves ``tf_fK`` / ``tf_fV`` [n_fast_layer, S, n_fast, fast_n_kv, 64] in the oracle's dtype, K after RoPE, and
    returns bit for bit the logits of the depth pass written out here without them (the loop as it stood before the rows were
    kept).  Position s's rows are those of the cached depth pass (``fast_decode``'s arithmetic) over hidden[s] and the codes of
    column s + 1: checked against that loop, step by step, to fp32 noise."""
    import lm_strict_helpers as H
    from oracle.lm_oracle import LMOracle, OracleLMConfig, _gqa_attend, rms_norm

    cfg, state, _, _ = _lm(name, 3)
    orc = LMOracle(OracleLMConfig.from_dict(cfg.__dict__), state, dtype=dtype)
    c = orc.cfg
    S, n = 11, c.max_fast_seqlen
    grid = torch.from_numpy(H.random_grid(cfg, S, torch.Generator().manual_seed(2))).long()
    tok, cb = orc.teacher_forced(grid)
    fK, fV = orc.tf_fK, orc.tf_fV
    assert fK.dtype == fV.dtype == dtype and tuple(fK.shape) == tuple(fV.shape) == (c.n_fast_layer, S, n, c.fast_n_local_heads, 64)
    # the depth pass without the kept rows, from the slow stack's hidden state
    x = orc.embed(grid.T.contiguous())[None]
    cs = orc.rope[:S][None, :, None]
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None]
    for L in orc.layers:
        q, k, v = L.qkv(x, cs)
        x = L.mlp(x + L.out(_gqa_attend(q, k, v, mask)))
    assert torch.equal(orc.slow_head(x[0]), tok)
    nxt = torch.zeros(S, grid.shape[0] - 2, dtype=torch.int64)
    nxt[:-1] = grid[1:-1, 1:].T
    off = torch.arange(0, c.codebook_size * (c.num_codebooks - 1), c.codebook_size)
    if not c.duplicate_code_0:
        off = off[1:]
    fe = orc.E_fast[nxt + off]
    fe[-1] = orc.E_fast[torch.zeros(fe.shape[1], dtype=torch.int64)]
    hid = x[0] if orc.proj_w is None else x[0] @ orc.proj_w.T + orc.proj_b
    h = torch.cat([hid[:, None], fe], dim=1)
    fmask = torch.tril(torch.ones(n, n, dtype=torch.bool))[None, None]
    for li, L in enumerate(orc.fast_layers):
        q, k, v = L.qkv(h, orc.fast_rope[:n][None, :, None])
        assert torch.equal(k, fK[li]) and torch.equal(v, fV[li])
        h = L.mlp(h + L.out(_gqa_attend(q, k, v, fmask)))
    want = torch.einsum("snd,nkd->snk", rms_norm(h, orc.fast_norm_w, c.norm_eps), orc.fast_out)
    want[-1] = 0
    assert torch.equal(want, cb)
    # the cached, step-by-step depth pass of position s = 4 (the decode loop's form) gives the same rows
    s = 4
    xin = hid[s][None]
    Kc = [torch.zeros(1, n, c.fast_n_local_heads, 64, dtype=dtype) for _ in orc.fast_layers]
    Vc = [torch.zeros_like(k) for k in Kc]
    for i in range(n):
        hh = xin[:, None]
        for li, L in enumerate(orc.fast_layers):
            q, k, v = L.qkv(hh, orc.fast_rope[i][None, None, None])
            Kc[li][:, i], Vc[li][:, i] = k[:, 0], v[:, 0]
            hh = L.mlp(hh + L.out(_gqa_attend(q, Kc[li][:, : i + 1], Vc[li][:, : i + 1], None)))
        if i + 1 < n:
            xin = fe[s, i][None]
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    for li in range(c.n_fast_layer):
        assert float((Kc[li][0] - fK[li, s]).abs().max()) < tol and float((Vc[li][0] - fV[li, s]).abs().max()) < tol
