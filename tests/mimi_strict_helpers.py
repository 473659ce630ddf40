"""Shared pieces of tests/test_mimi_strict_gpu.py, tests/test_seanet_fused_gpu.py and the CPU checks of their premises
(tests/test_oracle_cpu.py): the test states, the error measures and the messages that name a wrong sample's place."""
import numpy as np
import torch

SAMPLES_PER_FRAME = 1920
WINDOW_FRAMES = 140  # 280 transformer positions > window = 250


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def window_case():
    """(state, codes [1, 8, 140]) of the sliding-window case.  With the plain synthetic weights the attention branch is quiet
    (layer scale 0.2, near-uniform weights over 280 keys): ``window = 250`` moves the last frames by only 7e-5 RMS, which a
    decode that ignored the window could hide in.  Here the attention layer scale is 5 x and q_proj 8 x the synthetic ones
    (sharper, louder attention): the window then moves the last 15 frames by 2.2e-3 RMS (tests/test_oracle_cpu.py asserts
    > 1e-3) while the oracle's own fp32 noise stays at 9e-8."""
    from smoltts_amd.codec.synthetic import synthetic_mimi_state

    st = synthetic_mimi_state(seed=4)
    for k in list(st):
        if k.startswith("decoder_transformer.") and k.endswith("self_attn_layer_scale.scale"):
            st[k] = st[k] * 5.0
        if k.startswith("decoder_transformer.") and k.endswith("self_attn.q_proj.weight"):
            st[k] = st[k] * 8.0
    codes = torch.randint(0, 2048, (1, 8, WINDOW_FRAMES), generator=torch.Generator().manual_seed(140))
    return st, codes


def where_sample(sample: int) -> str:
    """Where a PCM sample of a slot comes from: its frame, its input row of the last SEANet stage (4 samples per row) and that
    row's place in the stage's 63-row tile stride and 32-row halves, in the resnet block's 32-row tiles one stage earlier."""
    row = sample // 4
    return (f"sample {sample} = frame {sample // SAMPLES_PER_FRAME}, sample {sample % SAMPLES_PER_FRAME} of it; last-stage row {row}: "
            f"row mod 63 = {row % 63}, row mod 32 = {row % 32} (tests/test_seanet_fused_gpu.py holds that stage)")


def strict_report(pcm: np.ndarray, ref32: np.ndarray, ref64: np.ndarray, factor: float = 4.0):
    """Per slot: E_ref = max|fp32 oracle - float64 oracle| and R_ref (its RMS), the reference's own noise; the HIP result is held
    to ``factor`` times each against the float64 oracle.  Returns (failure messages, worst max ratio, worst rms ratio)."""
    assert pcm.shape == ref32.shape == ref64.shape and ref64.dtype == np.float64
    msgs, worst_e, worst_r = [], 0.0, 0.0
    for b in range(pcm.shape[0]):
        own = ref32[b].astype(np.float64) - ref64[b]
        d = pcm[b].astype(np.float64) - ref64[b]
        e_ref, r_ref = float(np.abs(own).max()), rms(own)
        assert np.isfinite(pcm[b]).all() and e_ref > 0.0, f"slot {b}"
        i = int(np.abs(d).argmax())
        e, r = float(np.abs(d[i])), rms(d)
        worst_e, worst_r = max(worst_e, e / e_ref), max(worst_r, r / r_ref)
        if e > factor * e_ref or r > factor * r_ref:
            msgs.append(f"slot {b}: max err {e:.3e} = {e / e_ref:.2f} x E_ref ({e_ref:.3e}), rms {r:.3e} = {r / r_ref:.2f} x R_ref "
                        f"({r_ref:.3e}); worst at {where_sample(i)}")
    return msgs, worst_e, worst_r
