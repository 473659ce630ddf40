"""Shared pieces of tests/test_lm_strict_gpu.py, tests/test_lm_depth_strict_gpu.py and the CPU checks of their premises
(tests/test_oracle_cpu.py): the prompt grids, the two teacher-forced oracles, the per-layer error measure of the slow
transformer's K/V rows and of the depth transformer's, and the top-2 gap check, with messages that name a wrong element's place."""
import dataclasses
from collections import namedtuple

import numpy as np
import torch

FACTOR = 4.0  # the project's rule for two computations that differ by fp32 rounding (tests/test_gemm_b3_gpu.py)

# the shapes of tests/test_lm_strict_gpu.py that the CPU control repeats: (config, prompt lengths, decoded frames)
CASE2 = ("tiny", (1, 2, 17, 33, 64), 8)
CASE4 = ("smoltts_byte_70m", (3, 60, 130), 4)

Failure = namedtuple("Failure", "which layer slot segment pos head dim max_ratio rms_ratio msg")
DepthFailure = namedtuple("DepthFailure", "which layer slot frame step head dim max_ratio rms_ratio msg")
Refs = namedtuple("Refs", "K32 V32 K64 V64 K64_raw V64_raw K32_raw V32_raw tok32 cb32 tok64 cb64 fK32 fV32 fK64 fV64")

# the shapes of tests/test_lm_strict_gpu.py's 150m cases and of tests/test_lm_depth_strict_gpu.py that the CPU controls repeat
CASE150 = ("smoltts_byte_150m", (3, 40, 90), 4)
DEPTH_FRAMES = 4  # frames whose depth rows are read: frame 0 behind the prefill, then three decode frames
DEPTH_TS = {"tiny": (1, 2, 5, 9, 17), "tiny_nodup": (2, 5, 9), "tiny_proj": (2, 5, 9), "smoltts_byte_70m": tuple(3 + b % 5 for b in range(20)),
            "smoltts_byte_150m": (1, 3, 5)}


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def random_grid(cfg, T: int, gen: torch.Generator) -> np.ndarray:
    """A (1 + n_fast, T) prompt grid of exactly T columns: any text id, any codes, code 0 (row 1) non-zero so that the
    reference's embed mask (modeling :219) keeps the code sum of every column."""
    n_fast = cfg.num_codebooks - (0 if cfg.duplicate_code_0 else 1)
    g = torch.randint(0, cfg.codebook_size, (1 + n_fast, T), generator=gen)
    g[0] = torch.randint(0, cfg.vocab_size, (T,), generator=gen)
    g[1] = torch.randint(1, cfg.codebook_size, (T,), generator=gen)
    return g.numpy().astype(np.int32)


def make_oracles(cfgname: str, seed: int, kv_bf16: bool = False, block_cls=None, fp8: bool = False, n_layer=None, fast_block_cls=None):
    """(config, state, fp32 oracle, float64 oracle[, a third fp32 oracle whose slow blocks are ``block_cls`` and whose depth blocks
    are ``fast_block_cls``]).  ``n_layer``: the named config with that many slow layers (``dataclasses.replace``; the depth
    transformer keeps its dimensions).  ``fp8``: the oracles run on ``packing.fp8_reference_state(cfg, state)``, the model an engine
    with ``weight_format="fp8"`` computes; the config and state returned are still the ones that engine is built from."""
    from oracle.lm_oracle import LMOracle, OracleLMConfig
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config(cfgname)
    if n_layer is not None:
        cfg = dataclasses.replace(cfg, n_layer=n_layer)
    state = synthetic_lm_state(cfg, seed=seed)
    rcfg, rstate = cfg, state
    if fp8:
        from smoltts_amd.packing import fp8_reference_state

        rcfg, rstate = fp8_reference_state(cfg, state)
    ocfg = OracleLMConfig.from_dict(rcfg.__dict__)
    out = [cfg, state, LMOracle(ocfg, rstate, kv_bf16=kv_bf16), LMOracle(ocfg, rstate, kv_bf16=kv_bf16, dtype=torch.float64)]
    if block_cls is not None or fast_block_cls is not None:
        third = LMOracle(ocfg, rstate, kv_bf16=kv_bf16)
        for layers, cls in ((third.layers, block_cls), (third.fast_layers, fast_block_cls)):
            for L in layers:
                if cls is not None:
                    L.__class__ = cls
        out.append(third)
    return out


def two_pieces(x: torch.Tensor) -> torch.Tensor:
    """x cut to two bf16 pieces (16 significant bits): what a bf16 split that lost its third piece, and with it the cross terms
    of that piece, leaves of an activation."""
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


def _two_piece_block():
    from oracle.lm_oracle import _Block

    class TwoPieceBlock(_Block):
        """The fp32 oracle's block with the activation operand of every weight GEMM cut to two bf16 pieces."""

        def mm(self, x, w):
            return two_pieces(x) @ w.T

    return TwoPieceBlock


def teacher_kv(orc, grid):
    """Teacher-forced pass of one oracle over a (9, S) grid -> (K, V, K_raw, V_raw) float64 numpy [n_layer, S, n_kv, 64] (exact
    upcasts of the oracle's own values) and its (token logits, codebook logits)."""
    tok, cb = orc.teacher_forced(torch.as_tensor(np.asarray(grid)).long())
    kv = [t.double().numpy().copy() for t in (orc.tf_K, orc.tf_V, orc.tf_K_raw, orc.tf_V_raw)]
    return kv, tok.double().numpy(), cb.double().numpy()


def depth_kv(orc):
    """The depth K / V rows of an oracle's last teacher-forced pass -> float64 numpy [n_fast_layer, S, n_fast, fast_n_kv, 64] each
    (exact upcasts of the oracle's own values)."""
    return orc.tf_fK.double().numpy().copy(), orc.tf_fV.double().numpy().copy()


def teacher_refs(o32, o64, grid) -> Refs:
    (k32, v32, k32r, v32r), t32, c32 = teacher_kv(o32, grid)
    (k64, v64, k64r, v64r), t64, c64 = teacher_kv(o64, grid)
    return Refs(k32, v32, k64, v64, k64r, v64r, k32r, v32r, t32, c32, t64, c64, *depth_kv(o32), *depth_kv(o64))


def slot_rows(cache: np.ndarray, slot: int, S: int) -> np.ndarray:
    """The session's cache [n_layer, B, n_kv, max_seq, 64] -> the oracle's layout [n_layer, S, n_kv, 64] of one slot."""
    return np.ascontiguousarray(np.transpose(cache[:, slot, :, :S], (0, 2, 1, 3)))


def strict_kv_report(got: np.ndarray, ref32: np.ndarray, ref64: np.ndarray, T: int, slot: int, which: str, factor: float = FACTOR):
    """One slot's K (or V) rows [n_layer, S, n_kv, 64]: positions [0, T) are its prompt rows, [T, S) its decode rows.  Per layer
    and per segment: E_ref = max|fp32 oracle - float64 oracle| and R_ref (its RMS), the reference's own noise; ``got`` is held to
    ``factor`` times each against the float64 oracle.  Returns (failures, {segment: (worst max ratio, worst rms ratio)})."""
    assert got.shape == ref32.shape == ref64.shape and ref64.dtype == np.float64, (got.shape, ref32.shape, ref64.shape)
    fails, worst = [], {}
    S = got.shape[1]
    for seg, lo, hi in (("prompt", 0, T), ("decode", T, S)):
        if hi <= lo:
            continue
        we = wr = 0.0
        for l in range(got.shape[0]):
            own = ref32[l, lo:hi].astype(np.float64) - ref64[l, lo:hi]
            d = got[l, lo:hi].astype(np.float64) - ref64[l, lo:hi]
            e_ref, r_ref = float(np.abs(own).max()), rms(own)
            assert np.isfinite(got[l, lo:hi]).all() and e_ref > 0.0, f"{which} layer {l} slot {slot} {seg} rows"
            p, h, i = np.unravel_index(int(np.abs(d).argmax()), d.shape)
            e, r = float(np.abs(d[p, h, i])), rms(d)
            we, wr = max(we, e / e_ref), max(wr, r / r_ref)
            if e > factor * e_ref or r > factor * r_ref:
                msg = (f"{which} layer {l} slot {slot} {seg} rows: max err {e:.3e} = {e / e_ref:.2f} x E_ref ({e_ref:.3e}), rms {r:.3e} = "
                       f"{r / r_ref:.2f} x R_ref ({r_ref:.3e}); worst at position {lo + p} (row {p} of {hi - lo} {seg} rows), kv head {h}, dim {i}: "
                       f"got {got[l, lo + p, h, i]:.9g}, float64 {ref64[l, lo + p, h, i]:.9g}")
                fails.append(Failure(which, l, slot, seg, lo + int(p), int(h), int(i), e / e_ref, r / r_ref, msg))
        worst[seg] = (we, wr)
    return fails, worst


def slot_depth_rows(cache: np.ndarray, slot: int) -> np.ndarray:
    """The session's depth cache [n_fast_layer, B, fast_n_kv, n_fast, 64] -> the oracle's layout of one position
    [n_fast_layer, n_fast, fast_n_kv, 64] of one slot."""
    return np.ascontiguousarray(np.transpose(cache[:, slot], (0, 2, 1, 3)))


def depth_refs(ref: np.ndarray, T: int, frames: int) -> np.ndarray:
    """Teacher-forced depth rows [n_fast_layer, S, n_fast, fast_n_kv, 64] of a grid of T prompt columns + ``frames`` frames -> the rows
    of frames 0 .. frames - 1: frame f is picked at position T - 1 + f and its depth pass sees the codes of column T + f, so the grid
    must hold that column (S >= T + frames); the last position's pass sees the zero-padded column and is never a frame's."""
    assert ref.shape[1] >= T + frames, (ref.shape, T, frames)
    return ref[:, T - 1: T - 1 + frames]


def strict_depth_report(got: np.ndarray, ref32: np.ndarray, ref64: np.ndarray, slot: int, which: str, factor: float = FACTOR):
    """One slot's depth K (or V) rows [n_fast_layer, frames, n_fast, fast_n_kv, 64] (``frames`` = the frames read).  Per depth layer,
    pooled over the frames and the n_fast steps: E_ref = max|fp32 oracle - float64 oracle| and R_ref (its RMS), the reference's own
    noise; ``got`` is held to ``factor`` times each against the float64 oracle.  Returns (failures, (worst max ratio, worst rms
    ratio))."""
    assert got.shape == ref32.shape == ref64.shape and ref64.dtype == np.float64, (got.shape, ref32.shape, ref64.shape)
    fails, we, wr = [], 0.0, 0.0
    for l in range(got.shape[0]):
        own = ref32[l].astype(np.float64) - ref64[l]
        d = got[l].astype(np.float64) - ref64[l]
        e_ref, r_ref = float(np.abs(own).max()), rms(own)
        assert np.isfinite(got[l]).all() and e_ref > 0.0, f"depth {which} layer {l} slot {slot}"
        f, s, h, i = np.unravel_index(int(np.abs(d).argmax()), d.shape)
        e, r = float(np.abs(d[f, s, h, i])), rms(d)
        we, wr = max(we, e / e_ref), max(wr, r / r_ref)
        if e > factor * e_ref or r > factor * r_ref:
            msg = (f"depth {which} layer {l} slot {slot}: max err {e:.3e} = {e / e_ref:.2f} x E_ref ({e_ref:.3e}), rms {r:.3e} = "
                   f"{r / r_ref:.2f} x R_ref ({r_ref:.3e}) over {d.shape[0]} frames x {d.shape[1]} steps; worst at frame {f}, step {s}, "
                   f"kv head {h}, dim {i}: got {got[l, f, s, h, i]:.9g}, float64 {ref64[l, f, s, h, i]:.9g}")
            fails.append(DepthFailure(which, l, slot, int(f), int(s), int(h), int(i), e / e_ref, r / r_ref, msg))
    return fails, (we, wr)


def half_ulp_bf16(x: np.ndarray) -> np.ndarray:
    """Half a unit in the last place of bf16 (8 significant bits) at the magnitude of x (float64)."""
    _, ex = np.frexp(np.abs(x))  # |x| = m 2^ex, m in [0.5, 1): ulp = 2^(ex - 8)
    return np.where(x == 0.0, 0.0, np.ldexp(1.0, ex - 9))


def logit_rows(tok: np.ndarray, cb: np.ndarray, T: int, frames: int):
    """Teacher-forced logits -> {step: [frames, n_logits]}: frame f is picked at position T - 1 + f; step 0 is the slow head, step i
    the depth head of code i - 1 (include/smoltts_hip.h at smoltts_session_margin_at)."""
    pos = np.arange(T - 1, T - 1 + frames)
    rows = {0: tok[pos]}
    for i in range(cb.shape[1]):
        rows[1 + i] = cb[pos, i]
    return rows


def gaps(rows: np.ndarray) -> np.ndarray:
    top = np.partition(rows, -2, axis=-1)
    return top[..., -1] - top[..., -2]


def gap_report(margin: float, margin_at: int, refs: Refs, T: int, frames: int, slot: int, factor: float = FACTOR, steps=None):
    """The session's smallest top-2 gap of one slot and its place against the float64 logits: E_row = max|fp32 - float64| logit
    over the slot's rows of the same step; |margin - g64| <= 2 factor E_row at the place the session names, and no row of the slot
    with a float64 gap below margin - 2 factor E_row.  ``steps``: the steps whose picks are greedy and so keep gap records (default
    all; a slot whose depth codes are sampled records step 0 only).  Returns (failure messages, |margin - g64| / E_row)."""
    r32, r64 = logit_rows(refs.tok32, refs.cb32, T, frames), logit_rows(refs.tok64, refs.cb64, T, frames)
    if steps is not None:
        r32, r64 = {s: r32[s] for s in steps}, {s: r64[s] for s in steps}
    f, step = int(margin_at) // 64, int(margin_at) % 64
    assert 0 <= f < frames and step in r64, f"slot {slot}: margin_at {margin_at} names frame {f} step {step} outside the {frames} frames decoded"
    e_row = float(np.abs(r32[step] - r64[step]).max())
    assert e_row > 0.0
    g64 = float(gaps(r64[step][f]))
    msgs = []
    ratio = abs(float(margin) - g64) / e_row
    if ratio > 2 * factor:
        msgs.append(f"slot {slot}: margin {margin:.6e} at frame {f} step {step}, float64 gap there {g64:.6e}: differ by {ratio:.2f} x E_row "
                    f"({e_row:.3e}), bound {2 * factor:g}")
    for s, rows in r64.items():
        g = gaps(rows)
        ff = int(g.argmin())
        if g[ff] < float(margin) - 2 * factor * e_row:
            msgs.append(f"slot {slot}: float64 gap {g[ff]:.6e} at frame {ff} step {s} is below the session's minimum {margin:.6e} (found at "
                        f"frame {f} step {step}) by {(float(margin) - g[ff]) / e_row:.2f} x E_row ({e_row:.3e}), bound {2 * factor:g}")
    return msgs, ratio
