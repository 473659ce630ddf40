"""The depth (fast) transformer as the engine runs it, layer by layer and step by step: every K and V row of the session's depth
cache against the float64 oracle, judged by the fp32 oracle's own noise -- for every launch structure ``run_tail`` has.

tests/test_lm_strict_gpu.py holds the slow transformer's rows to float64; the depth transformer (8 steps x 4 layers per frame) it sees
only through the smallest top-2 gap of a slot, one place per slot.  Here the depth cache itself is read
(``LMSession.fast_kv_cache``: fp32 [n_fast_layer, B, fast_n_kv, n_fast, 64], one frame's rows until the next frame overwrites them).
Layer l's row of step i is a function of the layers below it at the steps <= i, so a wrong launch is named by layer and step; layer
l + 1's rows expose layer l's attention, wo, w13 and w2, and step i + 1's rows the pick and the embedding gather of step i.

Per case the session (``NumericsMode.torch_reference()``, no stop at <|im_end|>) prefills random prompts of exactly T_b columns and
the depth cache is read: frame 0.  Three times ``decode(1)``, synchronise, read: frames 1 .. 3.  Both CPU oracles are then
teacher-forced, per slot, on the prompt plus the engine's own 4 frames (frame f is picked at position T_b - 1 + f and its depth pass
sees the codes of column T_b + f; no near-tie flip matters).  Per depth layer, K and V apart, pooled over the 4 frames and the n_fast
steps of the slot:
    E_ref = max|fp32 oracle - float64 oracle|   and   R_ref = RMS of the same difference,
and required:  max|engine - float64| <= 4 E_ref   and   RMS(engine - float64) <= 4 R_ref   (the project's factor for two
computations that differ by fp32 rounding).  A failure names the case, K or V, depth layer, slot, frame, step, kv head and dimension
of the worst element, the value got and the float64 value.  The slot's ``margin`` / ``margin_at`` go through the strict file's gap
check as well (|margin - float64 gap| <= 2 * 4 E_row).

The real-size cases run ONE slow layer (``dataclasses.replace(named_config(...), n_layer=1)``): the depth rows inherit the slow
stack's fp32 noise, which at 10 layers drowns the depth chain's own -- a 2^-16-grade depth kernel then sits at 3.7 .. 5.3 x R_ref,
partly under the bound, against 5.7 .. 6.4 with one slow layer (tests/test_oracle_cpu.py::
test_lm_depth_control_is_drowned_by_the_full_slow_stack); the depth transformer keeps its true dimensions.  That the bound rejects
2^-16-grade depth arithmetic at every depth layer of every config here: test_lm_depth_bound_rejects_two_piece_activations.

Options (``OPTIONS``): defaults; the greedy pick as a launch of its own; the depth attention as a launch of its own (the fused
pick needs the fused attention, so this switches both); layer-0 q | k | v through the wqkv GEMM instead of the table; the slow token
and the last code picked outside the commit kernel; depth codes sampled at temperature 0.8 (the rows are still functions of the
engine's own ids; only the slow token keeps gap records then).

Measured on the MI355X, worst depth layer, slot and K / V per case: max err / E_ref, rms / R_ref (bound 4); then the gap check's worst
|margin - g64| / E_row (bound 8):
  tiny bf16: defaults, pick off, attention off, commit picks off   0.64, 0.54   gaps 0.16
             table off                                             0.64, 0.53   gaps 0.24
             sampled depth codes                                   0.68, 0.55   gaps 0.39
  tiny fp8:  defaults, pick off, attention off, commit picks off   0.72, 0.51   gaps 0.35
             table off                                             0.72, 0.52   gaps 0.35
             sampled depth codes                                   0.64, 0.50   gaps 0.24
  tiny_nodup bf16                                                  0.74, 0.50   gaps 0.19
  tiny_proj bf16                                                   0.67, 0.54   gaps 0.17
  70m, one slow layer, bf16, 20 slots: defaults                    0.82, 0.58   gaps 0.32
             table off                                             0.78, 0.58   gaps 0.47
  150m, one slow layer, fp8: defaults, pick off, attention off, commit picks off   0.71, 0.56   gaps 0.31
             table off                                             0.74, 0.56   gaps 0.38
             sampled depth codes                                   0.64, 0.55   gaps 0.18
i.e. the depth chain is as close to float64 as the fp32 CPU oracle is, in every launch structure.  The header's "same bits" held: on
tiny bf16, tiny fp8 and 150m fp8 the fused pick on / off and the fused attention on / off gave equal ids, bit-identical depth rows in
all 4 frames and (fused pick) identical gap records.  The module takes under 4 s on the MI355X, engines included (the 150m fp8 engine:
1 s to build; tests/test_fp8_gpu.py's 150m case, which builds the same model at 10 layers: 2.7 s).
"""
from collections import namedtuple

import numpy as np
import pytest
import torch

from lm_strict_helpers import (DEPTH_FRAMES, DEPTH_TS, FACTOR, depth_refs, gap_report, make_oracles, random_grid, slot_depth_rows,
                               strict_depth_report, teacher_refs)

pytestmark = pytest.mark.gpu

SEED = 3
OPTIONS = {
    "defaults": {},
    "pick_off": {"fused_pick": False},
    "attn_off": {"fused_attn": False},
    "table_off": {"table": False},
    "commit_off": {"commit": False},
    "sampled": {"sampled": True},
}
Run = namedtuple("Run", "prompts frames fK fV margin margin_at")


class _Model:
    """One config's engine and its two oracles, with the teacher-forced passes kept by grid and the runs kept by option."""

    def __init__(self, cfgname, fp8=False, n_layer=None):
        from smoltts_amd.config import NumericsMode, TokenConfig
        from smoltts_amd.engine import LMEngine
        from smoltts_amd.tokenizer import load_tokenizer

        self.name = f"{cfgname}{', one slow layer' if n_layer else ''}, {'fp8' if fp8 else 'bf16'}"
        self.Ts = DEPTH_TS[cfgname]
        self.cfg, state, self.o32, self.o64 = make_oracles(cfgname, SEED, fp8=fp8, n_layer=n_layer)
        self.eng = LMEngine(self.cfg, state, TokenConfig.from_tokenizer(load_tokenizer(), self.cfg), NumericsMode.torch_reference(),
                            weight_format="fp8" if fp8 else "bf16")
        assert self.eng.weight_format == ("fp8" if fp8 else "bf16")
        self._refs, self._runs = {}, {}

    def refs(self, grid):
        key = grid.tobytes()
        if key not in self._refs:
            self._refs[key] = teacher_refs(self.o32, self.o64, grid)
        return self._refs[key]

    def run(self, option) -> Run:
        if option not in self._runs:
            self._runs[option] = _run(self, **OPTIONS[option])
        return self._runs[option]


def _fixture(*args, **kw):
    @pytest.fixture(scope="module")
    def fx():
        m = _Model(*args, **kw)
        yield m
        m.eng.close()
    return fx


tiny = _fixture("tiny")
tiny_fp8 = _fixture("tiny", fp8=True)
tiny_nodup = _fixture("tiny_nodup")
tiny_proj = _fixture("tiny_proj")
m70_one = _fixture("smoltts_byte_70m", n_layer=1)
m150_one_fp8 = _fixture("smoltts_byte_150m", fp8=True, n_layer=1)


def _run(m, fused_pick=True, fused_attn=True, table=True, commit=True, sampled=False, seed=11) -> Run:
    """Prefill random prompts of exactly ``m.Ts`` columns and read the depth cache (frame 0); decode one frame, synchronise and read,
    three times -> Run(prompt grids, frames [B, 4, H], depth K and V per frame as float32 numpy [n_fast_layer, B, fast_n_kv, n_fast, 64],
    margin, margin_at)."""
    from smoltts_amd.engine import LMSession

    Ts, B = m.Ts, len(m.Ts)
    gen = torch.Generator().manual_seed(seed)
    prompts = [random_grid(m.cfg, T, gen) for T in Ts]
    sess = LMSession(m.eng, max_batch=B, max_seq=max(Ts) + DEPTH_FRAMES + 8, max_rows=max(sum(Ts), B), max_frames=DEPTH_FRAMES + 8)
    if not fused_pick:
        sess.use_fused_pick(False)
    if not fused_attn:
        sess.use_fused_depth_attention(False)
    if not table:
        sess.use_qkv_table(False)
    if not commit:
        sess.use_commit_picks(False)
    if sampled:
        sess.set_slot_sampling(list(range(B)), [0.0] * B, [0.8] * B, [0.0] * B, [1000 + b for b in range(B)])
    fK, fV = [], []

    def read():
        torch.cuda.current_stream().synchronize()
        k, v = sess.fast_kv_cache()
        assert k.dtype == v.dtype == torch.float32 and tuple(k.shape) == tuple(v.shape) == \
            (m.cfg.n_fast_layer, B, m.cfg.fast_n_local_heads, m.cfg.max_fast_seqlen, 64)
        fK.append(k.cpu().numpy().copy()); fV.append(v.cpu().numpy().copy())

    sess.prefill(prompts, stop_on_eos=False)
    read()
    for _ in range(DEPTH_FRAMES - 1):
        sess.decode(1)
        read()
    codes, nf, done, margin = sess.fetch()
    assert (nf == DEPTH_FRAMES).all() and not done.any(), (nf, done)
    run = Run(prompts, codes[:, :DEPTH_FRAMES].copy(), fK, fV, margin.copy(), sess.margin_at.cpu().numpy().copy())
    sess.close()
    return run


def _judge(m, option):
    """Every slot's depth rows of the 4 frames under the bound, per depth layer, K and V; then its gap record."""
    run, F = m.run(option), DEPTH_FRAMES
    label = f"{m.name}, {option}"
    if OPTIONS[option].get("sampled"):  # the temperature is in effect: the codes are not the greedy run's (the slow token of frame 0 is)
        greedy = m.run("defaults")
        assert np.array_equal(run.frames[:, 0, 0], greedy.frames[:, 0, 0]) and not np.array_equal(run.frames[:, :, 1:], greedy.frames[:, :, 1:])
    assert all(not np.array_equal(run.fK[f], run.fK[f + 1]) for f in range(F - 1))  # every read saw a new frame's rows
    fails, gmsgs, we, wr, wg = [], [], 0.0, 0.0, 0.0
    for b, T in enumerate(m.Ts):
        grid = np.concatenate([run.prompts[b], run.frames[b].T], axis=1)  # (H, T + 4): frame f's codes are column T + f
        r = m.refs(grid)
        for which, per_frame, r32, r64 in (("K", run.fK, r.fK32, r.fK64), ("V", run.fV, r.fV32, r.fV64)):
            got = np.stack([slot_depth_rows(c, b) for c in per_frame], axis=1)  # [n_fast_layer, 4, n_fast, kv, 64]
            f, (e, rr) = strict_depth_report(got, depth_refs(r32, T, F), depth_refs(r64, T, F), b, which, FACTOR)
            fails += f
            we, wr = max(we, e), max(wr, rr)
        steps = (0,) if OPTIONS[option].get("sampled") else None  # sampled depth codes keep no gap records
        mm, ratio = gap_report(float(run.margin[b]), int(run.margin_at[b]), r, T, F, b, FACTOR, steps=steps)
        gmsgs += mm
        wg = max(wg, ratio)
    print(f"{label}: depth rows, worst max err / E_ref {we:.2f}, rms / R_ref {wr:.2f} (bound {FACTOR:g}); top-2 gaps: worst |margin - g64| / "
          f"E_row {wg:.2f} (bound {2 * FACTOR:g})")
    fails.sort(key=lambda f: -max(f.max_ratio, f.rms_ratio))
    assert not fails, f"{label}: {len(fails)} (depth layer, slot, K / V) units over the bound, worst first:\n" + "\n".join(f.msg for f in fails[:6])
    assert not gmsgs, f"{label}: " + "\n".join(gmsgs[:6])


@pytest.mark.parametrize("option", list(OPTIONS))
def test_tiny_bf16(tiny, option):
    """tiny (2 depth layers, 6 / 2 heads), B = 5, T = 1, 2, 5, 9, 17: the whole option matrix."""
    _judge(tiny, option)


@pytest.mark.parametrize("option", list(OPTIONS))
def test_tiny_fp8(tiny_fp8, option):
    """The same with e4m3 weights against the oracles on ``fp8_reference_state``: the W8 depth launches, the fp8 head slices and the
    fp8-built qkv table."""
    _judge(tiny_fp8, option)


def test_tiny_nodup(tiny_nodup):
    """duplicate_code_0 off: 7 depth steps, an 8-row grid, ``emb_row_offset`` shifted by one codebook."""
    _judge(tiny_nodup, "defaults")


def test_tiny_proj(tiny_proj):
    """fast_dim != dim: ``fast_project_in`` (Linear + bias) in front of the depth layers, one kv head, a plain Linear depth head."""
    _judge(tiny_proj, "defaults")


@pytest.mark.parametrize("option", ["defaults", "table_off"])
def test_70m_one_slow_layer_twenty_slots(m70_one, option):
    """70m depth dimensions (9 / 3 heads, dim 576, 4 layers), B = 20, T = 3 + (b mod 5): more than 16 rows per depth launch."""
    _judge(m70_one, option)


@pytest.mark.parametrize("option", list(OPTIONS))
def test_150m_one_slow_layer_fp8(m150_one_fp8, option):
    """The benchmark's depth transformer (12 / 4 heads, dim 768, fp8 weights), B = 3: the whole option matrix."""
    _judge(m150_one_fp8, option)


def _assert_same_bits(m, a, b, gaps_too):
    """Runs ``a`` and ``b`` of one engine, where their ids are equal: the depth rows of all 4 frames bit for bit (and, for the fused
    pick, the gap records the header promises)."""
    ra, rb = m.run(a), m.run(b)
    if not np.array_equal(ra.frames, rb.frames):
        print(f"{m.name}: {a} and {b} produce different ids (a near-tie moved): bit equality is not defined, nothing compared")
        return
    for f in range(DEPTH_FRAMES):
        for which, xa, xb in (("K", ra.fK[f], rb.fK[f]), ("V", ra.fV[f], rb.fV[f])):
            if not np.array_equal(xa, xb):
                l, s, h, i, d = np.unravel_index(int(np.abs(xa.astype(np.float64) - xb).argmax()), xa.shape)
                raise AssertionError(f"{m.name}: depth {which} rows of {a} and {b} differ in frame {f}: {int((xa != xb).sum())} elements, largest at "
                                     f"depth layer {l}, slot {s}, kv head {h}, step {i}, dim {d}: {xa[l, s, h, i, d]:.9g} vs {xb[l, s, h, i, d]:.9g}")
    if gaps_too:
        assert np.array_equal(ra.margin, rb.margin) and np.array_equal(ra.margin_at, rb.margin_at), \
            f"{m.name}: gap records of {a} and {b} differ: {ra.margin} at {ra.margin_at} vs {rb.margin} at {rb.margin_at}"
    print(f"{m.name}: {a} and {b}: equal ids, depth rows of {DEPTH_FRAMES} frames bit-identical")


@pytest.mark.parametrize("model", ["tiny", "tiny_fp8", "m150_one_fp8"])
def test_fused_launches_leave_the_same_bits(model, request):
    """include/smoltts_hip.h: the fused depth attention forms "every sum in the stand-alone kernels' order: bit-identical to them", the
    fused pick gives "same ids, same gap records".  Fused attention on vs off (off also unfuses the pick) and fused pick on vs off,
    within one engine: the depth rows of every layer, step and frame bit for bit."""
    m = request.getfixturevalue(model)
    _assert_same_bits(m, "defaults", "pick_off", gaps_too=True)
    _assert_same_bits(m, "pick_off", "attn_off", gaps_too=False)
