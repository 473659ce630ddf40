"""Shared pieces of tests/test_mimi_encode_strict_gpu.py and the CPU checks of its premises (tests/test_mimi_encode_strict_cpu.py):
the cases, the two oracles' stage buffers laid out as the engine's workspace, and the four judges -- structure, chain bound, local
bound, RVQ -- whose messages name the stage, the row and the channel of a wrong element.

A "view set" is what ``MimiEncoder.stage_views`` returns, as numpy: every workspace buffer whole, [rows, channels], halo and
padding rows included (``kc`` / ``vc`` as [n_layers, 8, positions, 64]).  ``views_from_stages`` builds the same set from an oracle's
``stages``, so the CPU controls run the very judges the GPU tests run, with a CPU computation standing in for the engine.

K order: the engine's K cache keeps each head's dims in the kernel's interleaved-pair order (``packing._perm_heads``).  This helper
PERMUTES THE ORACLE'S K into that order (``kernel_k_order``); the engine's buffer is read as it is."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

FACTOR = 4.0       # the project's rule for two fp32 computations that differ by summation order (tests/test_gemm_b3_gpu.py)
GAP_FACTOR = 8.0   # a gap is the difference of two distances, each within FACTOR x E_d2 (the form of the LM gap tests)
PREMISE = 16.0     # every pick's float64 gap >= PREMISE x E_d2 with the fp32 oracle's latents: twice what the gap check allows
ELU_EPS = 6e-8     # the hardware exponential in ELU, absolute (header of tests/test_mimi_strict_gpu.py)
RATIOS = (4, 5, 6, 8)
STATE_SEED, PCM_SEED = 5, 4

Case = namedtuple("Case", "L window extra_right")
_LENGTHS = (("one", 1, 0), ("two_pos", 961, 0), ("three_pos", 960 + 1920, 0), ("ragged", 1920 * 5 + 333, 0),
            ("long", 1920 * 21 - 1, 0), ("long_w8", 1920 * 21 - 1, 8))
# every length is ragged (no multiple of 1920), so each also runs with the stride-alignment rows behind the data
CASES = {name + ("_right" if er else ""): Case(L, w, er) for er in (False, True) for name, L, w in _LENGTHS}

Layout = namedtuple("Layout", "T extra left F ds_extra ds_left")
Failure = namedtuple("Failure", "check stage row channel max_ratio rms_ratio msg")


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


@functools.lru_cache(maxsize=None)
def state(seed: int = STATE_SEED):
    from smoltts_amd.codec.synthetic import synthetic_mimi_encoder_state, synthetic_mimi_state

    return {**synthetic_mimi_state(seed=seed), **synthetic_mimi_encoder_state(seed=seed)}


def case_pcm(L: int) -> np.ndarray:
    from smoltts_amd.codec.synthetic import synthetic_pcm

    return synthetic_pcm(L, PCM_SEED)


@functools.lru_cache(maxsize=None)
def oracles(window: int, extra_right: bool):
    from oracle.mimi_oracle import MimiEncodeOracle

    st = state()
    return (MimiEncodeOracle(st, 8, window=window, extra_right=extra_right),
            MimiEncodeOracle(st, 8, window=window, extra_right=extra_right, dtype=torch.float64))


def two_pieces(x: torch.Tensor) -> torch.Tensor:
    """x cut to two bf16 pieces (16 significant bits), as tests/lm_strict_helpers.two_pieces: the rounding control's activations."""
    hi = x.bfloat16().to(x.dtype)
    return hi + (x - hi).bfloat16().to(x.dtype)


def py_layout(L: int, extra_right: bool) -> Layout:
    """Row counts of the workspace, restated from the oracle's padding rule (``_extra_padding``) and not from the engine's plan:
    the GPU tests hold ``smoltts_mimi_encode_layout`` to it."""
    from oracle.mimi_oracle import _extra_padding

    T, extra, left = [L], [], []
    for r in RATIOS:
        e = _extra_padding(T[-1], 2 * r, r)
        extra.append(e); left.append(r + (0 if extra_right else e)); T.append((T[-1] + e) // r)
    de = _extra_padding(T[4], 4, 2)
    return Layout(tuple(T), tuple(extra), tuple(left), (T[4] + de) // 2, de, 2 + (0 if extra_right else de))


def layout_of(lay) -> Layout:
    """The row counts of an ``abi.MimiEncLayout``."""
    return Layout(tuple(lay.T), tuple(lay.extra), tuple(lay.left), lay.F, lay.ds_extra, lay.ds_left)


def kernel_k_order(k: np.ndarray) -> np.ndarray:
    """The oracle's K [..., 64] (half-split RoPE pairs (j, j + 32)) in the kernel's order (pairs (2j, 2j + 1))."""
    from smoltts_amd import packing

    idx = packing._perm_heads(torch.arange(64)[:, None], n_heads=1)[:, 0].numpy()
    return k[..., idx]


def views_from_stages(s, lay: Layout, extra_right: bool):
    """An oracle's ``stages`` (batch of one) as a view set in the oracle's dtype: what the engine's workspace holds if it computes
    what that oracle computed.  Zero halo rows, edge rows of ``ds``, K in the kernel's order."""
    n = lambda t: t[0].numpy()
    v = {}
    pad = lambda a, front, back=0: np.concatenate([np.zeros((front, a.shape[1]), a.dtype), a, np.zeros((back, a.shape[1]), a.dtype)])
    for i in range(4):
        x = n(s[f"x{i}"])
        v[f"xraw{i}"] = x
        v[f"xelu{i}"] = pad(n(F.elu(s[f"x{i}"])), 2)
        v[f"helu{i}"] = n(s[f"h{i}"])
        v[f"yelu{i}"] = pad(n(s[f"y{i}"]), lay.left[i], RATIOS[i] + lay.extra[i] - lay.left[i])
    v["zelu"] = pad(n(F.elu(s["x4"])), 2)
    nl = sum(1 for k in s if k.startswith("K"))
    v["kc"] = np.stack([kernel_k_order(n(s[f"K{l}"])) for l in range(nl)])
    v["vc"] = np.stack([n(s[f"V{l}"]) for l in range(nl)])
    tr = n(s["tr"])
    back = 2 + lay.ds_extra - lay.ds_left
    v["ds"] = np.concatenate([np.repeat(tr[:1], lay.ds_left, 0), tr, np.repeat(tr[-1:], back, 0)])
    v["emb"] = n(s["emb"])
    return v


@functools.lru_cache(maxsize=None)
def references(case: Case):
    """(fp32 oracle's view set, float64 oracle's view set, their end-to-end codes [8, F]) of a case: computed once, shared, and
    not to be written to."""
    o32, o64 = oracles(case.window, case.extra_right)
    pcm = torch.from_numpy(case_pcm(case.L))[None, None]
    lay = py_layout(case.L, case.extra_right)
    s32, s64 = o32.stages(pcm), o64.stages(pcm)
    c32, c64 = (o.rvq_encode(s["emb"].transpose(1, 2))[0].numpy() for o, s in ((o32, s32), (o64, s64)))
    v32, v64 = views_from_stages(s32, lay, case.extra_right), views_from_stages(s64, lay, case.extra_right)
    for v in (v32, v64):
        for a in v.values():
            a.setflags(write=False)
    return v32, v64, c32, c64


# ---------------------------------------------------------------------------------------------- where an element sits
def data_rows(name: str, buf: np.ndarray, lay: Layout) -> np.ndarray:
    """The data rows of a workspace buffer (its halo / padding rows cut off)."""
    if name.startswith("xelu") or name == "zelu":
        return buf[2:]
    if name.startswith("yelu"):
        i = int(name[-1])
        return buf[lay.left[i]: lay.left[i] + lay.T[i]]
    if name == "ds":
        return buf[lay.ds_left: lay.ds_left + lay.T[4]]
    return buf


def where(name: str, row: int, ch: int, n_rows: int) -> str:
    """Stage, row and channel of an element; the row's place in a 64-row tile of the many-row GEMM and whether it ends the buffer."""
    last = ", the LAST row of its buffer" if row == n_rows - 1 else ""
    return f"{name} row {row} of {n_rows} (row mod 64 = {row % 64}{last}), channel {ch}"


def _judge(check, name, got, r32, r64, factor=FACTOR):
    """One buffer [rows, C] under  max|got - f64| <= factor E_ref  and  RMS <= factor R_ref,  E_ref / R_ref from r32 - r64."""
    assert got.shape == r32.shape == r64.shape, f"{check} {name}: shapes {got.shape}, {r32.shape}, {r64.shape}"
    assert np.isfinite(got).all(), f"{check} {name}: not finite"
    own = r32.astype(np.float64) - r64
    d = got.astype(np.float64) - r64
    e_ref, r_ref = float(np.abs(own).max()), rms(own)
    assert e_ref > 0.0, f"{check} {name}: the fp32 reference equals the float64 one, no yardstick"
    row, ch = np.unravel_index(int(np.abs(d).argmax()), d.shape)
    e, r = float(np.abs(d[row, ch])), rms(d)
    fail = None
    if e > factor * e_ref or r > factor * r_ref:
        fail = Failure(check, name, int(row), int(ch), e / e_ref, r / r_ref,
                       f"{check} bound, {where(name, int(row), int(ch), d.shape[0])}: max err {e:.3e} = {e / e_ref:.2f} x E_ref "
                       f"({e_ref:.3e}), rms {r:.3e} = {r / r_ref:.2f} x R_ref ({r_ref:.3e}), bound {factor:g}")
    return fail, e / e_ref, r / r_ref


def _heads_as_rows(c: np.ndarray) -> np.ndarray:
    """One layer's cache [8, T, 64] -> [T, 512] (channel = head * 64 + dim)."""
    return np.ascontiguousarray(c.transpose(1, 0, 2)).reshape(c.shape[1], -1)


CHAIN_GROUPS = ("conv0", "stage0", "stage1", "stage2", "stage3", "K", "V", "tr", "emb")


def _chain_items(views, lay):
    """(group, name, data rows) of every buffer the chain bound judges."""
    for i in range(4):
        made_by = "conv0" if i == 0 else f"stage{i - 1}"  # x_i comes out of conv0 / the strided conv of the stage before
        for nm, grp in (("xraw", made_by), ("xelu", made_by), ("helu", f"stage{i}"), ("yelu", f"stage{i}")):
            yield grp, f"{nm}{i}", data_rows(f"{nm}{i}", views[f"{nm}{i}"], lay)
    yield "stage3", "zelu", data_rows("zelu", views["zelu"], lay)
    for l in range(views["kc"].shape[0]):
        yield "K", f"K{l}", _heads_as_rows(views["kc"][l])
        yield "V", f"V{l}", _heads_as_rows(views["vc"][l])
    yield "tr", "ds", data_rows("ds", views["ds"], lay)
    yield "emb", "emb", views["emb"]


def chain_report(got, v32, v64, lay: Layout):
    """Every stage buffer and every layer's K / V of ``got`` against the float64 oracle's, by the fp32 oracle's own distance.
    Returns (failures in chain order, {name: (max ratio, rms ratio)})."""
    fails, ratios = [], {}
    for (grp, name, g), (_, _, a), (_, _, b) in zip(_chain_items(got, lay), _chain_items(v32, lay), _chain_items(v64, lay)):
        f, e, r = _judge("chain", name, g, a, b)
        ratios[name] = (grp, e, r)
        if f:
            fails.append(f)
    return fails, ratios


# ---------------------------------------------------------------------------------------------- single ops on the engine's own input
def _cf(a: np.ndarray, dtype) -> torch.Tensor:
    """Channel-last rows [T, C] -> the oracle's (1, C, T) in ``dtype``."""
    return torch.from_numpy(np.ascontiguousarray(a.T))[None].to(dtype)


def _cl(t: torch.Tensor) -> np.ndarray:
    return t[0].T.contiguous().numpy()


def local_ops(views, pcm: np.ndarray, lay: Layout, orc):
    """{op: output rows [T, C]} of every single op of the chain, each applied by ``orc`` (in its dtype) to the INPUT buffer found in
    ``views``: "conv0"; per stage i "k3_{i}" (xelu_i -> helu_i), "k1_{i}" (helu_i, xraw_i -> yelu_i), "s_{i}" (yelu_i -> xraw_{i+1},
    or zelu for i = 3); "downsample" (ds -> emb).  The padding is the oracle's own; the engine's padding rows are not read here."""
    dt = orc.dt
    out = {"conv0": _cl(orc.conv(_cf(pcm[:, None], dt), "0"))}
    li = 1
    for i, r in enumerate(RATIOS):
        out[f"k3_{i}"] = _cl(F.elu(orc.conv(_cf(data_rows(f"xelu{i}", views[f"xelu{i}"], lay), dt), f"{li}.block.1")))
        out[f"k1_{i}"] = _cl(F.elu(_cf(views[f"xraw{i}"], dt) + orc.conv(_cf(views[f"helu{i}"], dt), f"{li}.block.3")))
        s = orc.conv(_cf(data_rows(f"yelu{i}", views[f"yelu{i}"], lay), dt), str(li + 2), r)
        out[f"s_{i}"] = _cl(F.elu(s) if i == 3 else s)
        li += 3
    out["downsample"] = _cl(orc.downsample(_cf(data_rows("ds", views["ds"], lay), dt)))
    return out


def local_outputs(views, lay: Layout):
    """{op: the output buffer's data rows in ``views``}, keyed as ``local_ops``."""
    out = {"conv0": views["xraw0"], "downsample": views["emb"]}
    for i in range(4):
        out[f"k3_{i}"] = views[f"helu{i}"]
        out[f"k1_{i}"] = data_rows(f"yelu{i}", views[f"yelu{i}"], lay)
        out[f"s_{i}"] = views[f"xraw{i + 1}"] if i < 3 else data_rows("zelu", views["zelu"], lay)
    return out


LOCAL_OPS = ("conv0",) + tuple(f"{k}_{i}" for i in range(4) for k in ("k3", "k1", "s")) + ("downsample",)
_OUT_NAME = {"conv0": "xraw0", "downsample": "emb", **{f"k3_{i}": f"helu{i}" for i in range(4)}, **{f"k1_{i}": f"yelu{i}" for i in range(4)},
             **{f"s_{i}": (f"xraw{i + 1}" if i < 3 else "zelu") for i in range(4)}}


def local_report(got, pcm: np.ndarray, lay: Layout, o32, o64):
    """Every single op isolated from the noise before it: the float64 op on ``got``'s own input buffer against ``got``'s output
    buffer; the yardstick is fp32 torch running the same op on the same input.  Returns (failures, {op: (max ratio, rms ratio)})."""
    want64, want32, have = local_ops(got, pcm, lay, o64), local_ops(got, pcm, lay, o32), local_outputs(got, lay)
    fails, ratios = [], {}
    for op in LOCAL_OPS:
        f, e, r = _judge(f"local {op}", _OUT_NAME[op], have[op], want32[op], want64[op])
        ratios[op] = (e, r)
        if f:
            fails.append(f._replace(stage=op))
    return fails, ratios


# ---------------------------------------------------------------------------------------------- structure, exactly
def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def structure_report(got, lay: Layout, extra_right: bool):
    """Messages for: a halo / padding row that is not bit-zero, an edge row of ``ds`` that is not its neighbour's bits, an ELU copy
    further than ELU_EPS from the ELU of its raw copy."""
    msgs = []

    def zero_rows(name, rows, lo, hi, what):
        assert 0 <= lo <= hi <= rows.shape[0], (name, lo, hi, rows.shape)
        bad = np.argwhere(_bits(rows[lo:hi]) != 0)
        if len(bad):
            r, c = bad[0]
            msgs.append(f"structure: {name} {what} row {lo + r} (rows [{lo}, {hi}) must be bit-zero), channel {c}: "
                        f"{rows[lo + r, c]!r}; {len(bad)} non-zero elements")

    for i in range(4):
        zero_rows(f"xelu{i}", got[f"xelu{i}"], 0, 2, "halo")
        y = got[f"yelu{i}"]
        assert y.shape[0] == RATIOS[i] + lay.extra[i] + lay.T[i] and lay.left[i] == RATIOS[i] + (0 if extra_right else lay.extra[i])
        zero_rows(f"yelu{i}", y, 0, lay.left[i], "front padding")
        zero_rows(f"yelu{i}", y, lay.left[i] + lay.T[i], y.shape[0], "back padding")
        raw, elu = got[f"xraw{i}"].astype(np.float64), data_rows(f"xelu{i}", got[f"xelu{i}"], lay).astype(np.float64)
        d = np.abs(elu - np.where(raw > 0, raw, np.expm1(np.minimum(raw, 0.0))))
        if d.max() > ELU_EPS:
            r, c = np.unravel_index(int(d.argmax()), d.shape)
            msgs.append(f"structure: {where(f'xelu{i}', int(r), int(c), d.shape[0])} is {d.max():.3e} from ELU(xraw{i}) (bound {ELU_EPS:g})")
    zero_rows("zelu", got["zelu"], 0, 2, "halo")
    ds, T4 = got["ds"], lay.T[4]
    assert ds.shape[0] == 2 + lay.ds_extra + T4 and lay.ds_left == 2 + (0 if extra_right else lay.ds_extra)
    for lo, hi, src, what in ((0, lay.ds_left, lay.ds_left, "first"), (lay.ds_left + T4, ds.shape[0], lay.ds_left + T4 - 1, "last")):
        bad = np.argwhere(_bits(ds[lo:hi]) != _bits(ds[src: src + 1]))
        if len(bad):
            msgs.append(f"structure: ds edge row {lo + bad[0][0]} is not the bits of the {what} data row {src}, channel {bad[0][1]}")
    return msgs


# ---------------------------------------------------------------------------------------------- RVQ, teacher-forced
def e_d2(o32, walk64) -> np.ndarray:
    """E_d2(q, f) = max_j |fp32 oracle's d2 - float64 d2| on the float64 walk's residual (rounded to fp32 for the fp32 formula)."""
    nq = walk64["d2"].shape[1]
    d32 = torch.stack([o32.distance_row(walk64["before"][0, q].float(), q) for q in range(nq)])
    return (d32.double() - walk64["d2"][0]).abs().amax(-1).numpy()


def rvq_report(emb: np.ndarray, codes: np.ndarray, gap, res, o32, o64):
    """Teacher-forced on the given latents [F, 512] along the given codes [nq, F]: every code must be the float64 argmin, every
    gap within GAP_FACTOR x E_d2(q, f) of the float64 gap, the final residual [F, 256] within FACTOR x the fp32 walk's own error.
    ``gap`` / ``res`` None: not judged.  Returns (messages, {"gap": worst |err| / E_d2, "res": (max, rms ratio), "premise":
    min gap / E_d2})."""
    e = torch.from_numpy(np.ascontiguousarray(emb.T))[None]
    c = torch.from_numpy(np.asarray(codes))[None].long()
    w64, w32 = o64.rvq_walk(e, c), o32.rvq_walk(e, c)
    E = e_d2(o32, w64)
    g64, am = w64["gap"][0].numpy(), w64["argmin"][0].numpy()
    msgs, out = [], {"premise": float((g64 / E).min())}
    for q, f in np.argwhere(am != codes):
        msgs.append(f"rvq: codebook {q}, frame {f}: code {codes[q, f]}, float64 argmin {am[q, f]}, float64 gap {g64[q, f]:.3e}, "
                    f"E_d2 {E[q, f]:.3e}")
    if gap is not None:
        ratio = np.abs(gap.astype(np.float64) - g64) / E
        ratio[am != codes] = 0.0  # (already reported)
        out["gap"] = float(ratio.max())
        for q, f in np.argwhere(ratio > GAP_FACTOR):
            msgs.append(f"rvq gap: codebook {q}, frame {f}: code {codes[q, f]} (float64 argmin {am[q, f]}), gap {gap[q, f]:.6e}, float64 gap "
                        f"{g64[q, f]:.6e}, |err| = {ratio[q, f]:.2f} x E_d2 ({E[q, f]:.3e}), bound {GAP_FACTOR:g}")
    if res is not None:
        fail, er, rr = _judge("local input_proj + residual walk", "res", res, w32["after"][0, -1].numpy(), w64["after"][0, -1].numpy())
        out["res"] = (er, rr)
        if fail:
            msgs.append(fail.msg)
    return msgs, out


# ---------------------------------------------------------------------------------------------- the whole judgement of one call
def judge_call(label, case: Case, got, pcm, codes, gap, lay: Layout, expect_ok=True):
    """All four judges on one call's view set (plus its codes [8, F] and gaps): prints the worst ratio per stage group and returns
    (messages, ratios).  ``got["emb"]`` is the call's latents, ``got["res"]`` its final residual."""
    o32, o64 = oracles(case.window, case.extra_right)
    v32, v64, _, c64 = references(case)
    assert lay == py_layout(case.L, case.extra_right), f"{label}: layout {lay} != {py_layout(case.L, case.extra_right)}"
    msgs = structure_report(got, lay, case.extra_right)
    cf, cr = chain_report(got, v32, v64, lay)
    lf, lr = local_report(got, pcm, lay, o32, o64)
    rm, rr = rvq_report(got["emb"], codes, gap, got.get("res"), o32, o64)
    msgs += [f.msg for f in cf] + [f.msg for f in lf] + rm
    if not np.array_equal(codes, c64):
        msgs.append(f"codes: {int((codes != c64).sum())} differ from the float64 oracle's end-to-end codes, first at (q, f) = "
                    f"{tuple(np.argwhere(codes != c64)[0])}")
    groups = {g: (max(e for gg, e, _ in cr.values() if gg == g), max(r for gg, _, r in cr.values() if gg == g)) for g in CHAIN_GROUPS}
    loc = (max(e for e, _ in lr.values()), max(r for _, r in lr.values()))
    print(f"{label}: chain max/E_ref, rms/R_ref per group: " + "  ".join(f"{g} {e:.2f}, {r:.2f}" for g, (e, r) in groups.items()))
    print(f"{label}: local worst {loc[0]:.2f}, {loc[1]:.2f} (" + " ".join(f"{op} {e:.2f}" for op, (e, _) in lr.items()) + ")"
          + (f"; res {rr['res'][0]:.2f}, {rr['res'][1]:.2f}" if "res" in rr else "") + (f"; gap err / E_d2 {rr['gap']:.2f}" if "gap" in rr else "")
          + f"; min float64 gap / E_d2 {rr['premise']:.1f}")
    if expect_ok:
        assert not msgs, f"{label}: {len(msgs)} failures\n" + "\n".join(msgs[:8])
    return msgs, {"chain": cr, "groups": groups, "local": lr, "rvq": rr}
