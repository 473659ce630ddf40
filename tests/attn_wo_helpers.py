"""The variant matrix of attn_wo_kernel<G, T, TWO, W8, PICK, NBF> (gemm3.hip: the depth-step attention worked out inside the wo GEMM).

Shared by tests/test_attn_wo_matrix_gpu.py (every case against a float64 reference and, without PICK, against the two launches it
replaces), tests/test_attn_wo_coverage_cpu.py (the mirror below against the instantiations in the built code objects) and the
LDS-poison comparison, which runs the whole matrix in fresh processes: ``python tests/attn_wo_helpers.py OUT.npz`` with
``SMOLTTS_LIB`` naming the library.  Module-level and GPU-free at import."""
from __future__ import annotations

import sys
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

CACHE_LEN = 8
PAD_ROWS, PAD_COLS = 3, 16  # NaN rows / columns around resid / out that no launch may read or write
EMB_OFF = 5                 # SmolttsPickArgs.emb_row_offset of the PICK cases
AWO_U = 3                   # gemm3.hip AWO_U: 32-k chunks per GEMM wave


class Case(NamedTuple):
    M: int
    Hq: int
    KV: int
    pos: int
    w8: bool
    pick: bool

    @property
    def id(self) -> str:
        return f"M{self.M}-h{self.Hq}x{self.KV}-p{self.pos}" + ("-w8" if self.w8 else "") + ("-pick" if self.pick else "")


def instance(c: Case) -> tuple:
    """(G, T, TWO, W8, PICK, NBF) that launch_attn_wo_g launches for this case (N = K = Hq * 64)."""
    K = N = c.Hq * 64
    nchunks, ntiles = K // 32, (N + 15) // 16
    T = 3 if c.M > 16 else 1
    two = c.pos + 1 > 4
    nbf = nchunks // AWO_U if nchunks in (6 * AWO_U, 8 * AWO_U) and ntiles % T == 0 else 0
    G = c.Hq // c.KV
    if nbf == 6 and G not in (1, 3):  # (K = 576 is 9 query heads: never reached; the launch falls back to the general form)
        nbf = 0
    return (G, T, two, c.w8, c.pick, nbf)


def launchable() -> set:
    """Every instantiation some accepted call can reach: NBF = 6 needs 9 query heads, i.e. groups of 1 or 3."""
    out = set()
    for G in (1, 2, 3, 4):
        for nbf in (0, 6, 8):
            if nbf == 6 and G not in (1, 3):
                continue
            for T in (1, 3):
                for two in (False, True):
                    for w8 in (False, True):
                        for pick in (False, True):
                            out.add((G, T, two, w8, pick, nbf))
    return out


# head layouts (query heads, kv heads) per (G, NBF): 12 heads = K 768 (NBF 8), 9 heads = K 576 (NBF 6), anything else NBF 0;
# odd kv-head counts leave a (row, kv pair) unit with a kv head that is not there (hv == false); 12 x 12 has more units than waves
LAYOUTS = {(1, 8): [(12, 12)], (2, 8): [(12, 6)], (3, 8): [(12, 4)], (4, 8): [(12, 3)], (1, 6): [(9, 9)], (3, 6): [(9, 3)],
           (1, 0): [(5, 5), (2, 2), (1, 1)], (2, 0): [(8, 4), (6, 3), (2, 1)], (3, 0): [(6, 2), (3, 1)], (4, 0): [(8, 2), (4, 1)]}
M_T1 = [1, 5, 9, 15, 2, 16, 7]     # T = 1 (odd M: a last workgroup with one row)
M_T3 = [17, 65, 33, 32, 19, 47]    # T = 3 (65: 33 workgroup rows)


def cases() -> list:
    """One case per launchable instantiation, rotating row counts, layouts and positions 0..7 (PICK: 1..7)."""
    out, i = [], 0
    for (_g, _nbf), lays in LAYOUTS.items():
        for T in (1, 3):
            for two in (False, True):
                for w8 in (False, True):
                    for pick in (False, True):
                        Hq, KV = lays[i % len(lays)]
                        Ms = M_T1 if T == 1 else M_T3
                        poss = [4, 5, 6, 7] if two else ([1, 2, 3] if pick else [0, 1, 2, 3])
                        out.append(Case(Ms[i % len(Ms)], Hq, KV, poss[i % len(poss)], w8, pick))
                        i += 1
    return out


CASES = cases()


# ------------------------------------------------------------------------------------------------ references (CPU)
def bf16r(t):
    return t.to(torch.bfloat16).float()


def rel_err(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Byte equality (NaN == NaN when the bits are the same)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def attention_ref(q, kc, vc, pos, Hq):
    """q [M, Hq*64]; caches [M, KV, L, 64]; keys 0..pos of the row's own slot; float64."""
    M, KV = q.shape[0], kc.shape[1]
    G = Hq // KV
    qh = q.view(M, Hq, 64).double()
    k = kc[:, :, : pos + 1].double().repeat_interleave(G, dim=1)  # [M, Hq, L, 64]
    v = vc[:, :, : pos + 1].double().repeat_interleave(G, dim=1)
    s = torch.einsum("mhd,mhjd->mhj", qh, k) / 8.0
    p = torch.softmax(s, dim=-1)
    return torch.einsum("mhj,mhjd->mhd", p, v).reshape(M, Hq * 64).float()


def rope_table(n_pos: int = CACHE_LEN) -> torch.Tensor:
    """fp32 [pos][32][2] (cos, sin) of pair i of a 64-dim head."""
    inv = 10000.0 ** (-torch.arange(32, dtype=torch.float64) / 32)
    ang = torch.arange(n_pos, dtype=torch.float64)[:, None] * inv[None]
    return torch.stack([ang.cos(), ang.sin()], -1).float()


def rope_rows(v: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    """RoPE of fp32 rows [M, heads * 64] at one position (cs [32][2]), every product and sum rounded to fp32 as rope_gathered4 does."""
    M = v.shape[0]
    x = v.view(M, -1, 32, 2)
    a, b, c, s = x[..., 0], x[..., 1], cs[:, 0], cs[:, 1]
    return torch.stack([a * c - b * s, b * c + a * s], -1).reshape(M, -1)


def _gen(c: Case) -> torch.Generator:
    return torch.Generator().manual_seed(c.M * 1000003 + c.Hq * 10007 + c.KV * 1009 + c.pos * 101 + c.w8 * 11 + c.pick * 7)


def _weights(ops, g, N, K, w8):
    w = torch.randn(N, K, generator=g) * 0.04
    if w8:
        wt, scale, wdq = ops.pack_weight_fp8(w)
        return wt, scale, wdq
    w = bf16r(w)
    return ops.pack_weight(w), None, w


def _padded(x: torch.Tensor) -> torch.Tensor:
    M, N = x.shape
    buf = torch.full((M + PAD_ROWS, N + PAD_COLS), float("nan"))
    buf[:M, :N] = x
    return buf


# ------------------------------------------------------------------------------------------------ runs (GPU)
def run_plain(E, ops, c: Case) -> dict:
    """attn_q case: the fused launch in place (resid == out) and out of place, and the two launches it replaces; every buffer of
    resid / out carries NaN padding rows and columns.  CPU tensors of inputs and results."""
    g = _gen(c)
    M, Hq, KV, pos = c.M, c.Hq, c.KV, c.pos
    K = N = Hq * 64
    q = torch.randn(M, K, generator=g) * 1.5
    kc = torch.randn(M, KV, CACHE_LEN, 64, generator=g)
    vc = torch.randn(M, KV, CACHE_LEN, 64, generator=g)
    kc[:, :, pos + 1:] = float("nan")  # entries behind the row's position must never be read into a result
    vc[:, :, pos + 1:] = float("nan")
    wt, scale, wref = _weights(ops, g, N, K, c.w8)
    r = torch.randn(M, N, generator=g)
    ga = 1 + 0.1 * torch.randn(N, generator=g)
    qd, kd, vd, gad = q.cuda(), kc.cuda(), vc.cuda(), ga.cuda()
    attn = dict(attn_q=qd, attn_pos=pos, k_cache=kd, v_cache=vd, n_q_heads=Hq, n_kv_heads=KV, cache_len=CACHE_LEN)

    def fused(separate: bool):
        rd = _padded(r).cuda()
        od = torch.full_like(rd, float("nan")) if separate else rd
        ea, ssq = ops.x3_alloc(M, N), torch.zeros(M, N // 16).cuda()
        ops.linear3(None, wt, M, N, K, epilogue=E.EPI_RESID, resid=rd, out=od, emit_a=ea, gamma_a=gad, ssq_out=ssq, w_scale=scale, **attn)
        return od.cpu(), ops.x3_to_float(ea, M, N), ssq.cpu(), rd.cpu()

    out, emit, ssq, _ = fused(False)
    out_sep, emit_sep, ssq_sep, resid_after = fused(True)

    # the two launches it replaces: attn_short_kernel (X3 out) -> gemm3_kernel
    row_pos = torch.full((M,), pos, dtype=torch.int32).cuda()
    row_slot = torch.arange(M, dtype=torch.int32).cuda()
    ax3 = ops.x3_alloc(M, K)
    att2 = ops.attention(qd, kd, vd, row_pos, row_slot, Hq, out_x3=ax3)
    rd2 = _padded(r).cuda()
    ea2, ssq2 = ops.x3_alloc(M, N), torch.zeros(M, N // 16).cuda()
    ops.linear3(ax3, wt, M, N, K, epilogue=E.EPI_RESID, resid=rd2, out=rd2, emit_a=ea2, gamma_a=gad, ssq_out=ssq2, w_scale=scale)
    torch.cuda.synchronize()
    return dict(q=q, k_cache=kc, v_cache=vc, w=wref, resid=r, gamma=ga,
                out=out, emit=emit, ssq=ssq, out_sep=out_sep, emit_sep=emit_sep, ssq_sep=ssq_sep, resid_after=resid_after,
                att_two=att2.cpu(), out_two=rd2.cpu(), emit_two=ops.x3_to_float(ea2, M, N), ssq_two=ssq2.cpu())


def run_pick(E, ops, c: Case) -> dict:
    """PICK case: the head GEMM leaves its tile candidates, then the attention + wo launch picks each row's code, takes q | k | v
    from the table row and the residual from the embedding row, and writes the ids, the gap records and the new K / V cache rows."""
    g = _gen(c)
    M, Hq, KV, pos = c.M, c.Hq, c.KV, c.pos
    K = N = Hq * 64
    qd_, kd_ = Hq * 64, KV * 64
    Vc = (2048, 1040, 256)[(c.M + c.Hq + c.pos) % 3]  # codebook: 128 / 65 / 16 candidate tiles per row
    rows = Vc + EMB_OFF
    # head GEMM with equal columns inside and across tiles (the first one must win)
    Kh = 64
    xh = torch.randn(M, Kh, generator=g)
    wh = bf16r(torch.randn(Vc, Kh, generator=g) * 0.05)
    wh[7] = wh[3]
    wh[Vc - 1] = wh[Vc - 17]
    x3h, _, ssqh = ops.x3_pack(xh.cuda(), torch.ones(Kh).cuda())
    cand = torch.full((M, Vc // 16, 4), float("nan")).cuda()
    logits = ops.linear3(x3h, ops.pack_weight(wh), M, Vc, Kh, ssq_in=ssqh, cand_out=cand)

    table = torch.randn(rows, qd_ + 2 * kd_, generator=g)
    emb = torch.randn(rows, K, generator=g).to(torch.bfloat16)
    rope = rope_table()
    kc = torch.randn(M + 1, KV, CACHE_LEN, 64, generator=g)  # one slot more than rows: must stay as it is
    vc = torch.randn(M + 1, KV, CACHE_LEN, 64, generator=g)
    kc[:, :, pos:] = float("nan")  # key pos comes from the table: the cache entry there must not be read either
    vc[:, :, pos:] = float("nan")
    wt, scale, wref = _weights(ops, g, N, K, c.w8)
    ga = 1 + 0.1 * torch.randn(N, generator=g)
    margin = torch.rand(M, generator=g) * 0.3
    margin[::4] = float("inf")
    mask = (torch.randint(0, 3, (M,), generator=g) != 0).to(torch.int32)
    frames = torch.randint(0, 500, (M,), generator=g, dtype=torch.int32)

    kd, vd = kc.cuda(), vc.cuda()
    ids = torch.full((2 * M,), -7, dtype=torch.int32).cuda()  # stride 2: the odd entries stay
    md, mad = margin.cuda(), torch.full((M,), -1, dtype=torch.int32).cuda()
    pk = ops.Pick(cand=cand, table=table.cuda(), rope=rope.cuda(), emb=emb.cuda(), ids=ids, ids_stride=2, emb_row_offset=EMB_OFF,
                  margin=md, margin_mask=mask.cuda(), margin_at=mad, frames=frames.cuda(), step=pos)
    od = torch.full((M + PAD_ROWS, N + PAD_COLS), float("nan")).cuda()
    ea, ssq = ops.x3_alloc(M, N), torch.zeros(M, N // 16).cuda()
    ops.linear3(None, wt, M, N, K, epilogue=E.EPI_RESID, out=od, emit_a=ea, gamma_a=ga.cuda(), ssq_out=ssq, w_scale=scale,
                attn_pos=pos, k_cache=kd, v_cache=vd, n_q_heads=Hq, n_kv_heads=KV, cache_len=CACHE_LEN, pick=pk)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu(), table=table, emb=emb, rope=rope, k_cache=kc, v_cache=vc, w=wref, gamma=ga, margin_in=margin,
                mask=mask, frames=frames, out=od.cpu(), emit=ops.x3_to_float(ea, M, N), ssq=ssq.cpu(), ids=ids.cpu(),
                margin=md.cpu(), margin_at=mad.cpu(), k_cache_after=kd.cpu(), v_cache_after=vd.cpu())


def pick_reference(c: Case, d: dict) -> dict:
    """What the PICK launch must leave: ids = first argmax of the logits row, gap records as smoltts_k_argmax, cache row pos = the
    table row's K (RoPE at pos, fp32 arithmetic as rope_gathered4) / V, out = embedding row + attention @ wo^T (float64)."""
    M, Hq, KV, pos = c.M, c.Hq, c.KV, c.pos
    qd_, kd_ = Hq * 64, KV * 64
    lg = d["logits"]
    ids = lg.argmax(-1)
    top = lg.topk(2, dim=-1).values
    gap = top[:, 0] - top[:, 1]
    upd = (d["mask"] != 0) & (gap < d["margin_in"])
    e = ids + EMB_OFF
    trow = d["table"][e]
    cs = d["rope"][pos]
    q = rope_rows(trow[:, :qd_], cs)
    k_new = rope_rows(trow[:, qd_:qd_ + kd_], cs)
    kc, vc = d["k_cache"].clone(), d["v_cache"].clone()
    kc[:M, :, pos] = k_new.view(M, KV, 64)
    vc[:M, :, pos] = trow[:, qd_ + kd_:].reshape(M, KV, 64)
    att = attention_ref(q, kc[:M], vc[:M], pos, Hq)
    return dict(ids=ids.to(torch.int32), margin=torch.where(upd, gap, d["margin_in"]),
                margin_at=torch.where(upd, d["frames"] * 64 + pos, torch.full_like(d["frames"], -1)),
                k_cache=kc, v_cache=vc, out=d["emb"][e].float() + att.double().matmul(d["w"].double().T).float())


def save_evidence(path: Path, tensors: dict) -> Path:
    np.savez(path, **{k: v.numpy() for k, v in tensors.items()})
    return path


def differing(a: torch.Tensor, b: torch.Tensor, limit: int = 16) -> str:
    """The first differing (row, column) pairs of two [rows, cols] tensors, compared by bits."""
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    bad = (ai != bi).nonzero()
    diff = (a - b).abs()
    diff = diff[torch.isfinite(diff)]
    return (f"{len(bad)} of {a.numel()} differ; (row, column): {bad[:limit].tolist()}; "
            f"max |diff| {float(diff.max()) if diff.numel() else float('nan'):.3e}")


# ------------------------------------------------------------------------------------------------ the LDS-poison child
RESULT_KEYS = {False: ("out", "emit", "ssq", "out_sep", "resid_after", "att_two", "out_two", "emit_two", "ssq_two"),
               True: ("out", "emit", "ssq", "ids", "margin", "margin_at", "k_cache_after", "v_cache_after")}


def dump(out_path: str) -> None:
    """Every case of the matrix on the library that SMOLTTS_LIB names (or the product library): results into one .npz."""
    from smoltts_amd import engine as E
    from smoltts_amd import ops

    E.load_library()
    res = {}
    for i, c in enumerate(CASES):
        d = run_pick(E, ops, c) if c.pick else run_plain(E, ops, c)
        for k in RESULT_KEYS[c.pick]:
            res[f"{i:03d}_{k}"] = d[k].numpy()
    np.savez(out_path, **res)
    print(f"{len(CASES)} cases -> {out_path}", flush=True)


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    dump(sys.argv[1])
