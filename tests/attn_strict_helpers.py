"""The attention kernels of csrc/attention.hip held to float64: the case list, a mirror of launch_attention's dispatch, the two data
regimes, the CPU references and the report.

Shared by tests/test_attn_strict_gpu.py (every launchable kernel form against float64, judged by the fp32 reference's own noise)
and tests/test_attn_strict_cpu.py (the premises of that bound on every case's data, and the mirror below against the
instantiations in the built code objects).  Module-level and GPU-free at import.

Two seeded data regimes per case:
  flat     q, k, v ~ N(0, 1): a nearly flat softmax, every key carries weight -- the regime that judges the arithmetic;
  planted  q and k scaled so that q.k / 8 has a standard deviation of about 5 (the running maximum moves from block to block, so
           every rescale and merge runs with factors far from 1), and on top of that one dominant key per row: k = 8 t q / |q|^2
           for one query head of the row, whose score against that head is exactly t and against every other query an ordinary one.
           Inside the visible range (the first key j_lo or the last key pos) t is 12 above the row's largest other score, so a
           dropped edge key changes the output by O(1); outside it (key j_lo - 1 where a window cuts, key pos + 1 where the cache
           goes on) t is 40 above, so an admitted key takes a softmax weight above 0.999.  Every cache entry that no row of the
           case may see gets V + 1e3.  Everything stays finite: the tile kernels multiply masked entries by a zero weight.
A bf16 cache is built in fp32, rounded to bf16 once, and both references run on the rounded values."""
from __future__ import annotations

import functools
import random
import zlib
from typing import NamedTuple

import numpy as np
import torch

from lm_strict_helpers import FACTOR, rms, two_pieces

REGIMES = ("flat", "planted")
INSIDE, OUTSIDE, JUNK = 12.0, 40.0, 1e3
ATT_SPLIT_MAX_PAIRS, ATT_SPLIT_MIN_KEYS = 128, 512  # csrc/common.h, csrc/attention.hip
DECODE_KERNELS = ("attn_short_kernel", "attn_kernel", "attn_split_kernel")  # a row that sees one key: exp(0) * v / 1, bit for bit


class Case(NamedTuple):
    name: str
    entry: str        # ops.attention | ops.attention_split | ops.attention_rows3
    Hq: int
    Hkv: int
    cache_len: int
    window: int
    dtype: str        # cache format: "f32" | "bf16"
    row_pos: tuple
    row_slot: tuple
    slots: int
    rps: int = 0      # attention_rows3: rows per slot
    products: int = 6  # attention_rows3: bf16x3 products per operand pair

    @property
    def rows(self) -> int:
        return len(self.row_pos)

    def span(self, r: int):
        """(j_lo, pos) of row r, or None for a row with nothing cached (pos outside the cache)."""
        p = self.row_pos[r]
        if p < 0 or p >= self.cache_len:
            return None
        return (p + 1 - self.window if self.window > 0 and p + 1 > self.window else 0), p


# ------------------------------------------------------------------------------------------------ the dispatch mirror
def instance(c: Case) -> tuple:
    """(kernel, template arguments, waves per workgroup) that launch_attention / launch_attention_rows3 launch for this case."""
    if c.entry == "attention_rows3":
        return ("attn_rows3_kernel", (2, 3 if c.products == 3 else 6), 4)
    G, kb = c.Hq // c.Hkv, c.dtype == "bf16"
    cap = (c.window if 0 < c.window < c.cache_len else c.cache_len) + 3 & ~3
    pairs = c.rows * c.Hkv
    nwaves = 4 if pairs >= 1024 or cap <= 64 else 16
    if c.cache_len <= 16:
        assert not kb
        return ("attn_short_kernel", (G, 2 if c.cache_len <= 8 else 4), 4)
    if pairs >= 1024:
        return ("attn_prefill_kernel", (1, kb), 4)
    can_split = c.entry == "attention_split" and pairs <= ATT_SPLIT_MAX_PAIRS and cap > 128 and nwaves == 16
    if kb or can_split:
        return ("attn_split_kernel", (G, kb, 2 if can_split else 1), nwaves)
    return ("attn_kernel", (G, False), nwaves)


def form(c: Case) -> tuple:
    return instance(c)[:2]


def launchable() -> set:
    """Every instantiation some accepted call can reach."""
    out = set()
    for G in (1, 2, 3, 4):
        out |= {("attn_short_kernel", (G, 2)), ("attn_short_kernel", (G, 4)), ("attn_kernel", (G, False)),
                ("attn_split_kernel", (G, False, 2)), ("attn_split_kernel", (G, True, 1)), ("attn_split_kernel", (G, True, 2))}
    out |= {("attn_prefill_kernel", (1, False)), ("attn_prefill_kernel", (1, True)), ("attn_rows3_kernel", (2, 6)), ("attn_rows3_kernel", (2, 3))}
    return out


def form_id(f: tuple) -> str:
    return f[0] + "<" + ",".join(str(a).lower() for a in f[1]) + ">"


# ------------------------------------------------------------------------------------------------ the cases
LAYOUT = {1: (4, 4), 2: (4, 2), 3: (9, 3), 4: (8, 2)}        # (query heads, kv heads) of the long-cache decode kernels
SHORT_LAYOUT = {1: (3, 3), 2: (4, 2), 3: (3, 1), 4: (4, 1)}  # 3 query heads: rows x heads is no multiple of 4 (a partial last workgroup)
L4 = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64)                                      # 4 waves x 4 lane groups: 16 keys per step
L16 = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025)         # 16 waves: 64 keys per step, 512 per pass
LSPLIT = (1, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1040)            # ATT_SPLIT_MIN_KEYS = 512 lies between cases
# packed utterances whose boundaries fall on every residue 1..15 of a 16-row tile: 128 rows
PACK128 = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 11, 15, 3, 21)
assert sorted({b % 16 for b in np.cumsum(PACK128)[:-1]}) == list(range(1, 16)) and sum(PACK128) == 128


def _decode(name, entry, G, cache_len, window, dtype, poss, layout=LAYOUT):
    """One row per slot, slots in a shuffled order, one slot more than rows (no row ever reads it)."""
    Hq, Hkv = layout[G]
    order = list(range(len(poss) + 1))
    random.Random(zlib.crc32(name.encode())).shuffle(order)
    return Case(name, entry, Hq, Hkv, cache_len, window, dtype, tuple(poss), tuple(order[:len(poss)]), len(poss) + 1)


def _packed(name, Hq, Hkv, window, dtype, lengths, cache_len=140, bad=()):
    """Utterances of the given lengths packed row after row in a shuffled slot order; utterance i sits at positions
    [start_i, start_i + length_i) of its slot, behind start_i keys that are already cached.  ``bad``: (row, pos) overrides."""
    rnd = random.Random(zlib.crc32(name.encode()))
    order = list(range(len(lengths) + 1))
    rnd.shuffle(order)
    pos, slot = [], []
    for i, n in enumerate(lengths):
        start = 0 if i % 3 == 0 else rnd.randrange(0, cache_len - n + 1)
        pos += list(range(start, start + n))
        slot += [order[i]] * n
    for r, p in bad:
        pos[r] = p
    return Case(name, "attention", Hq, Hkv, cache_len, window, dtype, tuple(pos), tuple(slot), len(lengths) + 1)


def _rows3(name, slots, heads, rps, cache_len, starts, window, products):
    pos = [s + i for s in starts for i in range(rps)]
    slot = [s for s in range(slots) for _ in range(rps)]
    return Case(name, "attention_rows3", heads, heads, cache_len, window, "f32", tuple(pos), tuple(slot), slots, rps, products)


def cases() -> list:
    out = []
    for G in (1, 2, 3, 4):
        # attn_short_kernel<G, UN>: every position of the cache, window 0 and a window below cache_len
        for cl, win in ((8, 0), (8, 5), (16, 0), (16, 11)):
            out.append(_decode(f"short-g{G}-c{cl}-w{win}", "attention", G, cl, win, "f32", list(range(cl)) + [cl // 2], SHORT_LAYOUT))
        bad = G == 2  # the G = 2 cases over the whole long cache also hold rows with nothing cached (pos = -1, pos = cache_len)
        for dtype, tag in (("f32", "attn"), ("bf16", "bf16")):
            # attn_kernel<G, false> / attn_split_kernel<G, true, 1>, through ops.attention: 4 and 16 waves
            def dec(name, cl, win, poss):
                out.append(_decode(f"{tag}-g{G}-{name}", "attention", G, cl, win, dtype, poss + (bad and name == "16w") * [-1, cl]))
            dec("4w", 64, 0, [L - 1 for L in L4])
            dec("4w-win40", 100, 40, [0, 38, 39, 40, 41, 70, 99])
            dec("16w", 1040, 0, [L - 1 for L in L16])
            dec("16w-win300", 1040, 300, [100, 298, 299, 300, 301, 700, 1039])
            if dtype == "bf16":
                dec("4w-c17", 17, 0, [0, 1, 4, 15, 16])
            # attn_split_kernel<G, KB, 2>, through ops.attention_split
            def spl(name, win, poss):
                out.append(_decode(f"split-{tag}-g{G}-{name}", "attention_split", G, 1040, win, dtype, poss + (bad and name == "w0") * [-1, 1040]))
            spl("w0", 0, [L - 1 for L in LSPLIT])
            spl("win250", 250, [100, 249, 250, 251, 511, 700, 1039])                   # never shared
            spl("win600", 600, [300, 510, 511, 512, 598, 599, 600, 601, 1039])          # shared from 512 keys on, j_lo > 0 from 600 on
    for dtype in ("f32", "bf16"):
        # attn_prefill_kernel<1, KB>: rows x kv heads >= 1024 with the fewest rows
        out.append(_packed(f"prefill-{dtype}-8x8-w0", 8, 8, 0, dtype, PACK128, bad=((7, -1), (100, 140))))
        out.append(_packed(f"prefill-{dtype}-8x2-w7", 8, 2, 7, dtype, PACK128 + (130, 95, 67, 64, 28)))
        out.append(_packed(f"prefill-{dtype}-9x3-w50", 9, 3, 50, dtype, PACK128 + (130, 67, 27)))
    for products in (6, 3):
        for i, (slots, heads, rps, cl, starts, win) in enumerate([(3, 8, 64, 200, (0, 37, 130), 0), (2, 3, 32, 131, (5, 99), 0),
                                                                  (2, 8, 64, 300, (200, 17), 50), (1, 8, 96, 96, (0,), 0)]):
            out.append(_rows3(f"rows3-np{products}-{i}", slots, heads, rps, cl, starts, win, products))
    return out


CASES = cases()
BY_FORM = {}
for _c in CASES:
    BY_FORM.setdefault(form(_c), []).append(_c)


# ------------------------------------------------------------------------------------------------ data
class Plant(NamedTuple):
    row: int
    head: int   # query head that sees the key as dominant
    kind: str   # first | last (inside the visible range), before | after (outside it)
    j: int      # the key's position in the row's slot


class Data(NamedTuple):
    q: torch.Tensor   # fp32 [rows, Hq * 64]
    k: torch.Tensor   # fp32 [slots, Hkv, cache_len, 64] (bf16 caches: values that bf16 holds exactly)
    v: torch.Tensor
    plants: tuple


def _fmt(c: Case, x: torch.Tensor) -> torch.Tensor:
    return x.bfloat16().float() if c.dtype == "bf16" else x


@functools.lru_cache(maxsize=8)
def make_data(c: Case, regime: str) -> Data:
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{regime}".encode()))
    a = 1.0 if regime == "flat" else 5.0 ** 0.5  # q.k / 8 ~ N(0, a^4)
    q = torch.randn(c.rows, c.Hq * 64, generator=g) * a
    k = _fmt(c, torch.randn(c.slots, c.Hkv, c.cache_len, 64, generator=g) * a)
    v = torch.randn(c.slots, c.Hkv, c.cache_len, 64, generator=g)
    plants = []
    if regime == "planted":
        G = c.Hq // c.Hkv
        used = set()
        for r in range(c.rows):
            sp = c.span(r)
            if sp is None:
                continue
            lo, pos = sp
            s, head = c.row_slot[r], (7 * r + 3) % c.Hq
            where = {"first": lo if pos > lo else None, "last": pos if pos > lo else None, "before": lo - 1 if lo > 0 else None,
                     "after": pos + 1 if pos + 1 < c.cache_len else None}
            kinds = ("first", "after", "last", "before")
            for kind in kinds[r % 4:] + kinds[:r % 4]:
                j = where[kind]
                if j is None or (s, head // G, j) in used:
                    continue
                qv = q[r, head * 64:(head + 1) * 64].double()
                sc = k[s, head // G, lo:pos + 1].double() @ qv / 8.0
                if lo <= j <= pos and sc.numel() > 1:
                    sc = torch.cat([sc[:j - lo], sc[j - lo + 1:]])
                t = float(sc.max()) + (INSIDE if lo <= j <= pos else OUTSIDE)
                k[s, head // G, j] = _fmt(c, (8.0 * t * qv / qv.dot(qv)).float())
                used.add((s, head // G, j))
                plants.append(Plant(r, head, kind, j))
                break
        seen = torch.zeros(c.slots, c.cache_len, dtype=torch.bool)
        for r in range(c.rows):
            sp = c.span(r)
            if sp is not None:
                seen[c.row_slot[r], sp[0]:sp[1] + 1] = True
        v = v + JUNK * (~seen)[:, None, :, None]
    return Data(q, k, _fmt(c, v), tuple(plants))


# ------------------------------------------------------------------------------------------------ references (CPU)
def reference(c: Case, d: Data, dtype, spans=None, cut: bool = False) -> torch.Tensor:
    """softmax(q K^T / 8) V over keys [j_lo, pos] of the row's slot in ``dtype`` arithmetic, GQA by repeat_interleave; rows with
    nothing cached give zero rows.  ``spans`` {row: (lo, hi)} overrides a row's keys (the masking mutants).  ``cut``: the 2^-16-grade
    mutant -- K and V cut to two bf16 pieces; a bf16 cache holds one piece per value, so there q and the softmax weights are cut."""
    G = c.Hq // c.Hkv
    q, K, V = d.q, d.k, d.v
    cut_p = cut and c.dtype == "bf16"
    if cut:
        q, K, V = (two_pieces(q), K, V) if cut_p else (q, two_pieces(K), two_pieces(V))
    q, K, V = q.to(dtype).view(c.rows, c.Hq, 64), K.to(dtype), V.to(dtype)
    out = torch.zeros(c.rows, c.Hq * 64, dtype=dtype)
    for r in range(c.rows):
        sp = c.span(r)
        if sp is None:
            continue
        lo, hi = (spans or {}).get(r, sp)
        s = c.row_slot[r]
        Kr = K[s, :, lo:hi + 1].repeat_interleave(G, dim=0)  # [Hq, L, 64]
        Vr = V[s, :, lo:hi + 1].repeat_interleave(G, dim=0)
        w = torch.softmax(torch.einsum("hd,hjd->hj", q[r], Kr) / 8.0, dim=-1)
        if cut_p:
            w = two_pieces(w.float()).to(dtype)
        out[r] = torch.einsum("hj,hjd->hd", w, Vr).reshape(-1)
    return out


def _pieces(x: torch.Tensor):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def rows3_three_product_model(c: Case, d: Data, dtype, spans=None) -> torch.Tensor:
    """What attn_rows3_kernel<2, 3> computes, in ``dtype`` arithmetic: every operand of both products cut to its hi + mid bf16 pieces
    and the mid * mid product dropped (mfma_b3<3>).  The probabilities are an operand: the kernel cuts exp(s - m) with m the running
    maximum of its wave at that 32-key block (wave w of a 32-row workgroup takes blocks lo / 32 + w, + 4, ..), sums the uncut ones
    for the denominator, and merges the four waves at the end -- so the model follows that schedule.  ``spans``: as ``reference``."""
    assert c.entry == "attention_rows3" and c.rows % 32 == 0
    qh, qm = _pieces(d.q * 0.125)
    kh, km = _pieces(d.k)
    vh, vm = _pieces(d.v)
    qh, qm, kh, km, vh, vm = (t.to(dtype) for t in (qh, qm, kh, km, vh, vm))
    out = torch.zeros(c.rows, c.Hq * 64, dtype=dtype)
    ninf = float("-inf")
    override = spans or {}
    for r0 in range(0, c.rows, 32):
        spans = [override.get(r, c.span(r)) for r in range(r0, r0 + 32)]
        if all(sp is None for sp in spans):
            continue
        slot = c.row_slot[r0]
        lo = min(sp[0] for sp in spans if sp)
        hi = max(sp[1] for sp in spans if sp)
        b0, b1 = lo >> 5, hi >> 5
        n = (b1 + 1) * 32
        j = torch.arange(n)
        vis = torch.stack([(j >= sp[0]) & (j <= sp[1]) if sp else torch.zeros(n, dtype=torch.bool) for sp in spans])  # [32, n]
        pad = n - c.cache_len
        for h in range(c.Hq):
            def padded(t):
                t = t[slot, h]
                return torch.cat([t, torch.zeros(pad, 64, dtype=dtype)]) if pad > 0 else t[:n]
            Kh, Km, Vh, Vm = padded(kh), padded(km), padded(vh), padded(vm)
            Qh, Qm = qh[r0:r0 + 32, h * 64:(h + 1) * 64], qm[r0:r0 + 32, h * 64:(h + 1) * 64]
            S = Qh @ Kh.T + Qm @ Kh.T + Qh @ Km.T
            S = torch.where(vis, S, torch.full_like(S, ninf))
            ms, ls, Os = [], [], []
            for w in range(4):
                blocks = list(range(b0 + w, b1 + 1, 4))
                m = torch.full((32,), ninf, dtype=dtype)
                l = torch.zeros(32, dtype=dtype)
                O = torch.zeros(32, 64, dtype=dtype)
                for b in blocks:
                    sb = S[:, b * 32:(b + 1) * 32]
                    mn = torch.maximum(m, sb.max(dim=1).values)
                    live = mn > ninf
                    safe = torch.where(live, mn, torch.zeros_like(mn))
                    rs = torch.where(live, torch.exp(m - safe), torch.ones_like(mn))
                    p = torch.where(live[:, None], torch.exp(sb - safe[:, None]), torch.zeros_like(sb))
                    ph = p.bfloat16().to(dtype)
                    pm = (p - ph).bfloat16().to(dtype)
                    l = l * rs + p.sum(dim=1)
                    O = O * rs[:, None] + (ph @ Vh[b * 32:(b + 1) * 32] + pm @ Vh[b * 32:(b + 1) * 32] + ph @ Vm[b * 32:(b + 1) * 32])
                    m = mn
                ms.append(m), ls.append(l), Os.append(O)
            gm = torch.stack(ms).max(dim=0).values
            safe = torch.where(gm > ninf, gm, torch.zeros_like(gm))
            L = torch.zeros(32, dtype=dtype)
            O = torch.zeros(32, 64, dtype=dtype)
            for m, l, o in zip(ms, ls, Os):
                f = torch.where(m > ninf, torch.exp(m - safe), torch.zeros_like(m))
                L, O = L + l * f, O + o * f[:, None]
            ok = L > 0
            out[r0:r0 + 32, h * 64:(h + 1) * 64] = torch.where(ok[:, None], O / torch.where(ok, L, torch.ones_like(L))[:, None], torch.zeros_like(O))
    return out


@functools.lru_cache(maxsize=8)
def references(c: Case, regime: str):
    """(fp32 reference, float64 reference) of the case's data, computed once; attn_rows3_kernel<2, 3> is judged against its own model."""
    d = make_data(c, regime)
    fn = rows3_three_product_model if c.products == 3 else reference
    return fn(c, d, torch.float32), fn(c, d, torch.float64)


def admit_spans(c: Case, d: Data) -> dict:
    """The mutant that admits each row's planted outside key (j_lo - 1 or pos + 1)."""
    out = {}
    for p in d.plants:
        lo, pos = c.span(p.row)
        if p.kind == "before":
            out[p.row] = (lo - 1, pos)
        elif p.kind == "after":
            out[p.row] = (lo, pos + 1)
    return out


def drop_spans(c: Case, d: Data) -> dict:
    """The mutant that drops each row's planted inside edge key (j_lo or pos)."""
    out = {}
    for p in d.plants:
        lo, pos = c.span(p.row)
        if p.kind == "first":
            out[p.row] = (lo + 1, pos)
        elif p.kind == "last":
            out[p.row] = (lo, pos - 1)
    return out


# ------------------------------------------------------------------------------------------------ the report
def strict_report(got: torch.Tensor, ref32: torch.Tensor, ref64: torch.Tensor, c: Case, regime: str, factor: float = FACTOR):
    """``got`` [rows, Hq * 64] against the float64 reference.  Pooled over every row that sees at least two keys:
    E_ref = max|ref32 - ref64| and R_ref (the RMS of the same difference), the reference's own noise; required
    max|got - ref64| <= factor E_ref and rms(got - ref64) <= factor R_ref.  A row that sees exactly one key must equal that V row bit
    for bit in the per-row kernels (exp(0) v / 1) and stay within factor E_ref in the tile kernels; a row with nothing cached must
    be zero.  Returns (failure messages, (max ratio, rms ratio))."""
    kernel, targs, _ = instance(c)
    name = f"{form_id((kernel, targs))} {c.name} {regime}"
    assert got.shape == ref32.shape == ref64.shape and ref64.dtype == torch.float64, (got.shape, ref32.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    spans = [c.span(r) for r in range(c.rows)]
    many = torch.tensor([sp is not None and sp[1] > sp[0] for sp in spans])
    one = [r for r, sp in enumerate(spans) if sp is not None and sp[1] == sp[0]]
    none = [r for r, sp in enumerate(spans) if sp is None]
    g64 = got.double()
    own = (ref32.double() - ref64)[many]
    diff = (g64 - ref64)[many]
    e_ref, r_ref = float(own.abs().max()), rms(own.numpy())
    assert e_ref > 0.0, name
    idx = many.nonzero().flatten()
    i, col = divmod(int(diff.abs().argmax()), diff.shape[1])
    r = int(idx[i])
    e, rr = float(diff.abs().max()), rms(diff.numpy())
    fails = []

    def place(r, col):
        lo, pos = spans[r]
        return (f"row {r} (slot {c.row_slot[r]}, pos {pos}, j_lo {lo}), query head {col // 64}, dim {col % 64}: got {float(got[r, col]):.9g}, "
                f"float64 {float(ref64[r, col]):.9g}")

    if e > factor * e_ref or rr > factor * r_ref:
        fails.append(f"{name}: max err {e:.3e} = {e / e_ref:.2f} x E_ref ({e_ref:.3e}), rms {rr:.3e} = {rr / r_ref:.2f} x R_ref ({r_ref:.3e}) "
                     f"over {int(many.sum())} rows, bound {factor:g}; worst at {place(r, col)}")
    for r in one:
        if kernel in DECODE_KERNELS:
            if not torch.equal(got[r], ref64[r].float()):
                col = int((got[r] != ref64[r].float()).nonzero()[0])
                fails.append(f"{name}: a row that sees one key is not that V row bit for bit: {place(r, col)}")
        else:
            e1 = (g64[r] - ref64[r]).abs()
            if float(e1.max()) > factor * e_ref:
                fails.append(f"{name}: a row that sees one key: err {float(e1.max()):.3e} = {float(e1.max()) / e_ref:.2f} x E_ref ({e_ref:.3e}), "
                             f"bound {factor:g}; at {place(r, int(e1.argmax()))}")
    for r in none:
        if float(got[r].abs().max()) != 0.0:
            fails.append(f"{name}: row {r} (pos {c.row_pos[r]}: nothing cached) is not zero: max |got| {float(got[r].abs().max()):.3e}")
    return fails, (e / e_ref, rr / r_ref)


# ------------------------------------------------------------------------------------------------ runs (GPU)
def run_case(ops, c: Case, d: Data, scratch=None) -> torch.Tensor:
    """The case's launch on the GPU -> fp32 rows on the CPU.  The entries with an X3 output run twice, without and with it: the
    fp32 rows must not depend on it, and the X3 operand must hold the same numbers."""
    pos = torch.tensor(c.row_pos, dtype=torch.int32).cuda()
    slot = torch.tensor(c.row_slot, dtype=torch.int32).cuda()
    qd = d.q.cuda()
    if c.entry == "attention_rows3":
        k3, v3 = ops.kv3_encode(d.k, False).cuda(), ops.kv3_encode(d.v, True).cuda()
        return ops.attention_rows3(qd, k3, v3, pos, slot, c.rps, c.Hq, c.cache_len, c.window, b3_products=c.products).cpu()
    dt = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    kd, vd = d.k.to(dt).cuda(), d.v.to(dt).cuda()

    def launch(x3):
        if c.entry == "attention_split":
            return ops.attention_split(qd, kd, vd, pos, slot, c.Hq, scratch, c.window, out_x3=x3).cpu()
        return ops.attention(qd, kd, vd, pos, slot, c.Hq, c.window, out_x3=x3).cpu()

    plain = launch(None)
    x3 = ops.x3_alloc(c.rows, c.Hq * 64)
    out = launch(x3)
    assert torch.equal(plain.view(torch.int32), out.view(torch.int32)), f"{c.name}: the fp32 rows depend on the X3 output"
    assert torch.equal(ops.x3_to_float(x3, c.rows, c.Hq * 64), out), f"{c.name}: the X3 operand differs from the fp32 rows"
    return out
