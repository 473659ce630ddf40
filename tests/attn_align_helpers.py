"""``attn_align_kernel`` (csrc/attention.hip) held to float64: the cases, the two data regimes of ``attn_strict_helpers`` with the
dominant keys placed against a text window, the numpy references and the report.

Shared by tests/test_attn_align_gpu.py (the kernel against float64, judged by the fp32 reference's own noise) and
tests/test_attn_align_cpu.py (the premises of that bound).  Module-level and GPU-free at import.

What is computed, per row r (slot s, position pos) and query head h, over the slot's window [t0, t1):
    p = softmax_j (q_h . K[s, h // G, j] / 8),  j = 0 .. pos
    m = sum_{j in [t0, t1), j <= pos} p_j,   s1 = sum_{same j} p_j (j - t0)
A bf16 cache is built in fp32, rounded once, and both references run on the rounded values."""
from __future__ import annotations

import functools
import random
import zlib
from typing import NamedTuple, Optional

import numpy as np
import torch

from attn_strict_helpers import INSIDE, JUNK, OUTSIDE
from lm_strict_helpers import FACTOR, rms

LAYOUTS = ((4, 4), (4, 2), (9, 3), (8, 2))
DTYPES = ("f32", "bf16")
REGIMES = ("flat", "planted")
CACHE_LEN = 1040
POSITIONS = (0, 1, 15, 16, 63, 64, 65, 255, 256, 257, 1023, 1039)
MAX_FRAMES = 5
WINDOWS = ("first", "all", "clip", "beyond", "empty")
PLANTS = ("t0", "last", "before", "after", "pos1")  # where the planted regime puts a row's dominant key, one launch each
SENTINEL = -7.25  # what the output holds before a launch: a row that writes nothing keeps these bits
LDS_KEYS = 16368  # csrc/attention.hip ALIGN_LDS_KEYS: a longer cache takes the kernel's two-pass form


class Case(NamedTuple):
    name: str
    Hq: int
    Hkv: int
    cache_len: int
    dtype: str
    row_pos: tuple
    row_slot: tuple
    slots: int        # one more than the rows: no row reads the last one of the shuffled order

    @property
    def rows(self) -> int:
        return len(self.row_pos)

    def frame(self, r: int) -> int:
        return (3 * r + 1) % MAX_FRAMES


def make_case(name, Hq, Hkv, dtype, poss=POSITIONS, cache_len=CACHE_LEN) -> Case:
    order = list(range(len(poss) + 1))
    random.Random(zlib.crc32(name.encode())).shuffle(order)
    return Case(name, Hq, Hkv, cache_len, dtype, tuple(poss), tuple(order[:len(poss)]), len(poss) + 1)


CASES = [make_case(f"align-{hq}x{hkv}-{dt}", hq, hkv, dt) for hq, hkv in LAYOUTS for dt in DTYPES]
LONG_CASES = [make_case(f"align-long-{dt}", 2, 1, dt, (0, 100, LDS_KEYS + 31), LDS_KEYS + 32) for dt in DTYPES]


def window(kind: str, pos: int):
    """(t0, t1) of one row: the windows the kernel must get right at every position."""
    return {"first": (0, 1), "all": (0, pos + 1), "clip": (7, 307), "beyond": (pos + 1, pos + 6), "empty": (5, 5)}[kind]


def visible(t0: int, t1: int, pos: int):
    """[lo, hi): the window's keys among the visible ones 0 .. pos (hi <= lo: none)."""
    return max(t0, 0), min(t1, pos + 1)


def plant_position(kind: str, t0: int, t1: int, pos: int, cache_len: int) -> Optional[int]:
    """The key a dominant score goes to, or None where the case has no such key: ``t0`` and ``last`` (the window's first and last
    visible key, INSIDE above the rest; the same key under [0, 1)) need a row that sees two keys or more; ``before`` (t0 - 1) and ``after`` (t1) need that key
    to be visible -- it then takes the mass away from the window --; ``pos1`` is the first key the row must not see (under the
    window that begins there it would take all the mass)."""
    lo, hi = visible(t0, t1, pos)
    if kind == "t0":
        return lo if hi > lo and pos >= 1 else None
    if kind == "last":
        return hi - 1 if hi > lo and pos >= 1 else None
    if kind == "before":
        return t0 - 1 if hi > lo and 0 <= t0 - 1 else None
    if kind == "after":
        return t1 if hi > lo and t1 <= pos else None
    if kind == "pos1":
        return pos + 1 if pos + 1 < cache_len else None
    raise ValueError(kind)


def planted_head(c: Case, r: int) -> int:
    return (7 * r + 3) % c.Hq


class Data(NamedTuple):
    q: torch.Tensor        # fp32 [rows, Hq * 64]
    k: torch.Tensor        # fp32 [slots, Hkv, cache_len, 64] (bf16 caches: values that bf16 holds exactly)
    windows: np.ndarray    # int32 [slots, 2]
    planted: dict          # {row: key position} of the rows that carry a dominant key


def _fmt(c: Case, x: torch.Tensor) -> torch.Tensor:
    return x.bfloat16().float() if c.dtype == "bf16" else x


@functools.lru_cache(maxsize=4)
def _base(c: Case, regime: str):
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{regime}".encode()))
    a = 1.0 if regime == "flat" else 5.0 ** 0.5  # q.k / 8 ~ N(0, a^4)
    q = torch.randn(c.rows, c.Hq * 64, generator=g) * a
    k = _fmt(c, torch.randn(c.slots, c.Hkv, c.cache_len, 64, generator=g) * a)
    spare = (set(range(c.slots)) - set(c.row_slot)).pop()
    k[spare] = JUNK  # the slot no row reads
    return q, k


def make_data(c: Case, regime: str, win: str, plant: Optional[str] = None) -> Data:
    """The case's q and K with every row's window of kind ``win``; ``plant`` (planted regime): one dominant key per row, for the
    query head ``planted_head``: k = 8 t q / |q|^2, whose score against that head is t -- INSIDE above the row's largest other
    visible score for a key inside the window, OUTSIDE above it for a key outside."""
    q, k = _base(c, regime)
    G = c.Hq // c.Hkv
    windows = np.zeros((c.slots, 2), np.int32)
    planted = {}
    if plant is not None:
        assert regime == "planted"
        k = k.clone()
    for r in range(c.rows):
        pos, s = c.row_pos[r], c.row_slot[r]
        t0, t1 = window(win, pos)
        windows[s] = (t0, t1)
        j = plant_position(plant, t0, t1, pos, c.cache_len) if plant else None
        if j is None:
            continue
        head = planted_head(c, r)
        qv = q[r, head * 64:(head + 1) * 64].double()
        sc = k[s, head // G, :pos + 1].double() @ qv / 8.0
        if j <= pos and sc.numel() > 1:
            sc = torch.cat([sc[:j], sc[j + 1:]])
        t = float(sc.max()) + (INSIDE if plant in ("t0", "last") else OUTSIDE)
        k[s, head // G, j] = _fmt(c, (8.0 * t * qv / qv.dot(qv)).float())
        planted[r] = j
    return Data(q, k, windows, planted)


def reference(c: Case, d: Data, dtype, shift: int = 0, scale: float = 0.125) -> np.ndarray:
    """(m, s1) [rows, Hq, 2] in ``dtype`` numpy arithmetic.  The mutants: ``shift`` moves every window by that many keys, ``scale``
    replaces the 1 / 8."""
    G = c.Hq // c.Hkv
    q = d.q.numpy().astype(dtype).reshape(c.rows, c.Hq, 64)
    K = d.k.numpy().astype(dtype)
    out = np.zeros((c.rows, c.Hq, 2), dtype)
    for r in range(c.rows):
        pos, s = c.row_pos[r], c.row_slot[r]
        t0, t1 = (int(x) for x in d.windows[s])
        lo, hi = visible(t0 + shift, t1 + shift, pos)
        for h in range(c.Hq):
            sc = (K[s, h // G, :pos + 1] @ q[r, h]) * dtype(scale)
            e = np.exp(sc - sc.max())
            p = e / e.sum(dtype=dtype)
            if hi > lo:
                out[r, h, 0] = p[lo:hi].sum(dtype=dtype)
                out[r, h, 1] = (p[lo:hi] * (np.arange(lo, hi) - (t0 + shift)).astype(dtype)).sum(dtype=dtype)
    return out


def variants(regime: str) -> list:
    """(window kind, plant kind or None) of every launch of one (case, regime) test."""
    if regime == "flat":
        return [(w, None) for w in WINDOWS]
    # (no key lies in front of a window that begins at 0, none behind one that ends at pos + 1)
    return ([("first", p) for p in ("t0", "last", "after")] + [("all", p) for p in ("t0", "last", "pos1")]
            + [("clip", p) for p in ("t0", "last", "before", "after")] + [("beyond", "pos1"), ("empty", None)])


@functools.lru_cache(maxsize=64)
def references(c: Case, regime: str, win: str, plant: Optional[str]):
    """(data, fp32 reference, float64 reference) of one launch, computed once per process."""
    d = make_data(c, regime, win, plant)
    return d, reference(c, d, np.float32), reference(c, d, np.float64)


def judged_rows(c: Case) -> list:
    """Rows that see at least two keys: a row at position 0 has p = (1) exactly and is held to the exact value."""
    return [r for r in range(c.rows) if c.row_pos[r] >= 1]


class Pool:
    """Errors against float64 of the rows that see at least two keys, pooled over a test's launches per window kind and component
    (m | s1): E_ref = max|fp32 reference - float64| and R_ref (its RMS), the reference's own noise; required max|got - float64| <=
    factor E_ref and rms <= factor R_ref.  A component whose fp32 reference is exact everywhere ([0, 1): every j - t0 is 0) must be
    exact in ``got`` too."""

    def __init__(self):
        self.own, self.diff = {}, {}

    def add(self, key, got: np.ndarray, ref32: np.ndarray, ref64: np.ndarray, rows):
        for comp in (0, 1):
            self.own.setdefault((key, comp), []).append((ref32[rows, :, comp].astype(np.float64) - ref64[rows, :, comp]).ravel())
            self.diff.setdefault((key, comp), []).append((got[rows, :, comp].astype(np.float64) - ref64[rows, :, comp]).ravel())

    def report(self, name: str, factor: float = FACTOR):
        fails, worst, lines = [], 0.0, []
        for key in self.own:
            own, diff = np.concatenate(self.own[key]), np.concatenate(self.diff[key])
            e_ref, r_ref, e, rr = float(np.abs(own).max()), rms(own), float(np.abs(diff).max()), rms(diff)
            what = f"{name} window {key[0]} {'m' if key[1] == 0 else 's1'}"
            if e_ref == 0.0:
                lines.append(f"{what}: the fp32 reference is exact; max err {e:.3e}")
                if e != 0.0:
                    fails.append(f"{what}: the fp32 reference is exact, got differs by {e:.3e}")
                continue
            lines.append(f"{what}: max err {e:.3e} = {e / e_ref:.2f} x E_ref ({e_ref:.3e}), rms {rr:.3e} = {rr / r_ref:.2f} x R_ref ({r_ref:.3e})")
            worst = max(worst, e / e_ref, rr / r_ref)
            if e > factor * e_ref or rr > factor * r_ref:
                fails.append(lines[-1] + f", bound {factor:g}")
        return fails, worst, lines


def planted_checks(c: Case, d: Data, plant: str, vals: np.ndarray, ref64: np.ndarray, who: str) -> list:
    """The dominant keys of one launch against (m, s1) [rows, Hq, 2].  Inside the window (``t0``, ``last``): m > 0.999 and the
    centroid s1 / m within 1e-3 of the key.  The centroid of the exact distribution misses the key by d64 = sum_{j != key} p_j |j - key|
    / m, which a key 12 above the rest does not hold below 1e-3 in a window of hundreds of keys (measured in float64 on this data: 5.0e-3 at
    pos 255, 1.5e-2 at pos 1023, 1.9e-2 at pos 1039 under [0, pos + 1); 0.998e-3 at one row of [7, 307)).  So the centroid is held to within 1e-3 of the float64 centroid everywhere, and to within
    1e-3 of the key itself wherever the exact distribution leaves half of that tolerance (d64 <= 0.5e-3) -- the fp32 noise of s1 at
    these sizes is about 1e-4.  Outside the window (``before``, ``after``), and behind the visible keys where the window begins there
    (``pos1``): m < 1e-3; ``pos1`` under any other window is judged by the accuracy bound alone (the reference does not see it)."""
    fails = []
    for r, j in d.planted.items():
        t0 = int(d.windows[c.row_slot[r]][0])
        h = planted_head(c, r)
        m, s1 = (float(x) for x in vals[r, h])
        where = f"{who} {c.name} plant {plant} row {r} (pos {c.row_pos[r]}, window {tuple(int(x) for x in d.windows[c.row_slot[r]])}, key {j})"
        if plant in ("t0", "last"):
            c64 = float(ref64[r, h, 1] / ref64[r, h, 0])
            if not m > 0.999:
                fails.append(f"{where}: m = {m:.6f}, expected > 0.999")
            elif abs(s1 / m - c64) > 1e-3 or (abs(c64 - (j - t0)) <= 0.5e-3 and abs(s1 / m - (j - t0)) > 1e-3):
                fails.append(f"{where}: centroid {s1 / m:.6f}, expected {j - t0} within 1e-3 (float64: {c64:.6f})")
        elif plant == "pos1" and t0 != c.row_pos[r] + 1:
            continue
        elif not m < 1e-3:
            fails.append(f"{where}: m = {m:.6e}, expected < 1e-3")
    return fails


def run(ops, c: Case, d: Data, heads=None, mask=None, frames=None, out=None) -> torch.Tensor:
    """One launch on the GPU -> the output tensor [slots, MAX_FRAMES, heads, 2] on the CPU (prefilled with SENTINEL)."""
    heads = list(range(c.Hq)) if heads is None else heads
    dt = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    dev = lambda a: torch.tensor(a, dtype=torch.int32).cuda()
    if out is None:
        out = torch.full((c.slots, MAX_FRAMES, len(heads), 2), SENTINEL, dtype=torch.float32).cuda()
    frames = [c.frame(r) for r in range(c.rows)] if frames is None else frames
    mask = [1] * c.rows if mask is None else mask
    ops.attention_align(d.q.cuda(), d.k.to(dt).cuda(), dev(c.row_pos), dev(c.row_slot), dev(frames), dev(mask),
                        torch.from_numpy(d.windows).cuda(), heads, c.Hq, out)
    return out.cpu()


def gather(c: Case, out: torch.Tensor) -> np.ndarray:
    """[rows, heads, 2]: each row's entry at its slot and frame."""
    o = out.numpy()
    return np.stack([o[c.row_slot[r], c.frame(r)] for r in range(c.rows)])
