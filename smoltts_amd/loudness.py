"""Loudness normalisation of 24 kHz mono speech by the ITU-R BS.1770-4 meter: the numpy model that defines what
``csrc/loudness.hip`` computes.  The device reproduces it bit for bit: every fp64 operation below is a
single rounded multiply, add or divide in a fixed order, gains come from tables computed here once and uploaded, and nothing
depends on how calls cut the stream.

The meter: K-weighting (a high shelf, then a high pass, both as transposed direct form II biquads in fp64), hop energies over
``HOP`` samples, blocks of four hops, the absolute gate at -70 LUFS and the relative gate 10 LU under the mean of what passes it.
The filter runs in sub-blocks of ``SUB`` samples on the stream's own grid: each is filtered from a zero state, the true states are
carried from sub-block to sub-block with the ``SUB``-step transition matrix, and each is then filtered again from its true start
state, which is where its energy comes from.

Blocking rule (``normalize``): one gain min(10^((target - L) / 20), c / peak) from the whole utterance's gated loudness L.
Stream rule (``StreamState``): a piecewise-linear gain with knots at hop boundaries on a grid of 1 / ``GRID`` dB; both knots of a
hop are fixed from the samples in front of it, so every sample leaves as it arrives.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

FS = 24000
HOP = 2400            # 100 ms
SUB = 240             # filter sub-block (divides HOP)
BLOCK_HOPS = 4        # a block is 400 ms, 75 % overlap
RING = 512            # blocks the stream rule looks back over
GRID = 64             # knot steps per dB
RANGE_DB = 20         # knots stay within +- this
K_MAX = RANGE_DB * GRID
SLEW_STEPS = GRID // 2    # 0.5 dB per hop = 5 dB/s
CEILING_DB = -1.0         # c: no knot (and no static gain) takes the known peak above this
GATE_ABS_LUFS = -70.0
GATE_REL = 0.1            # -10 LU as a power ratio
OFFSET = -0.691
TARGET_MIN, TARGET_MAX = -40.0, -5.0
LANES = 256               # width of the fixed summation tree

# the analogue prototype of BS.1770's two filters (the fit whose bilinear transform at 48 kHz is the standard's table)
_SHELF = (3.999843853973347, 0.7071752369554196, 1681.974450955533)   # gain dB, Q, fc
_SHELF_VB_EXP = 0.4996667741545416
_HIGHPASS = (0.5003270373238773, 38.13547087602444)                  # Q, fc


def k_weighting(fs: float = FS):
    """(shelf b, shelf a, high-pass b, high-pass a) at ``fs``, a[0] = 1."""
    g, q, fc = _SHELF
    k = np.tan(np.pi * fc / fs)
    vh = 10.0 ** (g / 20.0)
    vb = vh ** _SHELF_VB_EXP
    a0 = 1.0 + k / q + k * k
    sb = np.array([(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0])
    sa = np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0])
    q, fc = _HIGHPASS
    k = np.tan(np.pi * fc / fs)
    a0 = 1.0 + k / q + k * k
    return sb, sa, np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0])


def check_target(loudness, what: str = "loudness") -> Optional[float]:
    """``loudness`` as a float target in LUFS, None when off; ``ValueError`` outside [-40, -5]."""
    if loudness is None:
        return None
    if isinstance(loudness, bool) or not isinstance(loudness, (int, float)) or not np.isfinite(loudness):
        raise ValueError(f"{what} must be a number of LUFS between {TARGET_MIN:g} and {TARGET_MAX:g}, or null")
    if not TARGET_MIN <= loudness <= TARGET_MAX:
        raise ValueError(f"{what} {loudness:g} outside [{TARGET_MIN:g}, {TARGET_MAX:g}] LUFS")
    return float(loudness)


def check_start_gain(db) -> float:
    """A stream's first knot in dB (None: 0), rounded to the knot grid; ``ValueError`` outside +-20 dB."""
    if db is None:
        return 0.0
    if isinstance(db, bool) or not isinstance(db, (int, float)) or not np.isfinite(db) or abs(db) > RANGE_DB:
        raise ValueError(f"loudness_start_gain_db must be a number within +-{RANGE_DB} dB")
    return knot_of_db(db) / GRID


def knot_of_db(db: float) -> int:
    return int(np.clip(np.rint(float(db) * GRID), -K_MAX, K_MAX))


def _step(c, x, s1, s2, s3, s4):
    """One sample through both biquads: (y, new states).  Each line is one rounding per operator, left to right."""
    y1 = c[0] * x + s1
    n1 = (c[1] * x - c[3] * y1) + s2
    n2 = c[2] * x - c[4] * y1
    y2 = c[5] * y1 + s3
    n3 = (c[6] * y1 - c[8] * y2) + s4
    n4 = c[7] * y1 - c[9] * y2
    return y2, n1, n2, n3, n4


class Tables:
    """What the device is given: ``coef`` (shelf b0 b1 b2 a1 a2, high pass b0 b1 b2 a1 a2), ``trans`` (the SUB-step transition
    matrix, row-major), the absolute gate as a mean square, the ceiling c, and the knots' linear gains and their squares."""

    def __init__(self):
        sb, sa, hb, ha = k_weighting(FS)
        self.coef = np.array([sb[0], sb[1], sb[2], sa[1], sa[2], hb[0], hb[1], hb[2], ha[1], ha[2]], np.float64)
        # column k of the transition matrix: SUB zero samples from the unit state e_k
        s = [np.eye(4)[i].copy() for i in range(4)]
        zero = np.zeros(4)
        for _ in range(SUB):
            _, *s = _step(self.coef, zero, *s)
        self.trans = np.ascontiguousarray(np.stack(s))  # [row, column]
        self.gate_abs = float(10.0 ** ((GATE_ABS_LUFS - OFFSET) / 10.0))
        self.ceiling = float(10.0 ** (CEILING_DB / 20.0))
        k = np.arange(-K_MAX, K_MAX + 1, dtype=np.float64)
        self.gain = 10.0 ** (k / (20.0 * GRID))
        self.gain2 = self.gain * self.gain
        assert np.all(np.diff(self.gain) > 0) and np.all(np.diff(self.gain2) > 0)

    def packed(self) -> np.ndarray:
        """The fp64 array ``smoltts_loudness_create`` takes."""
        return np.concatenate([self.coef, self.trans.reshape(-1), [self.gate_abs, self.ceiling], self.gain, self.gain2])


@lru_cache(maxsize=1)
def tables() -> Tables:
    return Tables()


def target_power(target: float) -> float:
    """The mean square of K-weighted signal that reads ``target`` LUFS."""
    return float(10.0 ** ((float(target) - OFFSET) / 10.0))


def lufs_of_power(p: float) -> float:
    return float(OFFSET + 10.0 * np.log10(p)) if p > 0 else float("-inf")


def _tree(v: np.ndarray):
    """The fixed-order sum: element t of each run of LANES is added, run after run, into lane t; the lanes are then summed as
    a binary tree of neighbours."""
    n = -(-max(v.size, 1) // LANES) * LANES
    w = np.zeros(n, v.dtype)
    w[:v.size] = v
    w = w.reshape(-1, LANES)
    acc = np.zeros(LANES, v.dtype)
    for row in w:
        acc = acc + row
    while acc.size > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def gated_power(z: np.ndarray) -> Tuple[float, int, int]:
    """(mean power of the blocks ``z`` that pass both gates, how many pass the absolute gate, how many pass both); power 0
    when none passes."""
    t = tables()
    z = np.asarray(z, np.float64)
    a = z > t.gate_abs
    n1 = int(_tree(a.astype(np.int64)))
    if n1 == 0:
        return 0.0, 0, 0
    rel = (_tree(np.where(a, z, 0.0)) / np.float64(n1)) * GATE_REL
    b = a & (z > rel)
    n2 = int(_tree(b.astype(np.int64)))
    return float(_tree(np.where(b, z, 0.0)) / np.float64(n2)), n1, n2


class _Filter:
    """The K-weighting filter's state on the sub-block grid, and the energy of the open sub-block."""

    def __init__(self):
        self.pos = 0
        self.s_start = np.zeros(4)  # the true state at the open sub-block's start
        self.s_run = np.zeros(4)    # the state at pos of the pass from s_start
        self.z_run = np.zeros(4)    # the state at pos of the pass from zero
        self.e_sub = 0.0            # sum of y^2 over the open sub-block so far

    def run(self, x: np.ndarray):
        """Consume ``x`` (float32, not empty): -> per piece (a sub-block's part inside the call) its energy, its peak, its
        length and whether it completes its sub-block.  An incomplete last piece's energy is the open sub-block's so far."""
        t = tables()
        c = t.coef
        n = int(x.size)
        r = self.pos % SUB
        first = min(n, SUB - r)
        bounds = np.unique(np.asarray([0, first] + list(range(first + SUB, n, SUB)) + [n], np.int64))
        off, ln = bounds[:-1], np.diff(bounds)
        npc = off.size
        xd = x.astype(np.float64)
        X = np.zeros((npc, SUB))
        A = np.abs(x)
        pk = np.zeros(npc, np.float32)
        for i in range(npc):
            X[i, :ln[i]] = xd[off[i]: off[i] + ln[i]]
            pk[i] = np.fmax.reduce(A[off[i]: off[i] + ln[i]], initial=np.float32(0))
        steps = int(ln.max())
        ragged = not np.all(ln == steps)

        def run_pass(s, e0):
            e = np.zeros(npc)
            e[0] = e0
            for j in range(steps):
                y, *new = _step(c, X[:, j], *s)
                e_new = e + y * y
                if ragged:
                    live = j < ln
                    s = [np.where(live, a, b) for a, b in zip(new, s)]
                    e = np.where(live, e_new, e)
                else:
                    s, e = new, e_new
            return s, e

        # pass 1: from zero (the first piece goes on from the open sub-block's zero-state pass)
        z = [np.zeros(npc) for _ in range(4)]
        if r:
            for k in range(4):
                z[k][0] = self.z_run[k]
        z, _ = run_pass(z, 0.0)
        done = (np.cumsum(ln) + self.pos) % SUB == 0  # the piece ends on the grid
        # the true start states, carried piece by piece
        start = np.zeros((npc + 1, 4))
        start[0] = self.s_start
        M = t.trans
        for i in range(npc):
            if done[i]:
                s0 = start[i]
                for k in range(4):
                    start[i + 1, k] = (((M[k, 0] * s0[0] + M[k, 1] * s0[1]) + M[k, 2] * s0[2]) + M[k, 3] * s0[3]) + z[k][i]
        # pass 2: from the true states
        s = [start[:npc, k].copy() for k in range(4)]
        if r:
            for k in range(4):
                s[k][0] = self.s_run[k]
        s, e = run_pass(s, self.e_sub if r else 0.0)
        self.pos += n
        if done[-1]:
            self.s_start = start[npc].copy()
            self.s_run = self.s_start.copy()
            self.z_run = np.zeros(4)
            self.e_sub = 0.0
        else:
            self.s_start = start[npc - 1].copy()
            self.s_run = np.array([s[k][-1] for k in range(4)])
            self.z_run = np.array([z[k][-1] for k in range(4)])
            self.e_sub = float(e[-1])
        return e, pk, ln, done


def _block(h0, h1, h2, h3):
    return (((h0 + h1) + h2) + h3) / np.float64(BLOCK_HOPS * HOP)


def hop_energies(x: np.ndarray) -> Tuple[np.ndarray, float]:
    """(energy of every complete hop of the utterance ``x``, max |x|)."""
    x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
    if x.size == 0:
        return np.zeros(0), 0.0
    e, pk, _, _ = _Filter().run(x)
    per = HOP // SUB
    nh = x.size // HOP
    hops = np.zeros(nh)
    for h in range(nh):
        acc = np.float64(0.0)
        for i in range(h * per, (h + 1) * per):
            acc = acc + e[i]
        hops[h] = acc
    return hops, float(np.fmax.reduce(pk, initial=np.float32(0)))


def measure_power(x: np.ndarray) -> Tuple[float, float]:
    """(gated mean power of the whole utterance, 0 when no block passes the absolute gate or it is shorter than a block; peak)."""
    hops, peak = hop_energies(x)
    if hops.size < BLOCK_HOPS:
        return 0.0, peak
    z = np.array([_block(*hops[j: j + BLOCK_HOPS]) for j in range(hops.size - BLOCK_HOPS + 1)])
    return gated_power(z)[0], peak


def measure(x: np.ndarray) -> Tuple[float, float]:
    """(integrated loudness in LUFS, -inf when nothing is measured; peak) of a whole utterance."""
    p, peak = measure_power(x)
    return lufs_of_power(p), peak


def static_gain(target: float, power: float, peak: float, cap: bool = True) -> float:
    """The blocking rule's gain from a measured power and peak (1 when nothing was measured).  ``cap`` false: the gain that
    reaches the target whatever the peak, for an utterance that a peak limiter (limiter.py) finishes."""
    if not power > 0:
        return 1.0
    g = float(10.0 ** ((float(target) - lufs_of_power(power)) / 20.0))
    return min(g, tables().ceiling / peak) if cap and peak > 0 else g


def apply_gain(x: np.ndarray, g: float) -> np.ndarray:
    return (np.asarray(x, np.float32).astype(np.float64) * np.float64(g)).astype(np.float32)


def normalize(x: np.ndarray, target: float, cap: bool = True) -> Tuple[np.ndarray, float]:
    """The blocking rule: (the utterance at ``target`` LUFS or at peak c, the gain applied).  Silence and utterances shorter
    than a block come back unchanged (gain 1).  ``cap`` false: at ``target`` whatever the peak (``static_gain``)."""
    x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
    p, peak = measure_power(x)
    g = static_gain(target, p, peak, cap)
    return (x.copy() if g == 1.0 else apply_gain(x, g)), g


def gain_db(g: float) -> float:
    return float(20.0 * np.log10(g))


class StreamState:
    """The stream rule for one slot.  ``process`` returns exactly as many samples as it is given."""

    def __init__(self, target: float, start_gain_db: float = 0.0):
        self.target = float(target)
        self.ptarget = target_power(target)
        self.f = _Filter()
        self.e_hop = 0.0
        self.hops = np.zeros(BLOCK_HOPS - 1)  # the last complete hops' energies, oldest first
        self.ring = np.zeros(RING)            # block j's mean square at j % RING
        self.peak = np.float32(0)
        self.ka = self.kb = knot_of_db(start_gain_db)  # the knots at both ends of the open hop
        self.knots = [self.ka, self.kb]       # every knot so far (the model's record; the device keeps the last two)
        self.passed = [0, 0]                  # blocks past the absolute gate in the ring when each knot was set
        self.caps = [K_MAX, K_MAX]            # the running peak's cap when each knot was set

    def _hop_done(self, nh: int, e) -> None:
        """Hop ``nh - 1`` is complete with energy ``e``: its block enters the ring and the knot behind the next hop is set."""
        t = tables()
        if nh >= BLOCK_HOPS:
            self.ring[(nh - BLOCK_HOPS) % RING] = _block(self.hops[0], self.hops[1], self.hops[2], e)
        self.hops = np.array([self.hops[1], self.hops[2], e])
        p, n1, _ = gated_power(self.ring)
        new = self.kb
        if n1:
            want = int(np.searchsorted(t.gain2 * np.float64(p), self.ptarget, side="right")) - 1 - K_MAX
            new = self.kb + max(-SLEW_STEPS, min(SLEW_STEPS, max(want, -K_MAX) - self.kb))
        cap = int(np.searchsorted(t.gain * np.float64(self.peak), t.ceiling, side="right")) - 1 - K_MAX
        cap = max(cap, -K_MAX)
        new = min(new, cap)
        self.caps.append(cap)
        self.ka, self.kb = self.kb, new
        self.knots.append(new)
        self.passed.append(n1)

    def process(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
        if x.size == 0:
            return x.copy()
        t = tables()
        pos0 = self.f.pos
        e, pk, ln, done = self.f.run(x)
        ga, d = np.zeros(ln.size), np.zeros(ln.size)
        pos = pos0
        for i in range(ln.size):
            ga[i] = t.gain[self.ka + K_MAX]
            d[i] = (t.gain[self.kb + K_MAX] - ga[i]) / np.float64(HOP)
            self.peak = np.fmax(self.peak, pk[i])
            pos += int(ln[i])
            if done[i]:
                self.e_hop = self.e_hop + e[i]
                if pos % HOP == 0:
                    self._hop_done(pos // HOP, self.e_hop)
                    self.e_hop = 0.0
        piece = np.repeat(np.arange(ln.size), ln)
        o = (pos0 + np.arange(x.size, dtype=np.int64)) % HOP
        g = ga[piece] + o.astype(np.float64) * d[piece]
        return (x.astype(np.float64) * g).astype(np.float32)

    def state(self) -> dict:
        """What ``LoudnessNormalizer.slot_state`` reads from the device."""
        return {"pos": self.f.pos, "ka": self.ka, "kb": self.kb, "peak": np.float32(self.peak),
                "filter": np.concatenate([self.f.s_start, self.f.s_run, self.f.z_run, [self.f.e_sub, self.e_hop], self.hops]),
                "ring": self.ring.copy()}


def stream_normalize(x: np.ndarray, target: float, start_gain_db: float = 0.0) -> np.ndarray:
    return StreamState(target, start_gain_db).process(x)
