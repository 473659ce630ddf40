"""Silence trimming per request (host side): a numpy model of the GPU trim stage (csrc/trim.hip), which
the kernel must match bit for bit.  Samples are only copied or dropped, so the equality is exact.

The stage stands first behind the codec, in front of the seam.  The rule, which is the definition:

* Blocks are the seam's: ``BLOCK`` = 240 samples counted from the segment's first sample; the last block of a segment may be
  partial.  A block is *silent* when ``max|x| < thr``, compared in float32; a NaN is not silence.  ``thr`` is per request:
  ``seam.THRESH`` (2^-8) exactly by default, else ``float32(10 ** (silence_threshold_db / 20))`` with the level in [-72, -6].
* A *run* is a maximal sequence of consecutive silent blocks, ``r`` its length in blocks.
* Per segment: ``flags`` (``seam.FIRST`` / ``seam.FINAL``; a plain stream is ``FIRST | FINAL``), ``trim`` (bool) and ``P``, the
  pause cap in blocks (0: none; else ``round(max_pause_s * 100)`` with ``max_pause_s`` in [0.1, 2.0], so P in [10, 200]).
  Constants: ``HEAD_KEEP`` = 2, ``TAIL_KEEP`` = 10, ``HOLD`` = 200 blocks.
* What is kept of a run; the first matching case applies:

  1. ``trim``, ``FIRST``, and the run starts at block 0: its last ``min(r, HEAD_KEEP)`` blocks (also an all-silent segment).
  2. ``trim``, ``FINAL``, and the run reaches the segment's end: its first ``min(r, K)`` blocks, ``K = TAIL_KEEP`` when
     ``P == 0``, else ``min(TAIL_KEEP, ceil(P/2))``.  Exception: when ``P == 0`` and ``r - K > HOLD``, its first ``r - HOLD``
     blocks, so that the tail never loses more than 2 s.
  3. ``P > 0`` and ``r > P``: its first ``ceil(P/2)`` and its last ``floor(P/2)`` blocks.
  4. Otherwise all of it.

  Non-silent blocks are always kept.  The output is the kept blocks in order.  Every cut lies in samples below ``thr``, so
  there are no fades, as in the seam.

Streaming: the output does not depend on how a segment is cut into calls.  A non-silent block leaves in the call that completes
it, together with whatever was held in front of it.  The rule is causal with bounded state: a slot holds at most ``HOLD`` blocks
and a partial block.  ``TrimState.start(flags, trim, P, thr)`` and ``push(x, end, last)`` define each call's output (``last``
ends the segment like ``end``; a run it cuts short in a segment that is not ``FINAL`` is released by cases 3 and 4).
``trim(x, ...)`` is the same rule written offline over a whole array, independently of ``TrimState``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .seam import BLOCK, FINAL, FIRST, RATE, THRESH

HEAD_KEEP = 2    # blocks of leading silence kept in front of the first word
TAIL_KEEP = 10   # blocks of trailing silence kept behind the last one
HOLD = 200       # blocks a slot holds back at most
MAX_CALL = 61_440  # samples one call of the stage takes at most (256 blocks)
DB_RANGE = (-72.0, -6.0)
PAUSE_RANGE = (0.1, 2.0)


def threshold(silence_threshold_db: Optional[float]) -> np.float32:
    """The silence threshold of a request: 2^-8 by default, else the level in dBFS as float32."""
    if silence_threshold_db is None:
        return THRESH
    db = float(silence_threshold_db)
    if not (DB_RANGE[0] <= db <= DB_RANGE[1]):  # (a NaN fails both)
        raise ValueError(f"silence_threshold_db must be within [{DB_RANGE[0]:g}, {DB_RANGE[1]:g}]")
    return np.float32(10.0 ** (db / 20.0))


def pause_blocks(max_pause_s: Optional[float]) -> int:
    """The pause cap of a request in blocks (0: none)."""
    if max_pause_s is None:
        return 0
    s = float(max_pause_s)
    if not (PAUSE_RANGE[0] <= s <= PAUSE_RANGE[1]):
        raise ValueError(f"max_pause_s must be within [{PAUSE_RANGE[0]:g}, {PAUSE_RANGE[1]:g}]")
    return int(round(s * 100.0))


def check_params(P: int, thr) -> None:
    if not (P == 0 or 10 <= P <= HOLD):
        raise ValueError("pause cap outside {0} and [10, 200] blocks")
    if not (0.0 < float(thr) <= 1.0):
        raise ValueError("silence threshold outside (0, 1]")


def silent(x: np.ndarray, thr) -> bool:
    return bool(np.max(np.abs(x)) < np.float32(thr))  # (a NaN makes the maximum NaN, and the comparison false)


def tail_keep(P: int) -> int:
    """K of case 2."""
    return TAIL_KEEP if P == 0 else min(TAIL_KEEP, (P + 1) // 2)


# ------------------------------------------------------------------------------- offline
def kept_of_run(r: int, at_start: bool, at_end: bool, flags: int, trim_on: bool, P: int) -> List[int]:
    """The indices (0..r-1) of the blocks kept of a run of ``r`` silent blocks, by the four cases."""
    if trim_on and (flags & FIRST) and at_start:
        return list(range(r - min(r, HEAD_KEEP), r))
    if trim_on and (flags & FINAL) and at_end:
        K = tail_keep(P)
        return list(range(r - HOLD if (P == 0 and r - K > HOLD) else min(r, K)))
    if P > 0 and r > P:
        return list(range((P + 1) // 2)) + list(range(r - P // 2, r))
    return list(range(r))


def trim(x, flags: int = FIRST | FINAL, trim: bool = True, P: int = 0, thr=THRESH) -> np.ndarray:
    """A whole segment trimmed by the rule."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    check_params(P, thr)
    blocks = [x[i:i + BLOCK] for i in range(0, x.size, BLOCK)]
    quiet = [silent(b, thr) for b in blocks]
    out, i, n = [], 0, len(blocks)
    while i < n:
        if not quiet[i]:
            out.append(blocks[i])
            i += 1
            continue
        j = i
        while j < n and quiet[j]:
            j += 1
        out.extend(blocks[i + k] for k in kept_of_run(j - i, i == 0, j == n, flags, bool(trim), P))
        i = j
    return np.concatenate(out) if out else np.zeros(0, np.float32)


# ------------------------------------------------------------------------------- streaming
class TrimState:
    """One slot: ``start(flags, trim, P, thr)`` opens a segment, ``push(x, end, last)`` consumes its samples and returns those
    that became final.  The held blocks are two lists: ``A``, the blocks of a run that a segment's end would drop and a
    non-silent block would keep (blocks K .. ceil(P/2) - 1 of a run in a trimmed ``FINAL`` segment with a cap), and ``B``, a
    queue of the run's newest blocks; whatever lies between them has been dropped."""

    COUNTERS = ("n_in", "judged", "emitted", "held", "dropped_head", "dropped_pause", "dropped_tail")

    def __init__(self):
        self.open = False
        self.n_in = self.judged = self.emitted = self.dropped_head = self.dropped_pause = self.dropped_tail = 0
        self.A: List[np.ndarray] = []
        self.B: List[np.ndarray] = []

    def start(self, flags: int = FIRST | FINAL, trim: bool = True, P: int = 0, thr=THRESH) -> None:
        check_params(P, thr)
        self.__init__()
        self.flags, self.trim, self.P, self.thr = int(flags), bool(trim), int(P), np.float32(thr)
        self.part = np.zeros(0, np.float32)  # the samples of the block that is not complete yet
        self.r = 0         # blocks of the run that is open (0: none)
        self.blocks = 0    # blocks judged
        self.run_drop = 0  # samples dropped from the middle of the open run (a pause's, unless the run turns out to be the tail)
        self.open = True

    @property
    def held(self) -> int:
        """Samples held back (without the partial block)."""
        return sum(b.size for b in self.A) + sum(b.size for b in self.B)

    def state(self) -> dict:
        return {k: int(getattr(self, k)) for k in self.COUNTERS}

    def _block(self, blk: np.ndarray, out: List[np.ndarray]) -> None:
        a, c = (self.P + 1) // 2, self.P // 2
        if not silent(blk, self.thr):
            out.extend(self.A + self.B)
            self.A, self.B, self.r, self.run_drop = [], [], 0, 0
            out.append(blk)
        else:
            i = self.r
            self.r += 1
            if self.trim and (self.flags & FIRST) and self.blocks == i:  # the run started at block 0
                self.B.append(blk)
                if len(self.B) > HEAD_KEEP:
                    self.dropped_head += self.B.pop(0).size
            elif self.trim and (self.flags & FINAL):
                if i < tail_keep(self.P):
                    out.append(blk)
                elif self.P == 0:
                    self.B.append(blk)
                    if len(self.B) > HOLD:
                        out.append(self.B.pop(0))
                elif i < a:
                    self.A.append(blk)
                else:
                    self._pause(blk, c)
            elif self.P > 0:
                if i < a:
                    out.append(blk)
                else:
                    self._pause(blk, c)
            else:
                out.append(blk)
        self.blocks += 1
        self.judged += blk.size

    def _pause(self, blk: np.ndarray, c: int) -> None:
        self.B.append(blk)
        if len(self.B) > c:
            n = self.B.pop(0).size
            self.dropped_pause += n
            self.run_drop += n

    def push(self, x, end: bool = False, last: bool = False) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        if not self.open:
            return np.zeros(0, np.float32)
        end = end or last
        buf = np.concatenate([self.part, x])
        self.n_in += x.size
        out: List[np.ndarray] = []
        i = 0
        while buf.size - i >= BLOCK:
            self._block(buf[i:i + BLOCK], out)
            i += BLOCK
        if end and i < buf.size:
            self._block(buf[i:], out)
            i = buf.size
        self.part = buf[i:].copy()
        if end:
            if self.r > 0:
                head = self.trim and (self.flags & FIRST) and self.blocks == self.r
                if not head and self.trim and (self.flags & FINAL):
                    self.dropped_tail += self.held + self.run_drop
                    self.dropped_pause -= self.run_drop
                else:
                    out.extend(self.A + self.B)
            self.A, self.B, self.open = [], [], False
        y = np.concatenate(out) if out else np.zeros(0, np.float32)
        self.emitted += y.size
        return y


def trim_chunked(x, sizes: Sequence[int], flags: int = FIRST | FINAL, trim: bool = True, P: int = 0, thr=THRESH,
                 last: bool = False) -> Tuple[np.ndarray, TrimState]:
    """``x`` pushed through a ``TrimState`` in calls of ``sizes`` samples, the last one ending the segment."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    assert sum(sizes) == x.size and len(sizes) > 0
    st = TrimState()
    st.start(flags, trim, P, thr)
    out, i = [], 0
    for j, n in enumerate(sizes):
        e = j == len(sizes) - 1
        out.append(st.push(x[i:i + n], end=e and not last, last=e and last))
        i += n
    return np.concatenate(out), st


def trimmed_seconds(n_in: int, n_out: int) -> float:
    return (int(n_in) - int(n_out)) / RATE
