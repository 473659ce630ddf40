"""The seam between the segments of a long text (host side): a numpy model of the GPU seam stage (csrc/seam.hip; DESIGN.md
section 13), which the kernel must match.

Every segment is its own utterance, with its own leading and trailing silence.  The seam stage joins them into one stream on the
codec's 24 kHz fp32 PCM, block by block.  The rule, which is the definition:

* Blocks are ``BLOCK`` = 240 samples counted from the segment's first sample; the last one of a segment may be partial.  A block
  is *silent* when ``max|x| < THRESH`` = 2^-8 (max-abs, so that numpy and the kernel decide the same bit for bit).
* Head of every segment but the stream's first: leading silent blocks are dropped while the dropped samples stay ``<= D`` = 1 s;
  emission starts at the first non-silent block, or at the first block that would pass D.
* Tail of every segment but the stream's last: a run of silent blocks is held back, at most ``H`` = 1 s of it; a non-silent block
  releases the held run unchanged in front of itself, and a run longer than H releases its oldest samples.  When the segment ends,
  the held run of r samples becomes its first ``min(r, G)`` samples followed by ``G - min(r, G)`` zeros, G the seam's pause.
* The stream's first segment may open with ``lead`` zeros and its last one close with ``G`` zeros (break tags at the ends).
  The head of the first segment and the tail of the last are otherwise never touched.

Every cut falls inside samples below the threshold, so the step at a cut is below 2^-8; there are no fades.  The output does not
depend on how a segment is cut into calls.  A whole text of one segment is never given to this stage; a text fed in pieces
(``longform.IncrementalSplitter``) always is, and a single segment passes through it unchanged.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

RATE = 24_000
BLOCK = 240
THRESH = np.float32(2.0 ** -8)
H = RATE       # tail samples held back at most
D = RATE       # head samples dropped at most
MAX_PAUSE = 10 * RATE  # samples of one seam's pause, or of the silence in front of the stream, at most
HIST = 24_576  # input samples a slot carries (a held run and a partial block: <= H + BLOCK - 1)

FIRST, FINAL = 1, 2  # segment flags (SMOLTTS_SEAM_FIRST / _FINAL)


def segment_flags(k: int, n: int) -> int:
    """The flags of segment k of a stream of n segments."""
    return (FIRST if k == 0 else 0) | (FINAL if k == n - 1 else 0)


def pause_samples(seconds: Optional[float]) -> int:
    """A pause in seconds -> samples at 24 kHz (rounded to nearest)."""
    return 0 if seconds is None else int(round(float(seconds) * RATE))


def silent(x: np.ndarray) -> bool:
    return x.size == 0 or bool(np.max(np.abs(x)) < THRESH)


class SeamState:
    """One slot: ``start(pause, flags, lead)`` opens a segment, ``push(x, end)`` consumes its samples and returns those that became
    final (``end``: the segment ends with them; ``last``: the stream ends with them, the held run is then released unchanged)."""

    def __init__(self):
        self.open = False

    def start(self, pause: int, flags: int, lead: int = 0) -> None:
        if not (0 <= pause <= MAX_PAUSE and 0 <= lead <= MAX_PAUSE):
            raise ValueError("seam pause outside [0, 10 s]")
        self.pause, self.flags, self.lead_owed = int(pause), int(flags), int(lead) if flags & FIRST else 0
        self.buf = np.zeros(0, np.float32)  # segment samples [ec, n_in): the held run, then the partial block
        self.n_in = self.judged = self.ec = 0
        self.head = not (flags & FIRST)
        self.open = True

    def push(self, x, end: bool = False, last: bool = False) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        if not self.open:
            return np.zeros(0, np.float32)
        end = end or last
        final = bool(self.flags & FINAL)
        base = self.ec  # self.buf[0] is sample base of the segment
        buf = np.concatenate([self.buf, x])
        n1 = self.n_in + x.size
        e0 = self.ec
        while True:
            s = self.judged
            ln = min(BLOCK, n1 - s)
            if ln <= 0 or (ln < BLOCK and not end):
                break
            quiet = silent(buf[s - base: s + ln - base])
            if self.head:
                if quiet and s + ln <= D:
                    self.judged = self.ec = e0 = s + ln
                    continue
                self.head = False
            self.judged = s + ln
            if final or not quiet:
                self.ec = self.judged
            elif self.judged - self.ec > H:
                self.ec = self.judged - H
        z1 = 0
        if end:
            if final or last:
                self.ec = n1
                z1 = self.pause if final else 0
            else:
                keep = min(self.judged - self.ec, self.pause)
                self.ec += keep
                z1 = self.pause - keep
        z0, self.lead_owed = self.lead_owed, 0
        y = np.concatenate([np.zeros(z0, np.float32), buf[e0 - base: self.ec - base], np.zeros(z1, np.float32)])
        self.n_in = n1
        if end:
            self.open = False
            self.buf = np.zeros(0, np.float32)
        else:
            self.buf = buf[self.ec - base:].copy()
        return y


def join(segments: Sequence[np.ndarray], pauses: Sequence[int], lead: int = 0, trail: int = 0,
         chunks: Optional[Sequence[Sequence[int]]] = None) -> np.ndarray:
    """Segments' PCM joined by the rule: ``pauses[k]`` (samples) is the seam after segment k (len(segments) - 1 of them);
    ``lead`` / ``trail`` zeros before the first / after the last.  ``chunks[k]``: the call sizes segment k is pushed in (default:
    one call).  One segment without lead or trail comes back unchanged."""
    segs = [np.asarray(s, dtype=np.float32).reshape(-1) for s in segments]
    if len(pauses) != max(len(segs) - 1, 0):
        raise ValueError("one pause per seam")
    st = SeamState()
    out: List[np.ndarray] = []
    for k, s in enumerate(segs):
        final = k == len(segs) - 1
        st.start(trail if final else int(pauses[k]), segment_flags(k, len(segs)), lead)
        sizes = list(chunks[k]) if chunks is not None else [s.size]
        assert sum(sizes) == s.size
        i = 0
        for j, n in enumerate(sizes):
            out.append(st.push(s[i:i + n], end=j == len(sizes) - 1))
            i += n
    return np.concatenate(out) if out else np.zeros(0, np.float32)
