"""Character timestamps from the slow transformer's attention: the host side.

The session measures, per audio frame f and chosen (layer, head) pair, the mass m its attention puts on the request's own text and
the first moment s1 of that mass over the text's positions (``LMSession.set_align_heads`` / ``set_slot_align``).  The tokenizer is a
byte-level BPE without merges, so a position is a byte (or an added token spelled out in the text), and s1 / m is "which byte the
head looks at" in units of tokens.  Here that curve is made monotone (weighted isotonic regression), cut into token intervals and
mapped to characters and seconds.  numpy only; nothing here touches the GPU except ``measure_heads`` and the command line, which run
the ranking tool on a checkpoint:

    python -m smoltts_amd.align rank --checkpoint DIR --texts FILE
    python -m smoltts_amd.align rank --checkpoint DIR --recordings FILE --mimi-checkpoint FILE

The second half is forced alignment: a recording and its transcript become the grid the model would have
produced (``recording_grid``), the session measures that grid's audio rows teacher-forced (``LMSession.measure_rows``), and
``recording`` turns the rows and scores into character and word times with a loss (``RecordingAlignment``).

Which heads of a checkpoint track the text is a property of that checkpoint; nobody has checked this on real speech (README).
"""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

FRAME_SAMPLES, SAMPLE_RATE = 1920, 24_000
FRAME_S = FRAME_SAMPLES / SAMPLE_RATE
# Frames whose chosen heads put less than this much mass (summed over the heads) on the text carry no weight in the fit: the
# centroid s1 / m of such a frame is a ratio of two small numbers -- the head is looking at the speaker turns, the audio history
# or its attention sink -- and its fp32 noise, about 1e-7 on m, is no longer small against m.  0.05 keeps every frame in which one
# head spends a twentieth of its attention on the text; DESIGN.md 21.
MIN_MASS = 0.05


def check_heads(heads, config=None) -> List[Tuple[int, int]]:
    """``alignment_heads`` of a front end -> sorted ``[(layer, head), ...]`` (None: none); ``ValueError`` for pairs that are no pairs
    of ints, for more than 16, for duplicates and, given the model's ``config``, for pairs outside it."""
    if heads is None:
        return []
    out = []
    for p in heads:
        if not isinstance(p, (list, tuple)) or len(p) != 2 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in p):
            raise ValueError(f"alignment_heads: {p!r} is not a [layer, head] pair")
        out.append((int(p[0]), int(p[1])))
    if len(out) > 16 or len(set(out)) != len(out):
        raise ValueError("alignment_heads: at most 16 distinct [layer, head] pairs")
    for l, h in out:
        if l < 0 or h < 0 or (config is not None and (l >= config.n_layer or h >= config.n_head)):
            raise ValueError(f"alignment_heads: [{l}, {h}] lies outside the model")
    return sorted(out)


# ------------------------------------------------------------------------------------------------ the prompt's text window
def window_of(row0: Sequence[int], tokenizer) -> Tuple[int, int]:
    """[t0, t1) of the request's own user text inside its prompt grid's token row: behind the last ``<|im_start|>user\\n``, up to
    that turn's closing ``<|im_end|>``.  With a cloned voice's speaker turns in front (user turns of their own) it is the last."""
    ids = [int(x) for x in row0]
    head = [tokenizer.token_to_id("<|im_start|>"), tokenizer.token_to_id("user"), tokenizer.token_to_id("\n")]
    end = tokenizer.token_to_id("<|im_end|>")
    if None in head or end is None:
        raise ValueError("the tokenizer has no ChatML tokens")
    starts = [i for i in range(len(ids) - 2) if ids[i:i + 3] == head]
    if not starts:
        raise ValueError("the prompt has no user turn")
    t0 = starts[-1] + 3
    ends = [i for i in range(t0, len(ids)) if ids[i] == end]
    if not ends:
        raise ValueError("the prompt's last user turn is not closed")
    return t0, ends[-1]


def token_spans(text: str, ids: Sequence[int], tokenizer=None) -> List[Tuple[int, int]]:
    """Per character of ``text`` the tokens [a, b) of ``ids`` (the text's own tokens, in order) that spell it.  A byte token
    belongs to the character whose UTF-8 encoding contains it (one token per byte; a vocabulary whose base is the latin-1 code
    points has one token per such character); an added token spelled out in the text covers all of its characters (``tokenizer``
    names it); a character the tokenizer dropped has an empty span where it would stand."""
    ids = [int(x) for x in ids]
    spans: List[Tuple[int, int]] = []
    k, i, n = 0, 0, len(text)
    while i < n:
        ch = text[i]
        if k < len(ids) and ids[k] >= 256 and tokenizer is not None:
            tok = tokenizer.id_to_token(ids[k])
            if tok and text.startswith(tok, i):
                spans += [(k, k + 1)] * len(tok)
                i, k = i + len(tok), k + 1
                continue
        b = list(ch.encode("utf-8"))
        if ids[k:k + len(b)] == b:
            spans.append((k, k + len(b)))
            k += len(b)
        elif ord(ch) < 256 and k < len(ids) and ids[k] == ord(ch):
            spans.append((k, k + 1))
            k += 1
        else:
            spans.append((k, k))  # dropped by the tokenizer
        i += 1
    if k != len(ids):
        raise ValueError(f"the ids do not spell the text: {len(ids) - k} of {len(ids)} tokens left over")
    return spans


# ------------------------------------------------------------------------------------------------ the fit
def isotonic(y: Sequence[float], w: Sequence[float]) -> np.ndarray:
    """Weighted isotonic regression (non-decreasing) by pool-adjacent-violators: the x that minimises sum w (x - y)^2 under
    x_0 <= x_1 <= ..; every weight > 0."""
    y, w = np.asarray(y, np.float64), np.asarray(w, np.float64)
    if y.size and not (w > 0).all():
        raise ValueError("isotonic: weights must be positive")
    vals: List[float] = []
    wts: List[float] = []
    cnt: List[int] = []
    for yi, wi in zip(y, w):
        vals.append(float(yi)); wts.append(float(wi)); cnt.append(1)
        while len(vals) > 1 and vals[-2] > vals[-1]:  # pool the two last blocks
            ww = wts[-2] + wts[-1]
            vals[-2] = (vals[-2] * wts[-2] + vals[-1] * wts[-1]) / ww
            wts[-2] = ww
            cnt[-2] += cnt[-1]
            vals.pop(); wts.pop(); cnt.pop()
    return np.repeat(np.asarray(vals, np.float64), cnt) if vals else np.zeros(0)


@dataclass
class Fit:
    starts: np.ndarray     # [n_tokens] start of each token, in frames
    ends: np.ndarray       # [n_tokens]
    mass: np.ndarray       # [frames] summed mass of the chosen heads (-1: not measured)
    centroid: np.ndarray   # [frames] s1 / m of the sums (nan where the frame carries no weight)
    curve: np.ndarray      # [frames] the fitted monotone curve at the frame centres (interpolated over the weightless frames)


def fit(m: np.ndarray, s1: np.ndarray, n_tokens: int) -> Fit:
    """``m``, ``s1`` [frames] or [frames, heads] -> token intervals in frames.  The chosen heads are summed per frame; a frame with
    m < 0 in any head (not measured) or a summed mass below ``MIN_MASS`` has weight 0, the others their mass.  The centroids are
    fitted by weighted isotonic regression; token i starts where the fitted curve, linear between frame centres f + 0.5, passes
    i - 0.5, and ends where token i + 1 starts; the first start is 0, the last end is the number of frames."""
    m, s1 = np.asarray(m, np.float64), np.asarray(s1, np.float64)
    if m.ndim == 1:
        m, s1 = m[:, None], s1[:, None]
    F = m.shape[0]
    measured = (m >= 0).all(axis=1) if m.shape[1] else np.zeros(F, bool)
    mass = np.where(measured, m.sum(axis=1), -1.0)
    ok = measured & (mass >= MIN_MASS)
    cen = np.full(F, np.nan)
    cen[ok] = s1.sum(axis=1)[ok] / mass[ok]
    x = np.nonzero(ok)[0] + 0.5
    yhat = isotonic(cen[ok], mass[ok])
    starts = np.zeros(max(n_tokens, 0))
    if x.size == 0:  # nothing measured: the tokens share the utterance evenly
        starts = np.arange(n_tokens) * (F / max(n_tokens, 1))
        curve = np.full(F, np.nan)
    else:
        curve = np.interp(np.arange(F) + 0.5, x, yhat)
        for i in range(1, n_tokens):
            level = i - 0.5
            k = int(np.searchsorted(yhat, level, side="left"))  # the first weighted frame at or above the level
            if k == 0:
                starts[i] = 0.0
            elif k == x.size:
                starts[i] = float(F)
            else:
                starts[i] = x[k - 1] + (level - yhat[k - 1]) / (yhat[k] - yhat[k - 1]) * (x[k] - x[k - 1])
    starts = np.minimum(np.maximum.accumulate(starts), F) if n_tokens else starts
    ends = np.append(starts[1:], float(F)) if n_tokens else starts
    return Fit(starts, ends, mass, cen, curve)


@dataclass
class Alignment:
    """ElevenLabs' alignment object, plus the per-frame mass and centroid the times were fitted to."""
    characters: List[str]
    start_s: List[float]
    end_s: List[float]
    mass: np.ndarray = field(default_factory=lambda: np.zeros(0))
    centroid: np.ndarray = field(default_factory=lambda: np.zeros(0))

    def to_json(self) -> dict:
        return {"characters": list(self.characters), "character_start_times_seconds": [float(t) for t in self.start_s],
                "character_end_times_seconds": [float(t) for t in self.end_s]}


def align(text: str, ids: Sequence[int], m: np.ndarray, s1: np.ndarray, tokenizer=None, speed: Optional[float] = None,
          duration_s: Optional[float] = None) -> Alignment:
    """``text`` and its tokens ``ids`` (the prompt's window), the rows ``m`` / ``s1`` [audio frames(, heads)] -> ``Alignment``.
    One frame is 1920 samples at 24 kHz.  ``speed`` other than 1: the times are divided by it -- nominal: the stretch (WSOLA) is
    piecewise and moves a sample by up to a search window around that.  ``duration_s``: what was delivered; the last end is set to
    it and no time lies behind it."""
    spans = token_spans(text, ids, tokenizer)
    ft = fit(m, s1, len(ids))
    scale = FRAME_S / (float(speed) if speed else 1.0)
    total = ft.mass.shape[0] * scale if duration_s is None else float(duration_s)
    ts, te = np.minimum(ft.starts * scale, total), np.minimum(ft.ends * scale, total)
    if te.size:
        te[-1] = total
    start_s, end_s = [], []
    for a, b in spans:
        if b > a:
            start_s.append(float(ts[a])); end_s.append(float(te[b - 1]))
        else:  # a dropped character: an empty interval where it would stand
            t = float(ts[a]) if a < ts.size else total
            start_s.append(t); end_s.append(t)
    return Alignment(list(text), start_s, end_s, ft.mass, ft.centroid)


# ------------------------------------------------------------------------------------------------ the causal fit
MIN_LAG, MAX_LAG, DEFAULT_LAG = 1, 64, 6


def check_lag(lag) -> int:
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not MIN_LAG <= int(lag) <= MAX_LAG:
        raise ValueError(f"timestamp_lag_frames must be an int in {MIN_LAG} .. {MAX_LAG}, got {lag!r}")
    return int(lag)


def check_live_timestamps(opts, stream: bool, has_heads: bool, takes: int = 1) -> None:
    """What every front end refuses of a request with ``live_timestamps`` (``opts``: its parsed ``request.SpeechOptions``)."""
    if not has_heads:
        raise ValueError("timestamps need alignment_heads: rank a checkpoint's heads with `python -m smoltts_amd.align rank`")
    if not stream:
        raise ValueError("live_timestamps apply to streams: use `timestamps` for a blocking request")
    if opts.timestamps:
        raise ValueError("live_timestamps cannot be combined with timestamps")
    if opts.segment is not None:
        raise ValueError("live_timestamps cannot be combined with segment: the seam cuts samples where the audio says so")
    if opts.trims:
        raise ValueError("live_timestamps cannot be combined with trim_silence or max_pause_s: the trim stage cuts samples where the audio says so")
    if takes > 1:
        raise ValueError("live_timestamps cannot be combined with best_of")


class StreamFit:
    """The causal fit of one stream, frame by frame: the specification of csrc/align_fit.hip, which gives the same bits.

    ``push`` takes one frame's ``m`` / ``s1`` of the chosen heads.  The weighted frames are pooled as ``isotonic`` pools them, in
    its order; token i's start is committed once a block at or above its level i - 0.5 begins at least ``lag`` frames back, as
    ``fit``'s crossing over the blocks so far, raised to the start in front of it.  A committed start is never revised.
    ``finish(F)`` gives every remaining token ``fit``'s value over what has been seen, cut at F.  ``lag`` is not checked here: at
    or above the number of frames nothing commits early and the starts are ``fit``'s."""

    def __init__(self, n_tokens: int, lag: int = DEFAULT_LAG):
        self.n, self.lag = max(int(n_tokens), 0), int(lag)
        self.frames = 0
        self.v: List[float] = []
        self.w: List[float] = []
        self.f0: List[int] = []
        self.f1: List[int] = []
        self.starts: List[float] = [0.0] if self.n > 0 else []
        self.finished = False

    @property
    def committed(self) -> int:
        return len(self.starts)

    def _crossing(self, i: int, lag: Optional[int], f: int) -> Optional[float]:
        """Where the curve over the blocks passes token i's level; None: no block reaches it (or, with ``lag``, too recently)."""
        level = i - 0.5
        j = len(self.v)  # from the top: the uncommitted levels live there
        while j > 0 and self.v[j - 1] >= level:
            j -= 1
        if j == len(self.v) or (lag is not None and f - self.f0[j] < lag):
            return None
        if j == 0:
            return 0.0
        xa, xb = self.f1[j - 1] + 0.5, self.f0[j] + 0.5
        return xa + (level - self.v[j - 1]) / (self.v[j] - self.v[j - 1]) * (xb - xa)

    def push(self, m, s1) -> None:
        if self.finished:
            raise ValueError("the stream has finished")
        m, s1 = np.asarray(m, np.float32).astype(np.float64).reshape(-1), np.asarray(s1, np.float32).astype(np.float64).reshape(-1)
        f = self.frames
        self.frames += 1
        measured = m.size > 0
        mass, s = 0.0, 0.0
        for h in range(m.size):  # one add at a time, in pair order (numpy's own sum is pairwise from 8 elements on)
            measured = measured and bool(m[h] >= 0)
            mass = mass + float(m[h])
            s = s + float(s1[h])
        if not (measured and mass >= MIN_MASS):
            return
        self.v.append(s / mass); self.w.append(mass); self.f0.append(f); self.f1.append(f)
        v, w = self.v, self.w
        while len(v) > 1 and v[-2] > v[-1]:
            ww = w[-2] + w[-1]
            v[-2] = (v[-2] * w[-2] + v[-1] * w[-1]) / ww
            w[-2] = ww
            self.f1[-2] = self.f1[-1]
            v.pop(); w.pop(); self.f0.pop(); self.f1.pop()
        while len(self.starts) < self.n:
            c = self._crossing(len(self.starts), self.lag, f)
            if c is None:
                break
            self.starts.append(max(c, self.starts[-1]))

    def push_rows(self, rows) -> None:
        """``rows`` [frames, heads, 2] as the session writes them."""
        for r in np.asarray(rows, np.float32):
            self.push(r[:, 0], r[:, 1])

    def finish(self, F: int) -> np.ndarray:
        """The stream delivers ``F`` frames of audio: the remaining starts, then all of them [n] in frames."""
        F = int(F)
        if not self.finished:
            self.finished = True
            while len(self.starts) < self.n:
                i = len(self.starts)
                if not self.v:
                    c = i * (F / max(self.n, 1))
                else:
                    c = self._crossing(i, None, 0)
                    c = float(F) if c is None else c
                self.starts.append(min(max(c, self.starts[-1]), float(F)))
        return np.asarray(self.starts, np.float64)


@dataclass
class AlignmentPart:
    """The characters of a stream whose end became known since the part before, with their times in seconds."""
    characters: List[str]
    start_s: List[float]
    end_s: List[float]

    def to_json(self) -> dict:
        return {"characters": list(self.characters), "character_start_times_seconds": [float(t) for t in self.start_s],
                "character_end_times_seconds": [float(t) for t in self.end_s]}


class StreamAligner:
    """Committed token starts -> ``AlignmentPart``s.  ``update(starts)`` takes the starts committed so far (in frames; a prefix
    that only grows) and returns the characters whose end they settle, or None; ``finish(starts, duration_s)`` takes all of
    them and returns the rest, clamped to the delivered duration, the last end set to it.  Seconds are frames * FRAME_S / speed,
    nominal at a speed other than 1 as ``align``'s are.  A part handed out is not revised; ``alignment()`` concatenates them."""

    def __init__(self, text: str, ids: Sequence[int], tokenizer=None, speed: Optional[float] = None):
        self.text = text
        self.spans = token_spans(text, ids, tokenizer)
        self.n = len(ids)
        self.speed = float(speed) if speed else 1.0
        self.scale = FRAME_S / self.speed
        self.next_char = 0
        self.parts: List[AlignmentPart] = []
        self.finished = False

    def _part(self, starts: np.ndarray, known: int, total: Optional[float]) -> Optional[AlignmentPart]:
        """The characters from ``next_char`` on whose times need only starts[:known] (and, at the end, ``total``)."""
        ts = np.asarray(starts, np.float64)[:known] * self.scale
        if total is not None:
            ts = np.minimum(ts, total)
        chars, a_s, e_s = [], [], []
        k = self.next_char
        while k < len(self.spans):
            a, b = self.spans[k]
            if b > a:
                if b < self.n:
                    if b >= known:
                        break
                    start, end = float(ts[a]), float(ts[b])
                elif total is None:
                    break  # the last token's end is the delivered duration
                else:
                    start, end = float(ts[a]), total
            else:  # a dropped character: an empty interval where it would stand
                if a < self.n:
                    if a >= known:
                        break
                    start = end = float(ts[a])
                elif total is None:
                    break
                else:
                    start = end = total
            chars.append(self.text[k]); a_s.append(start); e_s.append(end)
            k += 1
        if k == self.next_char:
            return None
        self.next_char = k
        part = AlignmentPart(chars, a_s, e_s)
        self.parts.append(part)
        return part

    def duration(self, frames: int) -> float:
        """What ``frames`` frames deliver, in seconds: their samples over the rate (the blocking route's figure), over the speed."""
        return int(frames) * FRAME_SAMPLES / SAMPLE_RATE / self.speed

    def update(self, starts) -> Optional[AlignmentPart]:
        if self.finished:
            raise ValueError("the stream has finished")
        return self._part(starts, min(len(starts), self.n), None)

    def finish(self, starts, duration_s: float) -> Optional[AlignmentPart]:
        if self.finished:
            return None
        if len(starts) < self.n:
            raise ValueError(f"finish needs every start: {len(starts)} of {self.n}")
        self.finished = True
        return self._part(starts, self.n, float(duration_s))

    def alignment(self) -> Alignment:
        return Alignment([c for p in self.parts for c in p.characters], [t for p in self.parts for t in p.start_s],
                         [t for p in self.parts for t in p.end_s])


# ------------------------------------------------------------------------------------------------ which heads track the text
@dataclass
class HeadScore:
    layer: int
    head: int
    mean_mass: float    # mean text mass over the measured frames
    monotone: float     # mass-weighted share of the frame-to-frame centroid steps that are >= 0
    coverage: float     # share of the text the fitted curve runs over

    @property
    def score(self) -> float:
        return self.mean_mass * self.monotone * self.coverage


def rank_heads(runs: Sequence[dict]) -> List[HeadScore]:
    """``runs``: per utterance ``{"pairs": [(layer, head), ..], "m": [frames, pairs], "s1": [frames, pairs], "n_tokens": n}`` ->
    one ``HeadScore`` per (layer, head), averaged over the utterances that measured it, best first."""
    acc: dict = {}
    for run in runs:
        m, s1, n = np.asarray(run["m"], np.float64), np.asarray(run["s1"], np.float64), int(run["n_tokens"])
        for i, pair in enumerate(run["pairs"]):
            mi, si = m[:, i], s1[:, i]
            ok = mi >= 0
            if not ok.any():
                continue
            mean_mass = float(mi[ok].mean())
            ft = fit(mi, si, n)
            good = ~np.isnan(ft.centroid)
            c, wgt = ft.centroid[good], mi[good]
            if c.size >= 2:
                step_w = np.minimum(wgt[1:], wgt[:-1])
                mono = float(step_w[np.diff(c) >= 0].sum() / step_w.sum())
                cov = float(np.clip((np.nanmax(ft.curve) - np.nanmin(ft.curve)) / max(n - 1, 1), 0.0, 1.0))
            else:
                mono, cov = 0.0, 0.0
            acc.setdefault((int(pair[0]), int(pair[1])), []).append((mean_mass, mono, cov))
    out = [HeadScore(l, h, *(float(np.mean([v[k] for v in vals])) for k in range(3))) for (l, h), vals in acc.items()]
    return sorted(out, key=lambda s: (-s.score, s.layer, s.head))


def measure_heads(engine, prompts, windows, pairs, settings=None, max_frames: int = 256):
    """The rows of ``pairs`` (at most ``abi.MAX_ALIGN_HEADS``) for each prompt grid with its text window, greedy unless
    ``settings`` says otherwise: a list of ``{"pairs", "m", "s1", "n_tokens"}`` as ``rank_heads`` takes them.  Runs on the GPU."""
    from .config import GenerationSettings, RequestSampling
    from .generate import BatchGenerator, resolve_sampling

    import dataclasses

    st = dataclasses.replace(settings or GenerationSettings.greedy(), max_new_tokens=max_frames)
    gen = BatchGenerator(engine, prompts, st, frames_per_sync=16, sampling=resolve_sampling(RequestSampling(), st, len(prompts)),
                         align=(pairs, windows))
    for _ in gen:
        pass
    rows = gen.alignment()
    gen.close()
    return [{"pairs": sorted((int(l), int(h)) for l, h in pairs), "m": r[:, :, 0], "s1": r[:, :, 1], "n_tokens": w[1] - w[0]}
            for r, w in zip(rows, windows)]


# ------------------------------------------------------------------------------------------------ forced alignment
@dataclass
class RecordingGrid:
    """A recording with its transcript as the model would have produced it: the prompt turns, then the recording's audio columns."""
    grid: np.ndarray          # (1 + depth, a0 + F) int32
    a0: int                   # the first audio column
    n_frames: int             # F
    window: Tuple[int, int]   # [t0, t1) of the transcript's tokens in row 0
    frame_of_row: np.ndarray  # [a0 + F] the frame a column's row produces: a0 - 1 + f -> f; -1 elsewhere
    targets: np.ndarray       # [a0 + F] the slow id that row should produce (-1: not scored); the last column's is <|im_end|>

    @property
    def end_row(self) -> int:
        return self.grid.shape[1] - 1


def recording_grid(encoder, tokenizer, token_config, text: str, codes, voice: str = "heart", sysprompt=None) -> RecordingGrid:
    """The grid of a recording: system turn (``voice``, or a cloned speaker's turns ``sysprompt``), user turn with ``text``, the
    assistant header, then the audio columns of ``encoder.encode_vq(codes)`` without its closing turn.  ``codes``: (n_codebooks,
    F >= 1) Mimi codes.  The row at position a0 - 1 + f produces frame f and is scored against ``codes[0, f] +
    semantic_start_id``; the last audio column's row is scored against ``<|im_end|>`` and has no frame."""
    if not isinstance(text, str) or not text.strip():
        raise ValueError("forced alignment needs a text")
    codes = np.asarray(codes)
    if codes.ndim != 2 or codes.shape[1] < 1:
        raise ValueError("the audio holds no full frame (1920 samples at 24 kHz)")
    F = int(codes.shape[1])
    prompt = np.asarray(encoder.build_prompt(text, voice, sysprompt))
    audio = encoder.encode_vq(codes.astype(np.int64))[:, :F]
    grid = np.concatenate([prompt, audio], axis=1).astype(np.int32)
    a0 = int(prompt.shape[1])
    frame_of_row = np.full(a0 + F, -1, np.int32)
    frame_of_row[a0 - 1: a0 - 1 + F] = np.arange(F, dtype=np.int32)
    targets = np.full(a0 + F, -1, np.int32)
    targets[a0 - 1: a0 - 1 + F] = codes[0].astype(np.int64) + token_config.semantic_start_id
    targets[a0 + F - 1] = token_config.im_end_id
    return RecordingGrid(grid, a0, F, window_of(grid[0, :a0], tokenizer), frame_of_row, targets)


def recording_limit_frames(a0: int, max_seq: int, max_frames: int) -> int:
    """The most frames a recording behind a prompt of ``a0`` columns may have in a session of ``max_seq`` / ``max_frames``."""
    return max(0, min(int(max_frames), int(max_seq) - 1 - int(a0)))


def check_recording_fits(a0: int, n_frames: int, max_seq: int, max_frames: int) -> None:
    limit = recording_limit_frames(a0, max_seq, max_frames)
    if n_frames > limit:
        raise ValueError(f"the recording has {n_frames * FRAME_S:.2f} s; behind this prompt the model's context allows "
                         f"{limit * FRAME_S:.2f} s (max_seq {max_seq}, max_frames {max_frames})")


def no_heads_error() -> ValueError:
    return ValueError("forced alignment needs alignment_heads: rank a checkpoint's heads with `python -m smoltts_amd.align rank`")


@dataclass
class Word:
    text: str
    start: float
    end: float
    loss: Optional[float]  # mean -logprob of the frames whose centre lies in [start, end); None: no such frame


@dataclass
class RecordingAlignment:
    """ElevenLabs' forced-alignment answer, plus what it was fitted to."""
    alignment: Alignment
    words: List[Word]
    logprobs: np.ndarray   # [F] float32: the model's log-probability of each frame's slow token under the transcript
    end_logprob: float     # ... of <|im_end|> behind the last frame (not part of the mean)
    loss: float            # -mean(logprobs)

    def to_json(self) -> dict:
        a = self.alignment
        return {"characters": [{"text": c, "start": float(s), "end": float(e)} for c, s, e in zip(a.characters, a.start_s, a.end_s)],
                "words": [{"text": w.text, "start": float(w.start), "end": float(w.end), "loss": None if w.loss is None else float(w.loss)}
                          for w in self.words],
                "loss": float(self.loss)}


def words_of(alignment: Alignment, logprobs: np.ndarray) -> List[Word]:
    """Maximal runs of non-whitespace characters with the start of their first and the end of their last character."""
    lp = np.asarray(logprobs, np.float64)
    centres = (np.arange(lp.shape[0]) + 0.5) * FRAME_S
    words: List[Word] = []
    chars, n = alignment.characters, len(alignment.characters)
    i = 0
    while i < n:
        if chars[i].isspace():
            i += 1
            continue
        j = i
        while j < n and not chars[j].isspace():
            j += 1
        start, end = float(alignment.start_s[i]), float(alignment.end_s[j - 1])
        inside = (centres >= start) & (centres < end)
        words.append(Word("".join(chars[i:j]), start, end, float(-lp[inside].mean()) if inside.any() else None))
        i = j
    return words


def recording(text: str, rg: RecordingGrid, rows: np.ndarray, logprobs: np.ndarray, tokenizer=None) -> RecordingAlignment:
    """``rows`` [F, heads, 2] (``LMSession.fetch_alignment`` of the measured slot) and ``logprobs`` [a0 + F]
    (``LMSession.measure_rows``) of ``rg`` -> the ``RecordingAlignment``.  Frame f spans [f, f + 1) * 1920 / 24000 s; the last end
    is the recording's duration."""
    F, (t0, t1) = rg.n_frames, rg.window
    rows = np.asarray(rows)[:F]
    al = align(text, rg.grid[0, t0:t1], rows[:, :, 0], rows[:, :, 1], tokenizer, duration_s=F * FRAME_S)
    lp = np.asarray(logprobs, np.float32)[rg.a0 - 1: rg.a0 - 1 + F].copy()
    return RecordingAlignment(al, words_of(al, lp), lp, float(np.asarray(logprobs)[rg.end_row]), float(-lp.astype(np.float64).mean()))


def measure_recording(session, slot: int, rg: RecordingGrid, chunk: Optional[int] = None, score: bool = True):
    """``rg`` measured in the idle ``slot`` of ``session`` (its heads are set): (rows [F, heads, 2], logprobs [a0 + F]).  GPU."""
    session.set_slot_align([slot], [rg.window[0]], [rg.window[1]])
    lp = session.measure_rows(rg.grid, slot, rg.frame_of_row, rg.targets if score else np.full_like(rg.targets, -1), chunk)
    return session.fetch_alignment(slot, rg.n_frames), lp


def recording_session(engine, pairs, a0: int, n_frames: int, kv_dtype: str = "fp32"):
    """A one-slot ``LMSession`` sized for a recording of ``n_frames`` behind ``a0`` prompt columns, measuring ``pairs``."""
    from .lm import LMSession

    T = a0 + n_frames
    sess = LMSession(engine, 1, max_seq=T + 1, max_rows=T, max_frames=n_frames, kv_dtype=kv_dtype)
    sess.set_align_heads(pairs)
    return sess


def measure_heads_recorded(engine, grids, windows, frame_maps, pairs):
    """``measure_heads`` without sampling: each grid (a recording behind its transcript, ``recording_grid``) goes teacher-forced
    through ``LMSession.measure_rows`` with its text window and its column -> frame map; -> the list ``rank_heads`` takes."""
    runs = []
    for g, w, fm in zip(grids, windows, frame_maps):
        g, fm = np.asarray(g), np.asarray(fm, np.int32)
        F = int(fm.max()) + 1
        sess = recording_session(engine, pairs, g.shape[1] - F, F)
        try:
            sess.set_slot_align([0], [w[0]], [w[1]])
            sess.measure_rows(g, 0, fm, np.full(g.shape[1], -1, np.int32))
            r = sess.fetch_alignment(0, F)
        finally:
            sess.close()
        runs.append({"pairs": sorted((int(l), int(h)) for l, h in pairs), "m": r[:, :, 0], "s1": r[:, :, 1], "n_tokens": w[1] - w[0]})
    return runs


def _rank_recordings(args) -> int:
    """``rank --recordings FILE``: every head, 16 pairs at a time, teacher-forced on the file's recordings."""
    from . import SmolTTS
    from .abi import MAX_ALIGN_HEADS
    from .server.voices import parse_wav, to_codec_rate

    lines = [l.rstrip("\n").split("\t", 1) for l in open(args.recordings, encoding="utf-8") if l.strip()]
    if not lines or any(len(l) != 2 or not l[1].strip() for l in lines):
        print("--recordings: every line is path.wav<TAB>transcript", file=sys.stderr)
        return 2
    if not args.mimi_checkpoint:
        print("--recordings needs --mimi-checkpoint (the full kyutai/mimi model: its encoder turns the recordings into codes)", file=sys.stderr)
        return 2
    tts = SmolTTS(checkpoint_dir=args.checkpoint, mimi_checkpoint=args.mimi_checkpoint)
    config = tts.config
    grids = []
    for path, text in lines:
        with open(path, "rb") as f:
            codes = tts.encode_audio(to_codec_rate(*parse_wav(f.read())))
        rg = recording_grid(tts.prompt_encoder, tts.tokenizer, tts.token_config, text.strip(), codes, args.voice)
        check_recording_fits(rg.a0, rg.n_frames, config.max_seq_len, 1 << 30)
        grids.append(rg)
    every = [(l, h) for l in range(config.n_layer) for h in range(config.n_head)]
    runs = []
    for i in range(0, len(every), MAX_ALIGN_HEADS):
        runs += measure_heads_recorded(tts.lm, [g.grid for g in grids], [g.window for g in grids], [g.frame_of_row for g in grids],
                                       every[i:i + MAX_ALIGN_HEADS])
    _print_ranking(runs, args.top)
    tts.lm.close()
    return 0


def _print_ranking(runs, top: int) -> None:
    print(f"{'layer':>5} {'head':>4} {'mass':>7} {'monotone':>8} {'coverage':>8} {'score':>7}")
    for s in rank_heads(runs)[:top]:
        print(f"{s.layer:5d} {s.head:4d} {s.mean_mass:7.4f} {s.monotone:8.4f} {s.coverage:8.4f} {s.score:7.4f}")


def _rank_main(args) -> int:
    if args.recordings:
        return _rank_recordings(args)
    if not args.texts:
        print("rank needs --texts FILE or --recordings FILE", file=sys.stderr)
        return 2
    from .abi import MAX_ALIGN_HEADS
    from .checkpoint import load_checkpoint
    from .config import NumericsMode, TokenConfig
    from .lm import LMEngine
    from .prompt import PromptEncoder

    texts = [t.strip() for t in open(args.texts, encoding="utf-8").read().splitlines() if t.strip()]
    if not texts:
        print("no texts", file=sys.stderr)
        return 2
    config, tokenizer, state = load_checkpoint(args.checkpoint)
    tc = TokenConfig.from_tokenizer(tokenizer, config)
    engine = LMEngine(config, state, tc, NumericsMode.torch_reference())
    enc = PromptEncoder.from_config(tokenizer, config, tc)
    prompts = [enc.build_prompt(t, args.voice) for t in texts]
    windows = [window_of(p[0], tokenizer) for p in prompts]
    every = [(l, h) for l in range(config.n_layer) for h in range(config.n_head)]
    runs = []
    for i in range(0, len(every), MAX_ALIGN_HEADS):  # the heads 16 at a time: the same greedy utterances every time
        runs += measure_heads(engine, prompts, windows, every[i:i + MAX_ALIGN_HEADS], max_frames=args.max_frames)
    _print_ranking(runs, args.top)
    engine.close()
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m smoltts_amd.align", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("rank", help="rank every (layer, head) of a checkpoint by how well it tracks the text; pick alignment_heads from the top")
    r.add_argument("--checkpoint", required=True)
    r.add_argument("--texts", help="a file with one text per line: the heads are ranked on what the model generates for them")
    r.add_argument("--recordings", help="a file with one `path.wav<TAB>transcript` per line: the heads are ranked teacher-forced "
                                        "on these recordings (no sampling); needs --mimi-checkpoint")
    r.add_argument("--mimi-checkpoint", help="the kyutai/mimi model.safetensors (with its encoder), for --recordings")
    r.add_argument("--voice", default="heart")
    r.add_argument("--max-frames", type=int, default=256)
    r.add_argument("--top", type=int, default=32)
    return _rank_main(ap.parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
