"""Long texts as chained sentence segments (host side).

A text that does not fit one prompt is spoken segment by segment: ``split_text`` cuts it into segments of at most ``max_bytes``
UTF-8 bytes at sentence ends, ``chain_prompt`` conditions segment k on segment k - 1's text and generated codes (the mechanism
``SmolTTS.create_speaker`` uses for cloned voices), ``segment_seed`` gives every segment its own seed, and the seam stage
(``seam.py``, ``csrc/seam.hip``) joins the segments' audio on the GPU.

The segmentation rule, which is the definition:

1. ElevenLabs break tags ``<break time="1.5s" />`` / ``<break time="750ms"/>`` (the slash and the space before it optional, single
   or double quotes) are taken out of the text first.  A tag ends a segment and sets the pause after it; a single tag's time
   must lie in [0, 3] s (``ValueError`` otherwise).  Consecutive tags add up, to at most ``MAX_PAUSE_S`` per seam.  Tags before
   the first segment or after the last become silence at that end (``Segment.pause_before_s`` of the first segment,
   ``pause_after_s`` of the last).
2. Between tags, the text is cut after a sentence end that is followed by whitespace -- one of ``. ! ? …``, then any closing
   quotes or brackets -- and at every newline.
3. Sentences are packed greedily into segments while the segment's UTF-8 byte count (sentences joined by one space) stays
   ``<= max_bytes``.
4. A sentence longer than ``max_bytes`` is cut at the last ``, ; : —`` (the cut after it) that leaves a head of at most
   ``max_bytes`` bytes, else at the last whitespace within that head, else at the last UTF-8 character boundary within it;
   the rest is cut again by the same rule.
5. Every piece is stripped of surrounding whitespace, its inner whitespace runs become single spaces, and empty pieces are
   dropped.  Joining the segments' texts with single spaces gives back the input with its whitespace normalised and its tags
   replaced by a space (a word longer than ``max_bytes``, cut at a character boundary, comes back with a space in it).

A seam without a tag has ``pause_after_s`` None: the caller's default pause (0.25 s) applies.  A text without a tag that fits in
one segment comes back as one segment, and the front ends then take the unsegmented path (``SegmentPlan.create`` is None).
"""
from __future__ import annotations

import re
from dataclasses import dataclass, replace
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from .seam import pause_samples, segment_flags

MAX_TAG_S = 3.0       # one break tag (ElevenLabs' limit)
MAX_PAUSE_S = 10.0    # the pauses of consecutive tags at one seam, summed
DEFAULT_MAX_BYTES = 300
DEFAULT_PAUSE_S = 0.25
SEED_STEP = 0x9E3779B97F4A7C15

_BREAK = re.compile(r"""<break\s+time\s*=\s*(["'])\s*([0-9]*\.?[0-9]+)\s*(ms|s)\s*\1\s*/?\s*>""", re.IGNORECASE)
_SENT_END = re.compile(r"""[.!?…]+["'”’»)\]}]*(?=\s)""")
_CLAUSE = ",;:—"


class Segment(NamedTuple):
    text: str
    pause_after_s: Optional[float]  # None: the default pause (a seam) or no silence (after the last segment)
    pause_before_s: float = 0.0     # silence in front of the first segment (break tags before any text); 0 elsewhere


@dataclass
class SegmentOptions:
    """``segment=`` of the façade, the scheduler and the pool: ``max_bytes`` per segment, the pause of a seam without a break tag
    (``pause_s``) and ``context``: ``"previous"`` conditions segment k on segment k - 1, ``"none"`` on the voice alone."""
    max_bytes: int = DEFAULT_MAX_BYTES
    pause_s: float = DEFAULT_PAUSE_S
    context: str = "previous"

    def __post_init__(self):
        if int(self.max_bytes) < 4:
            raise ValueError(f"segment max_bytes must be >= 4, got {self.max_bytes!r}")
        if not 0.0 <= float(self.pause_s) <= MAX_TAG_S:
            raise ValueError(f"segment pause must be in [0, {MAX_TAG_S}] s, got {self.pause_s!r}")
        if self.context not in ("previous", "none"):
            raise ValueError(f"segment context must be 'previous' or 'none', got {self.context!r}")


def segment_options(segment) -> Optional[SegmentOptions]:
    """``segment=`` -> options: False / None: off; True: the defaults; a ``SegmentOptions`` or a dict of its fields."""
    if segment is None or segment is False:
        return None
    if segment is True:
        return SegmentOptions()
    if isinstance(segment, SegmentOptions):
        return segment
    if isinstance(segment, dict):
        return SegmentOptions(**segment)
    raise ValueError(f"segment must be a bool, a dict or a SegmentOptions, got {type(segment).__name__}")


def _ws(s: str) -> str:
    return " ".join(s.split())


def _nbytes(s: str) -> int:
    return len(s.encode("utf-8"))


def _sentences(text: str) -> List[str]:
    out = []
    for line in text.split("\n"):
        i = 0
        for m in _SENT_END.finditer(line):
            out.append(line[i:m.end()])
            i = m.end()
        out.append(line[i:])
    return [p for p in (_ws(s) for s in out) if p]


def _cut_long(s: str, max_bytes: int) -> List[str]:
    out = []
    while _nbytes(s) > max_bytes:
        head = s.encode("utf-8")[:max_bytes].decode("utf-8", errors="ignore")  # the longest head on a character boundary
        cut = max((head.rfind(c) + 1 for c in _CLAUSE), default=0)
        if cut <= 0 or not head[:cut].strip():
            ws = [i for i, ch in enumerate(head) if ch.isspace()]
            cut = ws[-1] if ws and head[:ws[-1]].strip() else len(head)
        if cut <= 0:
            cut = 1  # (max_bytes >= 4 holds any character)
        piece, s = _ws(s[:cut]), _ws(s[cut:])
        if piece:
            out.append(piece)
    if s:
        out.append(s)
    return out


def _pack(text: str, max_bytes: int) -> List[str]:
    segs: List[str] = []
    cur = ""
    for sent in _sentences(text):
        for piece in ([sent] if _nbytes(sent) <= max_bytes else _cut_long(sent, max_bytes)):
            joined = f"{cur} {piece}" if cur else piece
            if _nbytes(joined) <= max_bytes:
                cur = joined
            else:
                if cur:
                    segs.append(cur)
                cur = piece
    if cur:
        segs.append(cur)
    return segs


def _tag_seconds(m) -> float:
    v = float(m.group(2)) / (1000.0 if m.group(3).lower() == "ms" else 1.0)
    if not 0.0 <= v <= MAX_TAG_S:
        raise ValueError(f"break time {m.group(0)!r} is outside [0, {MAX_TAG_S:g}] s")
    return v


def split_text(text: str, max_bytes: int = DEFAULT_MAX_BYTES) -> List[Segment]:
    """``text`` -> its segments, by the rule in this module's docstring (deterministic)."""
    if int(max_bytes) < 4:
        raise ValueError(f"max_bytes must be >= 4, got {max_bytes!r}")
    pieces: List[str] = []
    pauses: List[float] = []  # pauses[i]: the tags between pieces[i] and pieces[i + 1], summed (pieces around tags)
    i = 0
    for m in _BREAK.finditer(text):
        pieces.append(text[i:m.start()])
        pauses.append(_tag_seconds(m))
        i = m.end()
    pieces.append(text[i:])
    lead = 0.0
    segs: List[list] = []  # [text, pause_after or None]
    for j, piece in enumerate(pieces):
        for s in _pack(piece, int(max_bytes)):
            segs.append([s, None])
        if j < len(pauses):
            if segs:
                segs[-1][1] = (segs[-1][1] or 0.0) + pauses[j]
            else:
                lead += pauses[j]
    for s in segs:
        if s[1] is not None and s[1] > MAX_PAUSE_S + 1e-9:
            raise ValueError(f"the break tags after {s[0][-20:]!r} add up to {s[1]:g} s, more than {MAX_PAUSE_S:g} s")
    if lead > MAX_PAUSE_S + 1e-9:
        raise ValueError(f"the break tags in front of the text add up to {lead:g} s, more than {MAX_PAUSE_S:g} s")
    if not segs:
        return []
    out = [Segment(t, p) for t, p in segs]
    if lead:
        out[0] = out[0]._replace(pause_before_s=lead)
    return out


def needs_segments(segments: List[Segment]) -> bool:
    """False when ``segments`` is what a plain request speaks: one segment, no pause anywhere."""
    return not (len(segments) == 1 and segments[0].pause_after_s is None and segments[0].pause_before_s == 0.0)


def segment_seed(seed: Optional[int], k: int) -> Optional[int]:
    """Segment k's seed: ``(seed + k * 0x9E3779B97F4A7C15) mod 2^64`` (None stays None); segment 0 keeps the request's seed."""
    if seed is None:
        return None
    return (int(seed) + k * SEED_STEP) % (1 << 64)


def chain_prompt(encoder, prefix: np.ndarray, text: str, prev_text: Optional[str] = None, prev_codes: Optional[np.ndarray] = None,
                 max_new_tokens: int = 1024, max_seq: int = 2048) -> np.ndarray:
    """Segment k's prompt grid: ``prefix`` (the voice's system or speaker turns, as ``build_prompt`` puts them in front), then --
    when ``prev_text`` / ``prev_codes`` are given and the prompt still fits (``P + context + turn + max_new_tokens + 2 <=
    max_seq``) -- segment k - 1's user turn and ``encode_vq`` of its semantic frames (n_codebooks, F), then segment k's user
    turn and the assistant header.  Without the context turns this is ``build_prompt`` exactly."""
    prefix = np.asarray(prefix, dtype=np.int32)
    turn = np.concatenate([encoder.encode_text_turn("user", text), encoder.encode_text_turn("assistant")], axis=1)
    parts = [prefix]
    if prev_text is not None and prev_codes is not None and np.asarray(prev_codes).shape[1] > 0:
        ctx = np.concatenate([encoder.encode_text_turn("user", prev_text),
                              encoder.encode_vq(np.asarray(prev_codes)[:8].astype(np.int64))], axis=1)
        if prefix.shape[1] + ctx.shape[1] + turn.shape[1] + int(max_new_tokens) + 2 <= int(max_seq):
            parts.append(ctx)
    parts.append(turn)
    return np.concatenate(parts, axis=1).astype(np.int32)


def voice_prefix(encoder, voice: str, sysprompt: Optional[np.ndarray] = None) -> np.ndarray:
    """The prefix ``build_prompt`` puts in front of the user turn: the speaker grid, or the preset's system turn."""
    if sysprompt is not None:
        return np.asarray(sysprompt, dtype=np.int32)
    from .prompt import VOICE_MAP

    return encoder.encode_text_turn("system", f"<|speaker:{VOICE_MAP.get(voice, 0)}|>")


@dataclass(frozen=True)
class SegmentPlan:
    """A segmented request's segments and what follows from them, for every front end: segment k's prompt, seam arguments and
    sampling, and the blocking join's pauses, lead and trail (all in samples at 24 kHz)."""
    opts: SegmentOptions
    segs: Tuple[Segment, ...]

    @classmethod
    def create(cls, text: str, opts: SegmentOptions) -> Optional["SegmentPlan"]:
        """The plan of ``text``, or None where the plain path runs (one segment without break tags)."""
        segs = split_text(text, opts.max_bytes)
        if not segs:
            raise ValueError("the text has nothing to speak")
        return cls(opts, tuple(segs)) if needs_segments(segs) else None

    @property
    def pauses(self) -> List[int]:
        """The seam after every segment but the last: its break tags, or the default pause."""
        return [pause_samples(s.pause_after_s if s.pause_after_s is not None else self.opts.pause_s) for s in self.segs[:-1]]

    @property
    def lead(self) -> int:
        return pause_samples(self.segs[0].pause_before_s)

    @property
    def trail(self) -> int:
        return pause_samples(self.segs[-1].pause_after_s)

    def seam_args(self, k: int) -> Tuple[int, int, int]:
        """(pause, flags, lead) that open segment k in the seam stage."""
        n = len(self.segs)
        return (self.trail if k == n - 1 else self.pauses[k]), segment_flags(k, n), self.lead

    def prompt(self, k: int, encoder, prefix: np.ndarray, prev: Optional[Tuple[str, np.ndarray]], max_new_tokens: int,
               max_seq: int) -> np.ndarray:
        """Segment k's prompt: ``prev`` (segment k - 1's text and codes, None for segment 0) is its context unless the options
        say ``context="none"``."""
        ctx = prev if prev is not None and self.opts.context == "previous" else (None, None)
        return chain_prompt(encoder, prefix, self.segs[k].text, *ctx, max_new_tokens=max_new_tokens, max_seq=max_seq)

    @staticmethod
    def sampling(k: int, base):
        """Segment k's copy of ``base`` (a resolved ``RequestSampling``, or ``GenerationSettings``) with ``segment_seed``."""
        return replace(base, seed=segment_seed(base.seed, k))
