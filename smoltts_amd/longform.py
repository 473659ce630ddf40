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
_SENT_RUN = re.compile(r"""(?:[.!?…]+["'”’»)\]}]*)?\Z""")  # the sentence end a text may be ending in
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


def _cut_once(s: str, max_bytes: int) -> Tuple[str, str]:
    """One cut of a normalised sentence longer than ``max_bytes`` (rule 4): (its head, the rest), both normalised.  The head
    depends on the first ``max_bytes`` bytes of ``s`` alone."""
    head = s.encode("utf-8")[:max_bytes].decode("utf-8", errors="ignore")  # the longest head on a character boundary
    cut = max((head.rfind(c) + 1 for c in _CLAUSE), default=0)
    if cut <= 0 or not head[:cut].strip():
        ws = [i for i, ch in enumerate(head) if ch.isspace()]
        cut = ws[-1] if ws and head[:ws[-1]].strip() else len(head)
    if cut <= 0:
        cut = 1  # (max_bytes >= 4 holds any character)
    return _ws(s[:cut]), _ws(s[cut:])


def _cut_long(s: str, max_bytes: int) -> List[str]:
    out = []
    while _nbytes(s) > max_bytes:
        piece, s = _cut_once(s, max_bytes)
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

    def length_bounds(self, k: int, sampling, max_new_tokens: int, min_frames_per_byte: Optional[float] = None,
                      max_frames_per_byte: Optional[float] = None):
        """(sampling, max_new_tokens) of segment k under the bounds from its own text's length (``config.length_bounds``): every
        segment is an utterance whose frame counter starts at 0."""
        from .config import length_bounds

        return length_bounds(self.segs[k].text, sampling, max_new_tokens, min_frames_per_byte, max_frames_per_byte)


# ---------------------------------------------------------------------------------- text that arrives in pieces
def _tag_may_follow(s: str) -> bool:
    """Whether ``s`` (from a ``<`` to the end of what has arrived, no match of ``_BREAK`` at its start) may still grow into a
    break tag: every character of it fits the tag's grammar so far."""
    n = len(s)
    i = 0

    def lit(word):
        nonlocal i
        for c in word:
            if i == n:
                return True
            if s[i].lower() != c:
                return False
            i += 1
        return True

    def ws():
        nonlocal i
        while i < n and s[i].isspace():
            i += 1

    if not lit("<break"):
        return False
    if i == n:
        return True
    if not s[i].isspace():
        return False
    ws()
    if not lit("time"):
        return False
    ws()
    if not lit("="):
        return False
    ws()
    if i == n:
        return True
    quote = s[i]
    if quote not in "\"'":
        return False
    i += 1
    ws()
    j = i
    while i < n and s[i] in "0123456789":
        i += 1
    if i < n and s[i] == ".":
        i += 1
        k = i
        while i < n and s[i] in "0123456789":
            i += 1
        if i < n and i == k:  # a dot needs a digit behind it
            return False
    elif i < n and i == j:    # no digit and no dot
        return False
    ws()
    if i == n:
        return True
    if s[i].lower() == "m":
        i += 1
        if not lit("s"):
            return False
    elif not lit("s"):
        return False
    ws()
    if i == n:
        return True
    if s[i] != quote:
        return False
    i += 1
    ws()
    if i < n and s[i] == "/":
        i += 1
    ws()
    return i == n  # (the closing '>' would have matched _BREAK)


def _first_piece_bytes(p: str) -> int:
    """A lower bound of the bytes of the first piece that a sentence beginning with the normalised ``p`` (within ``max_bytes``)
    gives the packing rule, however it goes on: the sentence itself, or its head by rule 4 -- a cut behind its last clause
    mark, which later ones only move back; without one, at its last whitespace or behind ``p``."""
    cut = max(p.rfind(c) + 1 for c in _CLAUSE)
    if cut <= 0:
        ws = p.rfind(" ")
        cut = ws if ws > 0 else len(p)
    return _nbytes(_ws(p[:cut]))


class _Flush:
    def __repr__(self):
        return "longform.FLUSH"


FLUSH = _Flush()  # in an iterator of text pieces (``SmolTTS.stream``): speak what is buffered now


class IncrementalSplitter:
    """``split_text`` for a text that arrives in pieces: ``feed(piece)`` returns the segments that no later input can change,
    ``close()`` the rest.  For any text and any way of cutting it into pieces -- ``str``, or ``bytes`` of its UTF-8, which may
    cut a character -- everything ``feed`` returned followed by what ``close`` returns is ``split_text(text, opts.max_bytes)``.

    A segment is returned as soon as it is settled: its sentence end and the whitespace behind it have arrived (or a newline, or
    a sentence has outgrown ``max_bytes`` and is cut by the rule of ``_cut_long``), the segment behind it has been opened by the
    packing rule, and, for a segment in front of a break tag, the first text behind the tags has arrived (consecutive tags add
    up).  A ``<`` that may be the start of a break tag is held until it is one or cannot be.  ``ValueError`` as ``split_text``
    raises it, from the call that sees the bad tag.

    ``flush()`` speaks what is buffered now as if the text ended there (and then carries on): those segments need not be the
    whole text's."""

    def __init__(self, opts: Optional[SegmentOptions] = None):
        import codecs

        self.opts = opts or SegmentOptions()
        self.max_bytes = int(self.opts.max_bytes)
        self._dec = codecs.getincrementaldecoder("utf-8")(errors="replace")
        self._pend = ""       # from a '<' that may become a break tag
        self._raw = ""        # the unsettled text of the sentence that is arriving
        self._cur = ""        # the segment being packed
        self._last: Optional[list] = None  # [text, pause]: the segment in front of break tags, until text follows them
        self._lead = 0.0      # break tags in front of the first segment
        self._made = 0        # segments made so far (``_last`` included)
        self._emitted = 0     # segments handed out so far
        self._out: List[Segment] = []
        self.closed = False

    # -- the client's calls
    def feed(self, text) -> List[Segment]:
        if self.closed:
            raise ValueError("the text is closed")
        s = self._dec.decode(bytes(text)) if isinstance(text, (bytes, bytearray, memoryview)) else self._dec.decode(b"") + str(text)
        self._scan(self._pend + s, end=False)
        return self._take()

    def flush(self) -> List[Segment]:
        """The buffered remainder as segments, now (a character cut across two ``bytes`` pieces stays buffered)."""
        if self.closed:
            return []
        self._scan(self._pend, end=True)
        self._end_piece()
        self._emit_last()
        return self._take()

    def close(self) -> List[Segment]:
        if self.closed:
            return []
        self._scan(self._pend + self._dec.decode(b"", final=True), end=True)
        self._end_piece()
        self._emit_last()
        self.closed = True
        return self._take()

    @property
    def pending(self) -> bool:
        """Whether text that will be spoken is buffered: a later segment is certain."""
        return bool(self._cur or self._raw.strip() or self._last is not None)

    # -- tags and text
    def _take(self) -> List[Segment]:
        out, self._out = self._out, []
        return out

    def _scan(self, buf: str, end: bool) -> None:
        self._pend = ""
        start = i = 0
        while True:
            i = buf.find("<", i)
            if i < 0:
                break
            m = _BREAK.match(buf, i)
            if m is not None:
                self._text(buf[start:i])
                self._tag(_tag_seconds(m))
                start = i = m.end()
            elif not end and _tag_may_follow(buf[i:]):
                self._text(buf[start:i])
                self._pend = buf[i:]
                return
            else:
                i += 1
        self._text(buf[start:])

    def _tag(self, seconds: float) -> None:
        self._end_piece()
        if self._last is not None:
            self._last[1] = (self._last[1] or 0.0) + seconds
            if self._last[1] > MAX_PAUSE_S + 1e-9:
                raise ValueError(f"the break tags after {self._last[0][-20:]!r} add up to {self._last[1]:g} s, more than {MAX_PAUSE_S:g} s")
        else:  # (text arrives only behind an emitted ``_last``: none here means no segment yet)
            self._lead += seconds
            if self._lead > MAX_PAUSE_S + 1e-9:
                raise ValueError(f"the break tags in front of the text add up to {self._lead:g} s, more than {MAX_PAUSE_S:g} s")

    def _text(self, s: str) -> None:
        if not s:
            return
        if self._last is not None and s.strip():
            self._emit_last()  # text follows its tags: its pause is settled
        raw = self._raw + s
        # complete lines, by the rule of ``_sentences``
        while "\n" in raw:
            line, raw = raw.split("\n", 1)
            i = 0
            for m in _SENT_END.finditer(line):
                self._sentence(line[i:m.end()])
                i = m.end()
            self._sentence(line[i:])
        i = 0
        for m in _SENT_END.finditer(raw):  # (a match has its whitespace behind it: nothing later changes it)
            self._sentence(raw[i:m.end()])
            i = m.end()
        raw = raw[i:]
        # a sentence that has outgrown the cap is cut as ``_cut_long`` cuts it: its heads depend on nothing behind them
        norm = _ws(raw)
        if _nbytes(norm) > self.max_bytes:
            trail = raw[-1:].isspace()
            # ... except a cut inside the sentence end that may be arriving at the end of the text so far (`."` with its
            # whitespace still to come): the rest would no longer show it.  The next character decides
            run = 0 if trail else len(_SENT_RUN.search(norm).group(0))
            while _nbytes(norm) > self.max_bytes:
                piece, rest = _cut_once(norm, self.max_bytes)
                if len(rest) < run:
                    break
                norm = rest
                if piece:
                    self._piece(piece)
            raw = norm + (" " if trail else "")
        elif self._cur and norm and _first_piece_bytes(norm) > self.max_bytes - _nbytes(self._cur) - 1:
            self._segment(self._cur, None)  # whatever follows, the arriving sentence's first piece opens the next segment
            self._cur = ""
        self._raw = raw

    def _sentence(self, s: str) -> None:
        s = _ws(s)
        if s:
            for piece in _cut_long(s, self.max_bytes):
                self._piece(piece)

    def _piece(self, piece: str) -> None:
        joined = f"{self._cur} {piece}" if self._cur else piece
        if _nbytes(joined) <= self.max_bytes:
            self._cur = joined
        else:
            if self._cur:
                self._segment(self._cur, None)
            self._cur = piece

    def _end_piece(self) -> None:
        """The text between two tags (or in front of the end) is complete: its last sentence, its last segment."""
        raw, self._raw = self._raw, ""
        self._sentence(raw)
        if self._cur:
            cur, self._cur = self._cur, ""
            self._emit_last()
            self._last = [cur, None]
            self._made += 1

    def _segment(self, text: str, pause: Optional[float]) -> None:
        self._emit_last()
        self._made += 1
        self._put(text, pause)

    def _emit_last(self) -> None:
        if self._last is not None:
            (text, pause), self._last = self._last, None
            self._put(text, pause)

    def _put(self, text: str, pause: Optional[float]) -> None:
        self._out.append(Segment(text, pause, self._lead if self._emitted == 0 else 0.0))
        self._emitted += 1


class GrowingPlan:
    """A ``SegmentPlan`` whose segments arrive one by one (``IncrementalSplitter``), for a request fed in pieces: ``extend`` adds
    segments, ``close`` says that none will follow.  Segment k is *final* once the plan is closed and k is its last; until
    then it is opened as a segment with a seam behind it -- its own break tags, or the default pause."""

    def __init__(self, opts: SegmentOptions):
        self.opts = opts
        self.segs: List[Segment] = []
        self.closed = False

    def extend(self, segs) -> None:
        if self.closed:
            raise ValueError("the text is closed")
        self.segs.extend(segs)

    def close(self) -> None:
        self.closed = True

    def final(self, k: int) -> bool:
        return self.closed and k == len(self.segs) - 1

    @property
    def lead(self) -> int:
        return pause_samples(self.segs[0].pause_before_s)

    def seam_args(self, k: int) -> Tuple[int, int, int]:
        """(pause, flags, lead) that open segment k in the seam stage now: ``SegmentPlan.seam_args`` of the whole text once it is
        known whether segment k is the last."""
        from .seam import FINAL, FIRST

        s, fin = self.segs[k], self.final(k)
        pause = pause_samples(s.pause_after_s if fin or s.pause_after_s is not None else self.opts.pause_s)
        return pause, (FIRST if k == 0 else 0) | (FINAL if fin else 0), self.lead

    prompt = SegmentPlan.prompt
    sampling = staticmethod(SegmentPlan.sampling)
    length_bounds = SegmentPlan.length_bounds
