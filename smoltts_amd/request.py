"""One parse of a speech request's options, shared by every front end (``SmolTTS``, ``BatchScheduler``, ``GpuPool``, the HTTP
core): the checks and their ``ValueError`` messages live here once, and the front ends only route the normalised values."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

from .formats import ENC_OFF, check_container, parse_stream_format
from .longform import SegmentOptions, SegmentPlan, segment_options
from .limiter import ceiling_of_db, check_peak_limit
from .loudness import check_start_gain, check_target
from .trim import pause_blocks, threshold
from .tsm import parse_speed


@dataclass(frozen=True)
class SpeechOptions:
    output_format: Optional[str]     # pcm_<rate> / ulaw_8000 converted on the GPU; None: the codec's float32 at 24 kHz
    speed: Optional[float]           # the speed asked for, None at speed 1
    speed_q: Optional[int]           # the same in Q16 (tsm.py)
    container: Optional[str]         # "flac", or None
    segment: Optional[SegmentOptions]
    plan: Optional[SegmentPlan]      # None: the plain path (no segment options, or a text that is one plain segment)
    loudness: Optional[float] = None  # target in LUFS (loudness.py), None: the level is left as it is
    start_gain_db: float = 0.0        # a stream's first gain knot, on the knot grid
    watermark: Optional[bool] = None  # mark the audio with the front end's key (watermark.py); None: the front end's policy
    trim_silence: bool = False        # cut the leading and trailing silence (trim.py)
    max_pause_s: Optional[float] = None           # cap the pauses at this length, None: pauses are left alone
    silence_threshold_db: Optional[float] = None  # what counts as silence, in dBFS; None: the seam's 2^-8
    pause_blocks: int = 0             # max_pause_s in blocks (0: no cap)
    silence_thr: float = float(threshold(None))   # silence_threshold_db as a float32 amplitude
    timestamps: bool = False          # character timestamps from the slow attention (align.py); blocking requests only
    peak_limit_db: Optional[float] = None  # the ceiling of the peak limiter in dBFS (limiter.py), None: no limiter
    loudness_start_gain_db: Optional[float] = None  # start_gain_db as the caller gave it, None: not given

    def given(self) -> dict:
        """The options that are on, as ``parse_request`` keywords: ``parse_request(text, stream, **p.given()) == p`` (the plans
        compared by their segments).  This is how the value crosses a process boundary (``GpuPool``) and how the HTTP core
        hands it to a front end; a request with no option gives ``{}``."""
        kw = {"output_format": self.output_format, "speed": self.speed, "container": self.container, "segment": self.segment,
              "loudness": self.loudness, "loudness_start_gain_db": self.loudness_start_gain_db, "watermark": self.watermark,
              "trim_silence": self.trim_silence or None, "max_pause_s": self.max_pause_s,
              "silence_threshold_db": self.silence_threshold_db, "timestamps": self.timestamps or None,
              "peak_limit_db": self.peak_limit_db}
        return {k: v for k, v in kw.items() if v is not None}

    @property
    def ceiling(self) -> float:
        """The limiter's ceiling as an amplitude, 10^(peak_limit_db / 20); 0.0 without one (``SlotRoute.ceiling``)."""
        return 0.0 if self.peak_limit_db is None else ceiling_of_db(self.peak_limit_db)

    @property
    def trims(self) -> bool:
        """Whether the request goes through the trim stage at all."""
        return self.trim_silence or self.pause_blocks > 0

    @property
    def trim_route(self) -> Optional[Tuple[bool, int, float]]:
        """What ``stages.trim_pcm`` and ``StreamConverter.reset_slots`` take for the request (None: it does not trim)."""
        return (self.trim_silence, self.pause_blocks, self.silence_thr) if self.trims else None


def parse_request(text: str = "", stream: bool = False, output_format: Optional[str] = None, speed: Optional[float] = None,
                  container: Optional[str] = None, segment=None, loudness: Optional[float] = None,
                  loudness_start_gain_db: Optional[float] = None, watermark: Optional[bool] = None,
                  trim_silence: Optional[bool] = None, max_pause_s: Optional[float] = None,
                  silence_threshold_db: Optional[float] = None, timestamps: Optional[bool] = None,
                  pieces: bool = False, peak_limit_db: Optional[float] = None) -> SpeechOptions:
    """A request's options checked and normalised; ``ValueError`` for anything a front end refuses.  Every front end takes these
    keywords as its ``**options`` and hands them here whole, so this is the one list of the options and their ranges; a name
    that is not in it is a ``TypeError``.  ``output_format`` (``pcm_8000 / 16000 / 22050 / 44100 / 48000``: int16 chunks,
    ``ulaw_8000``: uint8 chunks; None / ``pcm_24000``: the codec's float32) and ``container`` (``"flac"``: FLAC frames of the
    stream's 16-bit samples, uint8 chunks behind one stream header) apply to streaming requests only, as does
    ``loudness_start_gain_db`` (within +-20 dB, default 0: the gain a stream starts from), which needs a ``loudness``.
    ``speed`` (0.25 to 4.0; None / 1.0: unchanged): the pitch-preserving time stretch (tsm.py).  ``segment`` (True, a dict or a
    ``longform.SegmentOptions``; None / False: off): a long text is spoken as chained segments (longform.py).  ``loudness``
    (a target in LUFS, -40 to -5; None: the level is left alone): BS.1770-4 normalisation (loudness.py).  ``watermark``: true, false, or None for the
    front end's own policy (the key and the strength are the front end's: one key per stage).  ``trim_silence`` (true, false or
    None: false), ``max_pause_s`` (0.1 to 2.0 seconds, None: no cap) and ``silence_threshold_db`` (-72 to -6 dBFS, which needs
    one of the other two) are the trim stage's (trim.py).  ``timestamps`` (true, false or None: false): character timestamps
    (align.py), for blocking requests of one utterance whose frames keep their place in the output: refused with ``segment``,
    with ``trim_silence`` / ``max_pause_s`` (the seam and the trim stage cut samples where the audio says so), with a stream, and
    with text fed in pieces (``pieces``: the front end's text is an iterator).  ``peak_limit_db`` (-12 to 0 dBFS, None: none):
    the ceiling of the peak limiter (limiter.py), the last float stage; it goes with every other option, because the stage
    copies samples one to one and only delays them."""
    speed_q = parse_speed(speed)
    peak_limit_db = check_peak_limit(peak_limit_db)
    if output_format is not None:
        if not stream:
            raise ValueError("output_format applies to streaming requests")
        if parse_stream_format(output_format)[1] == ENC_OFF:
            output_format = None
    if container is not None:
        if not stream:
            raise ValueError("container applies to streaming requests")
        check_container(container, output_format)
    opts = segment_options(segment)
    plan = SegmentPlan.create(text, opts) if opts is not None else None
    target = check_target(loudness)
    if loudness_start_gain_db is not None and (target is None or not stream):
        raise ValueError("loudness_start_gain_db applies to streaming requests with a loudness")
    if watermark is not None and not isinstance(watermark, bool):
        raise ValueError("watermark must be true, false or null")
    if trim_silence is not None and not isinstance(trim_silence, bool):
        raise ValueError("trim_silence must be true or false")
    for name, v in (("max_pause_s", max_pause_s), ("silence_threshold_db", silence_threshold_db)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float))):
            raise ValueError(f"{name} must be a number")
    blocks = pause_blocks(max_pause_s)
    if silence_threshold_db is not None and not (trim_silence or blocks):
        raise ValueError("silence_threshold_db applies with trim_silence or max_pause_s")
    if timestamps is not None and not isinstance(timestamps, bool):
        raise ValueError("timestamps must be true or false")
    if timestamps:
        if pieces:
            raise ValueError("timestamps cannot be combined with text fed in pieces: the seam cuts samples where the audio says so")
        if opts is not None:
            raise ValueError("timestamps cannot be combined with segment: the seam cuts samples where the audio says so")
        if trim_silence or blocks:
            raise ValueError("timestamps cannot be combined with trim_silence or max_pause_s: the trim stage cuts samples where the audio says so")
        if stream:
            raise ValueError("timestamps apply to blocking requests (a stream needs a causal fit)")
    return SpeechOptions(output_format, None if speed_q is None else float(speed), speed_q, container, opts, plan, target,
                         check_start_gain(loudness_start_gain_db), watermark, bool(trim_silence),
                         None if max_pause_s is None else float(max_pause_s),
                         None if silence_threshold_db is None else float(silence_threshold_db), blocks,
                         float(threshold(silence_threshold_db)), bool(timestamps), peak_limit_db,
                         None if loudness_start_gain_db is None else float(loudness_start_gain_db))
