"""The server's settings file, same schema and validation as the reference (server/settings.py:12-63): exactly one of
``model_id`` / ``checkpoint_dir``, a ``generation`` block (lm/generate.py:12-16) and a ``model_type`` block
(lm/config.py:5-12).  Extensions of this build: ``mimi_checkpoint`` (the reference downloads kyutai/mimi; there is no
network here), ``max_batch`` (slots per GPU), ``weight_format`` ("bf16" | "fp8"), ``max_voices`` (cloned voices held at once),
``long_text`` / ``segment_max_bytes`` / ``seam_pause_ms`` / ``max_input_chars`` (long texts as chained segments),
``idle_timeout_s`` / ``flush_after_s`` (text fed in pieces), ``watermark`` (a keyed mark on the audio).  ``model_id`` is accepted by the schema
but cannot be resolved without network access; ``get_checkpoint_dir`` says so."""
from __future__ import annotations

import json
from pathlib import Path
from typing import List, Literal, Optional, Tuple

from pydantic import BaseModel, Field, model_validator

from ..config import GenerationSettings as _GenerationSettings


class ModelType(BaseModel):
    family: Literal["fish", "dual_ar"] = "dual_ar"
    version: Optional[Literal["1.5", "1.4", "1.2"]] = None
    codec: Literal["mimi", "1.4", "1.2"] = "mimi"


class GenerationBlock(BaseModel):
    default_temp: float = 0.5
    default_fast_temp: Optional[float] = 0.0
    min_p: Optional[float] = 0.10
    max_new_tokens: int = Field(default=1024, ge=1)
    # extension: "reference" = what lm/utils/samplers.py:22-28 computes (its threshold never removes a token, so the draw is
    # categorical over logits / temp); "intended" = keep p >= min_p * p_max.  The drop-in default is the reference's behaviour.
    min_p_mode: Literal["reference", "intended"] = "reference"
    # extension: the filters of sampled picks that a request's body does not name (config.RequestSampling); all off
    top_p: float = Field(default=1.0, gt=0, le=1)
    top_k: int = Field(default=0, ge=0, lt=2**31)
    repetition_penalty: float = Field(default=1.0, ge=1, le=10)
    repetition_window: int = Field(default=16, ge=1, le=64)
    # extension: the length control of requests whose body does not name it (config.RequestSampling); both off
    min_frames: int = Field(default=0, ge=0, le=1024)
    eos_bias: float = Field(default=0.0, ge=-100, le=100, allow_inf_nan=False)

    def to_settings(self) -> _GenerationSettings:
        return _GenerationSettings(default_temp=self.default_temp, default_fast_temp=self.default_fast_temp, min_p=self.min_p,
                                   max_new_tokens=self.max_new_tokens, min_p_mode=self.min_p_mode, top_p=self.top_p, top_k=self.top_k,
                                   repetition_penalty=self.repetition_penalty, repetition_window=self.repetition_window,
                                   min_frames=self.min_frames, eos_bias=self.eos_bias)


class WatermarkBlock(BaseModel):
    """The server's watermark (watermark.py): ``key`` is 16 hex digits and is never logged or returned,
    ``strength_db`` the mark's level under the speech, ``apply`` which requests are marked: ``"all"``, or ``"cloned"``: only those
    that speak a voice registered through ``POST /v1/voices/add``."""
    key: str = Field(pattern=r"^[0-9a-fA-F]{16}$", repr=False)
    strength_db: float = Field(default=-26.0, ge=-40.0, le=-20.0, allow_inf_nan=False)
    apply: Literal["all", "cloned"] = "all"

    def to_watermark(self):
        from ..watermark import Watermark

        return Watermark(int(self.key, 16), self.strength_db)


def watermark_setting(value) -> Optional[WatermarkBlock]:
    """The ``watermark`` setting as a block: None, a ``WatermarkBlock`` or the dict it is made from (``ValueError`` for a bad one)."""
    if value is None or isinstance(value, WatermarkBlock):
        return value
    return WatermarkBlock(**value)


class ServerSettings(BaseModel):
    model_id: Optional[str] = None
    checkpoint_dir: Optional[str] = None
    generation: GenerationBlock = Field(default_factory=GenerationBlock)
    model_type: ModelType = Field(default_factory=ModelType)
    mimi_checkpoint: Optional[str] = None
    max_batch: int = Field(default=32, ge=1, le=256)
    weight_format: Literal["bf16", "fp8"] = "bf16"
    # (not in the reference's settings) bf16x3 products per operand pair in the codec's matrix-core kernels: 6 = fp32-grade (the
    # reference's codec runs fp32), 3 = the 2^-16-grade form: chunks 23 % faster, PCM RMS error 7e-7 (SMOLTTS_MIMI_OPT_PRODUCTS)
    codec_products: Literal[3, 6] = 6
    # (extension) cloned voices a server holds at once (POST /v1/voices/add); each costs its speaker prompt's KV rows on every GPU,
    # P x 20 KB at 150m (P: about 12.5 positions per second of reference audio, plus the transcripts)
    max_voices: int = Field(default=64, ge=0)
    # (extension) a text too long for one prompt: "refuse" answers 400 as before; "segment" speaks it as chained sentence segments
    # of at most segment_max_bytes UTF-8 bytes joined on the GPU with seam_pause_ms between them, break tags honoured
    # (longform.py); inputs over max_input_chars are then refused with 400.
    long_text: Literal["refuse", "segment"] = "refuse"
    segment_max_bytes: int = Field(default=300, ge=16, le=1000)
    seam_pause_ms: int = Field(default=250, ge=0, le=3000)
    max_input_chars: int = Field(default=5000, ge=1)
    # (extension) the loudness target in LUFS of requests whose body names none (loudness.py); null: the level is
    # left as the model gives it
    loudness: Optional[float] = Field(default=None, ge=-40.0, le=-5.0)
    # (extension) silence trimming of requests whose body does not say (trim.py): cut the leading and trailing
    # silence; cap the pauses at max_pause_s seconds (null: pauses are left alone)
    trim_silence: bool = False
    max_pause_s: Optional[float] = Field(default=None, ge=0.1, le=2.0)
    # (extension) the ceiling in dBFS of the look-ahead peak limiter for requests whose body names none (limiter.py, DESIGN.md
    # 22); null: no limiter.  A blocking response that was limited carries X-Peak-Reduction-Db
    peak_limit_db: Optional[float] = Field(default=None, ge=-12.0, le=0.0)

    # (extension) a keyed watermark added to the audio on the GPU; null: none.  {"key": "<16 hex digits>", "strength_db": -26.0,
    # "apply": "all" | "cloned"}; marked responses carry X-Watermark: 1, and POST /v1/watermark/detect tests a recording
    watermark: Optional[WatermarkBlock] = None

    # (extension) requests whose text is fed in pieces (POST .../stream-input): a slot that has waited this long for
    # text is closed as if its text had ended; with flush_after_s, text that has stopped arriving short of a sentence end for that
    # long is spoken as it is
    idle_timeout_s: float = Field(default=10.0, gt=0, allow_inf_nan=False)
    flush_after_s: Optional[float] = Field(default=None, gt=0, allow_inf_nan=False)

    # (extension) bounds on every utterance's length from its text's UTF-8 byte count n, per segment on the long-text path
    # (config.length_bounds): min_frames = max(request's, floor(n * min_frames_per_byte)), at most the cap - 1;
    # max_new_tokens = min(request's, ceil(n * max_frames_per_byte)), at least 1.  12.5 frames are one second of audio; the
    # ratios depend on the checkpoint's speaking rate and are the operator's to measure: null (off) by default
    min_frames_per_byte: Optional[float] = Field(default=None, ge=0, allow_inf_nan=False)
    max_frames_per_byte: Optional[float] = Field(default=None, ge=0, allow_inf_nan=False)

    # (extension) the most takes a request's ``best_of`` may ask for; a body above it is answered 400.  Every take
    # holds a slot for its whole length
    max_best_of: int = Field(default=4, ge=1, le=8)

    # (extension) the (layer, head) pairs of the slow attention that character timestamps are read from: at most 16
    # [layer, head] pairs; null (default): POST /v1/text-to-speech/{voice_id}/with-timestamps answers 501.  Which heads of a
    # checkpoint track the text is the operator's to find: python -m smoltts_amd.align rank --checkpoint DIR --texts FILE
    alignment_heads: Optional[List[Tuple[int, int]]] = Field(default=None, max_length=16)

    # (extension) how many frames (80 ms each) behind its audio a streamed character timestamp is committed:
    # POST /v1/text-to-speech/{voice_id}/stream/with-timestamps.  A committed time is never revised; a longer lag sees more
    timestamp_lag_frames: int = Field(default=6, ge=1, le=64)

    model_config = {"protected_namespaces": ()}

    @model_validator(mode="after")
    def validate_model_source(self):
        if self.model_id is not None and self.checkpoint_dir is not None:
            raise ValueError("Cannot specify both model_id and checkpoint_dir")
        if self.model_id is None and self.checkpoint_dir is None:
            raise ValueError("Must specify either model_id or checkpoint_dir")
        if self.model_type.family != "dual_ar" or self.model_type.codec != "mimi":
            raise ValueError("this build serves the dual_ar family with the mimi codec only")
        return self

    @classmethod
    def get_settings(cls, config_path: Optional[str]) -> "ServerSettings":
        if not config_path:
            raise ValueError("pass --config: the default settings name a Hugging Face model_id, which needs network access")
        return cls(**json.loads(Path(config_path).read_text()))

    def get_checkpoint_dir(self) -> Path:
        if self.checkpoint_dir is None:
            raise ValueError(f"model_id={self.model_id!r} would be downloaded from the Hugging Face hub; there is no network access: "
                             "set checkpoint_dir")
        return Path(self.checkpoint_dir)
