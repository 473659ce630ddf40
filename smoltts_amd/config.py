"""Model / token / generation configuration for the DualAR hot path.

Mirrors the reference's config surface so a reference checkpoint directory loads unchanged:

* ``RQTransformerModelArgs``  <- modeling/model/rq_transformer.py:25-114 (dataclass, derived
  defaults in ``__post_init__``) and its pydantic twin mlx_inference/.../lm/rq_transformer.py:10-48.
  Unknown JSON keys are ignored (the MLX twin ignores extras; training-only keys such as
  ``dropout`` / ``initializer_range`` / ``is_reward_model`` are accepted and kept).
* ``TokenConfig``             <- lm/rq_transformer.py:51-89.
* ``GenerationSettings``      <- lm/generate.py:12-16.
* ``ModelType``               <- lm/config.py:5-12.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field, fields
from pathlib import Path
from typing import Optional


def find_multiple(n: int, k: int) -> int:
    return n if n % k == 0 else n + k - (n % k)


@dataclass
class RQTransformerModelArgs:
    model_type: str = "dual_ar"

    vocab_size: int = 32000
    n_layer: int = 32
    n_head: int = 32
    dim: int = 4096
    intermediate_size: Optional[int] = 16_384
    n_local_heads: int = -1
    head_dim: int = 64
    rope_base: float = 10000
    norm_eps: float = 1e-5
    max_seq_len: int = 2048
    dropout: float = 0.0
    tie_word_embeddings: bool = True
    attention_qkv_bias: bool = False

    codebook_size: int = 160
    num_codebooks: int = 4

    use_gradient_checkpointing: bool = False
    initializer_range: float = 0.02
    is_reward_model: bool = False
    share_codebook_embeddings: bool = True
    scale_codebook_embeddings: bool = False

    fast_dim: Optional[int] = 1024
    n_fast_layer: int = 4
    fast_n_head: Optional[int] = 16
    fast_n_local_heads: Optional[int] = None
    fast_head_dim: Optional[int] = None
    fast_intermediate_size: Optional[int] = None
    fast_attention_qkv_bias: Optional[bool] = None
    depthwise_wte: Optional[bool] = False
    depthwise_output: Optional[bool] = False
    duplicate_code_0: Optional[bool] = True

    def __post_init__(self):
        if self.n_local_heads == -1:
            self.n_local_heads = self.n_head
        if self.intermediate_size is None:
            self.intermediate_size = find_multiple(int(2 * 4 * self.dim / 3), 256)
        self.head_dim = self.dim // self.n_head
        self.fast_dim = self.fast_dim or self.dim
        self.fast_n_head = self.fast_n_head or self.n_head
        self.fast_n_local_heads = self.fast_n_local_heads or self.n_local_heads
        self.fast_head_dim = self.fast_head_dim or self.head_dim
        self.fast_intermediate_size = self.fast_intermediate_size or self.intermediate_size
        self.fast_attention_qkv_bias = (
            self.fast_attention_qkv_bias
            if self.fast_attention_qkv_bias is not None
            else self.attention_qkv_bias
        )
        if self.duplicate_code_0 is None:
            self.duplicate_code_0 = True
        self.depthwise_wte = bool(self.depthwise_wte)
        self.depthwise_output = bool(self.depthwise_output)

    # ---- derived
    @property
    def max_fast_seqlen(self) -> int:
        return self.num_codebooks - (0 if self.duplicate_code_0 else 1)

    @property
    def grid_height(self) -> int:
        """Rows of the prompt / frame grid: 1 text row + code rows (9 when code 0 is duplicated)."""
        return 1 + self.max_fast_seqlen

    # ---- io
    @classmethod
    def from_dict(cls, data: dict) -> "RQTransformerModelArgs":
        known = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in data.items() if k in known})

    @classmethod
    def from_json_file(cls, path) -> "RQTransformerModelArgs":
        p = Path(path)
        if p.is_dir():
            p = p / "config.json"
        with open(p, "r", encoding="utf-8") as f:
            return cls.from_dict(json.load(f))

    from_pretrained = from_json_file

    def save(self, path) -> None:
        with open(path, "w") as f:
            json.dump(self.__dict__, f, indent=4, sort_keys=True, ensure_ascii=False)

    def validate_for_engine(self) -> None:
        """What the HIP engine supports; anything else fails loudly instead of mis-computing."""
        errs = []
        if self.head_dim != 64 or self.fast_head_dim != 64:
            errs.append("head_dim and fast_head_dim must be 64")
        if self.attention_qkv_bias or self.fast_attention_qkv_bias:
            errs.append("qkv bias is not supported")
        for name in ("dim", "fast_dim", "intermediate_size", "fast_intermediate_size"):
            if getattr(self, name) % 32:
                errs.append(f"{name} must be a multiple of 32")
        if self.n_head % self.n_local_heads or self.fast_n_head % self.fast_n_local_heads:
            errs.append("n_head must be a multiple of n_local_heads")
        if self.n_head * self.head_dim != self.dim or self.fast_n_head * self.fast_head_dim != self.fast_dim:
            errs.append("n_head * head_dim must equal dim")
        if self.codebook_size % 16 or self.vocab_size % 16:
            errs.append("codebook_size and vocab_size must be multiples of 16")
        if errs:
            raise ValueError("unsupported model config: " + "; ".join(errs))


@dataclass
class ModelType:
    family: str = "dual_ar"
    version: Optional[str] = None
    codec: str = "mimi"

    @classmethod
    def smoltts_v0(cls) -> "ModelType":
        return cls(family="dual_ar", version=None, codec="mimi")


@dataclass
class TokenConfig:
    im_end_id: int
    pad_id: int
    semantic_start_id: int
    semantic_end_id: Optional[int]

    @classmethod
    def from_tokenizer(cls, tokenizer, config: RQTransformerModelArgs) -> "TokenConfig":
        """dual_ar branch of lm/rq_transformer.py:58-89."""
        im_end = tokenizer.token_to_id("<|im_end|>")
        if im_end is None:
            raise ValueError("Tokenizer does not have <|im_end|>")
        start = tokenizer.token_to_id("<|semantic:0|>")
        end = tokenizer.token_to_id(f"<|semantic:{config.codebook_size - 1}|>")
        if start is None or end is None:
            raise ValueError("Tokenizer does not have the <|semantic:k|> range")
        pad = tokenizer.token_to_id("<|semantic|>") or 5
        return cls(im_end_id=im_end, pad_id=pad, semantic_start_id=start, semantic_end_id=end)


@dataclass
class GenerationSettings:
    """lm/generate.py:12-16. ``default_temp == 0.0`` / ``default_fast_temp`` None-or-<=0 => greedy."""

    default_temp: float = 0.7
    default_fast_temp: Optional[float] = 0.7
    min_p: Optional[float] = None
    max_new_tokens: int = 1024
    seed: Optional[int] = None  # extension: None draws a fresh seed per generator
    # What ``min_p`` does.  "reference": exactly what lm/utils/samplers.py:22-28 computes -- the threshold is built from the
    # token's OWN log-probability (``top_logprobs`` is the same array as ``sorted_logprobs``), so nothing is ever removed
    # and the draw is plain categorical over logits / temp.  "intended": the rule the code was taken from (MLX examples):
    # keep tokens with p >= min_p * p_max.  The drop-in default is what the reference does.
    min_p_mode: str = "reference"
    # extension: the defaults of the per-request filters of sampled rows (``RequestSampling``; all off)
    top_p: float = 1.0
    top_k: int = 0
    repetition_penalty: float = 1.0
    repetition_window: int = 16
    # extension: the defaults of the per-request length control (``RequestSampling``; both off)
    min_frames: int = 0
    eos_bias: float = 0.0

    def __post_init__(self):
        if self.min_p_mode not in ("reference", "intended"):
            raise ValueError(f"min_p_mode must be 'reference' or 'intended', got {self.min_p_mode!r}")
        RequestSampling(top_p=self.top_p, top_k=self.top_k, repetition_penalty=self.repetition_penalty,
                        repetition_window=self.repetition_window, min_frames=self.min_frames, eos_bias=self.eos_bias)  # the same ranges

    @property
    def effective_min_p(self) -> float:
        """The cut the device sampler applies (0 = none)."""
        return float(self.min_p or 0.0) if self.min_p_mode == "intended" else 0.0

    @classmethod
    def greedy(cls, max_new_tokens: int = 1024) -> "GenerationSettings":
        return cls(default_temp=0.0, default_fast_temp=0.0, min_p=None, max_new_tokens=max_new_tokens)

    @property
    def is_greedy(self) -> bool:
        fast_greedy = self.default_fast_temp is None or self.default_fast_temp <= 0
        return self.default_temp == 0.0 and fast_greedy


FRAMES_PER_SECOND = 12.5  # Mimi frames (slow tokens) per second of audio
MAX_MIN_FRAMES = 1024     # of the public interface; the device entry takes up to 2**30
MAX_EOS_BIAS = 100.0
MAX_BEST_OF = 8           # takes of one request (``RequestSampling.best_of``)


def min_frames_from(min_frames=None, min_duration_s=None) -> Optional[int]:
    """The ``min_frames`` of a request that may spell it as ``min_duration_s`` (seconds of audio, ``ceil(s * 12.5)`` frames)
    instead; giving both is an error.  Range errors are ``RequestSampling``'s."""
    import math

    if min_duration_s is None:
        return min_frames
    if min_frames is not None:
        raise ValueError("give min_frames or min_duration_s, not both")
    if isinstance(min_duration_s, bool) or not isinstance(min_duration_s, (int, float)) or not math.isfinite(min_duration_s) or min_duration_s < 0:
        raise ValueError(f"min_duration_s must be finite and >= 0, got {min_duration_s!r}")
    if min_duration_s * FRAMES_PER_SECOND > MAX_MIN_FRAMES:
        raise ValueError(f"min_duration_s must be at most {MAX_MIN_FRAMES / FRAMES_PER_SECOND:g} s, got {min_duration_s!r}")
    return int(math.ceil(min_duration_s * FRAMES_PER_SECOND))


def length_bounds(text: str, sampling: "RequestSampling", max_new_tokens: int, min_frames_per_byte: Optional[float] = None,
                  max_frames_per_byte: Optional[float] = None):
    """(sampling, max_new_tokens) of one utterance or segment under the operator's bounds from the text length: with n the UTF-8
    byte count of ``text``, ``max_new_tokens = max(1, min(request's, ceil(n * max_frames_per_byte)))`` and ``min_frames =
    min(max(request's, floor(n * min_frames_per_byte)), max_new_tokens - 1)``.  A ratio of ``None`` leaves its side alone; with
    both ``None`` the two arguments come back unchanged."""
    import dataclasses
    import math

    if min_frames_per_byte is None and max_frames_per_byte is None:
        return sampling, max_new_tokens
    n = len(text.encode("utf-8"))
    cap = int(max_new_tokens)
    if max_frames_per_byte is not None:
        cap = max(1, min(cap, int(math.ceil(n * float(max_frames_per_byte)))))
    if min_frames_per_byte is not None:
        own = int(sampling.min_frames or 0)
        want = min(max(own, int(math.floor(n * float(min_frames_per_byte)))), max(cap - 1, 0), MAX_MIN_FRAMES)
        if want != own:
            sampling = dataclasses.replace(sampling, min_frames=want)
    return sampling, cap


def finish_reason(slow_ids, im_end_id: int) -> str:
    """Why an utterance ended: ``"stop"`` if its last emitted slow id is ``<|im_end|>``, else ``"length"`` (the frame cap, the
    request's ``max_new_tokens`` or a full context)."""
    n = len(slow_ids)
    return "stop" if n > 0 and int(slow_ids[n - 1]) == int(im_end_id) else "length"


def merge_finish_reasons(reasons) -> str:
    """Of a segmented request: ``"length"`` if any segment was."""
    return "length" if any(r == "length" for r in reasons) else "stop"


def take_seed(seed: int, k: int) -> int:
    """The seed of take ``k`` of a ``best_of`` request: ``(seed + k) mod 2**64``.  Take 0 is the request without ``best_of``."""
    return (int(seed) + int(k)) % 2**64


def take_sampling(sampling: "RequestSampling", k: int) -> "RequestSampling":
    """The resolved entry of take ``k``: a plain scored request with that take's seed."""
    import dataclasses

    return dataclasses.replace(sampling, seed=take_seed(sampling.seed, k), logprobs=True, best_of=None)


def mean_logprob(logprobs) -> float:
    """Mean score of an utterance in float64 over its frames as the host clipped them (its ``<|im_end|>`` frame included);
    ``-inf`` for no frames."""
    n = len(logprobs)
    return float(sum(float(x) for x in logprobs) / n) if n else float("-inf")


def rank_takes(takes) -> list:
    """The order of a ``best_of`` request's takes, best first; ``takes[k]`` is ``(finish_reason, mean_logprob)`` of take k.
    Takes that ended with ``"stop"`` come before takes that ended with ``"length"``, then the higher mean wins, then the lower k."""
    return sorted(range(len(takes)), key=lambda k: (0 if takes[k][0] == "stop" else 1, -float(takes[k][1]), k))


def check_best_of(sampling: "RequestSampling", slots: int, stream: bool = False, segmented: bool = False) -> None:
    """The one check of ``best_of`` shared by every front end; ``sampling`` is resolved, ``slots`` the front end's slot count.
    A request with one take passes."""
    n = sampling.takes
    if n <= 1:
        return
    if stream:
        raise ValueError("best_of > 1 needs a blocking request: a stream's audio is out before the takes can be ranked")
    if segmented:
        raise ValueError("best_of > 1 is not available for segmented or incremental requests")
    if (sampling.temperature or 0.0) <= 0:
        raise ValueError("best_of > 1 needs a sampled slow token (temperature > 0): greedy takes are all the same")
    if n > int(slots):
        raise ValueError(f"best_of={n} exceeds the {int(slots)} slots of this engine")


@dataclass
class RequestSampling:
    """Sampling of one request (per-request settings of the server and the façade).  ``None`` fields take the server's or
    caller's ``GenerationSettings``: ``temperature`` <- ``default_temp``, ``fast_temperature`` <- ``default_fast_temp``,
    ``min_p`` <- ``min_p`` (then through that settings' ``min_p_mode``, ``effective_min_p``).  ``seed`` (0 .. 2**64 - 1) keys the
    request's draws: the same seed gives the same ids in any slot of any batch ("per-request sampling").

    Filters of the sampled picks, ``None`` <- the settings' field of the same name: ``top_p`` (0 < p <= 1; 1 =
    off), ``top_k`` (>= 0; 0 = off), ``repetition_penalty`` (1 .. 10; 1 = off) over the ids the same step produced in the
    request's last ``repetition_window`` (1 .. 64) frames.  They act only where the request samples: a greedy slow token or
    greedy depth codes ignore them.

    Length control, ``None`` <- the settings' field of the same name: ``min_frames`` (0 .. 1024; 0 = off) keeps
    ``<|im_end|>`` from being picked before that many frames have been emitted; ``eos_bias`` (-100 .. 100; 0 = off) is added to
    the ``<|im_end|>`` logit.  Both act on greedy and sampled slow tokens alike; the depth codes are never touched.

    Scores: ``logprobs`` asks for the log-probability, at temperature 1, of every slow id the request emits,
    under the row its pick saw (after the length control and the repetition penalty, before temperature and the other filters).
    ``best_of`` (1 .. 8; None or 1 = one take) draws that many takes, take k with seed ``(seed + k) mod 2**64``, and keeps the
    one ``rank_takes`` puts first; more than one take implies ``logprobs``.  Blocking, unsegmented, sampled requests only
    (``check_best_of``)."""

    temperature: Optional[float] = None
    fast_temperature: Optional[float] = None
    min_p: Optional[float] = None
    seed: Optional[int] = None
    top_p: Optional[float] = None
    top_k: Optional[int] = None
    repetition_penalty: Optional[float] = None
    repetition_window: Optional[int] = None
    min_frames: Optional[int] = None
    eos_bias: Optional[float] = None
    logprobs: bool = False
    best_of: Optional[int] = None

    def __post_init__(self):
        import math

        if not isinstance(self.logprobs, bool):
            raise ValueError(f"logprobs must be true or false, got {self.logprobs!r}")
        n = self.best_of
        if n is not None and not (isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= MAX_BEST_OF):
            raise ValueError(f"best_of must be an integer in [1, {MAX_BEST_OF}], got {n!r}")

        for name in ("temperature", "fast_temperature"):
            v = getattr(self, name)
            if v is not None and not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
        if self.min_p is not None and not (0 <= self.min_p < 1):
            raise ValueError(f"min_p must be in [0, 1), got {self.min_p!r}")
        if self.seed is not None and not (0 <= int(self.seed) < 2**64):
            raise ValueError(f"seed must be in [0, 2**64), got {self.seed!r}")
        if self.top_p is not None and not (0 < self.top_p <= 1):
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p!r}")
        if self.top_k is not None and not (isinstance(self.top_k, int) and not isinstance(self.top_k, bool) and 0 <= self.top_k < 2**31):
            raise ValueError(f"top_k must be an integer >= 0, got {self.top_k!r}")
        if self.repetition_penalty is not None and not (1 <= self.repetition_penalty <= 10):
            raise ValueError(f"repetition_penalty must be in [1, 10], got {self.repetition_penalty!r}")
        w = self.repetition_window
        if w is not None and not (isinstance(w, int) and not isinstance(w, bool) and 1 <= w <= 64):
            raise ValueError(f"repetition_window must be an integer in [1, 64], got {w!r}")
        m = self.min_frames
        if m is not None and not (isinstance(m, int) and not isinstance(m, bool) and 0 <= m <= MAX_MIN_FRAMES):
            raise ValueError(f"min_frames must be an integer in [0, {MAX_MIN_FRAMES}], got {m!r}")
        b = self.eos_bias
        if b is not None and not (isinstance(b, (int, float)) and not isinstance(b, bool) and math.isfinite(b) and abs(b) <= MAX_EOS_BIAS):
            raise ValueError(f"eos_bias must be finite and in [-{MAX_EOS_BIAS:g}, {MAX_EOS_BIAS:g}], got {b!r}")

    @property
    def takes(self) -> int:
        """How many takes the request draws (1 without ``best_of``)."""
        return int(self.best_of or 1)

    @property
    def scored(self) -> bool:
        """Whether the request's slow tokens are scored: it asked for ``logprobs``, or it has more than one take to rank."""
        return bool(self.logprobs) or self.takes > 1

    @property
    def length_on(self) -> bool:
        """Whether the length control of an entry is on: a minimum number of frames or a bias on ``<|im_end|>``."""
        return bool(self.min_frames) or bool(self.eos_bias)

    @property
    def filters_on(self) -> bool:
        """Whether some filter of a resolved entry is on (it still acts only on the picks that sample)."""
        return (self.top_p is not None and self.top_p < 1) or bool(self.top_k) or (self.repetition_penalty or 1.0) > 1

    @property
    def is_sampled(self) -> bool:
        return (self.temperature or 0.0) > 0 or (self.fast_temperature or 0.0) > 0

    def resolve(self, settings: "GenerationSettings", draw_seed: bool = True) -> "RequestSampling":
        """Every field filled in from ``settings``; ``min_p`` becomes the effective cut the device applies.  A sampled request
        without a seed gets one from ``os.urandom`` (``draw_seed``); a greedy one keeps ``seed`` as given (None: unused)."""
        import os

        fast_default = settings.default_fast_temp if settings.default_fast_temp is not None else 0.0
        t = float(self.temperature if self.temperature is not None else settings.default_temp)
        ft = float(self.fast_temperature if self.fast_temperature is not None else max(fast_default, 0.0))
        cut = GenerationSettings(min_p=self.min_p if self.min_p is not None else settings.min_p, min_p_mode=settings.min_p_mode).effective_min_p
        pick = lambda name: getattr(self, name) if getattr(self, name) is not None else getattr(settings, name)
        out = RequestSampling(max(t, 0.0), max(ft, 0.0), cut, self.seed, float(pick("top_p")), int(pick("top_k")),
                              float(pick("repetition_penalty")), int(pick("repetition_window")), int(pick("min_frames")),
                              float(pick("eos_bias")), bool(self.logprobs), self.best_of)
        if out.seed is None and draw_seed and out.is_sampled:
            out.seed = int.from_bytes(os.urandom(8), "little")
        return out


@dataclass
class NumericsMode:
    """Which half of the reference the arithmetic quirks follow (SURVEY.md §7 'quirks').

    ``embed_mask``: "torch" zeroes the codebook-embedding sum where code0 == 0
    (modeling/...:219); "mlx" zeroes it where the text-row token is not a semantic token
    (lm/rq_transformer.py:162-169).  ``rope_bf16``: cos/sin table rounded to bf16
    (modeling/...:624) or exact fp32 (MLX nn.RoPE)."""

    embed_mask: str = "torch"
    rope_bf16: bool = True

    @classmethod
    def torch_reference(cls) -> "NumericsMode":
        return cls("torch", True)

    @classmethod
    def mlx_reference(cls) -> "NumericsMode":
        return cls("mlx", False)
