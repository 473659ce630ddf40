"""``smoltts-server`` drop-in: the reference's HTTP surface over the HIP engine.

Routes, schemas, headers and status behaviour follow mlx_inference/src/smoltts_mlx/server/routes/
openai.py:6-28 (``POST /v1/audio/speech`` -> audio/wav attachment ``speech.wav``) and elevenlabs.py:14-63
(``POST /v1/text-to-speech/{voice_id}`` blocking with ``output_format`` pcm_*/wav_*; ``.../stream`` ->
chunked raw float32 PCM with ``X-Sample-Rate: 24000``), ``TTSCore`` (server/tts_core.py:15-84) and the
settings file (server/settings.py:12-63).  mp3 output needs pydub + ffmpeg, which the reference pulls in and this image
lacks: those formats answer 501 instead of being half-implemented.
"""
from __future__ import annotations

import argparse
import asyncio
import json
import math
import queue
import threading
from typing import Dict, List, Literal, Optional, Tuple, Union

import numpy as np
from fastapi import APIRouter, FastAPI, HTTPException, Query, Request, Response
from fastapi.exceptions import RequestValidationError
from fastapi.responses import JSONResponse, StreamingResponse
from pydantic import BaseModel, Field, model_validator

from ..formats import lin2ulaw
from .wav import pcm_to_wav_bytes

# output_format of the stream route: the codec's float32 at 24 kHz, or a format converted on the GPU (formats.py)
StreamFormat = Literal["pcm_24000", "pcm_8000", "pcm_16000", "pcm_22050", "pcm_44100", "pcm_48000", "ulaw_8000"]


class TTSCore:
    def __init__(self, model, settings=None, scheduler=None):
        self.model = model
        self.settings = settings
        self.scheduler = scheduler  # BatchScheduler: concurrent requests share the GPU batch
        self.voices: Dict[str, dict] = {}  # cloned voices registered through this server: id -> {"name", "prompt_positions"}
        self._voice_lock = threading.Lock()
        self.segments = 0  # segments of the segmented requests that completed (long_text="segment")
        from .settings import watermark_setting

        block = watermark_setting(self._setting("watermark", None))
        self.watermark = block.to_watermark() if block is not None else None  # the key a recording is tested against
        self.watermark_apply = block.apply if block is not None else None
        self._segments_lock = threading.Lock()
        # the model-only path: the settings' bounds from the text length are the façade's (a scheduler is built with its own)
        if scheduler is None and hasattr(model, "min_frames_per_byte") and hasattr(model, "max_frames_per_byte"):
            for name in ("min_frames_per_byte", "max_frames_per_byte"):
                if self._setting(name, None) is not None:
                    setattr(model, name, float(self._setting(name, None)))

    def _setting(self, name: str, default):
        st = self.settings
        v = st.get(name) if isinstance(st, dict) else getattr(st, name, None)
        return default if v is None else v

    @property
    def long_text(self) -> str:
        return self._setting("long_text", "refuse")

    def _marks(self, voice) -> Optional[bool]:
        """Whether a request that speaks ``voice`` is marked; None without a ``watermark`` setting (nothing is passed on)."""
        if self.watermark is None:
            return None
        if self.watermark_apply == "all":
            return True
        with self._voice_lock:
            return str(voice) in self.voices

    def _request_kw(self, text: str, speed: Optional[float], loudness=None, stream: bool = False, voice=None,
                    timestamps: bool = False, pieces: Optional[dict] = None, one_utterance: bool = False) -> Tuple[dict, int]:
        """(kwargs, segments): the request's options resolved -- the body's fields where it names them (null: off), else the
        server's settings -- parsed once, and handed on as the parsed value's own keywords (``SpeechOptions.given``): only the
        options that are on, so that the model sees the calls it saw before when none is.  ``loudness``: the body's
        ``LoudnessFields`` (None: the settings alone).  The segment options of ``long_text="segment"`` mode and ``watermark``
        (``_marks``) are added as the settings give them.  ``pieces`` (the format keywords of a stream fed in pieces, which is
        always spoken in segments whatever ``long_text`` says): they are parsed and handed on with the rest.  A bad option, a text
        over ``max_input_chars`` or with a bad break tag is the client's fault (ValueError).  The segments the request speaks
        (0: an unsegmented one) are counted once it has completed."""
        from ..request import parse_request

        st, body = self._setting, loudness
        seg_opts = {"max_bytes": int(st("segment_max_bytes", 300)), "pause_s": float(st("seam_pause_ms", 250)) / 1e3}
        seg = None
        if pieces is None and self.long_text == "segment":
            limit = int(st("max_input_chars", 5000))
            if len(text) > limit:
                raise ValueError(f"input has {len(text)} characters; max_input_chars is {limit}")
            if not timestamps and not one_utterance:  # (a request with timestamps, blocking or streamed, is one utterance: chained segments have none)
                seg = seg_opts
        target, start = body.resolve(st("loudness", None)) if body is not None else (st("loudness", None), None)
        on, pause, thr, ceiling = bool(st("trim_silence", False)), st("max_pause_s", None), None, st("peak_limit_db", None)
        if body is not None and hasattr(body, "trim_fields"):
            on, pause, thr = body.trim_fields(on, pause)
        if body is not None and hasattr(body, "peak_limit"):
            ceiling = body.peak_limit(ceiling)
        p = parse_request(text, stream=stream, speed=speed, segment=seg, loudness=target, loudness_start_gain_db=start,
                          trim_silence=on, max_pause_s=pause, silence_threshold_db=thr, timestamps=timestamps or None,
                          peak_limit_db=ceiling, **(pieces or {}))
        kw = p.given()
        if seg is not None or pieces is not None:
            kw["segment"] = seg_opts
        if self._marks(voice) is not None:
            kw["watermark"] = self._marks(voice)
        return kw, len(p.plan.segs) if p.plan is not None else 0

    def _count_segments(self, n: int) -> None:
        if n:
            with self._segments_lock:
                self.segments += n

    # -- cloned voices (extension: ElevenLabs' voices/add with JSON + base64 WAV samples instead of multipart)
    @property
    def max_voices(self) -> int:
        st = self.settings
        v = st.get("max_voices") if isinstance(st, dict) else getattr(st, "max_voices", None)
        return 64 if v is None else int(v)

    def add_voice(self, name: str, samples: List[dict], system_prompt: Optional[str] = None) -> str:
        """samples: [{"text", "audio": float32 at 24 kHz}] -> the new voice id.  ``ValueError``: a voice that cannot be served;
        ``NoEncoderError``: no encoder weights; ``OverflowError``: max_voices reached."""
        from .voices import new_voice_id

        with self._voice_lock:
            if len(self.voices) >= self.max_voices:
                raise OverflowError(f"{len(self.voices)} voices registered: max_voices is {self.max_voices}")
            voice_id = new_voice_id()
            self.voices[voice_id] = {"name": name, "prompt_positions": None}  # (holds the place while the voice is computed)
        try:
            if self.scheduler is not None:
                P = int(self.scheduler.add_voice(voice_id, samples=samples, system_prompt=system_prompt, name=name)["prompt_positions"])
            else:
                grid = self.model.create_speaker(samples, system_prompt=system_prompt)
                P = int(grid.shape[1])
                self._check_room(grid)
                self.model.add_voice(voice_id, grid)
        except BaseException:
            with self._voice_lock:
                self.voices.pop(voice_id, None)
            raise
        with self._voice_lock:
            self.voices[voice_id]["prompt_positions"] = P
        return voice_id

    def _check_room(self, grid) -> None:
        """The model-only path: a speaker prompt must leave room for an empty request and the frame budget (as the scheduler's)."""
        m = self.model
        if not all(hasattr(m, a) for a in ("prompt_encoder", "config", "_settings")):
            return
        P = int(grid.shape[1])
        t_min = int(m.prompt_encoder.build_prompt("", "", grid).shape[1]) - P
        max_new = m._settings(None).max_new_tokens or 0
        if P + t_min + max_new + 2 > m.config.max_seq_len:
            raise ValueError(f"speaker prompt of P={P} positions leaves no room for a request: P + {t_min} (an empty request) + "
                             f"max_new_tokens {max_new} + 2 > max_seq_len {m.config.max_seq_len}")

    def align_recording(self, pcm, rate: int, text: str, voice: str = "heart"):
        """Forced alignment of a recording (mono samples at ``rate``) against ``text`` -> ``align.RecordingAlignment``, through the
        scheduler (pool) where there is one, else the model.  ``ValueError``: what the call refuses; ``NoEncoderError``: no encoder."""
        target = self.scheduler if self.scheduler is not None else self.model
        return target.align_recording(pcm, text, voice=voice, rate=rate)

    def remove_voice(self, voice_id: str) -> None:
        with self._voice_lock:
            if voice_id not in self.voices or self.voices[voice_id]["prompt_positions"] is None:
                raise KeyError(voice_id)
            del self.voices[voice_id]
        if self.scheduler is not None:
            self.scheduler.remove_voice(voice_id)
        else:
            self.model.remove_voice(voice_id)

    def list_voices(self) -> List[dict]:
        from ..prompt import VOICES

        out = [{"voice_id": v, "name": v, "category": "premade"} for v in VOICES]
        with self._voice_lock:
            out += [{"voice_id": k, "name": v["name"], "category": "cloned", "prompt_positions": v["prompt_positions"]}
                    for k, v in self.voices.items() if v["prompt_positions"] is not None]
        return out

    def resolve_speaker_id(self, voice: Union[str, int]) -> int:
        if isinstance(voice, int):
            return voice
        if isinstance(voice, str) and voice.isnumeric():
            return int(voice)
        return 0

    def _model_sampling(self, sampling):
        """The model-only path: the request's sampling resolved against the façade's own defaults (its seed drawn here), or None
        when the request names none (the façade's unchanged behaviour)."""
        if sampling is None:
            return None
        from ..config import GenerationSettings

        base = self.model._settings(None) if hasattr(self.model, "_settings") else GenerationSettings()
        return sampling.resolve(base)

    def _check_best_of(self, sampling, stream: bool = False) -> None:
        """The routes' share of the ``best_of`` refusals (``ValueError`` -> 400): the settings' ``max_best_of`` (default 4), and a
        streaming route.  The engine's own check (``config.check_best_of``) refuses the rest."""
        n = getattr(sampling, "takes", 1) if sampling is not None else 1
        if n <= 1:
            return
        if stream:
            raise ValueError("best_of > 1 needs a blocking request: a stream's audio is out before the takes can be ranked")
        cap = int(self._setting("max_best_of", 4))
        if n > cap:
            raise ValueError(f"best_of={n} exceeds this server's max_best_of={cap}")

    @property
    def alignment_heads(self):
        """The (layer, head) pairs character timestamps are read from: the ``alignment_heads`` setting, else what the scheduler
        (pool) or the model was built with; empty: the with-timestamps route answers 501."""
        from ..align import check_heads

        for src in (self._setting("alignment_heads", None), getattr(self.scheduler, "alignment_heads", None),
                    getattr(self.model, "alignment_heads", None)):
            if src:
                return check_heads(src)
        return []

    def generate_audio(self, input_text: str, voice: Union[str, int], response_format: str = "wav_24000", sampling=None,
                       speed: Optional[float] = None, loudness=None, info: Optional[dict] = None, timestamps: bool = False):
        """-> (bytes, media type, the seed the request sampled with or None).  ``speed``: passed on only when it is not 1.
        ``timestamps``: the request also measures its character times (align.py): ``info["alignment"]`` is the ``align.Alignment``;
        it is spoken as one utterance whatever ``long_text`` says, and refused (``ValueError`` -> 400) with the trim options and
        ``best_of``.
        ``info["finish_reason"]``: ``"stop"`` or ``"length"`` (``config.finish_reason``).
        ``loudness``: the body's ``LoudnessFields``; ``info["loudness_gain_db"]`` is then the gain the utterance was given,
        ``info["peak_reduction_db"]`` what its peak limiter took off where the body or the server names a ``peak_limit_db``, and
        ``info["watermark"]`` true when the audio is marked."""
        used = None
        try:
            self._check_best_of(sampling)
            sp, n_seg = self._request_kw(input_text, speed, loudness, voice=voice, timestamps=timestamps)
            if info is not None:
                info["watermark"] = bool(sp.get("watermark"))
            if timestamps and sampling is not None and getattr(sampling, "takes", 1) > 1:
                raise ValueError("timestamps cannot be combined with best_of")
            if self.scheduler is not None:
                req = self.scheduler.submit(input_text, str(voice), stream=False, **({"sampling": sampling} if sampling is not None else {}), **sp)
                used = getattr(req, "sampling", None)
                pcm = np.concatenate(list(self.scheduler.iter_chunks(req)) or [np.zeros(0, np.float32)])
                gain = getattr(req, "loudness_gain_db", None)
                cut = getattr(req, "trimmed_s", 0.0)
                reason = getattr(req, "finish_reason", None)
                mean, n_takes = getattr(req, "mean_logprob", None), getattr(req, "best_of", 1)
                used = getattr(req, "sampling", None)  # (a best_of request's entry is the chosen take's by now)
                alignment = getattr(req, "alignment", None)
                reduction = getattr(req, "peak_reduction_db", None)
            else:
                used = self._model_sampling(sampling)
                kw = {"sampling": used} if used is not None else {}
                pcm = np.asarray(self.model(input_text, str(voice), **kw, **sp)).flatten()
                gain = getattr(self.model, "last_loudness_gain_db", None)
                cut = getattr(self.model, "last_trimmed_s", 0.0)
                reason = getattr(self.model, "last_finish_reason", None)
                mean, takes = getattr(self.model, "last_mean_logprob", None), getattr(self.model, "last_takes", None)
                n_takes = len(takes) if takes else 1
                if takes:
                    used = self.model.last_sampling[0]  # the chosen take's entry
                alignment = getattr(self.model, "last_alignment", None)
                reduction = getattr(self.model, "last_peak_reduction_db", None)
            if timestamps:
                if alignment is None:
                    raise RuntimeError("the engine returned no alignment for a request with timestamps")
                if info is not None:
                    info["alignment"] = alignment
            if info is not None and mean is not None:
                info["mean_logprob"], info["best_of"] = mean, n_takes
            if info is not None and reason is not None:
                info["finish_reason"] = reason
            if info is not None and ("trim_silence" in sp or "max_pause_s" in sp):
                info["trimmed_ms"] = 1e3 * float(cut or 0.0)
            if info is not None and "loudness" in sp:
                info["loudness_gain_db"] = gain
            if info is not None and "peak_limit_db" in sp:
                info["peak_reduction_db"] = float(reduction or 0.0)
        except ValueError as e:  # a request the engine refuses (e.g. a text too long for max_seq_len): the client's fault, not a 500
            raise HTTPException(status_code=400, detail=str(e))
        self._count_segments(n_seg)
        return (*self.format_audio_chunk(pcm, response_format), seed_used(used))

    def stream_audio(self, input_text: str, voice: Union[str, int], output_format: str = "pcm_24000", sampling=None,
                     speed: Optional[float] = None, container: Optional[str] = None, loudness=None, info: Optional[dict] = None):
        """-> (chunks as bytes, the seed the request samples with or None); ``info["watermark"]``: the stream is marked.  Chunks: float32 at 24 kHz for ``pcm_24000``;
        otherwise the int16 / mu-law samples the model or scheduler converted on the GPU (the format is passed on only when it is
        not ``pcm_24000``).  The request is submitted here, before the first chunk is asked for.  ``speed``: passed on only when
        it is not 1; the chunks are then the stretched stream (float32 for ``pcm_24000``).  ``container`` ``"flac"``: the
        chunks are the stream's FLAC bytes (framed on the GPU), the stream header in front of the first."""
        self._check_best_of(sampling, stream=True)
        kw = {} if output_format == "pcm_24000" else {"output_format": output_format}
        if container is not None:
            kw["container"] = container
        sp, n_seg = self._request_kw(input_text, speed, loudness, stream=True, voice=voice)
        if info is not None:
            info["watermark"] = bool(sp.get("watermark"))
        if self.scheduler is not None:
            req = self.scheduler.submit(input_text, str(voice), stream=True, **kw, **({"sampling": sampling} if sampling is not None else {}), **sp)
            chunks, used = self.scheduler.iter_chunks(req), getattr(req, "sampling", None)
        else:
            used = self._model_sampling(sampling)
            chunks = self.model.stream(input_text, str(voice), **kw, **({"sampling": used} if used is not None else {}), **sp)
        return self._stream_bytes(chunks, kw, n_seg), seed_used(used)

    def stream_audio_timed(self, input_text: str, voice: Union[str, int], output_format: str = "pcm_24000", sampling=None,
                           speed: Optional[float] = None, loudness=None, info: Optional[dict] = None):
        """``stream_audio`` of one utterance with character timestamps -> (``(bytes, align.AlignmentPart or
        None)`` pairs, the seed the request samples with or None).  The text is spoken as one utterance whatever ``long_text``
        says; ``ValueError``: the trim options, ``best_of``, a text the engine refuses."""
        self._check_best_of(sampling, stream=True)
        kw = {} if output_format == "pcm_24000" else {"output_format": output_format}
        sp, _ = self._request_kw(input_text, speed, loudness, stream=True, voice=voice, one_utterance=True)
        if info is not None:
            info["watermark"] = bool(sp.get("watermark"))
        if self.scheduler is not None:
            req = self.scheduler.submit(input_text, str(voice), stream=True, live_timestamps=True, **kw,
                                        **({"sampling": sampling} if sampling is not None else {}), **sp)
            pairs, used = self.scheduler.timed_chunks(req), getattr(req, "sampling", None)
        else:
            used = self._model_sampling(sampling)
            pairs = self.model.stream_with_timestamps(input_text, str(voice), **kw, **({"sampling": used} if used is not None else {}), **sp)
        return self._timed_bytes(pairs, kw), seed_used(used)

    @staticmethod
    def _timed_bytes(pairs, kw):
        try:
            for chunk, part in pairs:
                yield (np.asarray(chunk, dtype=np.float32) if not kw else np.ascontiguousarray(chunk)).tobytes(), part
        finally:
            pairs.close()  # a client that went away mid-stream: the scheduler takes its slot back

    def open_input_stream(self, voice: Union[str, int], output_format: str = "pcm_24000", sampling=None,
                          speed: Optional[float] = None, container: Optional[str] = None, loudness=None, info: Optional[dict] = None):
        """A stream whose text arrives in pieces -> (an ``InputStream``, the seed it samples with or None).  Behind a scheduler
        or pool it is ``submit_incremental``; a bare model streams from an iterator (``SmolTTS.stream(text_iter)``), which pulls
        the text as it speaks.  The segment options are the settings' ``segment_max_bytes`` / ``seam_pause_ms`` whatever
        ``long_text`` says (a text fed in pieces is always spoken in segments); ``idle_timeout_s`` and ``flush_after_s`` are
        the settings' too.  ``ValueError``: options the engine refuses."""
        self._check_best_of(sampling, stream=True)
        kw = {} if output_format == "pcm_24000" else {"output_format": output_format}
        if container is not None:
            kw["container"] = container
        sp, _ = self._request_kw("", speed, loudness, stream=True, voice=voice, pieces=kw)
        if info is not None:
            info["watermark"] = bool(sp.get("watermark"))
        if self.scheduler is not None:
            req = self.scheduler.submit_incremental(str(voice), **({"sampling": sampling} if sampling is not None else {}), **sp,
                                                    idle_timeout_s=float(self._setting("idle_timeout_s", 10.0)),
                                                    flush_after_s=self._setting("flush_after_s", None))
            used = getattr(req, "sampling", None)
            return InputStream(req.feed, req.flush, req.close, req.cancel, self._stream_bytes(self.scheduler.iter_chunks(req), kw)), seed_used(used)
        from ..longform import FLUSH

        used = self._model_sampling(sampling)
        texts: "queue.Queue" = queue.Queue()  # pieces, FLUSH marks, then None
        chunks = self.model.stream(iter(texts.get, None), str(voice), **({"sampling": used} if used is not None else {}), **sp)
        end = lambda: texts.put(None)  # (a bare model cannot be interrupted: it speaks what it has pulled, then ends)
        return InputStream(texts.put, lambda: texts.put(FLUSH), end, end, self._stream_bytes(chunks, kw)), seed_used(used)

    def _stream_bytes(self, chunks, kw, n_seg: int = 0):
        try:
            for chunk in chunks:
                if chunk is not None:
                    yield (np.asarray(chunk, dtype=np.float32) if not kw else np.ascontiguousarray(chunk)).tobytes()
            self._count_segments(n_seg)  # (the stream is through)
        finally:
            chunks.close()  # a client that went away mid-stream: the scheduler takes its slot back (BatchScheduler.cancel)

    def format_audio_chunk(self, pcm_data: np.ndarray, output_format: str = "pcm_24000"):
        """tts_core.py:49-84: resample when the format names another rate (FFT resampling, ``scipy.signal.resample``, as
        there), then raw PCM16 (rounded, as libsndfile writes it there), WAV (io/wav.py framing) or mp3 (not available)."""
        kind, _, rate = output_format.partition("_")
        sample_rate = int(rate.split("_")[0]) if rate else 24000
        pcm_data = np.asarray(pcm_data, dtype=np.float32).reshape(-1)
        if kind == "ulaw" and sample_rate != 8000:
            raise HTTPException(status_code=400, detail=f"Format {output_format} not yet supported (ulaw_8000 only)")
        if kind not in ("pcm", "wav", "mp3", "ulaw"):
            raise HTTPException(status_code=400, detail=f"Format {output_format} not yet supported")
        if kind == "mp3":
            raise HTTPException(status_code=501, detail="mp3 output is not available in this build (no encoder in the image)")
        if sample_rate != 24000:
            if sample_rate <= 0:
                raise HTTPException(status_code=400, detail=f"bad sample rate in {output_format}")
            from scipy import signal

            n = int(len(pcm_data) * sample_rate / 24000)
            pcm_data = signal.resample(pcm_data, n).astype(np.float32) if n > 0 else np.zeros(0, np.float32)
        if kind in ("pcm", "ulaw"):
            s16 = np.rint(np.clip(pcm_data, -1.0, 1.0) * 32767).astype(np.int16)
            return (s16.tobytes(), "audio/x-pcm") if kind == "pcm" else (lin2ulaw(s16).tobytes(), "audio/basic")  # ulaw: G.711 of the int16
        return pcm_to_wav_bytes(pcm_data, sample_rate), "audio/wav"


class InputStream:
    """The two ends of a stream fed in pieces: ``feed(text)`` / ``flush()`` / ``close()`` for the text, ``chunks`` (a generator
    of bytes, blocking) for the audio; closing ``chunks`` early cancels the request."""

    def __init__(self, feed, flush, close, cancel, chunks):
        self.feed, self.flush, self.close, self.cancel, self.chunks = feed, flush, close, cancel, chunks


def seed_used(sampling) -> Optional[int]:
    """The seed of a request that samples (its ``X-Seed``), or None: greedy, or no sampling known."""
    if sampling is None or sampling.seed is None:
        return None
    known_greedy = sampling.temperature is not None and sampling.fast_temperature is not None and not sampling.is_sampled
    return None if known_greedy else int(sampling.seed)


def _seed_headers(seed: Optional[int]) -> dict:
    return {} if seed is None else {"X-Seed": str(seed)}


def _gain_headers(info: dict) -> dict:
    g = info.get("loudness_gain_db")
    return {} if g is None else {"X-Loudness-Gain-Db": f"{g:.2f}"}


def _peak_headers(info: dict) -> dict:
    r = info.get("peak_reduction_db")
    return {} if r is None else {"X-Peak-Reduction-Db": f"{r:.2f}"}


def _trim_headers(info: dict) -> dict:
    t = info.get("trimmed_ms")
    return {} if t is None else {"X-Silence-Trimmed-Ms": f"{t:.0f}"}


def _mark_headers(info: dict) -> dict:
    return {"X-Watermark": "1"} if info.get("watermark") else {}


def _score_headers(info: dict) -> dict:
    """``X-Mean-Logprob`` (the chosen take's mean slow-token log-probability) and ``X-Best-Of`` of a blocking response that was scored."""
    m = info.get("mean_logprob")
    return {} if m is None else {"X-Mean-Logprob": f"{m:.4f}", "X-Best-Of": str(int(info.get("best_of") or 1))}


def _finish_headers(info: dict) -> dict:
    """``X-Finish-Reason: stop | length`` of a blocking response: whether the utterance ended with ``<|im_end|>`` or at its cap."""
    r = info.get("finish_reason")
    return {} if r is None else {"X-Finish-Reason": str(r)}


class SamplingFields(BaseModel):
    """Per-request sampling (extension; the ElevenLabs body's ``seed``): omitted fields take the server's generation settings.
    A sampled response carries ``X-Seed``: the seed it used, drawn by the server when the body names none."""
    seed: Optional[int] = Field(default=None, ge=0, le=2**64 - 1)
    temperature: Optional[float] = Field(default=None, ge=0, allow_inf_nan=False)
    fast_temperature: Optional[float] = Field(default=None, ge=0, allow_inf_nan=False)
    min_p: Optional[float] = Field(default=None, ge=0, lt=1)
    # filters of the sampled picks: accepted on a request that resolves to greedy too, where they have no effect
    top_p: Optional[float] = Field(default=None, gt=0, le=1)
    top_k: Optional[int] = Field(default=None, ge=0, lt=2**31)
    repetition_penalty: Optional[float] = Field(default=None, ge=1, le=10)
    repetition_window: Optional[int] = Field(default=None, ge=1, le=64)
    # length control, on greedy and sampled requests alike: ``<|im_end|>`` cannot be picked before ``min_frames``
    # frames (12.5 a second; ``min_duration_s`` spells it in seconds of audio, ceil(s * 12.5): one of the two), ``eos_bias`` is
    # added to its logit.  A blocking response carries ``X-Finish-Reason``
    min_frames: Optional[int] = Field(default=None, ge=0, le=1024)
    min_duration_s: Optional[float] = Field(default=None, ge=0, le=1024 / 12.5, allow_inf_nan=False)
    eos_bias: Optional[float] = Field(default=None, ge=-100, le=100, allow_inf_nan=False)
    # scores: ``logprobs`` scores the request's slow tokens; ``best_of`` (blocking routes, sampled requests, at most
    # the settings' ``max_best_of``) draws that many takes with seeds seed, seed + 1, ... and answers the best one.  A blocking
    # response then carries ``X-Mean-Logprob`` and ``X-Best-Of``, and its ``X-Seed`` is the chosen take's
    logprobs: Optional[bool] = None
    best_of: Optional[int] = Field(default=None, ge=1, le=8)

    @model_validator(mode="after")
    def _one_minimum(self):
        if self.min_frames is not None and self.min_duration_s is not None:
            raise ValueError("give min_frames or min_duration_s, not both")
        return self

    def request_sampling(self):
        from ..config import RequestSampling, min_frames_from

        min_frames = min_frames_from(self.min_frames, self.min_duration_s)
        fields = (self.seed, self.temperature, self.fast_temperature, self.min_p, self.top_p, self.top_k, self.repetition_penalty,
                  self.repetition_window, min_frames, self.eos_bias, self.logprobs or None, self.best_of)
        if all(v is None for v in fields):
            return None
        return RequestSampling(self.temperature, self.fast_temperature, self.min_p, self.seed, self.top_p, self.top_k,
                               self.repetition_penalty, self.repetition_window, min_frames, self.eos_bias, bool(self.logprobs), self.best_of)


# speaking speed (OpenAI's ``speed``, ElevenLabs' ``voice_settings.speed``): pitch-preserving time stretch on the GPU (tsm.py);
# an explicit null is speed 1, as an omitted field (such bodies were answered before speed was honoured, and still are)
SpeedField = Field(default=None, ge=0.25, le=4.0, allow_inf_nan=False)


class LoudnessFields(BaseModel):
    """Loudness normalisation (extension): ``loudness`` is a target in LUFS (-40 to -5, 400 otherwise; BS.1770-4, measured and
    applied on the GPU: loudness.py).  Omitted: the server's ``loudness`` setting; null: off.  A blocking response carries
    ``X-Loudness-Gain-Db``.  ``loudness_start_gain_db`` (streams only, within +-20): the gain a stream starts from."""
    loudness: Optional[float] = Field(default=None, allow_inf_nan=False)
    loudness_start_gain_db: Optional[float] = Field(default=None, allow_inf_nan=False)
    # Silence trimming (extension; trim.py, on the GPU first of the stages): ``trim_silence`` cuts the leading and trailing
    # silence, ``max_pause_s`` (0.1 to 2.0, 400 otherwise) caps the pauses; omitted: the server's ``trim_silence`` / ``max_pause_s``
    # settings; null: off.  ``silence_threshold_db`` (-72 to -6 dBFS, default 2^-8) needs one of the two.  A blocking response
    # carries ``X-Silence-Trimmed-Ms``.
    trim_silence: Optional[bool] = Field(default=None)
    max_pause_s: Optional[float] = Field(default=None, allow_inf_nan=False)
    silence_threshold_db: Optional[float] = Field(default=None, allow_inf_nan=False)
    # Peak limiting (extension; limiter.py, on the GPU last of the float stages): ``peak_limit_db`` is a ceiling in dBFS (-12 to
    # 0, 400 otherwise); omitted: the server's ``peak_limit_db`` setting; null: off.  A blocking response carries
    # ``X-Peak-Reduction-Db`` (0.00 when nothing was limited); with a ``loudness`` its gain is then not capped by the peak.
    peak_limit_db: Optional[float] = Field(default=None, allow_inf_nan=False)

    def peak_limit(self, default):
        """The ceiling in dBFS or None: the body's field where it names one (null: off), else the server's default."""
        return self.peak_limit_db if "peak_limit_db" in self.model_fields_set else default

    def trim_fields(self, default_trim: bool, default_pause):
        """(trim the ends, the pause cap or None, the threshold or None): the body's fields where it names them, else the defaults."""
        return (bool(self.trim_silence) if "trim_silence" in self.model_fields_set else default_trim,
                self.max_pause_s if "max_pause_s" in self.model_fields_set else default_pause, self.silence_threshold_db)

    def resolve(self, default):
        """(target or None, start gain or None): the body's field where it names one (null: off), else the server's default."""
        return (self.loudness if "loudness" in self.model_fields_set else default), self.loudness_start_gain_db


class SpeechRequest(SamplingFields, LoudnessFields):
    model: str = Field(default="tts-1-hd")
    input: str
    voice: Union[str, int] = Field(default="alloy")
    response_format: Literal["wav", "flac", "pcm"] = Field(default="wav")
    speed: Optional[float] = SpeedField


class VoiceSettings(BaseModel):
    """ElevenLabs' ``voice_settings``: ``speed`` is honoured; the other fields (stability, similarity_boost, ...) are accepted
    and ignored."""
    speed: Optional[float] = SpeedField


class CreateSpeechRequest(SamplingFields, LoudnessFields):
    text: str
    model_id: Optional[str] = Field(default=None)
    voice_settings: Optional[VoiceSettings] = Field(default=None)

    @property
    def speed(self) -> Optional[float]:
        return None if self.voice_settings is None else self.voice_settings.speed


openai_router = APIRouter(prefix="/v1", tags=["OpenAI"])
eleven_router = APIRouter(prefix="/v1", tags=["ElevenLabs"])


def _pcm16_bytes(chunks):
    """float32 chunks (bytes) -> int16 little-endian bytes, rint(clip(x, -1, 1) * 32767) as on the blocking route."""
    try:
        for b in chunks:
            x = np.frombuffer(b, dtype=np.float32)
            yield np.rint(np.clip(x, -1.0, 1.0) * np.float32(32767.0)).astype("<i2").tobytes()
    finally:
        chunks.close()


def _answer_first(chunks):
    """Pull the first chunk before the response starts, so that a request the engine refuses (e.g. a text too long for
    max_seq_len) is answered 400 with its reason, as on the blocking route; then the whole stream."""
    try:
        first = next(chunks)
    except StopIteration:
        return iter(())
    except ValueError as e:
        chunks.close()
        raise HTTPException(status_code=400, detail=str(e))

    def body():
        yield first
        yield from chunks

    return body()


@openai_router.post("/audio/speech")
def openai_speech(item: SpeechRequest, http_request: Request):
    """``wav``: the whole utterance at 24 kHz.  ``flac`` and ``pcm`` stream at 24 kHz (chunked): FLAC framed on the GPU, or
    int16 little-endian samples."""
    core = http_request.app.state.tts_core
    if item.response_format != "wav":
        container = "flac" if item.response_format == "flac" else None
        info: dict = {}
        try:
            chunks, seed = core.stream_audio(item.input, item.voice, "pcm_24000", sampling=item.request_sampling(), speed=item.speed,
                                             container=container, loudness=item, info=info)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        if container is None:
            chunks = _pcm16_bytes(chunks)
        media_type = "audio/flac" if container else "audio/x-pcm"
        return StreamingResponse(_answer_first(chunks), media_type=media_type, headers={
            "Content-Disposition": f'attachment; filename="speech.{item.response_format}"', "X-Sample-Rate": "24000",
            **_seed_headers(seed), **_mark_headers(info)})
    info: dict = {}
    audio, media_type, seed = core.generate_audio(item.input, item.voice, item.response_format + "_24000", sampling=item.request_sampling(),
                                                  speed=item.speed, loudness=item, info=info)
    return Response(audio, media_type=media_type, headers={"Content-Disposition": 'attachment; filename="speech.wav"', **_seed_headers(seed),
                                                           **_gain_headers(info), **_mark_headers(info), **_trim_headers(info),
                                                           **_peak_headers(info), **_finish_headers(info), **_score_headers(info)})


@eleven_router.post("/text-to-speech/{voice_id}")
def text_to_speech_blocking(voice_id: str, item: CreateSpeechRequest, http_request: Request,
                                  output_format: Optional[str] = Query(None, description="pcm_<rate> | wav_<rate>")):
    core = http_request.app.state.tts_core
    fmt = output_format or "wav_24000"
    info: dict = {}
    content, media_type, seed = core.generate_audio(item.text, voice_id, fmt, sampling=item.request_sampling(), speed=item.speed,
                                                    loudness=item, info=info)
    return Response(content=content, media_type=media_type, headers={
        "Content-Disposition": f'attachment; filename="elevenlabs_speech.{fmt.split("_")[0]}"',
        "X-Sample-Rate": fmt.split("_")[1] if "_" in fmt else "24000", **_seed_headers(seed), **_gain_headers(info), **_mark_headers(info),
        **_trim_headers(info), **_peak_headers(info), **_finish_headers(info), **_score_headers(info)})


@eleven_router.post("/text-to-speech/{voice_id}/with-timestamps")
def text_to_speech_with_timestamps(voice_id: str, item: CreateSpeechRequest, http_request: Request,
                                   output_format: Optional[str] = Query(None, description="pcm_<rate> | wav_<rate>")):
    """ElevenLabs' JSON: ``audio_base64`` (the blocking route's audio, in its formats), ``alignment`` and ``normalized_alignment``
    (the text is spoken as written, so the two are the same) with ``characters``, ``character_start_times_seconds`` and
    ``character_end_times_seconds``, read from the slow attention (align.py).  501 unless the server has ``alignment_heads``; 400
    with the trim options, ``best_of`` or a text the engine refuses."""
    import base64

    core = http_request.app.state.tts_core
    if not core.alignment_heads:
        raise HTTPException(status_code=501, detail="this server has no alignment_heads: rank the checkpoint's heads with "
                                                    "`python -m smoltts_amd.align rank --checkpoint DIR --texts FILE` and set them")
    fmt = output_format or "wav_24000"
    info: dict = {}
    content, _media, seed = core.generate_audio(item.text, voice_id, fmt, sampling=item.request_sampling(), speed=item.speed,
                                                loudness=item, info=info, timestamps=True)
    al = info["alignment"].to_json()
    return JSONResponse({"audio_base64": base64.b64encode(content).decode("ascii"), "alignment": al, "normalized_alignment": al},
                        headers={"X-Sample-Rate": fmt.split("_")[1] if "_" in fmt else "24000", **_seed_headers(seed),
                                 **_gain_headers(info), **_mark_headers(info), **_peak_headers(info), **_finish_headers(info)})


@eleven_router.post("/text-to-speech/{voice_id}/stream")
def stream_tts(voice_id: str, item: CreateSpeechRequest, http_request: Request,
                     output_format: StreamFormat = "pcm_24000"):
    """pcm_24000: raw float32 (the reference's stream); pcm_<rate>: int16 little-endian; ulaw_8000: G.711 mu-law bytes."""
    core = http_request.app.state.tts_core
    kind, rate = output_format.split("_")
    info: dict = {}
    try:
        chunks, seed = core.stream_audio(item.text, voice=voice_id, output_format=output_format, sampling=item.request_sampling(),
                                         speed=item.speed, loudness=item, info=info)
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))
    return StreamingResponse(chunks, media_type="audio/wav", headers={
        "Content-Disposition": f'attachment; filename="speech.{kind}"', "X-Sample-Rate": rate, **_seed_headers(seed), **_mark_headers(info)})


@eleven_router.post("/text-to-speech/{voice_id}/stream/with-timestamps")
def stream_tts_with_timestamps(voice_id: str, item: CreateSpeechRequest, http_request: Request,
                               output_format: StreamFormat = "pcm_24000"):
    """ElevenLabs' streamed JSON: newline-delimited objects, one per chunk, each with ``audio_base64`` (the ``/stream`` route's
    bytes, in its formats), ``alignment`` and ``normalized_alignment``: the characters whose times the chunk's tick committed
    (the two are the same part), or null where the chunk carries none.  A character's time follows its audio by the server's
    ``timestamp_lag_frames`` and is never revised (align.py).  501 unless the server has ``alignment_heads``; 400
    with the trim options, ``best_of`` or a text the engine refuses."""
    import base64
    import json

    core = http_request.app.state.tts_core
    if not core.alignment_heads:
        raise HTTPException(status_code=501, detail="this server has no alignment_heads: rank the checkpoint's heads with "
                                                    "`python -m smoltts_amd.align rank --checkpoint DIR --texts FILE` and set them")
    info: dict = {}
    try:
        pairs, seed = core.stream_audio_timed(item.text, voice=voice_id, output_format=output_format, sampling=item.request_sampling(),
                                              speed=item.speed, loudness=item, info=info)
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))

    def lines():
        try:
            for audio, part in pairs:
                al = None if part is None else part.to_json()
                yield (json.dumps({"audio_base64": base64.b64encode(audio).decode("ascii"), "alignment": al, "normalized_alignment": al}) + "\n").encode()
        finally:
            pairs.close()

    return StreamingResponse(_answer_first(lines()), media_type="application/x-ndjson", headers={
        "X-Sample-Rate": output_format.split("_")[1], **_seed_headers(seed), **_mark_headers(info)})


class StreamInputOptions(SamplingFields, LoudnessFields):
    """The first line of a ``stream-input`` body: the ``/stream`` body without its ``text``."""
    model_id: Optional[str] = Field(default=None)
    voice_settings: Optional[VoiceSettings] = Field(default=None)

    @property
    def speed(self) -> Optional[float]:
        return None if self.voice_settings is None else self.voice_settings.speed


class _DuplexResponse(StreamingResponse):
    """A streamed response whose handler is still reading the request body: it does not listen on ``receive`` for the client's
    disconnect, as ``StreamingResponse`` does below ASGI 2.4 (it would take body messages away from the reader, which sees a
    disconnect itself)."""

    async def __call__(self, scope, receive, send) -> None:
        try:
            await self.stream_response(send)
        except OSError:
            pass  # (the client went away: the body iterator has been closed)


async def _ndjson(body):
    """The lines of a newline-delimited JSON body, as they arrive: one parsed value per non-empty line (``ValueError`` for a line
    that is not JSON); the last line needs no newline."""
    buf = b""
    async for part in body:
        buf += part
        while b"\n" in buf:
            line, buf = buf.split(b"\n", 1)
            if line.strip():
                yield json.loads(line)
    if buf.strip():
        yield json.loads(buf)


def _input_line(obj) -> Tuple[str, Optional[str]]:
    """A line behind the first: ``{"text": "..."}`` or ``{"flush": true}`` -> ("text", the text) / ("flush", None)."""
    if isinstance(obj, dict) and set(obj) == {"text"} and isinstance(obj["text"], str):
        return "text", obj["text"]
    if isinstance(obj, dict) and set(obj) == {"flush"} and obj["flush"] is True:
        return "flush", None
    raise ValueError('a line must be {"text": "..."} or {"flush": true}')


@eleven_router.post("/text-to-speech/{voice_id}/stream-input")
async def stream_input_tts(voice_id: str, http_request: Request, output_format: StreamFormat = "pcm_24000"):
    """Text in as it is written, audio out as it is spoken (for a language model in front of the synthesiser).  The body is
    newline-delimited JSON, read as it arrives: the first line holds the options of the ``/stream`` body without ``text``
    (``{}`` for none), every later line is ``{"text": "..."}`` -- a piece of the text, cut anywhere -- or ``{"flush": true}``,
    which speaks what is buffered without waiting for its sentence to end; the end of the body ends the text.  The response is
    the chunked audio of ``/stream``, one stream for the whole text (``BatchScheduler.submit_incremental``).  A line that cannot
    be read answers 422 while no audio has gone out; after that it ends the stream."""
    from pydantic import ValidationError

    core = http_request.app.state.tts_core
    kind, rate = output_format.split("_")
    lines = _ndjson(http_request.stream())
    try:
        first = await lines.__anext__()
        item = StreamInputOptions.model_validate(first)
    except StopAsyncIteration:
        raise HTTPException(status_code=422, detail="the body is empty: its first line holds the options")
    except ValidationError as e:
        raise HTTPException(status_code=422, detail=_finite(json.loads(e.json(include_url=False, include_context=False))))
    except ValueError as e:
        raise HTTPException(status_code=422, detail=f"line 1: {e}")
    info: dict = {}
    try:
        stream, seed = core.open_input_stream(voice_id, output_format, sampling=item.request_sampling(), speed=item.speed, loudness=item,
                                              info=info)
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))
    loop = asyncio.get_running_loop()
    out: asyncio.Queue = asyncio.Queue()  # bytes, then None or an exception

    def pump():  # the chunk iterator blocks: it runs in a thread of its own
        end = None
        try:
            for b in stream.chunks:
                loop.call_soon_threadsafe(out.put_nowait, b)
        except Exception as e:
            end = e
        loop.call_soon_threadsafe(out.put_nowait, end)

    threading.Thread(target=pump, name="smoltts-stream-input", daemon=True).start()

    async def read_text():
        n = 1
        try:
            while True:
                n += 1
                try:
                    obj = await lines.__anext__()
                except StopAsyncIteration:
                    break
                what, text = _input_line(obj)
                stream.feed(text) if what == "text" else stream.flush()
        except Exception as e:  # a line that cannot be read, or text the engine refuses (a bad break tag): the request ends
            stream.cancel()
            raise ValueError(f"line {n}: {e}") if isinstance(e, ValueError) else e
        stream.close()

    reader = asyncio.ensure_future(read_text())
    getter = asyncio.ensure_future(out.get())
    while not getter.done():
        await asyncio.wait({getter} if reader.done() else {getter, reader}, return_when=asyncio.FIRST_COMPLETED)
        if reader.done() and reader.exception() is not None and not getter.done():
            getter.cancel()
            e = reader.exception()
            raise HTTPException(status_code=422 if isinstance(e, ValueError) else 500, detail=str(e))
    head = getter.result()
    if isinstance(head, ValueError):  # a request the engine refuses (as on /stream)
        raise HTTPException(status_code=400, detail=str(head))

    async def body():
        item = head
        try:
            while item is not None and not isinstance(item, Exception):
                yield item
                item = await out.get()
        finally:
            if item is not None:  # the client went away, or the engine failed: stop working for the request
                stream.cancel()
            if not reader.done():
                reader.cancel()
            elif not reader.cancelled():
                reader.exception()  # (a bad line behind the first chunk has ended the stream: there is nobody left to tell)

    return _DuplexResponse(body(), media_type="audio/wav", headers={
        "Content-Disposition": f'attachment; filename="speech.{kind}"', "X-Sample-Rate": rate, **_seed_headers(seed), **_mark_headers(info)})


class VoiceSample(BaseModel):
    text: Optional[str] = None
    audio: str  # base64 RIFF WAV: 16-bit PCM or 32-bit float (also WAVE_FORMAT_EXTENSIBLE), 8-48 kHz, any channel count


class AddVoiceRequest(BaseModel):
    name: str
    samples: List[VoiceSample] = Field(min_length=1)
    system_prompt: Optional[str] = None


@eleven_router.post("/voices/add")
def add_voice(item: AddVoiceRequest, http_request: Request):
    """Clone a voice from reference recordings and their transcripts; the answer's ``voice_id`` names it on every speech route."""
    from .. import NoEncoderError
    from .voices import decode_sample_audio

    core = http_request.app.state.tts_core
    samples = []
    for i, smp in enumerate(item.samples):
        if not smp.text or not smp.text.strip():
            raise HTTPException(status_code=400, detail=f"sample {i} has no text")
        try:
            samples.append({"text": smp.text, "audio": decode_sample_audio(smp.audio)})
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"sample {i}: {e}")
    try:
        voice_id = core.add_voice(item.name, samples, item.system_prompt)
    except NoEncoderError as e:
        raise HTTPException(status_code=501, detail=str(e))
    except OverflowError as e:
        raise HTTPException(status_code=409, detail=str(e))
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))
    return {"voice_id": voice_id}


class ForcedAlignmentRequest(BaseModel):
    audio: str  # base64 RIFF WAV, as a voice sample's (server/voices.py)
    text: str
    voice: Optional[str] = None


@eleven_router.post("/forced-alignment")
def forced_alignment(item: ForcedAlignmentRequest, http_request: Request):
    """ElevenLabs' forced alignment with a JSON body (base64 WAV in the forms and rates of ``/voices/add``) instead of multipart:
    ``characters`` [{text, start, end}], ``words`` [{text, start, end, loss}] and ``loss`` -- the times read from the slow attention
    while the recording's codes run through the model teacher-forced behind ``text``, the losses the model's own -log-probability of
    the recording's slow tokens (align.py).  501 unless the server has ``alignment_heads``; 400 for audio that cannot
    be read, an empty text, a recording shorter than one frame or longer than the model's context allows."""
    import base64
    import binascii

    from .. import NoEncoderError
    from .voices import parse_wav

    core = http_request.app.state.tts_core
    if not core.alignment_heads:
        raise HTTPException(status_code=501, detail="this server has no alignment_heads: rank the checkpoint's heads with "
                                                    "`python -m smoltts_amd.align rank --checkpoint DIR --texts FILE` and set them")
    try:
        pcm, rate = parse_wav(base64.b64decode(item.audio, validate=True))
    except (binascii.Error, ValueError, TypeError) as e:
        raise HTTPException(status_code=400, detail=f"audio: {e}")
    try:
        out = core.align_recording(pcm, rate, item.text, item.voice or "heart")
    except NoEncoderError as e:
        raise HTTPException(status_code=501, detail=str(e))
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))
    return JSONResponse(_finite(out.to_json()))


@eleven_router.get("/voices")
def list_voices(http_request: Request):
    return {"voices": http_request.app.state.tts_core.list_voices()}


@eleven_router.delete("/voices/{voice_id}")
def delete_voice(voice_id: str, http_request: Request):
    from ..prompt import VOICE_MAP

    if voice_id in VOICE_MAP:
        raise HTTPException(status_code=400, detail=f"{voice_id!r} is a premade voice")
    try:
        http_request.app.state.tts_core.remove_voice(voice_id)
    except KeyError:
        raise HTTPException(status_code=404, detail=f"no voice {voice_id!r}")
    return {"status": "ok"}


class DetectRequest(BaseModel):
    audio: str  # base64 RIFF WAV, as a voice sample's (server/voices.py)


@eleven_router.post("/watermark/detect")
def detect_watermark(item: DetectRequest, http_request: Request):
    """Whether a recording carries this server's watermark (extension; watermark.detect against the configured key, which is
    never returned): ``{"detected": bool, "score": float}``.  404 without a ``watermark`` setting, 422 for audio that cannot
    be read."""
    import base64
    import binascii

    from ..watermark import detect
    from .voices import parse_wav

    core = http_request.app.state.tts_core
    if core.watermark is None:
        raise HTTPException(status_code=404, detail="no watermark is configured")
    try:
        pcm, rate = parse_wav(base64.b64decode(item.audio, validate=True))
    except (binascii.Error, ValueError, TypeError) as e:
        raise HTTPException(status_code=422, detail=f"audio: {e}")
    d = detect(pcm, core.watermark.key, rate)
    return {"detected": d.detected, "score": round(d.score, 3)}


@eleven_router.get("/stats")
def stats(http_request: Request):
    """Not in the reference: serving counters (requests by outcome, frames delivered, slots in use) of the scheduler or pool."""
    core = http_request.app.state.tts_core
    sched = core.scheduler
    out = sched.stats() if sched is not None and hasattr(sched, "stats") else {}
    if core.long_text == "segment":
        out = {**out, "segments": core.segments}  # segments of completed segmented requests
    return out


def _finite(v):
    if isinstance(v, float) and not math.isfinite(v):
        return str(v)
    if isinstance(v, dict):
        return {k: _finite(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_finite(x) for x in v]
    return v


async def _validation_error(request, exc):
    """FastAPI's 422 answer, also for a body with NaN / Infinity (a speed of NaN): the echoed input is written as a string
    instead of failing the JSON encoding with a 500."""
    from fastapi.encoders import jsonable_encoder

    return JSONResponse(status_code=422, content={"detail": _finite(jsonable_encoder(exc.errors()))})


def create_app(model=None, settings: Optional[dict] = None, scheduler=None) -> FastAPI:
    """``model``: a ``smoltts_amd.SmolTTS`` (or any object with ``__call__``/``stream``); ``scheduler``: an
    optional ``BatchScheduler`` so that concurrent requests are decoded together (handlers are plain
    ``def`` and run in FastAPI's thread pool; the reference's ``async def`` handlers serialise requests)."""
    from contextlib import asynccontextmanager

    @asynccontextmanager
    async def lifespan(_app):
        yield
        if scheduler is not None and hasattr(scheduler, "close"):  # finish what is in flight, then release the GPU(s)
            try:
                scheduler.close(drain=True)
            except TypeError:  # a pool: its workers drain their own schedulers
                scheduler.close()

    app = FastAPI(lifespan=lifespan)
    app.add_exception_handler(RequestValidationError, _validation_error)
    app.include_router(openai_router)
    app.include_router(eleven_router)
    app.state.settings = settings
    app.state.tts_core = TTSCore(model, settings, scheduler)
    return app


def main():
    import functools

    import uvicorn

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, help="settings JSON: {checkpoint_dir, mimi_checkpoint, generation{...}, model_type{...}}")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--gpus", type=int, default=1, help="worker processes, one per GPU (request-level data parallelism); 1 = serve from this process")
    args = ap.parse_args()
    from .pool import GpuPool, scheduler_from_settings
    from .settings import ServerSettings

    try:
        settings = ServerSettings.get_settings(args.config)
        settings.get_checkpoint_dir()
    except ValueError as e:
        raise SystemExit(f"settings: {e}")
    settings = settings.model_dump()  # plain data: it travels to the worker processes

    if args.gpus > 1:
        # this process stays off the GPUs: it parses HTTP and relays audio; every worker owns one GPU and one scheduler
        st = ServerSettings(**settings)
        sched = GpuPool(functools.partial(scheduler_from_settings, settings), devices=list(range(args.gpus)),
                        generation_settings=st.generation.to_settings(),
                        watermark=st.watermark.to_watermark() if st.watermark is not None else None,
                        alignment_heads=st.alignment_heads)
        model = None
    else:
        sched = scheduler_from_settings(settings)
        model = sched.tts
    uvicorn.run(create_app(model, settings, sched), host="0.0.0.0", port=args.port)


if __name__ == "__main__":
    main()
