"""Continuous batching on top of the slot-restart primitives of the engine.

The reference serves one request at a time (its handlers call the model inline,
mlx_inference/.../server/routes/openai.py:17-28).  Here one worker thread owns an ``LMSession`` with
``max_batch`` slots: new requests are prefilled into free slots while the other slots keep decoding
(``smoltts_lm_prefill_deferred`` restarts only the listed slots and leaves frame 0 to the next frame graph), every tick
decodes a few frames for all slots, finished slots (``<|im_end|>`` or frame budget) are released.  Prompts longer than
``prefill_chunk`` columns are prefilled in chunks (``smoltts_lm_prefill_chunk``) with a tick for the speaking slots
between chunks.

The loop is pipelined so that the GPU never waits for Python: tick k is queued, a device-side snapshot of the output ring
is queued behind it, and *then* the host reads the snapshot of tick k-1 (on a copy stream) and does its bookkeeping while
tick k runs.  A slot that finished in tick k-1 is therefore refilled in tick k+1 (one tick of that slot is the price).
Codec work runs on a codec stream beside the ticks and its PCM is fetched on the copy stream when its event has fired:
streaming requests share one codec session whose slots mirror the LM slots (every slot keeps its own stream position,
``smoltts_mimi_reset_slots`` starts a new stream in a slot) and are decoded together, one codec pass per tick, launched once
the host has seen that tick's snapshot (so beside the next tick); a stream with a speed or an output format is stretched
and converted in the same pass (``route.StreamConverter``).  A blocking request is decoded when its utterance is complete,
up to ``CODEC_BATCH`` finished utterances per codec pass.  A request's PCM is identical to what
``SmolTTS.__call__`` / ``stream`` return for it alone.
"""
from __future__ import annotations

import queue
import threading
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from ..request import SpeechOptions, parse_request

NO_OPTIONS = parse_request()  # a request without any audio option


@dataclass
class _Request:
    text: str
    voice: str
    stream: bool
    max_new_tokens: int
    out: "queue.Queue" = field(default_factory=queue.Queue)  # np.ndarray chunks, then None (or an Exception)
    slot: int = -1
    emitted: int = 0
    pending: list = field(default_factory=list)  # blocking requests: audio-code columns awaiting their codec pass
    prompt: object = None
    first_tick: int = 0  # index of the tick that produces this request's frame 0: older snapshots show the slot's previous tenant
    last_tick: int = 1 << 62  # index of the tick in which the frame budget runs out (known at admission): the slot's next tenant may
                              # be queued right behind it, before the host has seen that tick's snapshot
    retired: bool = False     # the slot has been handed to the next tenant; later snapshots of the slot are not this request's
    stream_done: bool = False  # streaming: the last frames have been seen (the end marker goes out with the last codec pass)
    cancelled: bool = False  # set by the client side (cancel / an abandoned chunk iterator), honoured by the worker at its next look
    closed: bool = False  # the end marker (None or an exception) has been queued
    # the request's audio options as parsed at submit (request.py), read where a stage is started or applied: a stream's in its
    # codec pass (StreamConverter.start), a blocking utterance's whole.  A best_of take, a segment's codec job: the default value
    opts: SpeechOptions = NO_OPTIONS
    sampling: object = None  # config.RequestSampling, resolved at submit (seed drawn there for a sampled request without one)
    voice_entry: object = None  # _Voice of a registered voice, taken at submit (a later remove_voice does not affect the request)
    pos0: int = 0             # position of the prompt's first column: the voice's prefix length P for a registered voice
    prefix: object = None     # lm.PrefixKV installed into the slot at admission (None: the whole prompt is prefilled)
    stretch_in: list = field(default_factory=list)  # blocking requests with a speed: the utterance's PCM until its last pass
    seg: Optional["_Segmented"] = None  # a long text as chained segments (None: one utterance)
    part_of: object = None    # (request, k): this codec job decodes segment k of a blocking segmented request
    loudness_gain_db: Optional[float] = None  # blocking: the gain that was applied (set before the audio goes out)
    inc: Optional["_Incremental"] = None  # a stream whose text is fed in pieces (submit_incremental)
    watermark: bool = False   # the audio gets the scheduler's watermark: a stream in its codec pass, a blocking utterance whole, last
    trimmed_s: float = 0.0    # blocking: the seconds of silence that were cut (set before the audio goes out)
    finish_reason: Optional[str] = None  # "stop" / "length" (config.finish_reason), valid once the request has ended; a segmented
                                         # request is "length" if any segment was
    reasons: list = field(default_factory=list)  # ... of the utterances (segments) that have ended so far
    frame_counts: list = field(default_factory=list)  # ... and the frames each of them was given (its <|im_end|> frame included)
    request_cap: Optional[int] = None    # the request's own max_new_tokens; ``max_new_tokens`` is the cap of the utterance (segment)
                                         # in the slot, which the scheduler's max_frames_per_byte may lower
    slot_sampling: object = None         # the entry of the utterance (segment) in the slot: ``sampling`` (the segment's) with the
                                         # scheduler's min_frames_per_byte applied
    # scores.  A best_of request is a parent that never holds a slot: its takes are ordinary blocking requests
    # (``take_of`` = (parent, k)) that report to it when they end instead of going to the codec; the winner's codes then become
    # the parent's own codec job, and ``sampling`` the winner's entry (its seed replays the chosen audio as a plain request)
    lp: list = field(default_factory=list)  # a scored blocking request: its frames' scores, tick by tick
    logprobs: object = None              # float32 scores of the (chosen) utterance's frames, valid once the request has ended
    mean_logprob: Optional[float] = None  # ... and their float64 mean
    takes: object = None                 # parent: per take its seed, mean_logprob, min_logprob, frames, finish_reason, chosen
    take_reqs: list = field(default_factory=list)  # parent: the takes' requests
    take_of: object = None
    best_of: int = 1
    # character timestamps: a blocking request of one utterance whose frames measure where the scheduler's
    # alignment heads look over its own text
    align_window: object = None          # (t0, t1): the text's positions in the slot, known at admission
    align_ids: object = None             # ... and the text's token ids
    al: list = field(default_factory=list)  # its frames' rows [frames, heads, 2], tick by tick
    out_samples: int = 0                 # samples handed out so far: the delivered duration
    audio_frames: int = 0                # frames whose slow id was semantic: the ones the codec decodes
    alignment: object = None             # align.Alignment, set before the request's end marker
    # peak limiter: a stream is limited in its codec pass, last of the float stages; a blocking utterance whole, last
    peak_reduction_db: Optional[float] = None  # blocking: -20 log10 of the smallest gain applied (set before the audio goes out)
    # streamed character timestamps: a stream of one utterance whose slot the device fits causally, tick by tick;
    # ``alignment`` is then the concatenation of the parts handed out
    live_timestamps: bool = False
    aligner: object = None               # align.StreamAligner, made when the request takes its slot


@dataclass
class _Segmented:
    """A long text's progress (longform.SegmentPlan): the request keeps its slot from its first segment to its last."""
    plan: object              # longform.SegmentPlan
    sampling: object          # the sampling of segment k (its seed is seed_k)
    k: int = 0                # the segment in the slot now
    prev: object = None       # (text, (n_codebooks, F) codes) of segment k - 1: segment k's context
    cols: list = field(default_factory=list)   # streaming: semantic code columns of segment k so far
    pcm: list = field(default_factory=list)    # blocking: per segment, its PCM pieces from the codec
    parts: list = field(default_factory=list)  # blocking: the segments' codec jobs
    done: int = 0             # blocking: segments whose PCM is complete

    @property
    def final(self) -> bool:
        """No segment follows the one in the slot (a plan that grows: and none can)."""
        grows = getattr(self.plan, "final", None)
        return grows(self.k) if grows is not None else self.k == len(self.plan.segs) - 1


@dataclass
class _Incremental:
    """The text side of a request fed in pieces.  The client's calls run the splitter under ``lock`` and leave its segments in
    ``inbox``; the worker alone moves them into the request's plan (``_ingest``), so that a tick's codec pass and its
    bookkeeping see one and the same plan."""
    splitter: object                      # longform.IncrementalSplitter
    idle_timeout_s: float
    flush_after_s: Optional[float]
    lock: object = field(default_factory=threading.Lock)
    inbox: list = field(default_factory=list)
    close_asked: bool = False             # close() was called (or the idle timeout did it): the inbox holds the last segments
    last_input: float = 0.0               # time.monotonic() of the last feed
    parked_at: float = 0.0                # ... and of the park, while parked
    state: str = "waiting"                # "waiting" for its first segment (no slot yet), then "admitted"


@dataclass
class IncrementalRequest(_Request):
    """What ``submit_incremental`` returns: ``feed`` / ``flush`` / ``close`` for the text, iteration for the chunks, ``cancel``."""
    sched: object = None

    def feed(self, text) -> None:
        """More text (``str``, or ``bytes`` of UTF-8 cut anywhere).  ``ValueError``: a bad break tag, or text after ``close``
        (an idle timeout closes too)."""
        self.sched._inc_text(self, "feed", text)

    def flush(self) -> None:
        """Speak what is buffered now, without waiting for its sentence to end."""
        self.sched._inc_text(self, "flush")

    def close(self) -> None:
        """The text is complete: what is buffered is its last segment."""
        self.sched._inc_text(self, "close")

    def cancel(self) -> None:
        self.sched.cancel(self)

    def __iter__(self):
        return self.sched.iter_chunks(self)


@dataclass
class _Voice:
    voice_id: str
    grid: np.ndarray   # the speaker prompt grid (1 + n_fast, P)
    prefix: object     # lm.PrefixKV: its KV rows, computed once
    name: Optional[str] = None


@dataclass
class _CodecJob:
    req: _Request
    cols: np.ndarray  # (F, n_codebooks) int32 audio codes of the complete utterance
    done: int = 0     # frames already handed to the codec


@dataclass
class _Snapshot:
    """Device-side copies of the output ring queued behind tick ``tick_no``, and the event that fires when they are taken."""
    codes: object
    n_frames: object
    done: object
    event: object
    tick_no: int
    logprobs: object = None  # the score array, cloned only while some live slot scores
    alignment: object = None  # the alignment rows, cloned only while some live slot measures
    fit: object = None  # (committed counts, starts) of the causal fit, cloned only while some live stream asks for timestamps


@dataclass
class _Delivery:
    """A codec pass whose PCM goes out to its requests, in order, once ``event`` has fired (None: nothing to wait for)."""
    event: object
    pcm: object       # the pass's PCM on the device
    items: list       # [(request, codec slot, samples, last?)]
    urgent: bool = False  # a stream's first chunk is in it: handed out as soon as the pass is through
    keep: object = None   # device tensors the pass reads, kept alive until it has run
    conv: object = None   # route.StreamPass: the stream conversion of the pass (None: float32 rows of ``pcm``)
    parts: object = None  # {slot: align.AlignmentPart}: the timestamps this tick committed, handed out with its chunks


@dataclass
class _StretchJob:
    """A complete blocking utterance with a speed, stretched in pieces by ``_poll_stretches``."""
    req: _Request
    pcm: np.ndarray
    pos: int = 0                                   # input samples handed to the stretcher so far
    outs: list = field(default_factory=list)       # stretched pieces collected so far
    state: str = "waiting"  # "waiting" for a stretcher slot, "running" in it, or "ending": its last piece is in the call in flight
    slot: int = -1          # its stretcher slot while running or ending


def stream_ends(n, done, cap):
    """Whether a stream with frame budget ``cap`` is complete at a snapshot showing ``n`` frames and the ``done`` flag: the slot
    has stopped with a frame, or the budget is reached.  Elementwise on numpy values and torch tensors alike: the host closes a
    response with it and the device flushes the stretcher with it, from the same snapshot, so the two agree."""
    return (done != 0) & (n > 0) | (n >= cap)


class BatchScheduler:
    CODEC_BATCH, CODEC_CHUNK, CODEC_WAIT = 16, 64, 32  # slots, frames per slot and pass, LM frames a pass may wait for company

    def __init__(self, tts, max_batch: int = 32, frames_per_tick: int = 4, generation_settings=None, max_prompt_rows: int = 4096,
                 prefill_chunk: Optional[int] = 128, side_prefill: bool = True, side_prefill_min_active: Optional[int] = None,
                 codec_products: int = 6, watermark=None, min_frames_per_byte: Optional[float] = None,
                 max_frames_per_byte: Optional[float] = None, alignment_heads=None, timestamp_lag_frames: int = 6):
        """``alignment_heads`` (``[(layer, head), ...]``, at most 16; None: no request can ask for timestamps): the heads of the slow
        attention that ``submit(timestamps=True)`` reads character times from (align.py).
        ``timestamp_lag_frames`` (1 .. 64): how many frames behind its audio a stream with ``live_timestamps`` commits a
        character's time.
        ``watermark`` (a ``watermark.Watermark``; None: no request can be marked): the one key of this scheduler's marked
        requests; a request that does not say (``submit(watermark=None)``) is marked when there is one.
        ``min_frames_per_byte`` / ``max_frames_per_byte`` (None: off): bounds on every utterance's length from its text's UTF-8
        byte count, per segment on the long-text path (``config.length_bounds``)."""
        import torch

        from ..config import GenerationSettings
        from ..lm import LMSession
        from ..route import StreamConverter
        from ..stages import Finisher
        from ..generate import _apply_sampling

        from ..watermark import Watermark

        if watermark is not None and not isinstance(watermark, Watermark):
            raise ValueError("watermark must be a smoltts_amd.watermark.Watermark or None")
        from ..align import check_lag

        self.timestamp_lag_frames = check_lag(timestamp_lag_frames)
        self.watermark = watermark
        self.min_frames_per_byte, self.max_frames_per_byte = min_frames_per_byte, max_frames_per_byte
        self.tts = tts
        self.B = max_batch
        self.codec_products = codec_products  # SMOLTTS_MIMI_OPT_PRODUCTS of the codec sessions (6: fp32-grade)
        self.tick = frames_per_tick
        self.prefill_chunk = prefill_chunk  # columns per utterance per prefill call (None: whole prompts at once)
        # refills while most slots are speaking: the new prompts' KV rows are computed on a second stream beside the next tick
        # (LMSession.side_park / side_run / side_start) instead of in line between two ticks; the new tenants then start one
        # tick later.  With few slots speaking the in-line prefill answers sooner and stops nobody worth mentioning.
        self.side_prefill = side_prefill and __import__("os").environ.get("SMOLTTS_SIDE_PREFILL") != "0"  # (the switch of tools/bench_scheduler.py A/B runs)
        self.side_min_active = max(1, max_batch // 2) if side_prefill_min_active is None else side_prefill_min_active
        self._side = None  # the one refill in flight: {"h": handle, "reqs": [...], "state": "parked" | "running"}
        self.settings = generation_settings or GenerationSettings.greedy()
        self.max_frames = self.settings.max_new_tokens + 1
        self.session = LMSession(tts.lm, max_batch, max_seq=tts.config.max_seq_len, max_rows=max(max_prompt_rows, max_batch),
                                 max_frames=self.max_frames)
        _apply_sampling(self.session, self.settings)
        # per-request sampling: the session runs in slot mode, every slot with the configured settings until a request names its
        # own; a request's entry is written on the frame stream before its frame 0 can be picked, a freed slot gets the default back
        from ..config import RequestSampling

        self._default_sampling = RequestSampling().resolve(self.settings, draw_seed=False)
        self._slot_sampling: Dict[int, object] = {}  # the entry each slot has on the device
        self._write_sampling({b: self._default_sampling for b in range(max_batch)})
        from ..align import check_heads

        self.alignment_heads = check_heads(alignment_heads, tts.config)
        self._slot_align: Dict[int, tuple] = {}  # the window each slot has on the device (absent: off)
        self._fitter = None                      # lm.AlignFitter: the streams' causal fit, one slot per LM slot
        self._fit_on: set = set()                # the slots it is switched on in
        if self.alignment_heads:
            from ..lm import AlignFitter

            self.session.set_align_heads(self.alignment_heads)
            self._fitter = AlignFitter.for_session(self.session)  # (a slab and no launch: nothing runs until a stream asks)
        torch.cuda.current_stream().synchronize()  # (the worker's frame stream is another one)
        self.session.set_frames_per_graph(min(max(frames_per_tick, 1), 8))  # a tick is one graph launch where it fits
        self._torch = torch
        self._pending: "queue.Queue[_Request]" = queue.Queue()
        self._active: Dict[int, _Request] = {}
        self._retiring: List[_Request] = []     # budget-terminated requests whose slot already has its next tenant; their last
                                                # snapshots are still to be read
        self._free: List[int] = list(range(max_batch))
        self._stop = threading.Event()
        self._wake = threading.Event()          # set by submit(): the idle worker sleeps on it (no peeking into the queue)
        self._finished: List[_Request] = []     # complete blocking utterances waiting for a codec slot
        self._batch_codec = None                # codec session of the blocking requests: CODEC_BATCH slots, one utterance each
        self._codec_jobs: List[Optional[_CodecJob]] = [None] * self.CODEC_BATCH
        self._codec_fresh: List[int] = []       # slots whose utterance has not been through a pass yet (stream restart due)
        self._codec_slot_age = [0] * self.CODEC_BATCH  # passes a slot has seen since its last restart
        self._codec_wait = 0                    # ticks since the last pass while work was waiting
        self._stream_codec = None               # codec session whose slot b carries the stream of LM slot b (streaming requests)
        # behind it, slot b stretches and converts LM slot b's stream when it has a speed / a format
        self._stream_conv = StreamConverter(self.session.engine.device, max_batch, max(frames_per_tick, 1) * 1920, watermark=watermark)
        self._block_ts = None                   # stretcher of the blocking requests' whole utterances
        self._stretches: List[_StretchJob] = []  # blocking utterances with a speed, complete, being stretched (_poll_stretches)
        self._stretch_flight = None             # the stretch call in flight: (event, host output, host counts, keep-alive, [jobs])
        self._codec_age = [0] * max_batch       # codec passes each of its slots has seen since that slot's last reset
        self._deliveries: List[_Delivery] = []  # codec passes whose PCM has not been handed out yet, in order
        self._snaps: List[_Snapshot] = []       # snapshots of the output ring the host has not looked at yet (oldest first)
        self._tick_no = 0                       # ticks queued so far
        self._counts = {"completed": 0, "cancelled": 0, "failed": 0, "frames_delivered": 0, "prefix_installs": 0, "segments": 0,
                        "idle_timeouts": 0}
        self._refills: List[_Request] = []      # segmented requests whose slot waits for their next segment's prompt
        self._parked: List[_Request] = []       # ... and incremental ones whose slot waits for text that has not arrived yet
        self._incs: List[_Request] = []         # the incremental requests alive (worker side)
        self._inc_new: "queue.Queue[_Request]" = queue.Queue()  # ... and those the worker has not seen yet
        self._finisher = Finisher(self.session.engine.device)  # the blocking requests' chain behind the codec (stages made on first use)
        self._dead: Optional[Exception] = None  # why the worker stopped
        self._draining = False
        self._held: Optional[_Request] = None   # next in line, waiting for room in a prefill call
        self._gpu_wait_s = 0.0                  # time the worker spent waiting for the GPU (small => the host is the limit)
        self._voices: Dict[str, _Voice] = {}    # registered voices (add_voice); read by submit, written by the worker
        self._jobs: "queue.Queue[dict]" = queue.Queue()  # voice registrations waiting for the worker
        self._job = None                        # the registration in progress: {"job": ..., "steps": generator}
        self._scratch = None                    # one-slot session the voices' prefixes are computed in (created on first use)
        self._t0 = time.time()
        self._thread = threading.Thread(target=self._run, name="smoltts-scheduler", daemon=True)
        self._thread.start()

    # ------------------------------------------------------------------ client side
    def submit(self, text: str, voice: str = "heart", stream: bool = False, max_new_tokens: Optional[int] = None,
               output_format: Optional[str] = None, sampling=None, live_timestamps: bool = False, **options) -> _Request:
        """``sampling``: a ``config.RequestSampling``; missing fields take the configured settings, and a sampled request without
        a seed gets one here.  The resolved value is ``request.sampling``; its seed replays the request.
        ``live_timestamps`` (streams of one utterance; needs the scheduler's ``alignment_heads``; ``ValueError`` without a stream,
        with ``segment``, the trim options, ``best_of`` or ``timestamps``): ``timed_chunks(request)`` yields each chunk with the
        ``align.AlignmentPart`` its tick committed (or None), a character's time following its audio by ``timestamp_lag_frames``
        plus a tick at the most; ``request.alignment`` is their concatenation once the request has ended.  It is no audio option:
        the audio is what it is without it.
        ``output_format`` and ``options``: the request's audio options, handed whole to ``request.parse_request``, which lists
        them with their ranges and refuses a bad one here, before the request is queued (``ValueError``; ``TypeError`` for a
        name it does not know).  The parsed value is ``request.opts``.  Every stage runs on the GPU: a stream's in its codec
        pass (``StreamConverter.start`` when the stream takes its slot), a blocking utterance's over the whole utterance once
        its last codec pass is in, in the order and by the rules of ``stages.Finisher``.  What this front end adds to each:
        ``output_format``: the resampler's tail comes with the stream's last chunk.
        ``speed``: a stream is stretched in front of the format conversion, a blocking utterance as a whole.
        ``container``: FLAC framing in the same pass, behind the other stages; the stream header in front of the first chunk.
        ``segment``: a long text is spoken as chained segments in one slot, kept from the first segment to the last; each
        segment's end, seen in a snapshot, refills the slot with the next chained prompt.  A stream runs through the seam stage
        in front of its other stages (one stream); a blocking request decodes each segment as its own codec job and joins them
        on the GPU.  A text that is one segment without break tags is an ordinary request.
        ``loudness``: a stream is levelled causally, behind the seam and in front of the stretch, from
        ``loudness_start_gain_db``; a blocking utterance is measured whole and given one gain (``request.loudness_gain_db``),
        behind the seam join and in front of the stretch.
        ``watermark`` (None: marked when the scheduler has a key; True without a key: ``ValueError``): the scheduler's watermark
        (watermark.py), last of the float stages but for the limiter: a stream's behind the stretch, a blocking utterance's
        whole.  ``request.watermark`` says whether it was.
        ``trim_silence`` / ``max_pause_s`` / ``silence_threshold_db``: first of the stages: a stream segment by segment in front
        of the seam; a blocking utterance whole, each segment before the seam join (``request.trimmed_s`` is what was cut).
        ``peak_limit_db``: last of the float stages.  A stream is limited behind the watermark and in front of the conversion
        and the framing: it holds back 126 samples, which leave with its last chunk, and reports nothing.  A blocking utterance
        is limited whole behind everything else (``request.peak_reduction_db``: ``-20 log10`` of the smallest gain, 0.0 when
        nothing was limited), and with a ``loudness`` as well its one gain is not capped by the peak.
        ``timestamps`` (blocking requests of one utterance; needs the scheduler's ``alignment_heads``; ``ValueError`` with
        ``segment``, the trim options, a stream or ``best_of``): ``request.alignment`` is an ``align.Alignment`` -- per character of
        the text its start and end in seconds of the audio delivered -- once the request has ended.  The audio is not changed."""
        from ..config import RequestSampling, check_best_of, take_sampling

        p = parse_request(text, stream, output_format, **options)
        self._check_trim(p)
        resolved = (sampling if sampling is not None else RequestSampling()).resolve(self.settings)
        if live_timestamps:
            from ..align import check_live_timestamps

            check_live_timestamps(p, stream, bool(self.alignment_heads), resolved.takes)
        check_best_of(resolved, self.B, stream=stream, segmented=p.plan is not None)
        if p.timestamps:
            if not self.alignment_heads:
                raise ValueError("timestamps need alignment_heads: rank a checkpoint's heads with `python -m smoltts_amd.align rank`")
            if resolved.takes > 1:
                raise ValueError("timestamps cannot be combined with best_of")
        if self._dead is not None:  # the worker is gone (engine failure or close): nobody would ever answer
            raise RuntimeError(f"scheduler is not running: {self._dead}")
        if self._draining:
            raise RuntimeError("scheduler is not running: shutting down")
        req = _Request(text, voice, stream, min(max_new_tokens or self.settings.max_new_tokens, self.settings.max_new_tokens),
                       opts=p, sampling=resolved, voice_entry=self._voices.get(voice),
                       seg=_Segmented(p.plan, resolved) if p.plan is not None else None, watermark=self._marks(p.watermark),
                       live_timestamps=bool(live_timestamps))
        if resolved.takes > 1:
            # the parent carries the audio options and the response; its takes are plain blocking requests, admitted as slots
            # come free
            req.best_of = resolved.takes
            req.take_reqs = [_Request(text, voice, False, req.max_new_tokens, sampling=take_sampling(resolved, k), voice_entry=req.voice_entry,
                                      take_of=(req, k)) for k in range(resolved.takes)]
            for t in req.take_reqs:
                self._pending.put(t)
        else:
            self._pending.put(req)
        self._wake.set()
        if self._dead is not None:  # lost the race with a failing worker: answer it ourselves
            for t in req.take_reqs:
                self._end(t, RuntimeError(f"scheduler is not running: {self._dead}"))
            self._end(req, RuntimeError(f"scheduler is not running: {self._dead}"))
        return req

    def _check_trim(self, p) -> None:
        from ..trim import MAX_CALL

        if p.trims and self.tick * 1920 > MAX_CALL:
            raise ValueError(f"silence trimming takes at most {MAX_CALL // 1920} frames a tick")

    def _marks(self, asked: Optional[bool]) -> bool:
        """Whether a request that asked ``asked`` is marked: the scheduler's policy when it did not say."""
        if asked and self.watermark is None:
            raise ValueError("watermark asked for, and the scheduler has no watermark key")
        return self.watermark is not None if asked is None else bool(asked)

    def submit_incremental(self, voice: str = "heart", max_new_tokens: Optional[int] = None, output_format: Optional[str] = None,
                           sampling=None, segment=True, idle_timeout_s: float = 10.0, flush_after_s: Optional[float] = None,
                           **options) -> IncrementalRequest:
        """A stream whose text is not known yet: ``request.feed(text)`` as it arrives, ``request.close()`` at its end, the
        chunks by iterating the request (or ``iter_chunks``).  ``output_format`` and ``options`` are those of
        ``submit(stream=True, segment=...)`` (``segment``: True, a dict or a ``SegmentOptions``; it cannot be off).

        The text is cut by ``longform.IncrementalSplitter`` into the segments ``SegmentPlan.create`` gives the whole text, each
        handed over once no later input can change it, and spoken as a segmented stream whose segment list grows: the request
        takes its slot with its first segment and keeps it to its end.  When ``close()`` arrives before the last segment is
        opened, the stream is byte for byte that of ``submit(whole_text, stream=True, segment=...)``.

        *Latency over closing silence.*  Whether a segment is the last is not known while text may follow, and no segment
        waits to find out: segment k is opened as soon as it exists, as a segment with a seam behind it.  When the text is then
        closed with nothing behind segment k, the stream ends with it the way a stream's last segment ends: the seam stage's
        ``last`` marker releases its held trailing silence unchanged (``seam.SeamState.push(..., last=True)`` is the definition),
        and break tags behind the segment are dropped (they would have been the stream's trailing silence).

        *Parking.*  A slot whose segment ends before more text has arrived keeps its slot, its stage states and its conditioning
        context and takes no decode work -- the state of a segmented slot between two of its segments -- until a segment
        arrives.  The segment that ended has had its seam (its held silence cut or padded to the pause); a ``close()`` without
        more text then only flushes the stream's other stages.  A slot parked for ``idle_timeout_s`` without input is closed
        as if ``close()`` had been called.  ``cancel`` while parked frees the slot at once.

        ``flush_after_s`` (None: off): when no text has arrived for that long and the buffered text has not reached a sentence
        end, it is spoken as a segment of its own.  Such a segment is not one of the whole text's: the stream then differs
        from the whole text's."""
        from ..config import RequestSampling
        from ..longform import GrowingPlan, IncrementalSplitter, segment_options

        p = parse_request("", True, output_format, **options)
        self._check_trim(p)
        opts = segment_options(True if segment is None or segment is False else segment)
        if not float(idle_timeout_s) > 0.0 or (flush_after_s is not None and not float(flush_after_s) > 0.0):
            raise ValueError("idle_timeout_s and flush_after_s must be positive")
        resolved = (sampling if sampling is not None else RequestSampling()).resolve(self.settings)
        from ..config import check_best_of

        check_best_of(resolved, self.B, stream=True, segmented=True)
        if self._dead is not None or self._draining:
            raise RuntimeError(f"scheduler is not running: {self._dead or 'shutting down'}")
        req = IncrementalRequest("", voice, True, min(max_new_tokens or self.settings.max_new_tokens, self.settings.max_new_tokens),
                                 opts=p, sampling=resolved, voice_entry=self._voices.get(voice),
                                 seg=_Segmented(GrowingPlan(opts), resolved), watermark=self._marks(p.watermark), sched=self,
                                 inc=_Incremental(IncrementalSplitter(opts), float(idle_timeout_s),
                                                  None if flush_after_s is None else float(flush_after_s),
                                                  last_input=time.monotonic()))
        self._inc_new.put(req)
        self._wake.set()
        if self._dead is not None:
            self._end(req, RuntimeError(f"scheduler is not running: {self._dead}"))
        return req

    def _inc_text(self, req: _Request, what: str, text=None) -> None:
        """The client's ``feed`` / ``flush`` / ``close``: the splitter runs here, its segments wait for the worker."""
        inc = req.inc
        if self._dead is not None:
            raise RuntimeError(f"scheduler is not running: {self._dead}")
        with inc.lock:
            if inc.close_asked:
                if what == "feed":
                    raise ValueError("the request's text is closed")
                return
            if what == "feed":
                inc.inbox.extend(inc.splitter.feed(text))
                inc.last_input = time.monotonic()
            elif what == "flush":
                inc.inbox.extend(inc.splitter.flush())
            else:
                inc.inbox.extend(inc.splitter.close())
                inc.close_asked = True
        self._wake.set()

    def synthesize(self, text: str, voice: str = "heart", max_new_tokens: Optional[int] = None) -> np.ndarray:
        """Blocking: float32 PCM of the whole utterance."""
        return np.concatenate(list(self.iter_chunks(self.submit(text, voice, False, max_new_tokens))) or [np.zeros(0, np.float32)])

    def iter_chunks(self, req: _Request):
        """Chunks of one request; abandoning the iterator (a client that went away mid-stream) cancels the request."""
        pairs = self.timed_chunks(req)
        try:
            for chunk, _ in pairs:
                if len(chunk):  # (a stream with live_timestamps may hand out a part without audio)
                    yield chunk
        finally:
            pairs.close()

    def timed_chunks(self, req: _Request):
        """``(chunk, part)`` pairs of one request: ``part`` is the ``align.AlignmentPart`` of the characters whose times the
        chunk's tick committed, None for a chunk without one and for every chunk of a request without ``live_timestamps``.
        Abandoning the iterator cancels the request."""
        ended = False
        try:
            while True:
                item = req.out.get()
                if item is None or isinstance(item, Exception):
                    ended = True
                    if item is None:
                        return
                    raise item
                yield item if isinstance(item, tuple) else (item, None)
        finally:
            if not ended:
                self.cancel(req)

    def cancel(self, req: _Request) -> None:
        """Stop working for ``req``: its slot is handed to the next request at the worker's next look (within a tick); a
        request that is still queued never starts.  The slot itself simply keeps decoding until it is restarted — a batch
        step costs the same with or without it.  Nothing more is delivered except the end marker."""
        req.cancelled = True
        for part in list(req.seg.parts) if req.seg is not None else []:
            part.cancelled = True
        for t in req.take_reqs:  # a best_of request: its takes give their slots back at the worker's next look
            t.cancelled = True
        if req.take_reqs:
            self._wake.set()
        if req.inc is not None:
            self._wake.set()  # (a parked one is in no tick's books: the worker frees its slot when it looks at the text side)

    # ------------------------------------------------------------------ client side: registered voices
    def add_voice(self, voice_id: str, samples=None, grid=None, system_prompt: Optional[str] = None, name: Optional[str] = None) -> dict:
        """Register a cloned voice: ``samples`` (``SmolTTS.create_speaker`` input: [{"text", "audio" at 24 kHz}]) or a ready speaker
        ``grid``.  The worker encodes the samples (Mimi encoder) and computes the speaker turns' KV rows once, between ticks, a
        prefill chunk at a time; from then on a request naming ``voice_id`` gets those rows copied into its slot and prefills only
        its own turns.  Blocks until the voice is usable; ``ValueError`` for a voice the engine cannot serve.
        Returns {"voice_id", "prompt_positions"}."""
        from ..prompt import VOICE_MAP

        if (samples is None) == (grid is None):
            raise ValueError("pass samples or grid")
        if not isinstance(voice_id, str) or not voice_id or voice_id in VOICE_MAP:
            raise ValueError(f"voice id {voice_id!r} is empty or names a preset voice")
        return self._run_job({"voice_id": voice_id, "samples": samples, "grid": grid, "system_prompt": system_prompt, "name": name})

    def encode_speaker(self, samples, system_prompt: Optional[str] = None) -> np.ndarray:
        """The speaker grid of ``samples`` (``SmolTTS.create_speaker``), encoded on the worker thread between ticks."""
        return self._run_job({"voice_id": None, "samples": samples, "grid": None, "system_prompt": system_prompt, "name": None})

    def align_recording(self, audio, text: str, voice: str = "heart", speaker=None, rate: int = 24000):
        """Forced alignment (``SmolTTS.align_recording``) on the worker thread, between ticks: the Mimi
        encode, then the recording's grid through the scratch one-slot session of ``add_voice`` at most one ``prefill_chunk``-column
        chunk per loop turn, so the speaking slots are never held up by more than a chunk.  The scratch session has an alignment
        buffer of its own; the serving session's windows, forms and graphs are not touched.  Blocks until the
        ``align.RecordingAlignment`` is there.  ``ValueError`` (before the worker sees the request): no ``alignment_heads``, an
        empty text, audio shorter than one frame, prompt plus frames beyond the session's ``max_seq`` or ``max_frames``."""
        from ..align import check_recording_fits, no_heads_error
        from .voices import to_codec_rate

        if not self.alignment_heads:
            raise no_heads_error()
        if not isinstance(text, str) or not text.strip():
            raise ValueError("forced alignment needs a text")
        pcm = to_codec_rate(np.asarray(audio, dtype=np.float64).reshape(-1), int(rate))
        F = pcm.size // 1920
        if F < 1:
            raise ValueError("the audio holds no full frame (1920 samples at 24 kHz)")
        if speaker is None and voice in self._voices:
            speaker = self._voices[voice].grid
        a0 = int(self.tts.prompt_encoder.build_prompt(text, voice, speaker).shape[1])
        check_recording_fits(a0, F, self.session.max_seq, self.session.max_frames)
        return self._run_job({"align": True, "pcm": pcm[: F * 1920], "frames": F, "text": text, "voice": voice, "speaker": speaker})

    def _run_job(self, job: dict):
        job.update(done=threading.Event(), result=None, error=None)
        if self._dead is not None or self._draining:
            raise RuntimeError(f"scheduler is not running: {self._dead or 'shutting down'}")
        self._jobs.put(job)
        self._wake.set()
        while not job["done"].wait(timeout=0.1):
            if self._dead is not None and not job["done"].is_set():
                raise RuntimeError(f"scheduler is not running: {self._dead}")
        if job["error"] is not None:
            raise job["error"]
        return job["result"]

    def remove_voice(self, voice_id: str) -> None:
        """Forget a registered voice (``KeyError`` if there is none).  Requests already submitted for it keep its prefix."""
        del self._voices[voice_id]

    def voices(self) -> Dict[str, dict]:
        """Registered voices: id -> {"name", "prompt_positions"}."""
        return {k: {"name": v.name, "prompt_positions": int(v.grid.shape[1])} for k, v in list(self._voices.items())}

    def close(self, drain: bool = False, timeout: float = 300.0) -> None:
        """Stop the worker.  ``drain``: take no new requests but finish the ones in the books first (a server shutting down);
        otherwise requests in flight are answered with an error."""
        if drain and self._dead is None:
            self._draining = True
            deadline = time.time() + timeout
            while (self._thread.is_alive() and time.time() < deadline and
                   (self._active or self._side is not None or self._retiring or self._refills or self._parked or self._held is not None or not self._pending.empty() or self._codec_backlog() or self._deliveries or self._stretches)):
                time.sleep(0.01)
        self._stop.set()
        self._wake.set()
        self._thread.join(timeout=30)
        for name in ("_batch_codec", "_stream_codec", "_block_ts", "_scratch", "_fitter"):
            if getattr(self, name) is not None:
                getattr(self, name).close()
                setattr(self, name, None)
        self._finisher.close()
        self._stream_conv.close()
        self.session.close()

    # ------------------------------------------------------------------ worker: admission
    def _side_advance(self) -> None:
        """The refill in flight, one step on: parked -> its side call goes out (the host waits for the park, a few us behind the
        tick it was queued after); running -> the slots are armed on the frame stream and the requests enter the books: their
        frame 0 comes out of the next tick."""
        sd = self._side
        if sd is None:
            return
        if sd["state"] == "parked":
            with self._torch.cuda.stream(self._side_stream):
                t = time.perf_counter()
                self.session.side_run(sd["h"])
                self._gpu_wait_s += time.perf_counter() - t
            sd["state"] = "running"
            return
        t = time.perf_counter()
        self.session.side_start(sd["h"], stop_on_eos=True)
        self._gpu_wait_s += time.perf_counter() - t
        self._side = None
        self._enter(sd["reqs"])

    def _enter(self, new: List[_Request]) -> None:
        """Requests whose slots have just been armed: the streams' codec session, first / last tick, into the active set.  (A
        slot's codec stream restarts in ``_launch_stream_codec``, right before the pass of the request's first tick.)"""
        if self._stream_codec is None and any(r.stream for r in new):
            from ..mimi import MimiSession

            self._stream_codec = MimiSession(self.tts.codec, max_batch=self.B, max_chunk_frames=max(self.tick, 1), products=self.codec_products)
            self._stream_codec.reset()
        for r in new:
            r.first_tick = self._tick_no
            r.last_tick = self._tick_no + -(-(r.max_new_tokens + 1) // self.tick) - 1  # ceil(frames / tick) ticks from first_tick on
            self._active[r.slot] = r
        self._reset_fit(new)

    def _reset_fit(self, new: List[_Request]) -> None:
        """The causal fit of the slots that have just been armed, on the frame stream in front of their first tick (the slots'
        frame counters stand at 0 there): a stream with ``live_timestamps`` starts its own, any other tenant switches the slot
        off, so that nobody inherits a predecessor's state."""
        if self._fitter is None:
            return
        todo = [r for r in new if r.live_timestamps or r.slot in self._fit_on]
        if not todo:
            return
        for r in todo:
            (self._fit_on.add if r.live_timestamps else self._fit_on.discard)(r.slot)
        self._fitter.reset_slots([r.slot for r in todo], [len(r.align_ids) if r.live_timestamps else None for r in todo],
                                 [self.timestamp_lag_frames] * len(todo), [r.max_new_tokens + 1 for r in todo])

    def _convert(self, pcm, n_frames_d, done_d, reqs: List[_Request], tick_no: int):
        """The stream conversion of a codec pass (``route.StreamConverter``, current stream, right behind the decode): slot b of
        a request in ``reqs`` consumes the samples of the frames the tick's frame counter ``n_frames_d`` (device) gives it; every
        other slot none.  A slot with a speed ends its stream (flushes) in the tick where the host will see it finish, by the
        rule of ``_drain`` on the same snapshot (``n_frames_d``, ``done_d``).  Returns the ``route.StreamPass``, or None when the
        converter converts no slot of ``reqs`` (then nothing is uploaded or launched)."""
        conv, slots = self._stream_conv, [r.slot for r in reqs]
        if not any(conv.converts(b) for b in slots):
            return None
        from ..device import upload

        torch = self._torch
        f0 = np.zeros(self.B, np.int32)
        cap = np.zeros(self.B, np.int32)  # frames the request may have: 0 for slots without a live stream
        for r in reqs:
            f0[r.slot] = (tick_no - r.first_tick) * self.tick
            cap[r.slot] = r.max_new_tokens + 1
        f0_d, cap_d = upload([f0, cap], self.session.engine.device)
        n_d = n_frames_d.to(torch.int32)
        valid = ((torch.minimum(n_d, cap_d) - f0_d).clamp_(0, self.tick) * 1920).to(torch.int32)
        last = seg_end = None
        needs_last, segmented = conv.ends(slots)
        if segmented:
            # a segmented stream: its segment ends where an utterance would; the stream ends with its final segment only
            fin = np.zeros(self.B, np.int32)
            for r in reqs:
                fin[r.slot] = r.seg is None or r.seg.final
            fin_d, = upload([fin], self.session.engine.device)
            ends = stream_ends(n_d, done_d, cap_d) & (cap_d > 0)
            seg_end, last = ends.to(torch.int32), (ends & (fin_d != 0)).to(torch.int32)
        elif needs_last:
            last = (stream_ends(n_d, done_d, cap_d) & (cap_d > 0)).to(torch.int32)
        return conv.run(pcm, self.tick * 1920, valid, last, slots=slots, seg_end=seg_end)

    def _admit(self) -> None:
        if self._side is not None and self._side["state"] == "running":
            self._side_advance()
        new: List[_Request] = []
        rows = 0  # prompt rows of the (first) prefill call of this admission; the session's workspace holds max_rows
        side = self.side_prefill and self._side is None and len(self._active) >= self.side_min_active
        if self._side is not None:
            return  # one refill at a time: the next arrivals wait for it (at most a tick)
        if self._held is not None or not self._pending.empty() or self._refills:
            # A request that ends by its frame budget ends in a tick known since its admission.  Once that tick is queued the
            # slot can take its next tenant straight away: the prefill is queued behind the tick, and the snapshots (device-side
            # copies queued behind their ticks) still show the old tenant's last frames when the host gets to them.
            for slot, r in list(self._active.items()):
                if r.last_tick < self._tick_no and not r.cancelled and r.seg is None:  # (a segmented one keeps its slot)
                    r.retired = True
                    self._retiring.append(r)
                    del self._active[slot]
                    self._free.append(slot)
        freed = [b for b in self._free if self._slot_sampling[b] != self._default_sampling]  # handed back: the default again
        while self._refills or (self._free and (self._held is not None or not self._pending.empty())):
            refill = bool(self._refills)  # a segmented request's next segment: its slot is its own, it goes first
            if refill:
                req = self._refills.pop(0)
            else:
                req, self._held = (self._held, None) if self._held is not None else (self._pending.get_nowait(), None)
            if req.cancelled:
                if refill:
                    self._free.append(req.slot)
                self._end(req)
                continue
            if req.prompt is None:
                try:
                    v, sg, enc = req.voice_entry, req.seg, self.tts.prompt_encoder
                    # the utterance's (segment's) length entry and cap: the request's own, within the bounds from its text
                    from ..config import length_bounds

                    if req.request_cap is None:
                        req.request_cap = req.max_new_tokens
                    ratios = (self.min_frames_per_byte, self.max_frames_per_byte)
                    req.slot_sampling, req.max_new_tokens = (sg.plan.length_bounds(sg.k, sg.sampling, req.request_cap, *ratios) if sg is not None
                                                             else length_bounds(req.text, req.sampling, req.request_cap, *ratios))
                    if sg is not None:  # segment k's chained prompt
                        from ..longform import voice_prefix

                        prefix = voice_prefix(enc, req.voice, v.grid if v is not None else self.tts.voices.get(req.voice))
                        prompt = sg.plan.prompt(sg.k, enc, prefix, sg.prev, req.max_new_tokens, self.session.max_seq)
                    else:
                        prompt = enc.build_prompt(req.text, req.voice, v.grid) if v is not None else self.tts._get_prompt(req.text, req.voice)
                    if req.opts.timestamps or req.live_timestamps:  # the text's positions in the slot: of the whole prompt, a voice's speaker turns included
                        from ..align import window_of

                        req.align_window = window_of(prompt[0], self.tts.tokenizer)
                        req.align_ids = np.asarray(prompt[0, req.align_window[0]:req.align_window[1]]).copy()
                        if req.live_timestamps:  # (a text its tokens do not spell is refused here, as a bad request)
                            from ..align import StreamAligner

                            req.aligner = StreamAligner(req.text, req.align_ids, self.tts.tokenizer, speed=req.opts.speed)
                    if v is not None:  # a registered voice: its speaker turns' KV rows are installed, its own turns prefilled at P
                        P = int(v.grid.shape[1])
                        req.prompt, req.pos0, req.prefix = prompt[:, P:], P, v.prefix
                    else:
                        req.prompt = prompt
                    if req.pos0 + req.prompt.shape[1] + req.max_new_tokens + 2 > self.session.max_seq:
                        raise ValueError(f"prompt ({req.pos0} + {req.prompt.shape[1]} positions) + max_new_tokens ({req.max_new_tokens}) "
                                         f"exceed max_seq_len ({self.session.max_seq})")
                    if min(req.prompt.shape[1], self.prefill_chunk or req.prompt.shape[1]) > self.session.max_rows:
                        raise ValueError("prompt exceeds the session's prefill workspace")
                except Exception as e:  # bad request: answer it, keep serving
                    if refill:
                        self._free.append(req.slot)
                    self._end(req, e)
                    continue
            need = req.prompt.shape[1] if side else min(req.prompt.shape[1], self.prefill_chunk or req.prompt.shape[1])
            if side and need > self.session.max_rows:
                side = False if not new else side  # a prompt too long for one side call goes in line, in chunks (alone)
                if new:
                    self._hold(req, refill)
                    break
                need = min(req.prompt.shape[1], self.prefill_chunk or req.prompt.shape[1])
            if new and rows + need > self.session.max_rows:  # no room in this call: first in line next time
                self._hold(req, refill)
                break
            rows += need
            if not refill:
                req.slot = self._free.pop(0)
            new.append(req)
        entries = {b: self._default_sampling for b in freed}
        entries.update({r.slot: r.slot_sampling for r in new})
        self._write_sampling(entries)  # on the frame stream, ahead of the park / prefill of the new tenants
        if self.alignment_heads:
            # ... and the slots' text windows: a new tenant's own (its rows start as "not measured"), off for a tenant without
            # the option and for a slot handed back, so that nobody inherits a predecessor's window
            wins = {b: None for b in self._free if b in self._slot_align}
            wins.update({r.slot: r.align_window for r in new})
            self._write_align(wins)
        if not new:
            return
        if side:
            try:
                # queued behind the ticks so far; the voices' prefix rows go in first, in one launch, then the park at P + T - 1
                h = self.session.side_park([r.prompt for r in new], [r.slot for r in new], pos0=[r.pos0 for r in new],
                                           prefixes=[r.prefix for r in new])
                self._counts["prefix_installs"] += sum(1 for r in new if r.prefix is not None)
            except Exception as e:
                for r in new:
                    self._end(r, e)
                raise
            self._side = {"h": h, "reqs": new, "state": "parked"}
            return
        try:
            self._prefill(new)
        except Exception as e:  # these requests are in nobody's books yet: answer them here, then let the worker fail
            for r in new:
                self._end(r, e)
            raise
        self._enter(new)

    def _ingest(self) -> None:
        """The text side of the incremental requests, once per turn of the loop: segments the clients' calls left move into the
        plans (nothing else changes a plan, so a tick's codec pass and its bookkeeping agree on which segment is final), a
        request with its first segment joins the queue, a parked one with a new segment goes back to the refills, and one whose
        text has ended while parked is flushed and closed.  Idle timeout and early flush are decided here too."""
        while not self._inc_new.empty():
            self._incs.append(self._inc_new.get_nowait())
        if not self._incs:
            return
        now = time.monotonic()
        for r in list(self._incs):
            inc, sg = r.inc, r.seg
            parked = r in self._parked
            if r.cancelled and not r.closed and (parked or inc.state == "waiting"):
                if parked:
                    self._free.append(r.slot)
                    self._parked.remove(r)
                self._end(r)
            if r.closed:
                self._incs.remove(r)
                continue
            try:
                with inc.lock:
                    if not inc.close_asked:
                        if parked and (self._draining or now - max(inc.last_input, inc.parked_at) >= inc.idle_timeout_s):
                            inc.inbox.extend(inc.splitter.close())  # a stalled client does not pin a slot
                            inc.close_asked = True
                            self._counts["idle_timeouts"] += not self._draining
                        elif inc.flush_after_s is not None and inc.splitter.pending and now - inc.last_input >= inc.flush_after_s:
                            inc.inbox.extend(inc.splitter.flush())
                    segs, inc.inbox, closing = inc.inbox, [], inc.close_asked
            except ValueError as e:  # (the remainder held a bad break tag)
                segs, closing = [], True
                inc.close_asked = True
                if inc.state == "waiting":
                    self._end(r, e)
                    self._incs.remove(r)
                    continue
            if segs:
                sg.plan.extend(segs)
            if closing:
                sg.plan.close()
            if inc.state == "waiting":
                if sg.plan.segs:
                    inc.state = "admitted"
                    self._pending.put(r)
                elif closing:
                    self._end(r, ValueError("the text has nothing to speak"))
                    self._incs.remove(r)
            elif parked and sg.k < len(sg.plan.segs):
                self._parked.remove(r)
                self._refills.append(r)
            elif parked and closing:
                self._parked.remove(r)
                self._flush_parked(r)

    def _flush_parked(self, r: _Request) -> None:
        """A parked stream ends: one pass of its stages behind the seam with no samples and the ``last`` marker (the stretcher's
        and the FLAC encoder's flush, the resampler's tail), on the codec stream behind the passes so far; its end marker
        follows that chunk and the slot is free (a next tenant's stages are reset behind this pass)."""
        from ..device import upload

        torch = self._torch
        n = self.tick * 1920
        with torch.cuda.stream(self._codec_stream):
            none, last = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32)
            last[r.slot] = 1
            none_d, last_d = upload([none, last], self.session.engine.device)
            pcm = torch.zeros(self.B, n, dtype=torch.float32, device="cuda")
            conv = self._stream_conv.run(pcm, n, none_d, last_d, slots=[r.slot], seg_end=none_d)
            ev = torch.cuda.Event()
            ev.record(self._codec_stream)
        self._deliveries.append(_Delivery(ev, pcm, [(r, r.slot, 0, True)], urgent=True, keep=(none_d, last_d), conv=conv))
        r.stream_done = True
        self._free.append(r.slot)

    def _hold(self, req: _Request, refill: bool) -> None:
        if refill:
            self._refills.insert(0, req)
        else:
            self._held = req

    def _next_segment(self, r: _Request, cols: np.ndarray) -> None:
        """Segment k has ended (seen in a snapshot): its codes become the next one's context and the slot, still the request's,
        waits in ``_refills`` for the next chained prompt -- or, where the next segment's text has not arrived yet (an
        incremental request), in ``_parked`` for that."""
        sg = r.seg
        sg.prev = (sg.plan.segs[sg.k].text, cols.T.copy())
        sg.k += 1
        sg.sampling, sg.cols = sg.plan.sampling(sg.k, r.sampling), []
        r.prompt, r.emitted = None, 0
        del self._active[r.slot]
        if sg.k < len(sg.plan.segs):
            self._refills.append(r)
        else:
            r.inc.parked_at = time.monotonic()
            self._parked.append(r)

    def _write_sampling(self, entries: Dict[int, object]) -> None:
        """Slot b samples with ``entries[b]`` from the next pick on the current stream on (only changed entries are uploaded)."""
        from ..generate import _apply_slot_sampling

        todo = sorted(b for b, e in entries.items() if self._slot_sampling.get(b) != e)
        if todo:
            _apply_slot_sampling(self.session, todo, [entries[b] for b in todo])
        for b in todo:
            self._slot_sampling[b] = entries[b]

    def _write_align(self, wins: Dict[int, object]) -> None:
        """Slot b measures over ``wins[b]`` = (t0, t1) from the next frame on the current stream on; None: its window is off (only
        windows that were on are switched off; a window that is switched on is always written: it resets the slot's rows)."""
        todo = sorted(b for b, w in wins.items() if w is not None or b in self._slot_align)
        if not todo:
            return
        w = [wins[b] if wins[b] is not None else (0, 0) for b in todo]
        self.session.set_slot_align(todo, [x[0] for x in w], [x[1] for x in w])
        for b in todo:
            if wins[b] is None:
                self._slot_align.pop(b, None)
            else:
                self._slot_align[b] = tuple(wins[b])

    def _prefill(self, new: List[_Request]) -> None:
        """In-line admission: the registered voices' prefixes are installed in one launch, then every prompt (a registered
        voice's: its own turns only) is prefilled from its pos0.  Frame 0 of the new slots comes out of the next tick's first
        frame (no separate tail for all slots)."""
        prompts, slots = [r.prompt for r in new], [r.slot for r in new]
        prefixes, pos0 = [r.prefix for r in new], [r.pos0 for r in new]
        if self.prefill_chunk:
            # long prompts (voice-clone speakers) enter in chunks; the slots already speaking get a tick in between
            def between():
                if self._active:
                    self._tick_and_snapshot()
                    self._consume_snapshots(keep=1)

            self.session.prefill_chunked(prompts, slots=slots, stop_on_eos=True, chunk=self.prefill_chunk, between=between,
                                         defer_frame0=True, pos0=pos0, prefixes=prefixes)
        else:
            if any(p is not None for p in prefixes):  # (install_prefix refuses an empty list)
                self.session.install_prefix([p for p in prefixes if p is not None], [r.slot for r in new if r.prefix is not None])
            self.session.prefill(prompts, slots=slots, stop_on_eos=True, defer_frame0=True, pos0=pos0)
        self._counts["prefix_installs"] += sum(1 for p in prefixes if p is not None)

    # ------------------------------------------------------------------ worker: voice registrations
    def _job_step(self) -> None:
        """One step of the registration in progress (or of the next one waiting): the encode, then one prefill chunk of the
        speaker grid per step; the worker runs a tick of the speaking slots between steps."""
        if self._job is None:
            if self._jobs.empty():
                return
            job = self._jobs.get_nowait()
            self._job = {"job": job, "steps": self._align_steps(job) if job.get("align") else self._voice_steps(job)}
        job = self._job["job"]
        try:
            next(self._job["steps"])
            return
        except StopIteration:
            pass
        except Exception as e:  # (ValueError: a voice this engine cannot serve; the caller answers it, the worker goes on)
            job["error"] = e
        self._job = None
        job["done"].set()

    def _voice_steps(self, job):
        from ..abi import SmolttsError

        grid = job["grid"]
        if grid is None:
            try:
                grid = self.tts.create_speaker(job["samples"], job["system_prompt"])
            except SmolttsError as e:  # the encoder refuses the audio (e.g. beyond its position limit): the client's input
                raise ValueError(f"cannot encode the samples: {e}") from e
            if job["voice_id"] is None:  # (encode_speaker)
                job["result"] = grid
                return
            yield
        grid = np.ascontiguousarray(np.asarray(grid, dtype=np.int32))
        H = self.session.H
        if grid.ndim != 2 or grid.shape[0] != H or grid.shape[1] < 1:
            raise ValueError(f"speaker grid must be ({H}, P>=1), got {grid.shape}")
        P = int(grid.shape[1])
        cfg = self.tts.config
        if grid[0].min() < 0 or grid[0].max() >= cfg.vocab_size or grid[1:].min() < 0 or grid[1:].max() >= cfg.codebook_size:
            raise ValueError("speaker grid ids out of range")
        T_min = int(self.tts.prompt_encoder.build_prompt("", job["voice_id"], grid).shape[1]) - P  # a request's own turns, empty text
        if P + T_min + self.settings.max_new_tokens + 2 > self.session.max_seq:
            raise ValueError(f"speaker prompt of P={P} positions leaves no room for a request: P + {T_min} (an empty request) + "
                             f"max_new_tokens {self.settings.max_new_tokens} + 2 > max_seq_len {self.session.max_seq}")
        chunk = self.prefill_chunk or 128
        self._scratch_session()
        # the speaker grid alone, as non-final chunks (what a direct chunked prefill of the voice's prompts writes into a slot)
        for a in range(0, P, chunk):
            self._scratch.prefill([grid[:, a: a + chunk]], [0], pos0=[a], final=False)
            if a + chunk < P:
                yield
        prefix = self._scratch.save_prefix(0, P)  # on the frame stream: every later install is queued behind it
        self._voices[job["voice_id"]] = _Voice(job["voice_id"], grid, prefix, job["name"])
        job["result"] = {"voice_id": job["voice_id"], "prompt_positions": P}

    def _scratch_session(self):
        """The one-slot session the voices' prefixes are computed and recordings are measured in (created on first use).  Where the
        scheduler has ``alignment_heads`` it holds a recording's frames and an alignment buffer of its own."""
        from ..lm import LMSession

        if self._scratch is None:
            self._scratch = LMSession(self.tts.lm, 1, max_seq=self.session.max_seq, max_rows=self.prefill_chunk or 128,
                                      max_frames=self.session.max_frames if self.alignment_heads else 1, kv_dtype=self.session.kv_dtype)
            if self.alignment_heads:
                self._scratch.set_align_heads(self.alignment_heads)
        return self._scratch

    def _align_steps(self, job):
        """A forced alignment, a step per loop turn: the encode, then one chunk of the recording's grid per step."""
        from ..abi import SmolttsError
        from ..align import recording, recording_grid

        tts = self.tts
        try:
            codes = tts.encode_audio(job["pcm"])[:, :job["frames"]]
        except SmolttsError as e:  # the encoder refuses the audio (e.g. beyond its position limit): the client's input
            raise ValueError(f"cannot encode the recording: {e}") from e
        yield
        rg = recording_grid(tts.prompt_encoder, tts.tokenizer, tts.token_config, job["text"], codes, job["voice"], job["speaker"])
        s = self._scratch_session()
        s.set_slot_align([0], [rg.window[0]], [rg.window[1]])
        steps = s.iter_measure_rows(rg.grid, 0, rg.frame_of_row, rg.targets, self.prefill_chunk or 128)
        while True:
            try:
                next(steps)
            except StopIteration as done:
                lp_dev = done.value
                break
            yield
        rows, lp = s.fetch_alignment(0, rg.n_frames), lp_dev.cpu().numpy()  # (waits for the frame stream: the tick in flight)
        s.set_slot_align([0], [0], [0])
        job["result"] = recording(job["text"], rg, rows, lp, tts.tokenizer)

    # ------------------------------------------------------------------ worker: ticks and snapshots
    def _tick_and_snapshot(self) -> None:
        """Queue one tick of frames and, behind it, a device-side copy of the output ring with an event: the host reads
        that copy later, while the following tick runs."""
        torch = self._torch
        s = self.session
        s.decode(self.tick)
        scoring = any(r.slot_sampling is not None and r.slot_sampling.scored for r in list(self._active.values()) + self._retiring)
        measuring = any(r.opts.timestamps for r in list(self._active.values()) + self._retiring)
        fit = None
        live = [r for r in list(self._active.values()) + self._retiring if r.live_timestamps]
        if live:
            # the causal fit of the streams that ask for timestamps: one launch behind the frames; the host gets the committed
            # counts and the starts (up to the longest live text), not the rows
            self._fitter.push(s.alignment, s.n_frames, s.done)
            fit = (self._fitter.committed.clone(), self._fitter.starts[:, :max(max(len(r.align_ids) for r in live), 1)].clone())
        snap = _Snapshot(s.codes.clone(), s.n_frames.clone(), s.done.clone(), torch.cuda.Event(), self._tick_no,
                         s.logprobs.clone() if scoring else None, s.alignment.clone() if measuring else None, fit)
        snap.event.record(torch.cuda.current_stream())
        self._snaps.append(snap)
        self._tick_no += 1

    def _consume_snapshots(self, keep: int) -> None:
        """Read all but the ``keep`` newest snapshots (keep=1 in the steady state: the newest belongs to the tick that has
        only just been queued; its predecessor finished before that tick could start)."""
        torch = self._torch
        while len(self._snaps) > keep:
            snap = self._snaps.pop(0)
            # the host waits for the snapshot, then copies on the copy stream: a device-side wait would park a blocked barrier
            # packet in a second hardware queue for the whole tick, and the frame graphs' dependent launches get slower for it
            self._wait_event(snap.event)
            stream_pass = self._launch_stream_codec(snap)
            with torch.cuda.stream(self._copy_stream):
                codes = snap.codes.to("cpu", non_blocking=True)
                n_frames = snap.n_frames.to("cpu", non_blocking=True)
                done = snap.done.to("cpu", non_blocking=True)
                scores = snap.logprobs.to("cpu", non_blocking=True) if snap.logprobs is not None else None
                rows = snap.alignment.to("cpu", non_blocking=True) if snap.alignment is not None else None
                fit = [t.to("cpu", non_blocking=True) for t in snap.fit] if snap.fit is not None else None
            self._sync_copies()
            self._drain(codes.numpy(), n_frames.numpy(), done.numpy(), snap.tick_no, stream_pass, None if scores is None else scores.numpy(),
                        None if rows is None else rows.numpy(), None if fit is None else [t.numpy() for t in fit])

    def _launch_stream_codec(self, snap: _Snapshot) -> Optional[_Delivery]:
        """The codec pass of the streaming requests for tick ``snap.tick_no``, on the codec stream, from the tick's snapshot of
        the output ring (the host has just seen that snapshot's event, so the next tick is running meanwhile).  Returns the pass
        as a delivery without items (``_drain`` adds them), or None when no stream was alive in that tick."""
        torch = self._torch
        tick_no = snap.tick_no
        alive = [r for r in self._retiring + list(self._active.values())
                 if r.stream and r.first_tick <= tick_no <= r.last_tick and not r.closed and not r.stream_done]
        if not alive or self._stream_codec is None:
            return None
        from ..device import upload

        with torch.cuda.stream(self._codec_stream):
            live = {r.slot for r in alive}
            cap = int(self.tts.codec.c_cfg.max_positions)
            new = [r for r in alive if r.first_tick == tick_no]  # new streams start at position 0 ...
            restart = [r.slot for r in new]
            # ... and the slots without a stream (blocking requests, idle), which decode garbage that nobody reads, before their
            # stream position would reach the codec's capacity
            restart += [b for b in range(self.B) if b not in live and (self._codec_age[b] + 2) * 2 * self.tick > cap]
            if restart:
                self._stream_codec.reset_slots(sorted(set(restart)))
                # (a segmented stream's later segments restart the codec only: its other stages run on)
                fresh = [r for r in new if r.seg is None or r.seg.k == 0]
                self._stream_conv.start([r.slot for r in fresh], [r.opts for r in fresh], [r.watermark for r in fresh])
                segd = [r for r in new if r.seg is not None]
                if segd:
                    pauses, flags, leads = zip(*(r.seg.plan.seam_args(r.seg.k) for r in segd))
                    self._stream_conv.start_segments([r.slot for r in segd], pauses, flags, leads)
                for b in restart:
                    self._codec_age[b] = 0
            for b in range(self.B):
                self._codec_age[b] += 1
            # the frames this tick gives slot b sit at ring positions [f0_b, f0_b + tick): f0_b follows from the tick count
            # alone while the request is alive (frames of a slot that has stopped are garbage here and never delivered)
            f0 = np.zeros(self.B, np.int64)
            for r in alive:
                f0[r.slot] = (tick_no - r.first_tick) * self.tick
            f0_d, = upload([f0], self.session.engine.device)
            idx = (f0_d[:, None] + torch.arange(self.tick, device="cuda")[None]).clamp_(max=self.max_frames - 1)
            nq = self.tts.config.num_codebooks
            chunk = snap.codes[torch.arange(self.B, device="cuda")[:, None], idx][:, :, -nq:].contiguous()
            pcm = torch.empty(self.B, self.tick * 1920, dtype=torch.float32, device="cuda")
            self._stream_codec.decode_chunk(chunk, 0, self.tick, pcm, code_offset=0)
            conv = self._convert(pcm, snap.n_frames, snap.done, alive, tick_no)
            ev = torch.cuda.Event()
            ev.record(self._codec_stream)
        return _Delivery(ev, pcm, [], keep=snap, conv=conv)  # (the snapshot's tensors: kept alive until the pass has run)

    def _wait_event(self, ev) -> None:
        t = time.perf_counter()
        ev.synchronize()
        self._gpu_wait_s += time.perf_counter() - t

    def _sync_copies(self) -> None:
        t = time.perf_counter()
        self._copy_stream.synchronize()
        self._gpu_wait_s += time.perf_counter() - t

    def _drain(self, codes, n_frames, done, tick_no: int, stream_pass: Optional[_Delivery], scores=None, align_rows=None, fit=None) -> None:
        from ..config import finish_reason, merge_finish_reasons
        from ..generate import semantic_columns

        parts = {}         # {slot: align.AlignmentPart}: the timestamps this tick committed
        stream_items = []  # the streams' share of this tick's codec pass: (request, pcm row, samples, last?) handed out by _deliver
        urgent = False     # a stream's first chunk is among them
        nq = self.tts.config.num_codebooks
        tc = self.tts.token_config

        def release(r):  # the request needs its slot no longer (a retired one has handed it over already)
            if r.retired:
                self._retiring.remove(r)
            else:
                del self._active[r.slot]
                self._free.append(r.slot)

        for r in self._retiring + list(self._active.values()):
            slot = r.slot
            if r.cancelled:  # the client is gone: free the slot now, whatever the snapshot shows
                release(r)
                r.pending = []
                self._end(r)
                continue
            if tick_no < r.first_tick:  # the snapshot predates this request: it shows the slot's previous tenant
                continue
            if r.retired and tick_no > r.last_tick:  # (cannot happen: a retired request ends with its last tick's snapshot)
                release(r)
                self._end(r, RuntimeError("scheduler lost the last frames of a request"))
                continue
            n = min(int(n_frames[slot]), r.max_new_tokens + 1)
            finished = bool(stream_ends(n_frames[slot], done[slot], r.max_new_tokens + 1))
            seg_more = r.seg is not None and not r.seg.final  # a segment follows this one
            if finished:  # why: from the last slow id the request was given
                r.reasons.append(finish_reason(codes[slot, :n, 0], tc.im_end_id))
                r.frame_counts.append(n)
                r.finish_reason = merge_finish_reasons(r.reasons)
            if r.stream:
                # streaming requests decode every frame (__init__.py:88-92); this tick's PCM of the slot starts at its frame
                # r.emitted (== f0 of the tick: one codec frame per LM frame)
                k = n - r.emitted
                if r.seg is not None and k > 0:  # the next segment's context: this one's semantic frames
                    r.seg.cols.append(semantic_columns(codes[slot, r.emitted:n], tc, nq))
                if r.live_timestamps and (k > 0 or finished):
                    part = self._timed_part(r, fit, n, finished)
                    if part is not None:
                        parts[slot] = part
                if k > 0 or finished:
                    assert k == 0 or (stream_pass is not None and r.emitted == (tick_no - r.first_tick) * self.tick), "stream bookkeeping out of step"
                    stream_items.append((r, slot, max(k, 0) * 1920, finished and not seg_more))
                    urgent = urgent or r.emitted == 0
                r.emitted = n
                if finished:
                    if r.seg is not None:
                        self._counts["segments"] += 1
                    if seg_more:
                        self._next_segment(r, np.concatenate(r.seg.cols) if r.seg.cols else np.zeros((0, nq), np.int32))
                        continue
                    r.stream_done = True
                    release(r)  # the end marker follows the last chunk, in _deliver
                continue
            # blocking requests keep only frames whose slow id is a semantic token (generate_blocking, lm/generate.py:196-207)
            cols = semantic_columns(codes[slot, r.emitted:n], tc, nq)
            if r.seg is None and r.slot_sampling is not None and r.slot_sampling.scored and n > r.emitted:
                if scores is None:
                    raise RuntimeError("scheduler lost the scores of a request")
                r.lp.append(scores[slot, r.emitted:n].copy())
            if r.opts.timestamps and n > r.emitted:
                if align_rows is None:
                    raise RuntimeError("scheduler lost the alignment rows of a request")
                r.al.append(align_rows[slot, r.emitted:n].copy())
            r.emitted = n
            r.audio_frames += int(cols.shape[0])
            if cols.shape[0]:
                r.pending.append(cols)
            if finished and r.seg is not None:  # a segment of a blocking segmented request: its own codec job
                self._counts["segments"] += 1
                seg_cols = np.concatenate(r.pending) if r.pending else np.zeros((0, nq), np.int32)
                part = _Request(r.text, r.voice, False, r.max_new_tokens, pending=[seg_cols], part_of=(r, r.seg.k), cancelled=r.cancelled)
                r.seg.parts.append(part)
                r.seg.pcm.append([])
                r.pending = []
                self._finished.append(part)
                if seg_more:
                    self._next_segment(r, seg_cols)
                else:
                    release(r)  # its end marker follows the joined audio (_part_done)
                continue
            if finished:
                release(r)
                if r.lp:
                    from ..config import mean_logprob

                    r.logprobs = np.concatenate(r.lp)
                    r.mean_logprob = mean_logprob(r.logprobs)
                if r.take_of is not None:
                    self._end(r)  # (reports to its parent: only the winner's codes see the codec)
                else:
                    self._finished.append(r)
        if stream_items:
            d = stream_pass or _Delivery(None, None, [])
            d.items, d.urgent, d.parts = stream_items, urgent, parts
            self._deliveries.append(d)

    def _timed_part(self, r: _Request, fit, n: int, finished: bool):
        """The characters of a stream with ``live_timestamps`` whose times its slot's fit has committed since the part before
        (None: none), from the snapshot's copy ``fit`` = (committed counts, starts); at the stream's end the rest, cut at the
        frames it delivers (nominal at a speed other than 1), and ``r.alignment``."""
        if fit is None:
            raise RuntimeError("scheduler lost the fitted starts of a request")
        counts, starts = fit
        c = int(counts[r.slot])
        if not finished:
            return r.aligner.update(starts[r.slot, :c])
        if c != r.aligner.n:
            raise RuntimeError(f"the fit of a finished stream holds {c} of {r.aligner.n} starts")
        part = r.aligner.finish(starts[r.slot, :c], r.aligner.duration(n))
        r.alignment = r.aligner.alignment()
        return part

    # ------------------------------------------------------------------ worker: codec passes and delivery
    def _codec_backlog(self) -> bool:
        return bool(self._finished) or any(j is not None for j in self._codec_jobs)

    def _decode_finished(self, force: bool) -> None:
        """Codec work of the blocking requests: a pool of CODEC_BATCH codec slots, each decoding one complete utterance
        CODEC_CHUNK frames per pass; a slot whose utterance is through takes the next one waiting (its stream restarts at
        position 0), so a pass stays as wide as the backlog allows instead of narrowing towards the longest utterance.  A pass
        is queued when the pool is full, when work has waited long enough — CODEC_WAIT frames of LM ticks while the LM batch is busy (wide
        passes cost half as much per frame as narrow ones), one tick otherwise — or when nothing else is going on; its PCM
        goes out chunk by chunk through _deliver."""
        from ..device import upload
        from ..mimi import MimiSession

        torch = self._torch
        jobs = self._codec_jobs
        for b, j in enumerate(jobs):  # clients that went away
            if j is not None and j.req.cancelled:
                self._end(j.req)
                jobs[b] = None
        nq = self.tts.config.num_codebooks
        while self._finished and None in jobs:
            r = self._finished.pop(0)
            if r.cancelled:
                self._end(r)
                continue
            cols = np.concatenate(r.pending) if r.pending else np.zeros((0, nq), np.int32)
            r.pending = []
            if cols.shape[0] == 0:  # nothing to decode (every frame was non-semantic): just close the response, in order
                self._deliveries.append(_Delivery(None, None, [(r, 0, 0, True)]))
                continue
            b = jobs.index(None)
            jobs[b] = _CodecJob(r, cols)
            self._codec_fresh.append(b)
        occupied = [b for b, j in enumerate(jobs) if j is not None]
        if not occupied:
            self._codec_wait = 0
            return
        self._codec_wait += 1
        busy = (not self._pending.empty()) or 4 * len(self._active) >= 3 * self.B
        if not (force or len(occupied) == len(jobs) or self._codec_wait >= (max(1, self.CODEC_WAIT // self.tick) if busy else 1)):
            return
        self._codec_wait = 0
        # these passes depend on nothing the frame graphs produce on the device (their codes come from the host): they run on
        # the codec stream, beside the ticks
        with torch.cuda.stream(self._codec_stream):
            self._decode_finished_pass(jobs, occupied, nq)

    def _decode_finished_pass(self, jobs, occupied, nq) -> None:
        from ..device import upload
        from ..mimi import MimiSession

        torch = self._torch
        if self._batch_codec is None:
            self._batch_codec = MimiSession(self.tts.codec, max_batch=self.CODEC_BATCH, max_chunk_frames=self.CODEC_CHUNK, products=self.codec_products)
            self._batch_codec.reset()
        sess = self._batch_codec
        m = occupied[-1] + 1  # the pass runs over slots 0..m-1; a hole among them decodes zeros that nobody reads
        n = [min(self.CODEC_CHUNK, jobs[b].cols.shape[0] - jobs[b].done) if jobs[b] is not None else 0 for b in range(m)]
        nmax = max(n)
        # restart the streams of new utterances, and of holes before their position would reach the codec's capacity
        cap = int(self.tts.codec.c_cfg.max_positions)
        restart = sorted(set(self._codec_fresh) | {b for b in range(m) if jobs[b] is None and (self._codec_slot_age[b] + 2) * 2 * self.CODEC_CHUNK > cap})
        if restart:
            sess.reset_slots(restart)
            for b in restart:
                self._codec_slot_age[b] = 0
        self._codec_fresh = []
        grid = np.zeros((m, nmax, nq), np.int32)
        for b in range(m):
            if n[b]:
                grid[b, : n[b]] = jobs[b].cols[jobs[b].done: jobs[b].done + n[b]]
        codes, = upload([grid], self.session.engine.device)
        pcm = torch.empty(m, nmax * 1920, dtype=torch.float32, device="cuda")
        sess.decode_chunk(codes, 0, nmax, pcm, code_offset=0)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        items = []
        for b in range(m):
            self._codec_slot_age[b] += 1
            if not n[b]:
                continue
            j = jobs[b]
            j.done += n[b]
            fin = j.done >= j.cols.shape[0]
            items.append((j.req, b, n[b] * 1920, fin))
            if fin:
                jobs[b] = None
        self._deliveries.append(_Delivery(ev, pcm, items))

    def _deliver(self, wait: bool) -> None:
        """Hand finished codec passes to their requests, in order; ``wait``: block on the oldest one.  Finished stretches of
        blocking utterances go out first (never waited for)."""
        torch = self._torch
        self._poll_stretches()
        while self._deliveries:
            d = self._deliveries[0]
            wait = wait or any(x.urgent for x in self._deliveries)  # a stream's first chunk is somewhere in the line: do not dawdle
            host = None
            if d.event is not None:
                if not (wait or d.event.query()):
                    return
                self._wait_event(d.event)
                with torch.cuda.stream(self._copy_stream):
                    host = d.pcm.to("cpu", non_blocking=True)
                if d.conv is not None:
                    d.conv.to_host(self._copy_stream)
                self._sync_copies()
                host = host.numpy()
            self._deliveries.pop(0)
            for r, b, n, fin in d.items:
                if r.part_of is not None:  # a segment of a blocking segmented request
                    if n and not r.cancelled:
                        parent, k = r.part_of
                        parent.seg.pcm[k].append(host[b, :n].copy())
                        self._counts["frames_delivered"] += n // 1920
                    if fin:
                        self._part_done(r)
                    continue
                if r.live_timestamps:
                    # a stream with timestamps: each chunk goes out with the part its tick committed (a part alone where the
                    # stages hold the tick's samples back)
                    part = d.parts.get(b) if d.parts else None
                    if d.conv is not None and d.conv.converts(b):
                        chunk = d.conv.chunk(b, fin)
                    else:
                        chunk = host[b, :n].copy() if n else np.zeros(0, np.float32)
                    if (len(chunk) or part is not None) and not r.cancelled:
                        r.out.put((chunk, part))
                        self._counts["frames_delivered"] += n // 1920
                elif r.stream and d.conv is not None and d.conv.converts(b):
                    chunk = d.conv.chunk(b, fin)  # (the tail goes out with the last chunk)
                    if chunk.size and not r.cancelled:
                        r.out.put(chunk)
                        self._counts["frames_delivered"] += n // 1920
                elif not r.stream and self._finisher.needed(r.opts, self._key(r)):
                    # a blocking utterance that stages.Finisher has work on: finished whole once its last pass is in
                    if n and not r.cancelled:
                        r.stretch_in.append(host[b, :n].copy())
                        self._counts["frames_delivered"] += n // 1920
                    if fin and r.stretch_in and not r.cancelled:
                        self._finish(r, [np.concatenate(r.stretch_in)])
                        continue
                elif n and not r.cancelled:
                    self._put(r, host[b, :n].copy())
                    self._counts["frames_delivered"] += n // 1920
                if fin:
                    self._end(r)
            wait = False

    def _part_done(self, part: _Request) -> None:
        """A segment's PCM of a blocking segmented request is complete; once all are, they are joined and finished (``_finish``)."""
        r = part.part_of[0]
        sg = r.seg
        sg.done += 1
        if r.cancelled:
            self._end(r)
            return
        if sg.done < len(sg.plan.segs):
            return
        pcms = [np.concatenate(p) if p else np.zeros(0, np.float32) for p in sg.pcm]
        sg.pcm = []
        self._finish(r, pcms, sg.plan)

    def _key(self, r: _Request):
        """The watermark key of a request's audio, or None: unmarked."""
        return self.watermark if r.watermark else None

    def _finish(self, r: _Request, segments: List[np.ndarray], plan=None) -> None:
        """A complete blocking utterance (``plan``: the segments of a segmented one) goes through ``stages.Finisher`` on the
        stretch stream, waited for here, and out.  One with a speed leaves the chain between ``head`` and ``tail`` for the
        batched stretch (``_poll_stretches``)."""
        with self._torch.cuda.stream(self._stretch_stream):
            pcm, r.trimmed_s, r.loudness_gain_db = self._finisher.head(segments, r.opts, plan)
            if r.opts.speed_q:
                r.stretch_in = [pcm]
                self._start_stretch(r)  # (its end marker follows the stretched audio, in _poll_stretches)
                return
            pcm, r.peak_reduction_db = self._finisher.tail(pcm, r.opts, self._key(r))
        r.stretch_in = []
        self._put(r, pcm)
        self._end(r)

    STRETCH_SLOTS, STRETCH_PIECE = 16, 65536  # blocking utterances stretched side by side, input samples per slot and call

    def _start_stretch(self, r: _Request) -> None:
        """A blocking utterance with a speed is complete: it joins the stretch queue (``_poll_stretches`` runs it)."""
        pcm = np.ascontiguousarray(np.concatenate(r.stretch_in), dtype=np.float32)
        r.stretch_in = []
        self._stretches.append(_StretchJob(r, pcm))

    def _poll_stretches(self) -> None:
        """One step of the blocking utterances' stretches, never waited for.  Up to STRETCH_SLOTS utterances are stretched side by
        side, one stretcher slot each, in calls of at most STRETCH_PIECE input samples per slot (a call at speed 0.25 is ~9 ms on
        the GPU), queued on the stretch stream with an event.  A step collects the previous call once its event has fired (the
        utterances that ended in it go out, each with its end marker) and queues the next one."""
        from ..stages import TimeStretcher

        torch = self._torch
        fl = self._stretch_flight
        if fl is not None:
            ev, out_h, cnt_h, keep, ran = fl
            if not ev.query():
                return
            out, cnt = out_h.numpy(), cnt_h.numpy()
            for job in ran:
                if cnt[job.slot]:
                    job.outs.append(out[job.slot, : int(cnt[job.slot])].copy())
            for job in [j for j in ran if j.state == "ending"]:
                r = job.req
                if not r.cancelled:
                    with torch.cuda.stream(self._stretch_stream):
                        pcm, r.peak_reduction_db = self._finisher.tail(np.concatenate(job.outs) if job.outs else np.zeros(0, np.float32),
                                                                       r.opts, self._key(r))
                    self._put(r, pcm)
                self._end(r)
                self._stretches.remove(job)
            self._stretch_flight = None
        for job in [j for j in self._stretches if j.req.cancelled and j.state == "waiting"]:  # (a running one finishes)
            self._end(job.req)
            self._stretches.remove(job)
        if not self._stretches:
            return
        S, P = self.STRETCH_SLOTS, self.STRETCH_PIECE
        dev = self.session.engine.device
        with torch.cuda.stream(self._stretch_stream):
            if self._block_ts is None:
                self._block_ts = TimeStretcher(dev, S)
            ts = self._block_ts
            used = {j.slot for j in self._stretches if j.state == "running"}
            fresh = []
            for job in self._stretches:
                if job.state == "waiting" and len(used) < S:
                    job.state, job.slot = "running", min(set(range(S)) - used)
                    used.add(job.slot)
                    fresh.append(job)
            if fresh:
                ts.reset_slots([j.slot for j in fresh], [j.req.opts.speed_q for j in fresh])
            running = [j for j in self._stretches if j.state == "running"]
            batch = max(j.slot for j in running) + 1
            n_in = min(P, max(j.pcm.size - j.pos for j in running))
            x_h = torch.zeros(batch, max(n_in, 1), dtype=torch.float32).pin_memory()
            ctl_h = torch.zeros(2, batch, dtype=torch.int32).pin_memory()  # valid, last
            xn, ctl = x_h.numpy(), ctl_h.numpy()
            ending = []
            for job in running:
                b, piece = job.slot, job.pcm[job.pos: job.pos + n_in]
                xn[b, : piece.size] = piece
                job.pos += piece.size
                ctl[0, b] = piece.size
                if job.pos >= job.pcm.size:
                    ctl[1, b] = 1
                    ending.append(job)
            x = x_h.to(dev, non_blocking=True)
            ctl_d = ctl_h.to(dev, non_blocking=True)
            out, cnt = ts.new_outputs(batch, n_in)
            ts.chunk(x, n_in, out, cnt, valid=ctl_d[0], last=ctl_d[1])
            out_h = torch.empty(out.shape, dtype=torch.float32).pin_memory()
            cnt_h = torch.empty(cnt.shape, dtype=torch.int32).pin_memory()
            out_h.copy_(out, non_blocking=True)
            cnt_h.copy_(cnt, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stretch_stream)
        self._stretch_flight = (ev, out_h, cnt_h, (x_h, ctl_h, x, ctl_d, out, cnt), running)
        for job in ending:
            job.state = "ending"  # (done once this call is collected; its slot is free for the next call)

    # ------------------------------------------------------------------ worker: main loop
    def _run(self) -> None:
        torch = self._torch
        try:
            # the ticks are a chain of ~200 dependent launches per frame: their queue goes first wherever the command processor
            # has a choice (the codec passes beside them are ~100 launches per pass; measured with a kernel trace of
            # tools/bench_scheduler.py: no LM kernel gets longer beside a codec pass, the chain only loses time BETWEEN its kernels)
            prio = int(__import__("os").environ.get("SMOLTTS_TICK_PRIORITY", "-1"))
            compute = torch.cuda.Stream(priority=prio)
            self._copy_stream = torch.cuda.Stream()
            self._codec_stream = torch.cuda.Stream()
            self._side_stream = torch.cuda.Stream()
            self._stretch_stream = torch.cuda.Stream()  # blocking utterances' stretches (_start_stretch)
            with torch.cuda.stream(compute):
                while not self._stop.is_set():
                    self._job_step()  # a voice registration: at most one prefill chunk between two ticks
                    self._ingest()
                    self._admit()
                    if not self._active:
                        if self._side is not None:  # (its slots are the only ones taken: nothing to run beside)
                            self._side_advance()
                            continue
                        if self._job is not None or not self._jobs.empty():
                            continue
                        self._consume_snapshots(keep=0)
                        self._decode_finished(force=True)
                        if self._deliveries or self._codec_backlog():
                            self._deliver(wait=not self._codec_backlog())  # keep the passes coming while there is codec work
                            continue
                        if self._refills:  # a segmented request's next segment: admitted at the top of the loop
                            continue
                        if self._stretches:  # only stretches in flight: look again shortly, or sooner for a new request
                            self._poll_stretches()
                            self._wake.wait(timeout=0.0005)
                            self._wake.clear()
                            continue
                        self._wake.wait(timeout=0.05)  # idle: sleep until submit() (or close) without touching the queue
                        self._wake.clear()
                        continue
                    self._tick_and_snapshot()          # tick k and its snapshot are queued ...
                    self._decode_finished(force=False)
                    self._deliver(wait=False)
                    # ... while the host looks at what tick k-1 produced: the codec pass of tick k-1 goes out now, beside tick
                    # k.  Reading tick k itself right away (keep=0) would leave the GPU idle until the next tick is queued --
                    # with an arrival every other tick that was ~10 % of the wall time -- and would not bring a first chunk
                    # any earlier: it needs tick k finished either way
                    self._consume_snapshots(keep=1)
                    if any(d.urgent for d in self._deliveries):
                        self._deliver(wait=False)  # a first chunk: wait for its pass (the running tick leaves the host slack)
                    if self._side is not None and self._side["state"] == "parked":
                        self._side_advance()  # the tick before the park has been seen to finish: the side call runs beside this one
            self._fail_all(RuntimeError("scheduler closed"))  # requests still in flight when close() was called
        except Exception as e:  # engine failure: fail every waiter loudly
            self._fail_all(e)

    def _put(self, r: _Request, pcm: np.ndarray) -> None:
        """A piece of a blocking utterance's final audio goes out."""
        r.out_samples += int(pcm.size)
        r.out.put(pcm)

    def _aligned(self, r: _Request) -> None:
        """``r.alignment`` of a request with timestamps that has ended well: its frames' rows fitted to its text (align.py); the
        audio frames are the ones whose slow id is semantic, the delivered duration is what went out."""
        from ..align import align

        rows = np.concatenate(r.al) if r.al else np.zeros((0, len(self.alignment_heads), 2), np.float32)
        F = min(rows.shape[0], r.audio_frames)
        r.alignment = align(r.text, r.align_ids, rows[:F, :, 0], rows[:F, :, 1], self.tts.tokenizer, speed=r.opts.speed,
                            duration_s=r.out_samples / 24000.0)

    def _end(self, r: _Request, e: Optional[Exception] = None) -> None:
        """Queue the end marker of a request (exactly once)."""
        if r.part_of is not None:  # a segment's codec job: the segmented request ends, not its part
            if r.cancelled or e is not None:
                self._end(r.part_of[0], e)
            return
        if r.take_of is not None:  # a take of a best_of request: the parent answers
            if not r.closed:
                r.closed = True
                self._take_ended(r, e)
            return
        if not r.closed:
            r.closed = True
            self._counts["failed" if e is not None else ("cancelled" if r.cancelled else "completed")] += 1
            if r.opts.timestamps and e is None and not r.cancelled and r.align_ids is not None:
                try:
                    self._aligned(r)
                except Exception as err:  # (the request fails; the worker goes on)
                    e = err
            r.out.put(e)

    def _take_ended(self, take: _Request, e: Optional[Exception]) -> None:
        """A take of a best_of request has ended (its frames are through, it failed, or it was cancelled).  A failure fails the
        parent and cancels the other takes; when the last take has ended, the winner (``config.rank_takes``) becomes the parent's
        codec job, and only it is decoded."""
        from ..config import rank_takes

        parent = take.take_of[0]
        if parent.closed:
            return
        if e is not None:
            for t in parent.take_reqs:
                t.cancelled = True
            self._end(parent, e)
            return
        if not all(t.closed for t in parent.take_reqs):
            return
        if parent.cancelled or any(t.cancelled for t in parent.take_reqs):
            parent.cancelled = True
            self._end(parent)
            return
        ts = parent.take_reqs
        order = rank_takes([(t.finish_reason, t.mean_logprob) for t in ts])
        win = ts[order[0]]
        parent.takes = [{"seed": t.sampling.seed, "mean_logprob": t.mean_logprob, "min_logprob": float(t.logprobs.min()), "frames": int(len(t.logprobs)),
                         "finish_reason": t.finish_reason, "chosen": t is win} for t in ts]
        parent.sampling, parent.logprobs, parent.mean_logprob = win.sampling, win.logprobs, win.mean_logprob
        parent.finish_reason, parent.reasons, parent.frame_counts = win.finish_reason, list(win.reasons), list(win.frame_counts)
        parent.pending, parent.emitted = win.pending, win.emitted
        for t in ts:
            t.pending = []
        self._finished.append(parent)

    def stats(self) -> dict:
        """Counters since start (served by ``GET /v1/stats``): requests by outcome, audio frames handed to clients, ticks,
        slots in use, queue length."""
        up = time.time() - self._t0
        return dict(self._counts, ticks=self._tick_no, frames_per_tick=self.tick, slots=self.B, active=len(self._active), voices=len(self._voices),
                    queued=self._pending.qsize(), parked=len(self._parked), awaiting_codec=len(self._finished) + sum(1 for j in self._codec_jobs if j is not None), uptime_s=up, gpu_wait_s=self._gpu_wait_s,
                    delivered_frames_per_s=self._counts["frames_delivered"] / up if up > 0 else 0.0)

    def _fail_all(self, e: Exception) -> None:
        self._dead = e
        jobs = [self._job["job"]] if self._job is not None else []
        self._job = None
        while not self._jobs.empty():
            jobs.append(self._jobs.get_nowait())
        for job in jobs:
            job["error"] = RuntimeError(f"scheduler is not running: {e}")
            job["done"].set()
        if self._held is not None:
            self._end(self._held, e)
            self._held = None
        side = self._side["reqs"] if self._side is not None else []
        self._side = None
        while not self._inc_new.empty():
            self._incs.append(self._inc_new.get_nowait())
        for r in (list(self._active.values()) + side + self._retiring + self._refills + self._parked + self._incs + self._finished +
                  [j.req for j in self._codec_jobs if j is not None]):
            self._end(r, e)
        self._codec_jobs = [None] * len(self._codec_jobs)
        for d in self._deliveries:
            for r, _, _, _ in d.items:
                self._end(r, e)
        self._active.clear()
        self._retiring = []
        self._refills = []
        self._parked = []
        self._incs = []
        self._finished = []
        self._deliveries = []
        for job in self._stretches:
            self._end(job.req, e)
        self._stretches = []
        self._stretch_flight = None
        while not self._pending.empty():
            self._end(self._pending.get_nowait(), e)
