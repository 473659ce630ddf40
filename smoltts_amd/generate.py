"""Generation loop façade over the device-side frame loop.

Mirrors mlx_inference/src/smoltts_mlx/lm/generate.py: ``GenerationSettings`` (:12-16), ``VQToken``
(:19-22), ``SingleBatchGenerator`` (:25-171, an iterator of frames for one utterance) and
``generate_blocking`` (:174-216).  The reference runs one utterance and synchronises with the
device nine times per frame; here the frame loop (slow step, 8 depth steps, argmax, column feedback,
stop rule) runs on the GPU inside ``smoltts_lm_decode`` and the host only fetches finished columns.
``BatchGenerator`` is the same loop for B utterances at once.

Sampling follows the reference's rules (lm/generate.py:88-99,118-132): the slow token is greedy iff
``default_temp == 0``; the depth tokens are sampled iff ``default_fast_temp`` is set and > 0; ``min_p``
(lm/utils/samplers.py:8-34) follows ``GenerationSettings.min_p_mode``: "reference" (default) removes nothing, as the
reference's code does; "intended" keeps tokens with p >= min_p * p_max.  It runs on the device with a counter-based
generator keyed by ``GenerationSettings.seed`` (reproducible for a fixed seed; the reference's MLX
generator is not reproducible across processes, so parity for the sampled modes is statistical).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, Any, List, Optional, Sequence

import numpy as np
import torch

from .config import GenerationSettings, RequestSampling
from .lm import LMEngine, LMSession
from .request import SpeechOptions, parse_request
from .route import StreamConverter


@dataclass
class VQToken:
    semantic_code: int
    audio_codes: Optional[Any]  # (1, n_codebooks, 1) uint32 or None (non-semantic slow id)
    vq_tensor: Any              # (1, 1 + n_fast, 1) uint32


def _apply_sampling(session: LMSession, settings: GenerationSettings) -> None:
    fast = settings.default_fast_temp if settings.default_fast_temp is not None else 0.0
    seed = settings.seed
    if seed is None:
        import os

        seed = int.from_bytes(os.urandom(8), "little")
    session.set_sampling(temp=settings.default_temp, fast_temp=max(fast, 0.0), min_p=settings.effective_min_p, seed=seed)


def _apply_slot_sampling(session: LMSession, slots: Sequence[int], sampling: Sequence[RequestSampling]) -> None:
    """Slot ``slots[i]`` samples with the resolved ``sampling[i]`` (slot mode; a greedy entry's seed is 0)."""
    session.set_slot_sampling(list(slots), [r.temperature for r in sampling], [r.fast_temperature for r in sampling],
                              [r.min_p for r in sampling], [r.seed or 0 for r in sampling])
    # the slots' filter entries: uploaded where one is on, or where the slot's previous tenant left one on (cleared)
    slots, sampling = list(slots), list(sampling)
    todo = [i for i, (b, r) in enumerate(zip(slots, sampling)) if r.filters_on or b in session.filtered_slots]
    if todo:
        on = [sampling[i].filters_on for i in todo]
        session.set_slot_filters([slots[i] for i in todo], [sampling[i].top_p if o else 0.0 for i, o in zip(todo, on)],
                                 [sampling[i].top_k if o else 0 for i, o in zip(todo, on)],
                                 [sampling[i].repetition_penalty if o else 0.0 for i, o in zip(todo, on)],
                                 [sampling[i].repetition_window if o else 0 for i, o in zip(todo, on)])
    # ... and their length entries, by the same rule (a recycled slot must not inherit its predecessor's)
    todo = [i for i, (b, r) in enumerate(zip(slots, sampling)) if r.length_on or b in session.length_slots]
    if todo:
        session.set_slot_length([slots[i] for i in todo], [sampling[i].min_frames or 0 for i in todo],
                                [sampling[i].eos_bias or 0.0 for i in todo])
    # ... and their score flags (host flags: the session keeps scoring while any slot's is on)
    was = getattr(session, "scored_slots", ())
    todo = [i for i, (b, r) in enumerate(zip(slots, sampling)) if r.scored or b in was]
    if todo:
        session.set_slot_score([slots[i] for i in todo], [sampling[i].scored for i in todo])


def resolve_sampling(sampling, settings: GenerationSettings, n: int) -> Optional[List[RequestSampling]]:
    """``sampling=`` of the façade -> one resolved ``RequestSampling`` per utterance (None stays None: session-wide mode, unless
    the settings turn the length control on, which exists in slot mode only: every utterance then takes the settings whole)."""
    if sampling is None:
        if not (settings.min_frames or settings.eos_bias):
            return None
        sampling = RequestSampling(seed=settings.seed)
    items = list(sampling) if isinstance(sampling, (list, tuple)) else [sampling] * n
    if len(items) != n:
        raise ValueError(f"sampling: {len(items)} entries for {n} inputs")
    return [(r if r is not None else RequestSampling()).resolve(settings) for r in items]


def _frame_to_token(engine: LMEngine, col: np.ndarray) -> VQToken:
    """lm/generate.py:143-159: audio codes exist only when the slow id is a semantic token."""
    tc, cfg = engine.token_config, engine.cfg
    slow = int(col[0])
    vq = col.astype(np.uint32)[None, :, None]
    audio = None
    if tc.semantic_end_id is not None and tc.semantic_start_id <= slow <= tc.semantic_end_id:
        codes = col[1:] if cfg.duplicate_code_0 else np.concatenate([[slow - tc.semantic_start_id], col[1:]])
        audio = codes.astype(np.uint32)[None, :, None]
    return VQToken(semantic_code=slow, audio_codes=audio, vq_tensor=vq)


def semantic_columns(rows: np.ndarray, token_config, n_codebooks: int) -> np.ndarray:
    """Output-ring rows (F, 1 + n_fast) -> the audio codes (F', n_codebooks) int32 of the frames whose slow id is a semantic
    token, the frames ``generate_blocking`` keeps (lm/generate.py:196-207): the last ``n_codebooks`` ids of each."""
    slow = rows[:, 0]
    keep = (slow >= token_config.semantic_start_id) & (slow <= token_config.semantic_end_id)
    return rows[keep][:, -n_codebooks:].astype(np.int32)


class BatchGenerator:
    """Frames for B utterances; ``next()`` returns a list with one VQToken (or None once the
    utterance has stopped) per slot.  ``frames_per_sync`` > 1 lets the GPU run ahead."""

    def __init__(self, engine: LMEngine, prompts: Sequence[np.ndarray], generation_settings: GenerationSettings,
                 audio_only: bool = True, frames_per_sync: int = 1, session: Optional[LMSession] = None,
                 sampling: Optional[Sequence[RequestSampling]] = None, align: Optional[tuple] = None):
        """``sampling``: one resolved ``RequestSampling`` per prompt (``resolve_sampling``): the session runs in slot mode with
        them; None: every utterance samples with ``generation_settings`` (session-wide).
        ``align``: ``(pairs, windows)`` -- the (layer, head) pairs and per prompt its text window ``(t0, t1)`` or None: the frames
        measure where those heads look (``alignment()``; align.py).  Slot mode only: it needs ``sampling``."""
        self.engine = engine
        self.settings = generation_settings
        self.audio_only = audio_only
        self.B = len(prompts)
        max_new = generation_settings.max_new_tokens if generation_settings.max_new_tokens is not None else engine.cfg.max_seq_len
        self.max_frames = max_new + 1  # input_pos counts 0..max_new_tokens inclusive (generate.py:60,161)
        max_T = max(int(p.shape[1]) for p in prompts)
        self.session = session or LMSession(engine, self.B, max_seq=min(engine.cfg.max_seq_len, max_T + self.max_frames + 1),
                                            max_rows=sum(int(p.shape[1]) for p in prompts), max_frames=self.max_frames)
        _apply_sampling(self.session, generation_settings)
        if sampling is not None:
            if len(sampling) != self.B:
                raise ValueError(f"sampling: {len(sampling)} entries for {self.B} prompts")
            _apply_slot_sampling(self.session, range(self.B), sampling)
        if align is not None:
            if sampling is None:
                raise ValueError("align needs per-utterance sampling entries (slot mode)")
            pairs, windows = align
            if len(windows) != self.B:
                raise ValueError(f"align: {len(windows)} windows for {self.B} prompts")
            if self.session.align_pairs != sorted((int(l), int(h)) for l, h in pairs):
                self.session.set_align_heads(pairs)
            wins = [w if w is not None else (0, 0) for w in windows]
            self.session.set_slot_align(list(range(self.B)), [w[0] for w in wins], [w[1] for w in wins])
        self._prompts = list(prompts)
        self._started = False
        self._emitted = np.zeros(self.B, dtype=np.int64)
        self._per_sync = max(1, frames_per_sync)
        self._pending: List[List[Optional[VQToken]]] = []
        self.last_slow: List[Optional[int]] = [None] * self.B  # each utterance's last emitted slow id so far
        # wall-clock figures of the reference (prefill ms, frames/s, x realtime: lm/generate.py:187-214), from events on the
        # launch stream so that measuring does not add a synchronisation
        self._ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]  # before prefill, after it, after the last decode

    def __iter__(self):
        return self

    def _run(self) -> None:
        s = self.session
        if not self._started:
            self._ev[0].record()
            s.prefill(self._prompts, stop_on_eos=self.audio_only)
            self._ev[1].record()
            self._started = True
            if self._per_sync > 1:
                s.decode(self._per_sync - 1)
        else:
            s.decode(self._per_sync)
        self._ev[2].record()
        codes, n_frames, done, _ = s.fetch()
        top = int(n_frames.max())
        lo = int(self._emitted.min()) if (n_frames > self._emitted).any() else top
        for f in range(lo, top):
            row: List[Optional[VQToken]] = []
            any_new = False
            for b in range(self.B):
                if self._emitted[b] <= f < n_frames[b]:
                    row.append(_frame_to_token(self.engine, codes[b, f]))
                    any_new = True
                else:
                    row.append(None)
            if any_new:
                self._pending.append(row)
        self._emitted = np.maximum(self._emitted, n_frames)
        self._all_done = bool(done.all())
        self.last_slow = [int(codes[b, n_frames[b] - 1, 0]) if n_frames[b] > 0 else None for b in range(self.B)]

    def finish_reasons(self) -> List[str]:
        """Per utterance, why it ended (``config.finish_reason`` of its last emitted slow id), once the generator is through."""
        from .config import finish_reason

        im_end = self.engine.token_config.im_end_id
        return [finish_reason([] if s is None else [s], im_end) for s in self.last_slow]

    def logprobs(self) -> List[np.ndarray]:
        """Per utterance, the float32 scores of the frames it has emitted so far, its ``<|im_end|>`` frame included (meaningful
        where the utterance's entry asked for them: ``RequestSampling.scored``).  Call before ``close``."""
        lp = self.session.fetch_logprobs()
        return [lp[b, :int(self._emitted[b])].copy() for b in range(self.B)]

    def alignment(self) -> List[np.ndarray]:
        """Per utterance, the rows [frames emitted so far, pairs, 2] = (m, s1) of its frames (m = -1: not measured; frame 0 comes
        out of the prefill and is never measured here).  Needs ``align``.  Call before ``close``."""
        torch.cuda.current_stream().synchronize()
        rows = self.session.alignment.cpu().numpy()
        return [rows[b, :int(self._emitted[b])].copy() for b in range(self.B)]

    def __next__(self) -> List[Optional[VQToken]]:
        if not self._pending:
            if self._started and getattr(self, "_all_done", False):
                raise StopIteration
            self._run()
            if not self._pending:
                raise StopIteration
        return self._pending.pop(0)

    def stats(self) -> dict:
        """Prefill time (prompt -> frame 0) and decode rate of what has run so far; the rate is the reference's
        "x realtime": frames after the first / 12.5 / decode seconds, summed over the batch (prefill and codec excluded)."""
        if not self._started:
            return {}
        torch.cuda.current_stream().synchronize()
        prefill_ms = self._ev[0].elapsed_time(self._ev[1])
        decode_s = self._ev[1].elapsed_time(self._ev[2]) / 1e3
        frames = int(self._emitted.sum())
        after_first = max(frames - self.B, 0)
        rate = after_first / decode_s if decode_s > 0 and after_first else 0.0
        n_prompt = sum(int(p.shape[1]) for p in self._prompts)
        return {"utterances": self.B, "prompt_tokens": n_prompt, "prefill_ms": prefill_ms,
                "prefill_tokens_per_s": n_prompt / (prefill_ms / 1e3) if prefill_ms > 0 else 0.0, "frames": frames,
                "decode_s": decode_s, "frames_per_s": rate, "ms_per_frame_step": 1e3 * decode_s / max(after_first / self.B, 1e-9) if after_first else 0.0,
                "realtime_x": rate / 12.5}

    def close(self) -> None:
        self.session.close()


class SingleBatchGenerator:
    """One utterance, one frame per ``next()`` (reference class of the same name)."""

    def __init__(self, model: LMEngine, prompt: np.ndarray, generation_settings: GenerationSettings, audio_only: bool = True):
        prompt = np.asarray(prompt)
        if prompt.ndim == 3:
            prompt = prompt[0]
        self._inner = BatchGenerator(model, [prompt], generation_settings, audio_only=audio_only)

    def __iter__(self):
        return self

    def __next__(self) -> VQToken:
        return next(self._inner)[0]

    def close(self) -> None:
        self._inner.close()


def generate_blocking(model: LMEngine, prompt: np.ndarray, generation_settings: GenerationSettings, audio_only: bool = True) -> np.ndarray:
    """-> (1, n_codebooks, F) uint32 audio codes (frames whose slow id is not semantic are dropped,
    lm/generate.py:196-207), or the (1, 1+n_fast, F) columns when ``audio_only`` is False."""
    prompt = np.asarray(prompt)
    if prompt.ndim == 3:
        prompt = prompt[0]
    gen = BatchGenerator(model, [prompt], generation_settings, audio_only=audio_only, frames_per_sync=16)
    out = []
    for row in gen:
        tok = row[0]
        if tok is None:
            continue
        if audio_only:
            if tok.audio_codes is not None:
                out.append(tok.audio_codes)
        else:
            out.append(tok.vq_tensor)
    gen.close()
    if not out:
        return np.zeros((1, model.cfg.num_codebooks if audio_only else model.grid_height, 0), dtype=np.uint32)
    return np.concatenate(out, axis=-1)


class LiveTimestamps:
    """What ``stream_pcm`` needs to hand out character timestamps with its chunks: a one-slot ``AlignFitter``
    beside ``session`` (its alignment heads and slot 0's window are set) and the ``align.StreamAligner`` of the text."""

    def __init__(self, session: LMSession, aligner, lag: int):
        from .lm import AlignFitter

        self.aligner, self.lag, self.n = aligner, int(lag), int(aligner.n)
        self.fitter = AlignFitter.for_session(session)
        self.count = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.starts = torch.zeros(max(self.n, 1), dtype=torch.float64).pin_memory()

    def start(self, cap: int) -> None:
        """Current stream: slot 0 starts its fit; the stream ends at ``cap`` frames at the latest."""
        self.fitter.reset_slots([0], [self.n], [self.lag], [cap])

    def queue(self, session: LMSession, n_d, done_d) -> None:
        """Current stream: the frames up to the counter ``n_d`` are fitted, and the committed starts travel to the host."""
        self.fitter.push(session.alignment, n_d, done_d)
        self.count.copy_(self.fitter.committed, non_blocking=True)
        self.starts.copy_(self.fitter.starts[0, :self.starts.numel()], non_blocking=True)

    def part(self, n: int, last: bool):
        """Once the stream has been waited for: the ``align.AlignmentPart`` of this frame (None: none); ``last``: the stream ends
        here with ``n`` frames delivered."""
        c = int(self.count[0])
        starts = self.starts.numpy()[:c].copy()
        if not last:
            return self.aligner.update(starts)
        if c != self.n:
            raise RuntimeError(f"the fit of a finished stream holds {c} of {self.n} starts")
        return self.aligner.finish(starts, self.aligner.duration(n))

    def close(self) -> None:
        self.fitter.close()


def stream_pcm(session: LMSession, msession, prompt: np.ndarray, stop_on_eos: bool = True, max_frames: Optional[int] = None,
               overlap: bool = True, conv: Optional[StreamConverter] = None, final: bool = True,
               options: Optional[SpeechOptions] = None, watermark=None, live: Optional[LiveTimestamps] = None) -> Iterator[np.ndarray]:
    """One utterance in slot 0 of ``session`` -> one 1920-sample float32 chunk per generated frame, as the reference's
    ``SmolTTS.stream`` yields them (mlx_inference/src/smoltts_mlx/__init__.py:83-95: every frame of ``SingleBatchGenerator`` through
    ``codec.decode_step``), the terminating ``<|im_end|>`` frame included.

    At one utterance both halves of a frame are chains of dependent launches that leave the chip almost empty (188 LM launches,
    ~100 codec launches: DESIGN.md 5), so with ``overlap`` they run side by side: frame f + 1 is queued on the LM stream before
    the codec step of frame f goes out on a second stream -- the host has waited for frame f's event by then, it never parks a
    device-side wait in a queue.  Every chunk still leaves as soon as its own codec step has run; the numbers are those of the
    one-stream loop (``overlap=False``), only the order in which the GPU sees the launches changes.  A frame queued behind the
    last one is not a frame: a stopped slot is frozen (smoltts_lm_decode).

    ``options`` (a ``request.SpeechOptions``; None: a request without any): what the stream goes through behind its codec decode,
    on the codec stream right behind it (``StreamConverter.start``: the route is ``SlotRoute.of`` the options, and only the
    stages it names are made and launched).  Silence is trimmed first of all (the stream is one segment; a frame that
    completes no block that is kept yields nothing), then come the loudness stage, whose 1920 samples leave with their frame,
    and the stretch (a chunk holds the samples that became final with its frame; a frame that finalised none yields
    nothing).  The limiter, the last float stage, holds back 126 samples, which leave with the end of the stream.  An
    ``output_format`` makes every chunk int16 / uint8 samples -- the outputs that became final with it; the resampler's tail
    (<= 20 samples) follows the last chunk.  A frame the slot did not produce is not fed to the stages (its valid count is taken
    from the device's frame counter), so the tail is that of the last real frame.  A FLAC ``container`` frames the stream's
    16-bit samples behind the other stages: uint8 chunks, the stream header in front of the first.  Where a stage must see the
    end of the stream (``StreamConverter.ends``), it is derived on the device from the same snapshot of the frame counter and
    ``done`` that the host reads.

    ``watermark`` (a ``watermark.Watermark``; None: no launch): every frame's PCM gets the key's mark on the codec stream
    (``stages.Watermarker``), last of the float stages but for the limiter: behind the stretch, in front of the conversion and
    the framing.  Whether a request is marked is its front end's policy, so it is not read from ``options``.

    ``conv``: the utterance is one segment of a long text (``longform``): the caller's ``StreamConverter(seam=True)``, with the
    stream's stages started in slot 0 and this segment opened (``start_segments``), converts it and is not closed here;
    ``options`` and ``watermark`` are then ignored.  The end of the utterance, derived on the device, is the seam's end
    of segment, and the end of the stream only where ``final``; the resampler's tail follows the final segment only.

    ``live`` (a ``LiveTimestamps``; one utterance, no ``conv``): the generator yields ``(chunk, align.AlignmentPart or None)``
    instead of chunks: behind each frame's codec step the causal fit consumes the frames of the same counter snapshot the host
    reads, and the part holds the characters whose times that committed.  A part without samples comes with an empty chunk."""
    s = session
    limit = s.max_frames if max_frames is None else min(max_frames, s.max_frames)
    dev = s.engine.device
    lm_stream = torch.cuda.Stream(dev) if overlap else torch.cuda.current_stream(dev)
    codec_stream = torch.cuda.Stream(dev) if overlap else lm_stream
    caller = torch.cuda.current_stream(dev)
    lm_stream.wait_stream(caller)
    codec_stream.wait_stream(caller)
    pcm_dev = torch.empty(1, 1920, dtype=torch.float32, device=dev)
    pcm_host = torch.empty(1, 1920, dtype=torch.float32).pin_memory()
    state_host = torch.zeros(2, dtype=torch.int32).pin_memory()  # n_frames[0], done[0]
    own = conv is None
    if own:
        conv = StreamConverter(dev, 1, 1920, watermark=watermark)  # (its stages are made by start, as the stream needs them)
    with torch.cuda.stream(codec_stream):
        msession.reset()
        if own:
            conv.start([0], [options if options is not None else parse_request()], [watermark is not None])
        if live is not None:
            live.start(limit)
    converted = conv.converts(0)
    ends_on_device, segmented = conv.ends([0])  # a stage must see the end of the stream / of the segment
    with torch.cuda.stream(lm_stream):
        s.prefill([prompt], stop_on_eos=stop_on_eos)  # frame 0
        ev = torch.cuda.Event()
        ev.record(lm_stream)
    f = 0
    try:
        while f < limit:
            nxt = None
            if overlap and f + 1 < limit:
                with torch.cuda.stream(lm_stream):
                    s.decode(1)  # frame f + 1 runs beside the codec step of frame f
                    nxt = torch.cuda.Event()
                    nxt.record(lm_stream)
            ev.synchronize()  # frame f is in the output ring
            out = None
            with torch.cuda.stream(codec_stream):
                if not ends_on_device and live is None:
                    state_host[0:1].copy_(s.n_frames[0:1], non_blocking=True)
                    state_host[1:2].copy_(s.done[0:1], non_blocking=True)
                    n_d, done_d = s.n_frames[0:1], s.done[0:1]
                else:  # one device snapshot: the stretcher's `last` and the host's decision below come from the same values
                    snap = torch.cat([s.n_frames[0:1], s.done[0:1]])
                    state_host.copy_(snap, non_blocking=True)
                    n_d, done_d = snap[0:1], snap[1:2]
                msession.decode_chunk(s.codes[:, f:f + 1], 0, 1, pcm_dev, code_offset=1)  # (decode_chunk writes frame f0 at pcm[:, 1920 f0:])
                if converted:
                    valid = (n_d > f).to(torch.int32) * 1920  # 0 once the slot has stopped: garbage is not consumed
                    # the stream ends with this frame (done at it, or the frame limit), or had ended before it unseen by the host
                    last = None if not ends_on_device else ((n_d <= f) | ((done_d != 0) & (n_d == f + 1)) | (f + 1 >= limit)).to(torch.int32)
                    seg_end = None
                    if segmented:  # a segment: it ends where an utterance would; the stream only with the final one
                        seg_end, last = last, (last if final else None)
                    out = conv.run(pcm_dev, 1920, valid, last, seg_end=seg_end)
                    out.to_host(codec_stream)
                else:
                    pcm_host.copy_(pcm_dev, non_blocking=True)
                if live is not None:
                    live.queue(s, n_d, done_d)
            codec_stream.synchronize()
            n, done = int(state_host[0]), int(state_host[1])
            part = None
            if live is not None:  # (the stream ends with this frame by the rule of the three exits below)
                part = live.part(min(n, limit), n <= f or bool(done and n == f + 1) or f + 1 >= limit)
            if out is not None:
                # (a call after the slot stopped consumed nothing: its tail is that of the last frame)
                chunk = out.chunk(0, last=final and (n <= f or bool(done and n == f + 1) or f + 1 >= limit))
                # (a stretched frame that finalised no sample yields nothing, nor does a float stage fed no sample)
                if live is not None:
                    if chunk.size or part is not None:
                        yield chunk, part
                elif chunk.size or (not ends_on_device and chunk.dtype != np.float32):
                    yield chunk
            elif live is not None and n <= f and part is not None:
                yield np.zeros(0, np.float32), part
            if n <= f:  # the slot had stopped before this frame
                break
            if out is None:
                yield pcm_host.numpy().reshape(-1).copy() if live is None else (pcm_host.numpy().reshape(-1).copy(), part)
            if done and n == f + 1:
                break
            if not overlap and f + 1 < limit:
                s.decode(1)
                nxt = torch.cuda.Event()
                nxt.record(lm_stream)
            if nxt is None:
                break
            ev = nxt
            f += 1
    finally:
        lm_stream.synchronize()
        codec_stream.synchronize()
        if own:
            conv.close()
