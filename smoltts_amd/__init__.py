"""smoltts_amd: MI355X-native DualAR + Mimi decode hot path.

``SmolTTS`` mirrors the reference façade mlx_inference/src/smoltts_mlx/__init__.py:25-151: same
constructor arguments, ``__call__(input, voice) -> float32 PCM`` and ``stream(input, voice)`` yielding
80 ms chunks (1920 samples at 24 kHz).  Everything heavy runs in ``libsmoltts_hip.so``.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Iterator, List, Optional

__version__ = "0.1.0"


class NoEncoderError(ValueError):
    """Voice cloning asked of a model whose Mimi checkpoint carries no encoder weights."""


class SmolTTS:
    def __init__(self, model_id: Optional[str] = None, checkpoint_dir: Optional[str] = None,
                 mimi_checkpoint: Optional[str] = None, numerics=None, state=None, config=None, mimi_state=None,
                 codec_window: int = 0, weight_format: str = "bf16", verbose: bool = False, watermark=None,
                 alignment_heads=None):
        """``checkpoint_dir``: config.json + tokenizer.json + model.safetensors | model.pth (reference
        layouts).  ``mimi_checkpoint``: the Hugging Face kyutai/mimi ``model.safetensors`` (or its
        directory).  ``state``/``config``/``mimi_state`` allow in-memory (e.g. synthetic) weights.
        ``model_id`` (Hugging Face download in the reference) needs network access and is refused.
        ``weight_format="fp8"`` stores the Linears as e4m3 with per-row scales (``packing.fp8_reference_state`` is the model
        then computed).  ``watermark`` (a ``watermark.Watermark``; None: none): everything ``__call__`` and ``stream`` return
        carries the key's mark, added on the GPU last of the float stages (watermark.py).
        ``alignment_heads`` (``[(layer, head), ...]``, at most 16; None: none): the heads of the slow attention that
        ``__call__(..., timestamps=True)`` reads character times from (align.py).  Which heads of a checkpoint track
        the text is the operator's to find: ``python -m smoltts_amd.align rank``."""
        import torch  # noqa: F401

        from .align import check_heads

        self.last_alignment = None  # align.Alignment of the last call that asked for timestamps

        from .watermark import Watermark

        if watermark is not None and not isinstance(watermark, Watermark):
            raise ValueError("watermark must be a smoltts_amd.watermark.Watermark or None")
        self.watermark = watermark

        from .checkpoint import load_checkpoint, load_mimi_state
        from .config import NumericsMode, TokenConfig
        from .lm import LMEngine
        from .mimi import MimiEngine
        from .prompt import PromptEncoder
        from .tokenizer import load_tokenizer

        if checkpoint_dir is None and state is None:
            raise ValueError("pass checkpoint_dir (or state+config); downloading model_id=%r needs network access" % (model_id,))
        if checkpoint_dir is not None:
            config, tokenizer, state = load_checkpoint(checkpoint_dir)
        else:
            tokenizer = load_tokenizer(None, config.codebook_size)
        if mimi_state is None:
            if mimi_checkpoint is None:
                raise ValueError("pass mimi_checkpoint (kyutai/mimi model.safetensors) or mimi_state")
            mimi_state = load_mimi_state(mimi_checkpoint)
        self.config = config
        self.alignment_heads = check_heads(alignment_heads, config)
        self.tokenizer = tokenizer
        self.token_config = TokenConfig.from_tokenizer(tokenizer, config)
        self.lm = LMEngine(config, state, self.token_config, numerics or NumericsMode.torch_reference(), weight_format=weight_format)
        self.prompt_encoder = PromptEncoder.from_config(tokenizer, config, self.token_config)
        self.codec = MimiEngine(mimi_state, num_codebooks=config.num_codebooks, window=codec_window, max_positions=2 * (1026 + 64))  # 1025 frames + a scheduler tick of overshoot, 2 positions per frame
        # the encode half (voice-clone prompts) is packed on first use, and only if the checkpoint carries it
        self._mimi_encoder_state = mimi_state if "encoder.layers.0.conv.weight" in mimi_state else None
        self._codec_window = codec_window
        self._encoder = None
        self.sampling_rate = 24_000
        self.voices: Dict[str, "np.ndarray"] = {}  # registered voice id -> speaker grid (add_voice)
        self.verbose = verbose  # print the reference's per-call timing lines (lm/generate.py:187-214)
        self.last_sampling = None  # resolved RequestSampling list of the last call that was given sampling= (seeds included)
        from .stages import Finisher

        self._finish = Finisher(self.lm.device)  # the blocking calls' chain behind the codec (its stages are made on first use)
        self.last_trimmed_s = 0.0  # seconds of silence the last blocking call trimmed (trim_silence / max_pause_s)
        self.last_segments: list = []  # per segment of the last segmented call: text, prompt, codes, seed, frames
        self.last_loudness_gain_db = None  # gain of the last call that was given loudness=
        self.last_peak_reduction_db = None  # -20 log10(min g) of the last call that was given peak_limit_db= (0.0: never limited)
        self.last_stats: dict = {}  # timing of the last generate_codes / __call__ (BatchGenerator.stats + codec_ms)
        # why the last call's utterance ended: "stop" (its last slow id is <|im_end|>) or "length" (the frame cap or a full
        # context); a segmented call is "length" if any segment was.  last_finish_reasons: one per input of generate_codes
        self.last_finish_reason: Optional[str] = None
        self.last_finish_reasons: List[str] = []
        # scores of the last call whose sampling= asked for them (RequestSampling.logprobs / best_of): the float32
        # log-probabilities of the (chosen) utterance's slow ids, their float64 mean, and per take of a best_of call its seed,
        # mean_logprob, min_logprob, frames, finish_reason, chosen and codes.  last_logprobs_all: one array per input of generate_codes
        self.last_logprobs = None
        self.last_mean_logprob: Optional[float] = None
        self.last_takes: Optional[list] = None
        self.last_logprobs_all: Optional[list] = None
        # bounds on an utterance's (a segment's) length from its text's UTF-8 byte count (config.length_bounds);
        # None: off.  12.5 frames are one second of audio: the ratios are the operator's to measure
        self.min_frames_per_byte: Optional[float] = None
        self.max_frames_per_byte: Optional[float] = None

    # -- prompt (``_get_prompt``, __init__.py:120-151)
    def _get_prompt(self, input: str, voice: str, sysprompt=None):
        """A registered voice id (``add_voice``) brings its speaker grid as the prompt's prefix; other names are presets, and
        unknown ones fall back to speaker 0 as in the reference."""
        if sysprompt is None and voice in self.voices:
            sysprompt = self.voices[voice]
        return self.prompt_encoder.build_prompt(input, voice, sysprompt)

    # -- registered (cloned) voices: a voice id names a speaker grid (``create_speaker``) wherever a voice is named
    def add_voice(self, voice_id: str, speaker_grid) -> None:
        """Register ``speaker_grid`` under ``voice_id``: ``tts(text, voice_id)`` and ``stream(text, voice_id)`` then condition
        on it, exactly as ``speaker=speaker_grid`` does.  The façade computes the whole prompt every call (the serving
        scheduler is the one that caches the speaker turns' KV rows)."""
        import numpy as np

        from .prompt import VOICE_MAP

        if not isinstance(voice_id, str) or not voice_id or voice_id in VOICE_MAP:
            raise ValueError(f"voice id {voice_id!r} is empty or names a preset voice")
        g = np.asarray(speaker_grid)
        if g.ndim != 2 or g.shape[0] != self.prompt_encoder.depth + 1 or g.shape[1] < 1:
            raise ValueError(f"speaker grid must be ({self.prompt_encoder.depth + 1}, T>=1), got {g.shape}")
        self.voices[voice_id] = np.ascontiguousarray(g.astype(np.int32))

    def remove_voice(self, voice_id: str) -> None:
        if voice_id not in self.voices:
            raise KeyError(voice_id)
        del self.voices[voice_id]

    def _settings(self, generation_settings):
        from .config import GenerationSettings

        # the reference façade always uses GenerationSettings() (temp 0.7 / 0.7, __init__.py:77,85)
        return generation_settings or GenerationSettings()

    def generate_codes(self, inputs: List[str], voices: Optional[List[str]] = None, generation_settings=None, speakers=None,
                       sampling=None, timestamps: bool = False):
        """Batched synthesis to audio-code grids: one (n_codebooks, F_b) uint32 array per input.
        ``sampling``: a ``config.RequestSampling`` for every input, or a list of one per input; missing fields come from the
        generation settings, and a sampled entry without a seed draws one (see ``last_sampling``).  The inputs then sample
        independently, each with the request key of its seed: the same seed gives the same codes whatever the
        other inputs are, as long as the batch selects the same kernel variants.  None: every input samples with the settings.
        ``timestamps`` (needs ``sampling`` and the instance's ``alignment_heads``): the frames also measure where those heads look
        over each input's own text; ``_align_rows`` then holds per input (rows [frames, heads, 2], text window, token row)."""
        voices = voices or ["heart"] * len(inputs)
        speakers = speakers or [None] * len(inputs)
        prompts = [self._get_prompt(t, v, sp) for t, v, sp in zip(inputs, voices, speakers)]
        return self.generate_prompt_codes(prompts, generation_settings, sampling, timestamps=timestamps)

    def generate_prompt_codes(self, prompts, generation_settings=None, sampling=None, timestamps: bool = False):
        """``generate_codes`` of ready prompt grids ((1 + depth, T) each: ``build_prompt``, ``longform.chain_prompt``)."""
        import numpy as np

        from .generate import BatchGenerator, resolve_sampling

        settings = self._settings(generation_settings)
        resolved = resolve_sampling(sampling, settings, len(prompts))
        self.last_sampling = resolved  # what the call sampled with, seeds included (None: the settings, session-wide)
        windows = None
        if timestamps:
            from .align import window_of

            if not self.alignment_heads or resolved is None:
                raise ValueError("timestamps need alignment_heads and per-input sampling entries")
            windows = [window_of(np.asarray(p)[0], self.tokenizer) for p in prompts]
        gen = BatchGenerator(self.lm, prompts, settings, frames_per_sync=16, sampling=resolved,
                             align=None if windows is None else (self.alignment_heads, windows))
        cols: List[list] = [[] for _ in prompts]
        for row in gen:
            for b, tok in enumerate(row):
                if tok is not None and tok.audio_codes is not None:
                    cols[b].append(tok.audio_codes[0, :, 0])
        self.last_stats = gen.stats()
        from .config import merge_finish_reasons

        self.last_finish_reasons = gen.finish_reasons()
        self.last_finish_reason = merge_finish_reasons(self.last_finish_reasons)
        # per input, the float32 scores of its frames (None where the input did not ask: RequestSampling.logprobs / best_of)
        scores = gen.logprobs() if resolved is not None and any(r.scored for r in resolved) else None
        self.last_logprobs_all = None if scores is None else [lp if r.scored else None for lp, r in zip(scores, resolved)]
        self._align_rows = None if windows is None else [(r, w, np.asarray(p)[0].copy()) for r, w, p in zip(gen.alignment(), windows, prompts)]
        gen.close()
        if self.verbose and self.last_stats:
            st = self.last_stats
            print(f"Prompt: {st['prompt_tokens']} tokens in {st['prefill_ms']:.1f} ms ({st['prefill_tokens_per_s']:.0f} tokens/s)")
            print(f"Generated {st['frames']} frames: {st['frames_per_s']:.1f} frames/s, {st['ms_per_frame_step']:.3f} ms/frame-step, "
                  f"{st['realtime_x']:.1f}x realtime")
        nq = self.config.num_codebooks
        return [np.stack(c, axis=1).astype(np.uint32) if c else np.zeros((nq, 0), np.uint32) for c in cols]

    def decode_codes(self, codes) -> "np.ndarray":
        """(n_codebooks, F) -> float32 PCM (1920 F,)  == codec.decode(gen) of the reference."""
        import numpy as np
        import torch

        from .mimi import MimiSession

        F_ = int(codes.shape[1])
        if F_ == 0:
            return np.zeros(0, np.float32)
        import time

        t0 = time.perf_counter()
        sess = MimiSession(self.codec, max_batch=1, max_chunk_frames=min(16, F_))
        dev = torch.from_numpy(np.ascontiguousarray(codes.T.astype(np.int32)))[None].cuda()
        pcm = sess.decode(dev).cpu().numpy().reshape(-1)
        sess.close()
        self.last_stats = dict(self.last_stats, codec_ms=(time.perf_counter() - t0) * 1e3, codec_frames=F_)
        if self.verbose:
            print(f"Decoded {F_} frames to PCM in {self.last_stats['codec_ms']:.1f} ms")
        return pcm

    def __call__(self, input: str, voice: Optional[str] = "heart", speaker=None, generation_settings=None, sampling=None,
                 **options):
        """Returns flattened float32 PCM (reference __call__, __init__.py:64-81).  ``sampling``: a ``config.RequestSampling``
        (per-request temperature / min_p / seed, as in ``generate_codes``).  ``options``: the blocking request's audio options,
        handed whole to ``request.parse_request``, which lists them with their ranges and refuses a bad one before any work
        (``ValueError``; ``TypeError`` for a name it does not know).  Here every stage takes the utterance whole on the GPU,
        in the order and by the rules of ``stages.Finisher``:
        ``trim_silence`` / ``max_pause_s`` / ``silence_threshold_db`` (``trim.py``): ``last_trimmed_s`` is what was cut.
        ``segment``: the segments are spoken one after another, each decoded as its own utterance, and joined (``seam``); a
        text that is one segment without break tags takes the plain path.  ``last_segments`` then lists each segment's text,
        seed and codes.
        ``loudness``: the utterance's integrated loudness is measured and one gain brings it to the target, capped where its
        peak would pass -1 dBFS (``loudness.py``); ``last_loudness_gain_db`` is the gain applied.
        ``speed``: the time stretch, pitch kept (``tsm.py``): ``tsm.out_length(1920 F, speed_q)`` samples.
        ``watermark`` (None: marked when the instance has a ``watermark``; True without one: ``ValueError``): the utterance gets
        the instance's mark (``watermark.py``).
        ``timestamps`` (needs the instance's ``alignment_heads``; not with ``segment``, the trim options or ``best_of``):
        ``last_alignment`` becomes the ``align.Alignment`` of the audio returned -- per character of ``input`` its start and end in
        seconds, read from where the chosen heads of the slow attention look while each frame is produced.  The option changes no
        id: with ``sampling=`` (its seed) or greedy settings the audio is the one the call returns without it.  A call without
        ``sampling=`` whose settings sample runs in the per-request mode here (the measurement exists only there) and draws a
        request seed, so its audio is another draw than the session-wide one; ``last_sampling`` carries the seed that replays it.
        ``peak_limit_db``: the look-ahead peak limiter, last of all (``limiter.py``); ``last_peak_reduction_db`` is
        ``-20 log10`` of the smallest gain applied, 0.0 when nothing was limited.  With a ``loudness`` as well, the loudness gain
        is not capped by the peak: the limiter takes the peaks down instead."""
        from .request import parse_request

        req = parse_request(input, False, **options)  # a bad request is refused before any work
        self.last_alignment = None
        self.last_peak_reduction_db = None
        if req.timestamps:
            if not self.alignment_heads:
                raise ValueError("timestamps need alignment_heads: rank a checkpoint's heads with `python -m smoltts_amd.align rank`")
            if sampling is not None and getattr(sampling, "takes", 1) > 1:
                raise ValueError("timestamps cannot be combined with best_of")
        marked = self._marks(req.watermark)
        voice = voice if voice is not None else "heart"
        self.last_trimmed_s = 0.0
        self.last_finish_reason = None  # (known once the call is through)
        self.last_takes = self.last_logprobs = self.last_mean_logprob = None
        self._check_best_of(sampling, generation_settings, segmented=req.plan is not None)
        if req.plan is not None:
            pcms = self._call_segmented(req.plan, voice, speaker, generation_settings, sampling)
        else:
            if self._bounds_on or sampling is not None or req.timestamps:  # (the measurement exists in slot mode only)
                from .config import RequestSampling
                from .generate import resolve_sampling

                if sampling is None and req.timestamps:
                    sampling = RequestSampling()

                st = self._settings(generation_settings)
                generation_settings, one = self._bounded(input, st, resolve_sampling(sampling, st, 1))
                sampling = None if one is None else one[0]
            if sampling is not None and sampling.takes > 1:
                codes = self._best_of(input, voice, speaker, generation_settings, sampling)
            else:
                codes = self.generate_codes([input], [voice], generation_settings, speakers=None if speaker is None else [speaker],
                                            sampling=sampling, timestamps=req.timestamps)[0]
                if self.last_logprobs_all is not None and self.last_logprobs_all[0] is not None:
                    from .config import mean_logprob

                    self.last_logprobs = self.last_logprobs_all[0]
                    self.last_mean_logprob = mean_logprob(self.last_logprobs)
            pcms = [self.decode_codes(codes)]
        pcm, self.last_trimmed_s, gain, self.last_peak_reduction_db = self._finish(pcms, req, marked, req.plan)
        if req.loudness is not None:
            self.last_loudness_gain_db = gain
        if req.timestamps:
            from .align import align

            rows, (t0, t1), row0 = self._align_rows[0]
            F = int(codes.shape[1])  # audio frames: the <|im_end|> frame carries none
            self.last_alignment = align(input, row0[t0:t1], rows[:F, :, 0], rows[:F, :, 1], self.tokenizer, speed=req.speed,
                                        duration_s=pcm.size / self.sampling_rate)
        return pcm

    def _check_best_of(self, sampling, generation_settings, stream: bool = False, segmented: bool = False) -> None:
        """``config.check_best_of`` of a call's ``sampling=`` (one entry, or a list of one), before any work."""
        from .config import MAX_BEST_OF, RequestSampling, check_best_of

        items = list(sampling) if isinstance(sampling, (list, tuple)) else [sampling]
        if not any(isinstance(r, RequestSampling) and r.takes > 1 for r in items):
            return
        st = self._settings(generation_settings)
        for r in items:
            if r is not None:
                check_best_of(r.resolve(st, draw_seed=False), MAX_BEST_OF, stream=stream, segmented=segmented)

    def _best_of(self, text: str, voice: str, speaker, generation_settings, sampling):
        """The takes of a resolved ``best_of`` entry as one batch -> the winner's audio codes (``config.rank_takes``); only they
        go through the codec.  Sets ``last_takes``, ``last_logprobs``, ``last_mean_logprob``, and ``last_sampling`` to the
        winner's entry: a plain request with its seed gives the same audio."""
        from .config import mean_logprob, rank_takes, take_sampling

        n = sampling.takes
        entries = [take_sampling(sampling, k) for k in range(n)]
        codes = self.generate_codes([text] * n, [voice] * n, generation_settings, speakers=None if speaker is None else [speaker] * n,
                                    sampling=entries)
        scores, reasons = self.last_logprobs_all, self.last_finish_reasons
        means = [mean_logprob(lp) for lp in scores]
        order = rank_takes(list(zip(reasons, means)))
        win = order[0]
        self.last_takes = [{"seed": entries[k].seed, "mean_logprob": means[k], "min_logprob": float(scores[k].min()) if len(scores[k]) else float("-inf"),
                            "frames": int(len(scores[k])), "finish_reason": reasons[k], "chosen": k == win, "codes": codes[k]} for k in range(n)]
        self.last_logprobs, self.last_mean_logprob = scores[win], means[win]
        self.last_sampling = [self.last_sampling[win]]
        self.last_finish_reason = reasons[win]
        self.last_finish_reasons = [reasons[win]]
        return codes[win]

    @property
    def _bounds_on(self) -> bool:
        return self.min_frames_per_byte is not None or self.max_frames_per_byte is not None

    def _bounded(self, text: str, settings, resolved, plan=None, k: int = 0):
        """``settings`` and the resolved sampling list (or None) of the utterance that speaks ``text`` (segment ``k`` of ``plan``
        where one is given), under the instance's ``min_frames_per_byte`` / ``max_frames_per_byte``: the cap becomes the settings'
        ``max_new_tokens``, the minimum the entry's ``min_frames``.  A call without an entry (session-wide mode) gets the minimum
        in its settings and, the length control existing in slot mode only, the entry resolved from them."""
        if not self._bounds_on:
            return settings, resolved
        import dataclasses

        from .config import RequestSampling, length_bounds
        from .generate import resolve_sampling

        carrier = resolved[0] if resolved is not None else RequestSampling(min_frames=settings.min_frames)
        ratios = (self.min_frames_per_byte, self.max_frames_per_byte)
        bounded, cap = (plan.length_bounds(k, carrier, self._max_new(settings), *ratios) if plan is not None
                        else length_bounds(text, carrier, self._max_new(settings), *ratios))
        if resolved is None:
            settings = dataclasses.replace(settings, max_new_tokens=cap, min_frames=bounded.min_frames or 0)
            return settings, resolve_sampling(None, settings, 1)
        return dataclasses.replace(settings, max_new_tokens=cap), [bounded]

    def _stream_reason(self, sess) -> str:
        """``finish_reason`` of the utterance a stream's one-slot session has just spoken."""
        from .config import finish_reason

        codes, n_frames, _, _ = sess.fetch()
        return finish_reason(codes[0, :int(n_frames[0]), 0], self.token_config.im_end_id)

    def _marks(self, asked: Optional[bool]):
        """The ``watermark.Watermark`` of a request that asked ``asked`` (None: the instance's policy), or None: unmarked."""
        if asked and self.watermark is None:
            raise ValueError("watermark asked for, and the model has no watermark key")
        return self.watermark if asked is None or asked else None

    # -- voice-clone prompts (``create_speaker``, __init__.py:97-118)
    def encode_audio(self, audio) -> "np.ndarray":
        """24 kHz mono float PCM (any shape, flattened) -> (n_codebooks, F) uint32 Mimi codes (``codec.encode``)."""
        import numpy as np

        from .mimi import MimiEncoder

        if self._encoder is None:
            if self._mimi_encoder_state is None:
                raise NoEncoderError("the Mimi checkpoint has no encoder.* weights: voice-clone prompts need the full kyutai/mimi model")
            self._encoder = MimiEncoder(self._mimi_encoder_state, num_codebooks=8, window=self._codec_window)
            self._mimi_encoder_state = None
        pcm = np.asarray(audio, dtype=np.float32).reshape(-1)
        return self._encoder.encode(pcm).cpu().numpy().astype(np.uint32)

    def create_speaker(self, samples: List[dict], system_prompt: Optional[str] = None) -> "np.ndarray":
        """Speaker prompt grid from reference recordings: per sample the user turn with its transcript, then
        its Mimi codes closed by ``<|im_end|>\\n``; optionally a leading system turn.  Pass the result as
        ``speaker=`` to ``__call__``."""
        import numpy as np

        turns = []
        for sample in samples:
            if "audio" not in sample or "text" not in sample:
                raise ValueError(f"Sample must contain both 'text' and 'audio' but got {sample.keys()}")
            turns.append(self.prompt_encoder.encode_text_turn("user", sample["text"]))
            turns.append(self.prompt_encoder.encode_vq(self.encode_audio(sample["audio"])[:8, :].astype(np.int64)))
        if system_prompt is not None:
            turns = [self.prompt_encoder.encode_text_turn("system", system_prompt), *turns]
        return np.concatenate(turns, axis=1).astype(np.int32)

    # -- forced alignment (align.py)
    def recording_grid(self, audio, text: str, voice: str = "heart", speaker=None, rate: int = 24000, max_seq: Optional[int] = None,
                       max_frames: int = 1 << 30):
        """The ``align.RecordingGrid`` of a recording and its transcript, after every refusal of ``align_recording`` (``ValueError``):
        no ``alignment_heads``, an empty text, audio without a full frame, prompt plus frames beyond ``max_seq`` (default: the
        model's) or ``max_frames``."""
        import numpy as np

        from .align import check_recording_fits, no_heads_error, recording_grid
        from .server.voices import to_codec_rate

        if not self.alignment_heads:
            raise no_heads_error()
        if not isinstance(text, str) or not text.strip():
            raise ValueError("forced alignment needs a text")
        pcm = to_codec_rate(np.asarray(audio, dtype=np.float64).reshape(-1), int(rate))
        F = pcm.size // 1920
        if F < 1:
            raise ValueError("the audio holds no full frame (1920 samples at 24 kHz)")
        sysprompt = speaker if speaker is not None else self.voices.get(voice)
        a0 = int(self.prompt_encoder.build_prompt(text, voice, sysprompt).shape[1])
        check_recording_fits(a0, F, max_seq or self.config.max_seq_len, max_frames)  # (before the encoder runs)
        codes = self.encode_audio(pcm[: F * 1920])[:, :F]
        return recording_grid(self.prompt_encoder, self.tokenizer, self.token_config, text, codes, voice, sysprompt)

    def align_recording(self, audio, text: str, voice: str = "heart", speaker=None, rate: int = 24000):
        """Forced alignment: mono float PCM ``audio`` at ``rate`` Hz (resampled to 24 kHz as a voice sample is) and its transcript
        ``text`` -> ``align.RecordingAlignment``: per character and per word its start and end in seconds, and the model's own
        log-probability of the recording's slow tokens under the text (``loss``: a wrong transcript scores worse).  The recording's
        Mimi codes go through the slow transformer teacher-forced behind the prompt of ``text`` (``voice`` / ``speaker`` as in
        ``__call__``) and the instance's ``alignment_heads`` are read on every audio row.  ``ValueError`` without
        ``alignment_heads``, for an empty text, for audio shorter than one frame and for a recording that does not fit the
        model's context."""
        from .align import measure_recording, recording, recording_session

        rg = self.recording_grid(audio, text, voice, speaker, rate)
        sess = recording_session(self.lm, self.alignment_heads, rg.a0, rg.n_frames)
        try:
            rows, lp = measure_recording(sess, 0, rg)
        finally:
            sess.close()
        return recording(text, rg, rows, lp, self.tokenizer)

    def stream(self, input: str, voice: Optional[str] = "heart", generation_settings=None, overlap: bool = True,
               reference_upsample: bool = False, output_format: Optional[str] = None, sampling=None,
               **options) -> Iterator["np.ndarray"]:
        """Yields one 1920-sample float32 chunk per generated frame, including the terminating
        <|im_end|> frame (reference stream, __init__.py:83-95, decodes vq_tensor[:, 1:, :] of every
        frame).  The codec carries its streaming state, so the chunks concatenate to the batch decode.
        ``reference_upsample``: up-sample every frame on its own as the reference's ``decode_step`` does (codec/mimi.py:77:
        no tap overlap from the previous frame) -- the chunks then equal the reference's own ``stream`` and no longer its batch
        decode; a quirk kept switchable like ``NumericsMode``'s.
        ``overlap``: the codec step of frame f runs beside frame f + 1 on a second stream (``generate.stream_pcm``); the chunks
        are the same numbers either way.
        ``sampling``: a ``config.RequestSampling`` (as in ``generate_codes``); it is resolved when the generator starts.
        ``output_format`` and ``options``: the streaming request's audio options, handed whole to ``request.parse_request``,
        which lists them with their ranges.  Here every stage runs on the GPU chunk by chunk, right behind the frame's codec
        step (``generate.stream_pcm``):
        ``output_format``: the int16 / uint8 chunks concatenate over the utterance to ``scipy.signal.resample_poly`` of the
        float32 stream, quantised (formats.py).
        ``speed``: the stream is time-stretched in front of the conversion; each chunk holds the samples that became final with
        its frame (none for some frames: no chunk then).
        ``container``: the FLAC frames decode to exactly the stream's 16-bit samples (those of ``pcm_<rate>``, or the float32 of
        ``pcm_24000`` quantised as rint(clip(x, -1, 1) * 32767)); the stream header stands in front of the first chunk (flac.py).
        ``segment``: a long text streams segment after segment in slot 0, each one's codec output through the seam stage in
        front of the stream's other stages, which run on across the segments: one stream (one FLAC header).
        ``loudness``: the stream is levelled causally behind the seam and in front of the stretch, by a gain that moves towards
        the target at 5 dB/s at most, from ``loudness_start_gain_db``; every frame's samples still leave with the frame
        (``loudness.StreamState``).
        ``watermark`` (as in ``__call__``): the stream is marked last of the float stages but for the limiter, behind the stretch
        and in front of the conversion and the framing; a segmented stream keeps one mark grid across its seams.
        ``trim_silence`` / ``max_pause_s`` / ``silence_threshold_db``: the stream is trimmed first of its stages, segment by
        segment in front of the seam; a non-silent block leaves with the frame that completes it, silence is held back until
        it is known whether it is kept (``trim.TrimState``).
        ``peak_limit_db``: the stream is peak-limited last of the float stages, behind the watermark and in front of the
        conversion and the framing; the limiter holds back 126 samples (5.25 ms), which leave with the stream's last chunk, and
        its state runs on across the seams of a segmented stream (``limiter.StreamState``).  A stream reports no reduction, and
        its loudness rule is the causal one, unchanged.
        ``input`` may be an iterator or generator of strings (or UTF-8 ``bytes``, cut anywhere) in place of a string: text that is
        still being written.  It implies ``segment=True`` (or the options given), is cut by ``longform.IncrementalSplitter``
        and spoken segment after segment while the text is pulled: before segment k starts, just enough text is pulled to have
        it whole and to know whether anything follows it, so the stream is that of the joined text with ``segment``.
        ``longform.FLUSH`` as an item speaks the buffered remainder without waiting for its sentence to end."""
        import numpy as np

        from .mimi import MimiSession
        from .generate import resolve_sampling, stream_pcm
        from .request import parse_request

        self.last_finish_reason = None  # (known once the stream has been consumed to its end)
        self.last_takes = self.last_logprobs = self.last_mean_logprob = None
        self._check_best_of(sampling, generation_settings, stream=True)
        if not isinstance(input, (str, bytes)):
            yield from self._stream_incremental(iter(input), voice if voice is not None else "0", generation_settings, overlap,
                                                reference_upsample, output_format, sampling, **options)
            return
        req = parse_request(input, stream=True, output_format=output_format, **options)
        marked = self._marks(req.watermark)
        voice = voice if voice is not None else "0"
        if req.plan is not None:
            yield from self._stream_segmented(req, voice, generation_settings, overlap, reference_upsample, sampling, marked=marked)
            return
        prompt = np.asarray(self._get_prompt(input, voice))
        if prompt.ndim == 3:
            prompt = prompt[0]
        settings = self._settings(generation_settings)
        settings, self.last_sampling = self._bounded(input if isinstance(input, str) else input.decode("utf-8", "replace"), settings,
                                                     resolve_sampling(sampling, settings, 1))
        sess = self._stream_session(prompt, settings, self.last_sampling)
        msess = MimiSession(self.codec, max_batch=1, max_chunk_frames=1, stateless_upsample=reference_upsample)
        try:
            yield from stream_pcm(sess, msess, prompt, stop_on_eos=True, overlap=overlap, options=req, watermark=marked)
            self.last_finish_reason = self._stream_reason(sess)
            if self.last_sampling is not None and self.last_sampling[0].scored:
                from .config import mean_logprob

                _, n_frames, _, _ = sess.fetch()
                self.last_logprobs = sess.fetch_logprobs()[0, :int(n_frames[0])].copy()
                self.last_mean_logprob = mean_logprob(self.last_logprobs)
        finally:
            msess.close()
            sess.close()

    def stream_with_timestamps(self, input: str, voice: Optional[str] = "heart", generation_settings=None, overlap: bool = True,
                               output_format: Optional[str] = None, sampling=None, timestamp_lag_frames: int = 6, **options):
        """``stream`` of one utterance with character timestamps as it goes: yields ``(chunk, part)`` -- the
        chunks of ``stream`` and, with the chunk whose frame committed them, the ``align.AlignmentPart`` of the characters whose
        end became known (None: none; a part that comes without samples has an empty chunk).  A character's time follows its
        audio by ``timestamp_lag_frames`` (1 .. 64) frames and is never revised; the parts concatenate to ``last_alignment``.
        Needs the instance's ``alignment_heads``; ``ValueError`` with ``segment``, the trim options, ``best_of`` or
        ``timestamps``.  The audio is ``stream``'s with the same ``sampling``; a call without ``sampling=`` runs in the
        per-request mode, as ``__call__`` with ``timestamps`` does."""
        import numpy as np

        from .align import StreamAligner, check_lag, check_live_timestamps, window_of
        from .config import RequestSampling
        from .generate import LiveTimestamps, resolve_sampling, stream_pcm
        from .mimi import MimiSession
        from .request import parse_request

        if not isinstance(input, str):
            raise ValueError("stream_with_timestamps takes the text whole")
        req = parse_request(input, stream=True, output_format=output_format, **options)
        check_live_timestamps(req, True, bool(self.alignment_heads), getattr(sampling, "takes", 1) if sampling is not None else 1)
        lag = check_lag(timestamp_lag_frames)
        self._check_best_of(sampling, generation_settings, stream=True)
        marked = self._marks(req.watermark)
        voice = voice if voice is not None else "0"
        self.last_alignment = None
        self.last_finish_reason = None
        prompt = np.asarray(self._get_prompt(input, voice))
        if prompt.ndim == 3:
            prompt = prompt[0]
        settings = self._settings(generation_settings)
        settings, self.last_sampling = self._bounded(input, settings, resolve_sampling(sampling if sampling is not None else RequestSampling(),
                                                                                      settings, 1))
        t0, t1 = window_of(prompt[0], self.tokenizer)
        aligner = StreamAligner(input, prompt[0, t0:t1], self.tokenizer, speed=req.speed)
        sess = self._stream_session(prompt, settings, self.last_sampling)
        msess = live = None
        try:
            sess.set_align_heads(self.alignment_heads)
            sess.set_slot_align([0], [t0], [t1])
            live = LiveTimestamps(sess, aligner, lag)
            msess = MimiSession(self.codec, max_batch=1, max_chunk_frames=1)
            yield from stream_pcm(sess, msess, prompt, stop_on_eos=True, overlap=overlap, options=req, watermark=marked, live=live)
            self.last_finish_reason = self._stream_reason(sess)
            self.last_alignment = aligner.alignment()
        finally:
            if msess is not None:
                msess.close()
            if live is not None:
                live.close()
            sess.close()

    def _max_new(self, settings) -> int:
        return settings.max_new_tokens if settings.max_new_tokens is not None else self.config.max_seq_len

    def _stream_session(self, prompt, settings, sampling):
        """The one-slot ``LMSession`` a stream of ``prompt`` runs in, sampling with ``settings``, or slot 0 with the resolved
        ``sampling`` list when there is one."""
        from .lm import LMSession
        from .generate import _apply_sampling, _apply_slot_sampling

        max_new, T = self._max_new(settings), int(prompt.shape[1])
        sess = LMSession(self.lm, 1, max_seq=min(self.config.max_seq_len, T + max_new + 2), max_rows=T, max_frames=max_new + 1)
        _apply_sampling(sess, settings)
        if sampling is not None:
            _apply_slot_sampling(sess, [0], sampling)
        return sess

    # -- long texts as chained segments (``longform``, ``seam``)
    def _segments(self, plan, voice: str, speaker, generation_settings, sampling):
        """Segment after segment of ``plan``: (k, its ``last_segments`` entry with its prompt, its settings, its sampling list or
        None).  The caller stores the segment's ``"codes"`` in the entry before it asks for the next one, which they condition."""
        import dataclasses
        import os

        from .generate import resolve_sampling
        from .longform import voice_prefix

        settings = self._settings(generation_settings)
        prefix = voice_prefix(self.prompt_encoder, voice, speaker if speaker is not None else self.voices.get(voice))
        resolved = resolve_sampling(sampling, settings, 1)
        self.last_sampling = resolved
        # segment k samples with segment_seed(seed, k): the request's seed, or the settings' (drawn here when they have none)
        if resolved is not None:
            base = resolved[0]
        else:
            base = settings if settings.seed is not None else dataclasses.replace(settings, seed=int.from_bytes(os.urandom(8), "little"))
        self.last_segments = info = []
        for k, seg in enumerate(plan.segs):
            prev = (info[-1]["text"], info[-1]["codes"]) if info else None
            samp = plan.sampling(k, base)
            # (every segment is an utterance of its own: its bounds come from its own text, its length entry is set anew)
            st_k, samp_k = (self._bounded(seg.text, settings, [samp], plan, k) if resolved is not None
                            else self._bounded(seg.text, samp, None, plan, k))
            info.append({"text": seg.text, "prompt": plan.prompt(k, self.prompt_encoder, prefix, prev, self._max_new(st_k),
                                                                 self.config.max_seq_len),
                         "codes": None, "seed": samp.seed, "frames": None})
            yield k, info[-1], st_k, samp_k
        self.last_sampling = resolved  # (generate_prompt_codes sets it per segment)

    def _call_segmented(self, plan, voice, speaker, generation_settings, sampling):
        """The PCM of ``plan``'s segments, each spoken and decoded as its own utterance."""
        from .config import merge_finish_reasons

        pcms, reasons = [], []
        for k, seg, st_k, samp_k in self._segments(plan, voice, speaker, generation_settings, sampling):
            seg["codes"] = self.generate_prompt_codes([seg["prompt"]], st_k, samp_k)[0]
            seg["frames"] = int(self.last_stats.get("frames", 0))  # every frame the segment emitted, its <|im_end|> frame included
            reasons.append(self.last_finish_reason)
            self.last_finish_reason = merge_finish_reasons(reasons)
            pcms.append(self.decode_codes(seg["codes"]))
        return pcms

    def _stream_incremental(self, texts, voice, generation_settings, overlap, reference_upsample, output_format, sampling,
                            segment=False, **options):
        """``stream`` of a text that ``texts`` yields in pieces: the segmented stream of a plan that grows as the text is pulled
        (``segment``: its options; it cannot be off)."""
        from .longform import FLUSH, GrowingPlan, IncrementalSplitter, segment_options
        from .request import parse_request

        req = parse_request("", stream=True, output_format=output_format, **options)
        marked = self._marks(req.watermark)
        opts = segment_options(segment or True)
        plan, splitter = GrowingPlan(opts), IncrementalSplitter(opts)

        def pull(k: int) -> bool:
            """Pull text until segment k is whole and it is known whether it is the last; False: there is no segment k."""
            while not plan.closed and (len(plan.segs) <= k or (len(plan.segs) == k + 1 and not splitter.pending)):
                try:
                    piece = next(texts)
                except StopIteration:
                    plan.extend(splitter.close())
                    plan.close()
                    break
                plan.extend(splitter.flush() if piece is FLUSH else splitter.feed(piece))
            return k < len(plan.segs)

        if not pull(0):
            raise ValueError("the text has nothing to speak")
        yield from self._stream_segmented(req, voice, generation_settings, overlap, reference_upsample, sampling, plan, pull, marked)

    def _stream_segmented(self, req, voice, generation_settings, overlap, reference_upsample, sampling, plan=None, pull=None, marked=None):
        """``plan`` / ``pull``: a ``longform.GrowingPlan`` in place of the request's, and what completes its segment k;
        ``marked``: the stream's ``watermark.Watermark`` or None."""
        import numpy as np
        import torch

        from .mimi import MimiSession
        from .route import StreamConverter
        from .generate import semantic_columns, stream_pcm

        from .config import merge_finish_reasons

        plan = plan if plan is not None else req.plan
        dev = self.lm.device
        reasons: list = []
        conv = StreamConverter(dev, 1, 1920, seam=True, watermark=marked)
        msess = MimiSession(self.codec, max_batch=1, max_chunk_frames=1, stateless_upsample=reference_upsample)
        try:
            conv.start([0], [req], [marked is not None])
            segments = self._segments(plan, voice, None, generation_settings, sampling)
            for k in range(1 << 30):
                if pull(k) if pull is not None else k < len(plan.segs):
                    _, seg, st_k, samp_k = next(segments)  # (it walks the plan's list, which has grown by now)
                else:
                    next(segments, None)  # (its epilogue)
                    break
                final = plan.final(k) if pull is not None else k == len(plan.segs) - 1
                sess = self._stream_session(seg["prompt"], st_k, samp_k)
                try:
                    pause, flags, lead = plan.seam_args(k)
                    conv.start_segments([0], [pause], [flags], [lead])
                    yield from stream_pcm(sess, msess, seg["prompt"], stop_on_eos=True, overlap=overlap, conv=conv, final=final)
                    codes_all, n_frames, _, _ = sess.fetch()
                    seg["frames"] = int(n_frames[0])
                    reasons.append(self._stream_reason(sess))
                    self.last_finish_reason = merge_finish_reasons(reasons)
                    seg["codes"] = semantic_columns(codes_all[0, :int(n_frames[0])], self.token_config,
                                                    self.config.num_codebooks).T.astype(np.uint32)
                finally:
                    sess.close()
        finally:
            torch.cuda.synchronize(dev)
            msess.close()
            conv.close()
