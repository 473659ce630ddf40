"""What a stream goes through behind its codec decode: the per-slot route, the plan of a pass over the live slots, and the
converter that runs the stages (stages.py) by that plan."""
from __future__ import annotations

from dataclasses import dataclass, replace
from functools import cached_property
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .abi import FLAC_F32, FLAC_OFF, FLAC_S16, SEAM_FINAL, SEAM_FIRST, SEAM_OFF
from .device import upload
from .formats import ENC_OFF, ENC_ULAW, check_container, parse_stream_format
from .request import SpeechOptions
from .seam import THRESH
from .stages import FlacEncoder, LoudnessNormalizer, PeakLimiter, Resampler, SeamJoiner, SilenceTrimmer, TimeStretcher, Watermarker  # noqa: F401  (STAGE_TABLE names them)
from .tsm import out_bound


class StageSpec(NamedTuple):
    """One stage of a pass, as the route, the plan and the converter know it."""
    name: str        # its name in a plan
    attr: str        # the converter attribute that holds its instance
    cls: str         # its class: looked up in this module when the stage is made
    fp32: bool       # fp32 in, fp32 out: the stages behind read its rows
    on: Callable     # (route) -> whether a slot with that route goes through it
    start: Callable  # (stage, slots, their new routes): start the new streams in it; a slot that does not use it is switched off
    args: Callable = lambda conv: ()  # (converter) -> what its constructor takes behind (device, max_batch)
    call: str = "chunk"               # the method a pass calls


# The stages of a pass in launch order, the one place that lists them: the watermark behind the stretch (a speed does not rescale
# the chips), the limiter the last float stage (nothing behind it can raise a peak again), then the conversion and the framing.
STAGE_TABLE = (
    StageSpec("trim", "tr", "SilenceTrimmer", True, lambda r: r.trims,  # (a plain stream is one segment, the first and the last)
              lambda st, slots, rs: st.start_segments(slots, [SEAM_FIRST | SEAM_FINAL if r.trims else SEAM_OFF for r in rs],
                                                      [r.trim for r in rs], [r.pause_blocks for r in rs], [r.thr for r in rs])),
    StageSpec("seam", "sj", "SeamJoiner", True, lambda r: r.segmented,  # (no new stream is segmented: ``start_segments`` makes it)
              lambda st, slots, rs: st.start_segments(slots, [0] * len(slots), [SEAM_OFF] * len(slots))),
    StageSpec("loudness", "ln", "LoudnessNormalizer", True, lambda r: r.loudness is not None,
              lambda st, slots, rs: st.reset_slots(slots, [r.loudness for r in rs], [r.start_gain_db for r in rs])),
    StageSpec("stretch", "ts", "TimeStretcher", True, lambda r: r.speed_q != 65536,
              lambda st, slots, rs: st.reset_slots(slots, [r.speed_q for r in rs])),
    StageSpec("watermark", "wm", "Watermarker", True, lambda r: r.watermark_gain > 0.0,
              lambda st, slots, rs: st.reset_slots(slots, [r.watermark_gain for r in rs]), lambda conv: (conv.watermark,)),
    StageSpec("limit", "lim", "PeakLimiter", True, lambda r: r.ceiling > 0.0,
              lambda st, slots, rs: st.reset_slots(slots, [r.ceiling for r in rs]), call="run"),  # (``run``: rows of any width)
    StageSpec("resample", "rs", "Resampler", False, lambda r: r.enc != ENC_OFF,
              lambda st, slots, rs: st.reset_slots(slots, [r.format for r in rs]), lambda conv: (out_bound(conv.n_in),)),
    StageSpec("flac", "fl", "FlacEncoder", False, lambda r: r.flac,
              lambda st, slots, rs: st.reset_slots(slots, [r.rate for r in rs], [
                  FLAC_OFF if not r.flac else (FLAC_F32 if r.enc == ENC_OFF else FLAC_S16) for r in rs])),
)
END_MARKERS = {s.name: globals()[s.cls].END_MARKERS for s in STAGE_TABLE}  # stage -> the end markers its class declares
LIMIT_ORDER = tuple(s.name for s in STAGE_TABLE)
LIMIT_FLOAT_STAGES = tuple(s.name for s in STAGE_TABLE if s.fp32)
# Historical names, kept for callers: the orders before the limiter, the trim, the watermark and the loudness stage came.
TRIM_ORDER, TRIM_FLOAT_STAGES = (tuple(s for s in o if s != "limit") for o in (LIMIT_ORDER, LIMIT_FLOAT_STAGES))
PASS_ORDER, FLOAT_STAGES = (tuple(s for s in o if s != "trim") for o in (TRIM_ORDER, TRIM_FLOAT_STAGES))
LAUNCH_ORDER = tuple(s for s in PASS_ORDER if s != "watermark")
STAGES = tuple(s for s in LAUNCH_ORDER if s != "loudness")


@dataclass(frozen=True)
class SlotRoute:
    """What a slot's stream goes through behind the codec (``StreamConverter``): its format (rate, SMOLTTS_RESAMPLE_*), its Q16
    speed, FLAC framing, whether it is segmented (``start_segments``), its stream generation in the slot and whether its FLAC
    stream header is still owed.  A restarted slot gets a new record: a pass keeps the records of its run."""
    rate: int = 24000
    enc: int = ENC_OFF
    speed_q: int = 65536
    flac: bool = False
    segmented: bool = False
    gen: int = 0
    head_owed: bool = False
    loudness: Optional[float] = None  # target in LUFS (None: the slot never enters the loudness stage)
    start_gain_db: float = 0.0        # its stream's first knot
    watermark_gain: float = 0.0       # 10^(strength_db / 20) (0: the slot never enters the watermark stage)
    ceiling: float = 0.0              # 10^(peak_limit_db / 20) (0: the slot never enters the limiter stage)
    trim: bool = False                # its leading and trailing silence is trimmed
    pause_blocks: int = 0             # its pauses are capped at this many blocks (0: not); neither: the slot never enters the trim stage
    thr: float = float(THRESH)        # the silence threshold of its trim stage

    @cached_property
    def stages(self) -> Tuple[str, ...]:
        """The stages the slot goes through, in launch order."""
        return tuple(s.name for s in STAGE_TABLE if s.on(self))

    @property
    def trims(self) -> bool:
        return self.trim or self.pause_blocks > 0

    @property
    def format(self) -> str:
        """The ``output_format`` of the route's rate and encoding (``pcm_24000``: not converted)."""
        return "ulaw_8000" if self.enc == ENC_ULAW else f"pcm_{self.rate}"

    @classmethod
    def of(cls, options: SpeechOptions, watermark_gain: float, gen: int) -> "SlotRoute":
        """The route of a new stream with a request's ``options``: the one place that maps an option to what a slot goes
        through.  ``watermark_gain``: the converter's key's gain for a marked stream, else 0; ``gen``: the stream's generation
        in its slot."""
        rate, enc = parse_stream_format(options.output_format or "pcm_24000")
        flac = options.container is not None
        return cls(rate, enc, options.speed_q or 65536, flac, gen=gen, head_owed=flac, loudness=options.loudness,
                   start_gain_db=options.start_gain_db, watermark_gain=watermark_gain, ceiling=options.ceiling,
                   trim=options.trim_silence, pause_blocks=options.pause_blocks, thr=options.silence_thr)


class PassPlan(NamedTuple):
    stages: List[str]                 # the stages to launch, in order
    rows: Dict[str, List[int]]        # the live slots each of them serves
    through: Dict[str, List[int]]     # float stage (trim, seam, loudness, stretch, watermark, limit) -> the live slots it does not serve that a later stage does
    source: Dict[int, Optional[str]]  # live slot -> the last stage it goes through (None: its codec rows are its output)
    host: List[str]                   # the stages whose outputs are copied to the host: the sources of the live slots
    routes: Dict[int, SlotRoute]      # live slot -> its route when planned


def plan_pass(routes: Dict[int, SlotRoute]) -> PassPlan:
    """The plan of one converter pass over the live slots' routes (``{slot: SlotRoute}``, in slot order); no device involved."""
    rows = {s: [] for s in LIMIT_ORDER}
    through = {s: [] for s in LIMIT_FLOAT_STAGES}
    source = {}
    for b, r in routes.items():
        path = r.stages
        source[b] = path[-1] if path else None
        for s in path:
            rows[s].append(b)
        for s in through:
            if path and s not in path and LIMIT_ORDER.index(path[-1]) > LIMIT_ORDER.index(s):
                through[s].append(b)
    stages = [s for s in LIMIT_ORDER if rows[s]]
    return PassPlan(stages, {s: rows[s] for s in stages}, {s: through[s] for s in through if rows[s]}, source,
                    [s for s in stages if s in source.values()], routes)


class StreamConverter:
    """What a stream's PCM goes through behind its codec decode, per slot of ``max_batch``: the stages of ``STAGE_TABLE`` that
    its route (``SlotRoute``) switches on, in the table's order.  Each stage reads the output of the one in front: the float
    stages hand on float32 rows, FLAC frames the resampler's int16, or the float32 at 24 kHz.  A slot that trims goes through
    the trim stage segment by segment, and the state of the stages behind the seam carries from segment to segment.  Each stage
    is created the first time a slot needs it (``seam``: the seam stage at once) and held in the table's attribute (``tr``,
    ``sj``, ``ln``, ``ts``, ``wm``, ``lim``, ``rs``, ``fl``; None until then).  ``n_in``: codec samples per slot and call."""

    def __init__(self, device: torch.device, max_batch: int, n_in: int, seam: bool = False, watermark=None):
        self.device, self.B, self.n_in = device, max_batch, n_in
        self.watermark = watermark  # a watermark.Watermark: the one key of this converter's marked slots (None: no slot may ask)
        for s in STAGE_TABLE:
            setattr(self, s.attr, None)
        if seam:
            self.sj = SeamJoiner(device, max_batch)
        self.routes = [SlotRoute()] * max_batch
        self._plan: Optional[PassPlan] = None  # the last pass's plan

    def reset_slots(self, slots: Sequence[int], formats: Sequence[Optional[str]], speed_q: Sequence[Optional[int]],
                    containers: Optional[Sequence[Optional[str]]] = None, loudness: Optional[Sequence[Optional[float]]] = None,
                    start_gain_db: Optional[Sequence[Optional[float]]] = None, watermark: Optional[Sequence[bool]] = None,
                    trim: Optional[Sequence[Optional[tuple]]] = None, limit: Optional[Sequence[Optional[float]]] = None) -> None:
        """Start new streams in ``slots`` on the current stream: ``formats[i]`` an ``output_format`` (None / ``pcm_24000``:
        float32), ``speed_q[i]`` a Q16 speed (None / 65536: none), ``containers[i]`` None or ``"flac"`` (FLAC frames of the
        slot's 16-bit samples at its rate), ``loudness[i]`` a target in LUFS (None: none) reached from ``start_gain_db[i]``,
        ``watermark[i]`` true for a slot that gets the converter's watermark, ``trim[i]`` None or (trim the ends, the pause cap
        in blocks, the threshold or None) of a slot that trims silence, ``limit[i]`` the ceiling of a slot's peak limiter as
        an amplitude in (0, 1] (``SpeechOptions.ceiling``; None / 0: none).  A slot with none of them is switched off.
        The list form of ``start``, for callers that drive the stages without a request."""
        if not slots:
            return
        formats = [f or "pcm_24000" for f in formats]
        routes = []
        none = [None] * len(slots)
        for b, f, q, c, lt, sg, g, tr, lim in zip(slots, formats, speed_q, containers or none, loudness or none, start_gain_db or none,
                                                  self._gains(watermark, len(slots)), trim or none, limit or none):
            rate, enc = parse_stream_format(f)
            flac = check_container(c, f) is not None
            routes.append(SlotRoute(rate, enc, q or 65536, flac, segmented=False, gen=self.routes[b].gen + 1, head_owed=flac,
                                    loudness=lt, start_gain_db=sg or 0.0, watermark_gain=g, ceiling=float(lim or 0.0),
                                    **({} if tr is None else {"trim": bool(tr[0]), "pause_blocks": int(tr[1]),
                                                              "thr": float(THRESH if tr[2] is None else tr[2])})))
        self._start(slots, routes)

    def start(self, slots: Sequence[int], options: Sequence[SpeechOptions], marked: Optional[Sequence[bool]] = None) -> None:
        """Start new streams in ``slots`` on the current stream, each by its request's options (``SlotRoute.of``); ``marked[i]``
        true for a slot that gets the converter's watermark (the front end's policy applied to the request's wish)."""
        if not slots:
            return
        gains = self._gains(marked, len(slots))
        self._start(slots, [SlotRoute.of(o, g, self.routes[b].gen + 1) for b, o, g in zip(slots, options, gains)])

    def _gains(self, marked: Optional[Sequence[bool]], n: int) -> List[float]:
        """The watermark gain of each of ``n`` new streams; a slot may ask only of a converter that has a key."""
        if marked is not None and any(marked) and self.watermark is None:
            raise ValueError("a slot asks for a watermark, and the converter has no key")
        return [self.watermark.gain if m else 0.0 for m in (marked or [False] * n)]

    def _start(self, slots: Sequence[int], routes: Sequence[SlotRoute]) -> None:
        """The new streams' stages, each created the first time a route needs it, then reset for every slot in ``slots``."""
        for s in STAGE_TABLE:
            stage = getattr(self, s.attr)
            if stage is None and any(s.on(r) for r in routes):
                stage = globals()[s.cls](self.device, self.B, *s.args(self))
                setattr(self, s.attr, stage)
            if stage is not None:
                s.start(stage, slots, routes)
        for b, r in zip(slots, routes):
            self.routes[b] = r

    def start_segments(self, slots: Sequence[int], pauses: Sequence[int], flags: Sequence[int],
                       leads: Optional[Sequence[int]] = None) -> None:
        """Open the next segment of the segmented streams in ``slots`` (``SeamJoiner.start_segments``), after ``reset_slots``
        started the streams; the other stages' state is kept.  The trim stage opens the segment of its slots with the same flags."""
        own = [(b, int(f) & (SEAM_FIRST | SEAM_FINAL)) for b, f in zip(slots, flags) if self.routes[b].trims and not int(f) & SEAM_OFF]
        if own:
            rs = [self.routes[b] for b, _ in own]
            self.tr.start_segments([b for b, _ in own], [f for _, f in own], [r.trim for r in rs], [r.pause_blocks for r in rs],
                                   [r.thr for r in rs])
        if self.sj is None:
            self.sj = SeamJoiner(self.device, self.B)
        self.sj.start_segments(slots, pauses, flags, leads)
        for b, f in zip(slots, flags):
            self.routes[b] = replace(self.routes[b], segmented=not int(f) & SEAM_OFF)

    def converts(self, b: int) -> bool:
        """Whether slot ``b``'s stream goes through a stage: its chunks are ``StreamPass.chunk``'s, not the codec's float32."""
        return bool(self.routes[b].stages)

    def plan(self, slots: Sequence[int]) -> PassPlan:
        """The plan of a pass over the live ``slots``: the last one again while they and their routes stay the same."""
        p, slots = self._plan, tuple(slots)
        if p is None or tuple(p.routes) != slots or any(self.routes[b] is not r for b, r in p.routes.items()):
            p = self._plan = plan_pass({b: self.routes[b] for b in slots})
        return p

    def ends(self, slots: Sequence[int]):
        """The end markers a pass over ``slots`` needs, (``last``, ``seg_end``): those that a planned stage's class declares."""
        need = {m for s in self.plan(slots).stages for m in END_MARKERS[s]}
        return "last" in need, "seg_end" in need

    def _through(self, plan: PassPlan, stage: str, out: torch.Tensor, counts: torch.Tensor, pcm: torch.Tensor, n_in: int,
                 valid: torch.Tensor) -> torch.Tensor:
        """After a float stage: its rows of the slots it passes through (``plan.through``) take the ``pcm`` it read, so that the
        stages behind serve all slots in one launch each; returns the valid counts of its rows."""
        plain = plan.through[stage]
        if not plain:
            return counts
        served = np.zeros(out.shape[0], np.int32)
        served[plan.rows[stage]] = 1
        served_d, plain_d = upload([served, np.asarray(plain, np.int64)], self.device)
        out[plain_d, :n_in] = pcm[plain_d]
        return torch.where(served_d != 0, counts, valid)

    def run(self, pcm: torch.Tensor, n_in: int, valid: torch.Tensor, last: Optional[torch.Tensor] = None,
            slots: Optional[Sequence[int]] = None, seg_end: Optional[torch.Tensor] = None) -> Optional["StreamPass"]:
        """Queue the planned stages, in ``STAGE_TABLE``'s order (the float stages, then the resampler and FLAC), for ``n_in``
        samples of every row of ``pcm`` (device fp32 [batch, >= n_in]) on the current stream.  ``valid`` (device int32 [batch]):
        the samples of each row that are real; ``last`` / ``seg_end`` (device int32 [batch], needed as ``ends`` says): nonzero
        where the row's stream / segment ends with this call.  ``slots``: the live streams (default: every slot); the others
        consume what ``valid`` gives them and are never read.  None when no live slot converts: no launch."""
        plan = self.plan(range(self.B) if slots is None else slots)
        if not plan.stages:
            return None
        batch, outs, ends = pcm.shape[0], {}, {"seg_end": seg_end, "last": last}
        for s in STAGE_TABLE:  # (each float stage's rows, counts and width are what the stages behind it read)
            if s.fp32 and s.name in plan.rows:
                stage = getattr(self, s.attr)
                out, counts = outs[s.name] = stage.new_outputs(batch, n_in)
                getattr(stage, s.call)(pcm, n_in, out, counts, valid=valid, **{m: ends[m] for m in END_MARKERS[s.name]})
                valid, pcm, n_in = self._through(plan, s.name, out, counts, pcm, n_in, valid), out, out.shape[1]
        if "resample" in plan.stages:
            out, counts = outs["resample"] = self.rs.new_outputs(batch, n_in)
            self.rs.chunk(pcm, n_in, out, counts, valid=valid)
        if "flac" in plan.stages:
            s16, s16_counts = outs["resample"] if any(plan.routes[b].enc != ENC_OFF for b in plan.rows["flac"]) else (None, None)
            fout, fsizes = outs["flac"] = self.fl.new_outputs(batch, max(n_in, s16.shape[1] // 2 if s16 is not None else 0))
            self.fl.chunk(batch, fout, fsizes, pcm=pcm, n_in=n_in, valid=valid, s16=s16, s16_counts=s16_counts, last=last)
        return StreamPass(self, {s: outs[s] for s in plan.host}, plan)

    def close(self):
        for s in STAGE_TABLE:
            if getattr(self, s.attr) is not None:
                getattr(self, s.attr).close()
                setattr(self, s.attr, None)


class StreamPass:
    """The outputs of one ``StreamConverter.run``: on the device, then (``to_host``) on the host, read slot by slot (``chunk``).
    It reads each slot by the plan of its run: a slot may have been restarted by the time its chunk is read."""

    def __init__(self, conv: StreamConverter, dev: Dict[str, tuple], plan: PassPlan):
        self.conv, self.rs = conv, conv.rs
        self.dev = dev    # source stage -> its (output, counts) on the device
        self.plan = plan
        self.host = None

    def converts(self, b: int) -> bool:
        """Whether slot ``b`` was converted in the run (its chunk is ``chunk(b, ...)``)."""
        return self.plan.source.get(b) is not None

    def to_host(self, stream) -> None:
        """Queue the host copies on ``stream``; ``chunk`` reads them once ``stream`` has run them."""
        with torch.cuda.stream(stream):
            self.host = {s: tuple(t.to("cpu", non_blocking=True) for t in ts) for s, ts in self.dev.items()}

    def chunk(self, b: int, last: bool) -> np.ndarray:
        """Slot ``b``'s chunk from its source stage: its FLAC frames as uint8 (behind the stream header on the stream's first
        chunk), its converted samples (with the resampler's tail when ``last``), or the stretched / joined / trimmed / limited float32."""
        route, source = self.plan.routes[b], self.plan.source[b]
        out, counts = (t.numpy() for t in self.host[source])
        if source == "flac":
            from .flac import stream_header

            data = b"".join(FlacEncoder.slot_frames(out, counts, b))
            now = self.conv.routes[b]
            if now.head_owed and now.gen == route.gen:
                self.conv.routes[b] = replace(now, head_owed=False)
                data = stream_header(route.rate) + data
            return np.frombuffer(data, dtype=np.uint8).copy()
        if source == "resample":
            return self.rs.slot_bytes(out, counts, b, tail=last, enc=route.enc)
        return out[b, : int(counts[b])].copy()
