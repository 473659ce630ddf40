"""The stages behind the codec, one class per C stage (resampler, time stretch, trim, seam, loudness, watermark, limiter, FLAC), and
their whole-utterance helpers, with the blocking front ends' chain over those (``Finisher``)."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .abi import FLAC_F32, FLAC_S16, RESAMPLE_ULAW, SEAM_FIRST, SEAM_OFF, SmolttsError, check, load_library
from .device import ClosesOnDel, _alloc_slab, current_stream_ptr, dptr
from .formats import parse_stream_format
from .seam import segment_flags


# ------------------------------------------------------------------------------- streamed output formats
def resample_design(out_rate: int):
    """(taps float64 [2 half_len + 1], up, down, half_len) of ``out_rate``: scipy.signal.resample_poly's default filter, designed
    on the host by the library (no device needed).  Raises SmolttsError for an unsupported rate."""
    lib = load_library()
    up, down, half = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.smoltts_resample_design(int(out_rate), None, 0, C.byref(up), C.byref(down), C.byref(half)), "smoltts_resample_design")
    taps = np.zeros(2 * half.value + 1, np.float64)
    check(lib.smoltts_resample_design(int(out_rate), taps.ctypes.data, taps.size, C.byref(up), C.byref(down), C.byref(half)),
          "smoltts_resample_design")
    return taps, up.value, down.value, half.value


class _Stage(ClosesOnDel):
    """What the stages behind the codec share: a slab of ``smoltts_<C_NAME>_bytes(max_batch)`` bytes that the handle of
    ``smoltts_<C_NAME>_create`` lives in, destroyed by ``close`` once the device is idle, and the checks of a ``chunk`` call."""

    C_NAME = ""
    END_MARKERS: Tuple[str, ...] = ()  # the end markers the stage's ``chunk`` takes, of ``seg_end`` and ``last``, in the C call's order

    def __init__(self, device: torch.device, max_batch: int):
        self.lib = load_library()
        self.device, self.B = device, max_batch
        need = getattr(self.lib, f"smoltts_{self.C_NAME}_bytes")(max_batch)
        if need == 0:
            raise SmolttsError(f"smoltts_{self.C_NAME}_bytes returned 0 (bad sizes)")
        self.slab = _alloc_slab(need, device, settle=True)
        h = C.c_void_p()
        check(getattr(self.lib, f"smoltts_{self.C_NAME}_create")(dptr(self.slab), need, max_batch, *self._create_args(), C.byref(h)),
              f"smoltts_{self.C_NAME}_create")
        self.handle = h

    def _create_args(self) -> tuple:
        """What the stage's create call takes between ``max_batch`` and the handle."""
        return ()

    def _call(self, suffix: str, *args) -> None:
        """``smoltts_<C_NAME>_<suffix>(handle, *args, current stream)``, checked."""
        name = f"smoltts_{self.C_NAME}_{suffix}"
        check(getattr(self.lib, name)(self.handle, *args, current_stream_ptr()), name)

    def out_samples(self, n_in: int) -> int:
        """Output samples per row that a call of ``n_in`` input samples needs."""
        return int(getattr(self.lib, f"smoltts_{self.C_NAME}_out_samples")(int(n_in)))

    def new_outputs(self, batch: int, n_in: int):
        """Device buffers of one call of at most ``n_in`` input samples: (fp32 [batch, out_samples(n_in)], counts int32 [batch])."""
        return (torch.empty(batch, self.out_samples(n_in), dtype=torch.float32, device=self.device),
                torch.empty(batch, dtype=torch.int32, device=self.device))

    @staticmethod
    def _ints(v: Sequence[int]):
        """``v`` as a host int32 array for the C calls."""
        return (C.c_int32 * len(v))(*[int(x) for x in v])

    def _check(self, batch: int, pcm: Optional[torch.Tensor], n_in: int, out: torch.Tensor, dtype, width: int,
               counts: torch.Tensor, per_row: int, *controls: Optional[torch.Tensor]) -> None:
        """``pcm``: device fp32 [>= batch, >= n_in] with unit-stride rows (None: not read); ``out``: contiguous ``dtype``
        [>= batch, >= width]; ``counts``: contiguous int32 of ``per_row`` entries per row; ``controls``: None or contiguous
        device int32 [>= batch]."""
        assert batch <= self.B and out.dtype == dtype and out.is_contiguous() and out.shape[0] >= batch and out.shape[1] >= width
        assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.shape[0] >= batch and counts.numel() >= per_row * batch
        assert pcm is None or (pcm.dtype == torch.float32 and pcm.stride(1) == 1 and pcm.shape[0] >= batch and 0 <= n_in <= pcm.shape[1])
        for t in controls:
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= batch)

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize()
            getattr(self.lib, f"smoltts_{self.C_NAME}_destroy")(self.handle)
            self.handle = None


class _FloatStage(_Stage):
    """A stage that reads fp32 rows and writes fp32 rows, so that the stage behind it can read them: one ``chunk`` for all of
    them.  A class declares the end markers its C call takes (``END_MARKERS``)."""

    def _width(self, n_in: int) -> int:
        """The least width of ``out`` in a call of ``n_in`` input samples."""
        return self.out_samples(n_in)

    def _chunk_args(self) -> tuple:
        """What the stage's chunk call takes between the end markers and ``out``."""
        return ()

    def chunk(self, pcm: torch.Tensor, n_in: int, out: torch.Tensor, counts: torch.Tensor, valid: Optional[torch.Tensor] = None,
              seg_end: Optional[torch.Tensor] = None, last: Optional[torch.Tensor] = None) -> None:
        """Run ``n_in`` samples of every row of ``pcm`` (device fp32 [batch, >= n_in], contiguous rows) through the stage on the
        current stream.  ``valid``: device int32 [batch], the samples of each row that are real; ``seg_end`` / ``last``: device
        int32 [batch], nonzero where the row's segment / stream ends with this call (a stage takes the ones it declares, and
        refuses another).  ``counts[b]``: the samples slot b wrote to ``out[b]``."""
        given = {"seg_end": seg_end, "last": last}
        assert all(t is None or m in self.END_MARKERS for m, t in given.items()), f"{type(self).__name__} takes {self.END_MARKERS}"
        ends = [given[m] for m in self.END_MARKERS]
        batch = pcm.shape[0]
        self._check(batch, pcm, n_in, out, torch.float32, self._width(n_in), counts, 1, valid, *ends)
        self._call("chunk", dptr(pcm), pcm.stride(0), batch, n_in, dptr(valid), *map(dptr, ends), *self._chunk_args(), dptr(out),
                   out.shape[1], dptr(counts))


class _SameLengthStage(_FloatStage):
    """A float stage whose slots emit exactly the samples they read: no end marker."""

    def out_samples(self, n_in: int) -> int:
        """A slot emits what it reads (one sample of room for an empty call)."""
        return max(int(n_in), 1)

    def _width(self, n_in: int) -> int:
        return n_in


class Resampler(_Stage):
    """Per-slot conversion of streamed 24 kHz fp32 PCM to ``pcm_<rate>`` int16 / ``ulaw_8000`` bytes on the GPU
    (include/smoltts_hip.h, "Streamed output formats"): one launch per call for every slot, each at its own format.  Slots
    start off; ``reset_slots`` starts a new stream in a slot with its format."""

    C_NAME = "resampler"

    def __init__(self, device: torch.device, max_batch: int, max_in: int):
        super().__init__(device, max_batch)
        self.out_stride = int(self.lib.smoltts_resampler_out_bytes(max_in))
        self.formats = [(24000, 0)] * max_batch  # (rate, SMOLTTS_RESAMPLE_*) per slot

    def reset_slots(self, slots: Sequence[int], formats: Sequence[str]) -> None:
        """Start new streams in ``slots`` with their ``output_format`` (``pcm_24000``: the slot is not converted)."""
        parsed = [parse_stream_format(f) for f in formats]
        self._call("reset_slots", self._ints(slots), self._ints([p[0] for p in parsed]), self._ints([p[1] for p in parsed]), len(slots))
        for b, p in zip(slots, parsed):
            self.formats[b] = p

    def new_outputs(self, batch: int, n_in: Optional[int] = None):
        """Device buffers of one call: (bytes uint8 [batch, out_stride], counts int32 [batch, 2]); ``n_in``: size them for calls of
        at most that many input samples instead of ``max_in``."""
        stride = self.out_stride if n_in is None else int(self.lib.smoltts_resampler_out_bytes(n_in))
        return (torch.empty(batch, stride, dtype=torch.uint8, device=self.device),
                torch.empty(batch, 2, dtype=torch.int32, device=self.device))

    def chunk(self, pcm: torch.Tensor, n_in: int, out: torch.Tensor, counts: torch.Tensor, valid: Optional[torch.Tensor] = None) -> None:
        """Convert ``n_in`` samples of every row of ``pcm`` (device fp32 [batch, >= n_in], contiguous rows) on the current stream;
        ``valid``: device int32 [batch], the samples of each row that are real (the rest is not consumed)."""
        batch = pcm.shape[0]
        self._check(batch, pcm, n_in, out, torch.uint8, int(self.lib.smoltts_resampler_out_bytes(n_in)), counts, 2, valid)
        check(self.lib.smoltts_resample_chunk(self.handle, dptr(pcm), pcm.stride(0), batch, n_in, dptr(valid), dptr(out), out.shape[1],
                                              dptr(counts), current_stream_ptr()), "smoltts_resample_chunk")

    def slot_bytes(self, host_out: np.ndarray, host_counts: np.ndarray, b: int, tail: bool = False,
                   enc: Optional[int] = None) -> np.ndarray:
        """Slot ``b``'s samples of a call, copied to the host: int16 for pcm_*, uint8 for ulaw_8000; with the tail if ``tail``.
        ``enc``: the encoding the call ran with, when the slot may have been restarted since (default: its current one)."""
        enc = self.formats[b][1] if enc is None else enc
        n = int(host_counts[b, 0]) + (int(host_counts[b, 1]) if tail else 0)
        width = 1 if enc == RESAMPLE_ULAW else 2
        return host_out[b, : n * width].view(np.uint8 if enc == RESAMPLE_ULAW else np.int16).copy()


# ------------------------------------------------------------------------------- speaking speed
class TimeStretcher(_FloatStage):
    """Per-slot pitch-preserving time stretch of streamed 24 kHz fp32 PCM on the GPU (include/smoltts_hip.h, "Speaking speed";
    the numpy model is ``tsm.Stretcher``): one launch per call for every slot, each at its own speed.  Slots start off;
    ``reset_slots`` starts a new stream in a slot at its ``speed_q`` (65536: off).  A slot flushes with ``last``."""

    C_NAME = "tsm"
    END_MARKERS = ("last",)

    def reset_slots(self, slots: Sequence[int], speed_q: Sequence[int]) -> None:
        self._call("reset_slots", self._ints(slots), self._ints(speed_q), len(slots))

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s counters (synchronises the current stream): k (next segment), p_prev, n_in, n_out, ended."""
        v = (C.c_int64 * 5)()
        self._call("slot_state", int(slot), v)
        return dict(zip(("k", "p_prev", "n_in", "n_out", "ended"), list(v)))


def _f32(pcm) -> np.ndarray:
    """``pcm`` as a contiguous float32 1-D host array."""
    return np.ascontiguousarray(np.asarray(pcm, dtype=np.float32).reshape(-1))


@contextlib.contextmanager
def _held(cls, device: torch.device, given, *args):
    """The one-slot ``cls`` stage of a whole-utterance call, with ``device`` current: the caller's (``given``), or one made for
    the call and closed behind it.  The whole-utterance calls take no slot or reset slot 0, so a held stage carries nothing from
    one utterance to the next."""
    with torch.cuda.device(device):
        stage = given if given is not None else cls(device, 1, *args)
        try:
            yield stage
        finally:
            if given is None:
                stage.close()


def _whole_row(stage: _Stage, x: np.ndarray, launch):
    """A whole utterance through slot 0 of ``stage``: ``x`` (host, contiguous) goes up as the device row [1, n] (one zero sample
    when empty), and ``launch(row, n, out, counts)`` queues the stage's call into ``stage.new_outputs(1, n)``.  Waits, and
    returns the output row cut to its count, or for FLAC (counts: frame sizes [1, blocks, 2]) the row's frames."""
    n = int(x.size)
    row = torch.from_numpy(x).to(stage.device)[None] if n else torch.zeros(1, 1, dtype=torch.from_numpy(x).dtype, device=stage.device)
    out, counts = stage.new_outputs(1, n)
    launch(row, n, out, counts)
    if counts.dim() == 1:
        return out[0, :int(counts.cpu()[0])].cpu().numpy()
    return FlacEncoder.slot_frames(out.cpu().numpy(), counts.cpu().numpy(), 0)


def stretch_pcm(pcm: np.ndarray, speed_q: int, device: torch.device, held: Optional[TimeStretcher] = None) -> np.ndarray:
    """A whole utterance (float32 at 24 kHz) stretched on ``device`` (the model's) in one call with ``last`` set: exactly
    ``tsm.out_length(len(pcm), speed_q)`` samples (``SmolTTS.__call__``).  Waits for the result.  ``speed_q == 65536`` returns
    ``pcm`` untouched.  ``held``: a caller's ``TimeStretcher`` whose slot 0 is used (default: one made for the call)."""
    pcm = _f32(pcm)
    if speed_q == 65536:
        return pcm
    with _held(TimeStretcher, device, held) as ts:
        ts.reset_slots([0], [speed_q])
        return _whole_row(ts, pcm, lambda x, n, out, cnt: ts.chunk(x, n, out, cnt, last=torch.ones(1, dtype=torch.int32, device=device)))


# ------------------------------------------------------------------------------- silence: trimmed ends, capped pauses
class SilenceTrimmer(_FloatStage):
    """Per-slot silence trimming of streamed 24 kHz fp32 PCM on the GPU (include/smoltts_hip.h, "Trim"; the numpy model is
    ``trim.TrimState``): one launch per call, of at most ``trim.MAX_CALL`` samples, for every slot.  Slots start off;
    ``start_segments`` opens a segment in a slot with its flags (``SEAM_FIRST`` / ``SEAM_FINAL``; ``SEAM_OFF`` switches the slot
    off), whether its ends are trimmed, its pause cap in blocks and its threshold; ``seg_end`` / ``last`` end it."""

    C_NAME = "trim"
    END_MARKERS = ("seg_end", "last")

    def start_segments(self, slots: Sequence[int], flags: Sequence[int], trims: Sequence[bool], pauses: Sequence[int],
                       thrs: Sequence[float]) -> None:
        n = len(slots)
        if not n:
            return
        self._call("reset_slots", self._ints(slots), self._ints(flags), self._ints([bool(t) for t in trims]), self._ints(pauses),
                   (C.c_float * n)(*[float(t) for t in thrs]), n)

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s state (synchronises the current stream): ``trim.TrimState.COUNTERS`` in samples, and open."""
        from .trim import TrimState

        v = (C.c_int64 * 8)()
        self._call("slot_state", int(slot), v)
        return dict(zip(TrimState.COUNTERS + ("open",), list(v)))


def trim_pcm(pcm: np.ndarray, flags: int, device: torch.device, trim: bool = True, pause_blocks: int = 0, thr: Optional[float] = None,
             held: Optional[SilenceTrimmer] = None) -> np.ndarray:
    """A whole segment (float32 at 24 kHz) trimmed on ``device`` by the trim rule: what ``trim.trim`` computes
    (``SmolTTS.__call__``).  The row goes through slot 0 in calls of at most ``trim.MAX_CALL`` samples, the last one ending the
    segment; one wait for all of them.  ``held``: a caller's ``SilenceTrimmer`` whose slot 0 is used (default: one made for the
    call)."""
    from .trim import MAX_CALL, THRESH

    x = _f32(pcm)
    with _held(SilenceTrimmer, device, held) as st:
        st.start_segments([0], [flags], [trim], [pause_blocks], [THRESH if thr is None else thr])
        row = torch.from_numpy(x).to(device)[None] if x.size else torch.zeros(1, 1, dtype=torch.float32, device=device)
        end = torch.ones(1, dtype=torch.int32, device=device)
        outs = []
        for i in range(0, max(x.size, 1), MAX_CALL):
            n = min(MAX_CALL, x.size - i)
            out, counts = st.new_outputs(1, n)
            st.chunk(row[:, i:i + max(n, 1)], n, out, counts, seg_end=end if i + n >= x.size else None)
            outs.append((out, counts))
        counts = torch.cat([c for _, c in outs]).cpu().numpy()
        return np.concatenate([o[0, :int(c)].cpu().numpy() for (o, _), c in zip(outs, counts)])


# ------------------------------------------------------------------------------- long texts: the seam between segments
class SeamJoiner(_FloatStage):
    """Per-slot joining of a long text's segments on the GPU (include/smoltts_hip.h, "Seam"; the numpy model is
    ``seam.SeamState``): one launch per call for every slot.  Slots start off; ``start_segments`` opens a segment in a slot with
    its pause and flags (``SEAM_FIRST`` / ``SEAM_FINAL``; ``SEAM_OFF`` switches the slot off)."""

    C_NAME = "seam"
    END_MARKERS = ("seg_end", "last")

    def __init__(self, device: torch.device, max_batch: int):
        super().__init__(device, max_batch)
        self.zeros = [0] * max_batch  # zeros the slot's open segment owes at most (its lead and its pause)

    def out_samples(self, n_in: int) -> int:
        """Output samples per row of a call of ``n_in`` input samples, for the segments open now."""
        return int(self.lib.smoltts_seam_out_samples(int(n_in), max(self.zeros)))

    def start_segments(self, slots: Sequence[int], pauses: Sequence[int], flags: Sequence[int],
                       leads: Optional[Sequence[int]] = None) -> None:
        """Open a segment in each of ``slots`` on the current stream: its pause G (samples), flags, and the zeros in front of a
        ``SEAM_FIRST`` segment (``leads``)."""
        n = len(slots)
        if not n:
            return
        leads = leads or [0] * n
        self._call("reset_slots", self._ints(slots), self._ints(pauses), self._ints(flags), self._ints(leads), n)
        for b, p, f, ld in zip(slots, pauses, flags, leads):
            self.zeros[b] = 0 if int(f) & SEAM_OFF else int(p) + (int(ld) if int(f) & SEAM_FIRST else 0)

    def _chunk_args(self) -> tuple:
        return (max(self.zeros),)

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s state (synchronises the current stream): n_in, judged, ec, head, open, lead, pause, flags."""
        v = (C.c_int64 * 8)()
        self._call("slot_state", int(slot), v)
        return dict(zip(("n_in", "judged", "ec", "head", "open", "lead", "pause", "flags"), list(v)))


def seam_join(segments: Sequence[np.ndarray], pauses: Sequence[int], device: torch.device, lead: int = 0, trail: int = 0,
              held: Optional[SeamJoiner] = None) -> np.ndarray:
    """Whole segments (float32 at 24 kHz) joined on ``device`` by the seam rule, one call per segment with its end set: what
    ``seam.join`` computes (``SmolTTS.__call__`` with ``segment``).  ``pauses[k]``: the seam after segment k, in samples.
    ``held``: a caller's ``SeamJoiner`` whose slot 0 is used (default: one made for the call).  Waits for the result."""
    segs = [_f32(s) for s in segments]
    if len(pauses) != max(len(segs) - 1, 0):
        raise ValueError("one pause per seam")
    out = []
    with _held(SeamJoiner, device, held) as sj:
        end = torch.ones(1, dtype=torch.int32, device=device)
        for k, x in enumerate(segs):
            final = k == len(segs) - 1
            sj.start_segments([0], [trail if final else pauses[k]], [segment_flags(k, len(segs))], [lead])
            out.append(_whole_row(sj, x, lambda xd, n, y, cnt: sj.chunk(xd, n, y, cnt, seg_end=end, last=end if final else None)))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


# ------------------------------------------------------------------------------- loudness
class LoudnessNormalizer(_SameLengthStage):
    """Per-slot loudness normalisation of streamed 24 kHz fp32 PCM on the GPU (include/smoltts_hip.h, "Loudness"; the numpy
    model is ``loudness.StreamState``): one launch per call for every slot, each towards its own target.  A slot emits exactly
    the samples it reads: ``counts[b]`` is its valid ones, 0 for a slot that is off.  Slots start off; ``reset_slots`` starts a
    new stream in a slot (target None: off)."""

    C_NAME = "loudness"

    def _create_args(self) -> tuple:
        from .loudness import tables

        self._tables = tables().packed()  # (read by the create call only)
        assert self._tables.size == self.lib.smoltts_loudness_table_doubles()
        return self._tables.ctypes.data, int(self._tables.size)

    def reset_slots(self, slots: Sequence[int], targets: Sequence[Optional[float]],
                    start_gain_db: Optional[Sequence[Optional[float]]] = None) -> None:
        """Start new streams in ``slots`` towards their ``targets`` (LUFS; None: the slot is off) from their first knots
        (``start_gain_db``, default 0 dB)."""
        from .loudness import knot_of_db, target_power

        n = len(slots)
        if not n:
            return
        power = (C.c_double * n)(*[0.0 if t is None else target_power(t) for t in targets])
        knots = self._ints([knot_of_db(g or 0.0) for g in (start_gain_db or [0.0] * n)])
        self._call("reset_slots", self._ints(slots), power, knots, n)

    def measure(self, row: torch.Tensor, n: int) -> Tuple[float, float]:
        """(gated mean power, peak) of the whole utterance ``row[:n]`` (device fp32, contiguous); waits for the result."""
        hops = torch.empty(n // 2400 + 1, dtype=torch.float64, device=self.device)
        res = torch.empty(4, dtype=torch.float64, device=self.device)
        self._call("measure", dptr(row), int(n), dptr(hops), hops.numel(), dptr(res))
        p, peak = res.cpu().numpy()[:2]
        return float(p), float(peak)

    def scale(self, row: torch.Tensor, n: int, gain: float, out: torch.Tensor) -> None:
        """``out[:n] = float32(row[:n] * gain)`` on the current stream."""
        check(self.lib.smoltts_loudness_scale(dptr(row), int(n), float(gain), dptr(out), current_stream_ptr()), "smoltts_loudness_scale")

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s state (synchronises the current stream), in the layout of ``loudness.StreamState.state``, with
        ``on`` and ``ptarget``."""
        ints, v = (C.c_int64 * 4)(), np.zeros(19 + 512, np.float64)
        self._call("slot_state", int(slot), ints, v.ctypes.data)
        return {"pos": int(ints[0]), "ka": int(ints[1]), "kb": int(ints[2]), "on": int(ints[3]), "peak": np.float32(v[17]),
                "ptarget": float(v[18]), "filter": v[:17].copy(), "ring": v[19:].copy()}


def _loudness_whole(pcm: np.ndarray, device: torch.device, target: Optional[float], cap: bool = True, held=None):
    """(power, peak, gain, output or None) of a whole utterance on ``device``: measured in one launch, and with a ``target``
    scaled by the blocking rule's gain (``cap`` false: not capped by the peak) in a second one.  ``held``: a caller's
    ``LoudnessNormalizer`` (default: one made for the call)."""
    from .loudness import static_gain

    x = _f32(pcm)
    with _held(LoudnessNormalizer, device, held) as ln:
        seen = {}

        def launch(row, n, out, counts):
            seen["p"], seen["peak"] = ln.measure(row, n) if n else (0.0, 0.0)
            seen["g"] = 1.0 if target is None else static_gain(target, seen["p"], seen["peak"], cap)
            ln.scale(row, n, seen["g"], out)
            counts.fill_(n)

        y = _whole_row(ln, x, launch)
    return seen["p"], seen["peak"], seen["g"], (x if seen["g"] == 1.0 else y)


def measure_loudness(pcm: np.ndarray, device: torch.device, held: Optional[LoudnessNormalizer] = None) -> Tuple[float, float]:
    """(integrated loudness in LUFS by BS.1770-4, -inf when no block passes the absolute gate or the utterance is shorter than
    400 ms; peak) of a whole utterance (float32 at 24 kHz), measured on ``device``: ``loudness.measure``.  Waits."""
    from .loudness import lufs_of_power

    p, peak, _, _ = _loudness_whole(pcm, device, None, held=held)
    return lufs_of_power(p), peak


def loudness_normalize(pcm: np.ndarray, target: float, device: torch.device, with_gain: bool = False, cap: bool = True, held=None):
    """A whole utterance (float32 at 24 kHz) brought to ``target`` LUFS on ``device`` by one gain, capped so that its peak
    stays at -1 dBFS: ``loudness.normalize`` (``SmolTTS.__call__``).  An utterance that measures nothing comes back
    unchanged.  ``with_gain``: -> (samples, the gain applied).  ``cap`` false: the gain is not capped by the peak (a request
    whose peaks a limiter takes down behind it).  Waits for the result."""
    from .loudness import check_target

    _, _, g, y = _loudness_whole(pcm, device, check_target(target), cap, held)
    return (y, g) if with_gain else y


# ------------------------------------------------------------------------------- watermark
class Watermarker(_SameLengthStage):
    """Per-slot watermarking of streamed 24 kHz fp32 PCM on the GPU (include/smoltts_hip.h, "Watermark"; the numpy model is
    ``watermark.StreamState``): one launch per call for every slot.  One key per stage: its chip table is uploaded here.  A slot
    emits exactly the samples it reads: ``counts[b]`` is its valid ones, 0 for a slot that is off, whose row is left alone.
    Slots start off; ``reset_slots`` starts a new stream in a slot (gain 0: off)."""

    C_NAME = "watermark"

    def __init__(self, device: torch.device, max_batch: int, wm):
        self.wm = wm
        super().__init__(device, max_batch)

    def _create_args(self) -> tuple:
        self._tables = self.wm.packed()  # (read by the create call only)
        assert self._tables.size == self.lib.smoltts_watermark_table_doubles()
        return self._tables.ctypes.data, int(self._tables.size)

    def reset_slots(self, slots: Sequence[int], gains: Sequence[float]) -> None:
        """Start new streams in ``slots`` at their ``gains`` (10^(strength_db / 20); 0: the slot is off)."""
        n = len(slots)
        if not n:
            return
        self._call("reset_slots", self._ints(slots), (C.c_double * n)(*[float(g) for g in gains]), n)

    def embed(self, row: torch.Tensor, n: int, gain: float, out: torch.Tensor) -> None:
        """``out[:n]``: the whole utterance ``row[:n]`` (device fp32, contiguous) marked from position 0, on the current stream."""
        self._call("embed", dptr(row), int(n), float(gain), dptr(out))

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s state (synchronises the current stream), in the layout of ``watermark.StreamState.state``, with ``on``."""
        ints, v = (C.c_int64 * 2)(), np.zeros(5, np.float64)
        self._call("slot_state", int(slot), ints, v.ctypes.data)
        return {"pos": int(ints[0]), "on": int(ints[1]), "values": v}


def watermark_embed(pcm: np.ndarray, wm, device: torch.device, held: Optional[Watermarker] = None) -> np.ndarray:
    """A whole utterance (float32 at 24 kHz) marked with ``wm`` (a ``watermark.Watermark``) on ``device`` in one launch from
    position 0: ``watermark.embed`` (``SmolTTS.__call__``).  ``held``: a caller's ``Watermarker`` of that key (default: one made
    for the call).  Waits for the result."""
    x = _f32(pcm)
    if x.size == 0:
        return x
    with _held(Watermarker, device, held, wm) as st:
        assert st.wm is wm, "the held Watermarker carries another key's chip table"

        def launch(row, n, out, counts):
            st.embed(row, n, wm.gain, out)
            counts.fill_(n)

        return _whole_row(st, x, launch)


# ------------------------------------------------------------------------------- peak limiter
class PeakLimiter(_FloatStage):
    """Per-slot look-ahead peak limiting of streamed 24 kHz fp32 PCM on the GPU (include/smoltts_hip.h, "Limiter"; the numpy
    model is ``limiter.StreamState``): one launch per call, of at most ``limiter.MAX_CALL`` samples, for every slot, each under
    its own ceiling.  A slot holds back ``limiter.HOLD_BACK`` samples until its stream ends (``last``: it flushes); the row of a
    slot that is off is left alone, with a count of 0.  Slots start off; ``reset_slots`` starts a new stream in a slot
    (ceiling 0: off)."""

    C_NAME = "limiter"
    END_MARKERS = ("last",)

    def _create_args(self) -> tuple:
        from .limiter import packed

        self._tables = packed()  # (read by the create call only)
        assert self._tables.size == self.lib.smoltts_limiter_table_doubles()
        return self._tables.ctypes.data, int(self._tables.size)

    def reset_slots(self, slots: Sequence[int], ceilings: Sequence[float]) -> None:
        """Start new streams in ``slots`` under their ``ceilings`` (10^(peak_limit_db / 20); 0: the slot is off)."""
        n = len(slots)
        if not n:
            return
        self._call("reset_slots", self._ints(slots), (C.c_double * n)(*[float(c) for c in ceilings]), n)

    def out_samples(self, n_in: int) -> int:
        """Output samples per row of a pass of ``n_in`` input samples (``run``): what the C call says up to the most one call
        takes, the same rule past it."""
        from .limiter import HOLD_BACK, MAX_CALL

        return super().out_samples(n_in) if n_in <= MAX_CALL else int(n_in) + HOLD_BACK

    def run(self, pcm: torch.Tensor, n_in: int, out: torch.Tensor, counts: torch.Tensor, valid: torch.Tensor,
            last: Optional[torch.Tensor] = None) -> None:
        """``chunk`` for rows of any width (the stages in front can hand over more than one call takes: a trim stage that
        releases what it held, stretched): the row goes through in pieces of ``limiter.MAX_CALL`` samples, the stream's end with
        the last one, and each piece's samples are moved behind those of the pieces in front.  No wait."""
        from .limiter import MAX_CALL

        if n_in <= MAX_CALL:
            return self.chunk(pcm, n_in, out, counts, valid=valid, last=last)
        batch = pcm.shape[0]
        at = torch.arange(out.shape[1], device=self.device)[None]
        total = torch.zeros(batch, dtype=torch.int64, device=self.device)
        for i in range(0, n_in, MAX_CALL):
            w = min(MAX_CALL, n_in - i)
            part, cnt = self.new_outputs(batch, w)
            self.chunk(pcm[:, i:i + w], w, part, cnt, valid=(valid - i).clamp(0, w).to(torch.int32),
                       last=last if i + w >= n_in else None)
            idx = at - total[:, None]
            mine = (idx >= 0) & (idx < cnt[:, None])
            out.copy_(torch.where(mine, part.gather(1, idx.clamp(0, part.shape[1] - 1)), out))
            total += cnt
        counts.copy_(total.to(torch.int32))

    def apply(self, row: torch.Tensor, n: int, ceiling: float, out: torch.Tensor, result: torch.Tensor) -> None:
        """``out[:n]``: the whole utterance ``row[:n]`` (device fp32, contiguous) limited under ``ceiling`` from position 0 to its
        end, on the current stream; ``result[0]`` (device fp64): the smallest gain applied."""
        assert result.dtype == torch.float64 and result.numel() >= 1 and out.numel() >= n
        self._call("apply", dptr(row), int(n), float(ceiling), dptr(out), dptr(result))

    def slot_state(self, slot: int) -> dict:
        """Slot ``slot``'s state (synchronises the current stream), in the layout of ``limiter.StreamState.state``, with ``on``."""
        from .limiter import HOLD_BACK, R_HIST

        ints, v = (C.c_int64 * 3)(), np.zeros(2 + R_HIST + HOLD_BACK, np.float64)
        self._call("slot_state", int(slot), ints, v.ctypes.data)
        return {"pos": int(ints[0]), "on": int(ints[1]), "ended": int(ints[2]), "c": float(v[0]), "min_g": float(v[1]),
                "r": v[2:2 + R_HIST].copy(), "x": v[2 + R_HIST:].astype(np.float32)}


def peak_limit(pcm: np.ndarray, peak_limit_db: float, device: torch.device, held: Optional[PeakLimiter] = None) -> Tuple[np.ndarray, float]:
    """A whole utterance (float32 at 24 kHz) limited under ``peak_limit_db`` dBFS on ``device`` in one launch: ``limiter.limit``
    (``SmolTTS.__call__``) -> (samples, as many as went in; the reduction in dB, ``-20 log10(min g)``, 0.0 when nothing was
    limited).  ``held``: a caller's ``PeakLimiter`` (default: one made for the call).  Waits for the result."""
    from .limiter import ceiling_of_db, check_peak_limit, reduction_db

    c = ceiling_of_db(check_peak_limit(peak_limit_db))
    x = _f32(pcm)
    if x.size == 0:
        return x, 0.0
    with _held(PeakLimiter, device, held) as st:
        res = torch.empty(1, dtype=torch.float64, device=device)
        row = torch.from_numpy(x).to(device)
        out = torch.empty_like(row)
        st.apply(row, x.size, c, out, res)
        return out.cpu().numpy(), reduction_db(float(res.cpu()[0]))


# ------------------------------------------------------------------------------- a blocking utterance, finished
class Finisher:
    """What both blocking front ends do to a complete utterance behind the codec, on ``device``'s current stream, each step
    waited for as its helper waits.  The order: trim -> seam join -> loudness -> stretch -> watermark -> limiter.
    Segment k of n is trimmed with ``segment_flags(k, n)`` (a plain utterance is one segment, first and final) and the trimmed
    seconds are summed over the segments; the loudness gain is capped by the peak exactly when no limiter follows; the
    watermark stands behind the stretch and the limiter is last of all.  ``head`` is the part in front of the stretch and
    ``tail`` the part behind it, for a caller that stretches by its own means (the scheduler's batched stretch).
    At most one one-slot stage per class is held (``held``), made by ``_make`` when an option first needs it."""

    def __init__(self, device: torch.device):
        self.device = device
        self.held: dict = {}  # stage class -> its one-slot stage

    def _make(self, cls, *args):
        with torch.cuda.device(self.device):
            return cls(self.device, 1, *args)

    def _stage(self, cls, *args):
        if cls not in self.held:
            self.held[cls] = self._make(cls, *args)
        return self.held[cls]

    def close(self) -> None:
        for stage in self.held.values():
            stage.close()
        self.held = {}

    @staticmethod
    def needed(opts, mark) -> bool:
        """Whether a request with ``opts`` and the key ``mark`` (None: unmarked) has anything done to it here."""
        return bool(opts.trims or opts.loudness is not None or opts.speed_q or mark is not None or opts.peak_limit_db is not None)

    def head(self, segments: Sequence[np.ndarray], opts, plan=None):
        """``segments`` (host float32; one entry: a plain utterance) trimmed, joined by ``plan`` (a ``longform`` segment plan)
        and levelled -> (samples, seconds trimmed, loudness gain in dB or None)."""
        from .loudness import gain_db

        whole, gain = segments, None
        if opts.trims:
            segments = [trim_pcm(x, segment_flags(k, len(whole)), self.device, *opts.trim_route, held=self._stage(SilenceTrimmer))
                        for k, x in enumerate(whole)]
        trimmed_s = float(sum((x.size - y.size) / 24000.0 for x, y in zip(whole, segments)))
        if plan is not None:
            pcm = seam_join(segments, plan.pauses, self.device, lead=plan.lead, trail=plan.trail, held=self._stage(SeamJoiner))
        else:
            pcm, = segments
        if opts.loudness is not None:
            pcm, g = loudness_normalize(pcm, opts.loudness, self.device, with_gain=True, cap=opts.peak_limit_db is None,
                                        held=self._stage(LoudnessNormalizer))
            gain = gain_db(g)
        return pcm, trimmed_s, gain

    def tail(self, pcm: np.ndarray, opts, mark):
        """``pcm`` marked with the key ``mark`` (a ``watermark.Watermark``; None: unmarked), then limited -> (samples, peak
        reduction in dB or None).  The held ``Watermarker`` is one key's: another key object has it made anew."""
        reduction = None
        if mark is not None:
            if Watermarker in self.held and self.held[Watermarker].wm is not mark:
                self.held.pop(Watermarker).close()
            pcm = watermark_embed(pcm, mark, self.device, held=self._stage(Watermarker, mark))
        if opts.peak_limit_db is not None:
            pcm, reduction = peak_limit(pcm, opts.peak_limit_db, self.device, held=self._stage(PeakLimiter))
        return pcm, reduction

    def __call__(self, segments: Sequence[np.ndarray], opts, mark, plan=None):
        """The whole chain -> (samples, seconds trimmed, loudness gain in dB or None, peak reduction in dB or None)."""
        pcm, trimmed_s, gain = self.head(segments, opts, plan)
        if opts.speed_q:
            pcm = stretch_pcm(pcm, opts.speed_q, self.device, held=self._stage(TimeStretcher))
        pcm, reduction = self.tail(pcm, opts, mark)
        return pcm, trimmed_s, gain, reduction


# ------------------------------------------------------------------------------- FLAC framing
class FlacEncoder(_Stage):
    """Per-slot FLAC framing of streamed samples on the GPU (include/smoltts_hip.h, "FLAC"; the numpy model is
    ``flac.StreamEncoder``): one launch per call for every slot, each reading fp32 PCM or the resampler's int16 at its own rate.
    Slots start off; ``reset_slots`` starts a new stream in a slot.  The stream header (``flac.stream_header``) is the caller's."""

    C_NAME = "flac"
    END_MARKERS = ("last",)

    def reset_slots(self, slots: Sequence[int], rates: Sequence[int], sources: Sequence[int]) -> None:
        """Start new streams in ``slots`` at their rate and source (``FLAC_F32`` / ``FLAC_S16``; ``FLAC_OFF``: off)."""
        self._call("reset_slots", self._ints(slots), self._ints(rates), self._ints(sources), len(slots))

    def new_outputs(self, batch: int, n_max: int):
        """Device buffers of one call in which a slot reads at most ``n_max`` samples: (bytes uint8 [batch, out_bytes],
        sizes int32 [batch, max_blocks, 2])."""
        blocks = int(self.lib.smoltts_flac_max_blocks(int(n_max)))
        return (torch.empty(batch, int(self.lib.smoltts_flac_out_bytes(int(n_max))), dtype=torch.uint8, device=self.device),
                torch.empty(batch, blocks, 2, dtype=torch.int32, device=self.device))

    def chunk(self, batch: int, out: torch.Tensor, sizes: torch.Tensor, pcm: Optional[torch.Tensor] = None, n_in: int = 0,
              valid: Optional[torch.Tensor] = None, s16: Optional[torch.Tensor] = None, s16_counts: Optional[torch.Tensor] = None,
              last: Optional[torch.Tensor] = None) -> None:
        """Frame the samples of slots [0, batch) on the current stream: F32 slots read ``n_in`` samples of ``pcm`` (device fp32
        [batch, >= n_in]; ``valid``: device int32 [batch], the real ones), S16 slots the resampler's ``s16`` bytes (uint8
        [batch, row]) and ``s16_counts`` (int32 [batch, 2]: finals, tail); ``last`` (device int32 [batch]) nonzero where the
        stream ends with this call.  ``sizes[b, j]``: {offset, bytes} of slot b's frame j in ``out[b]``."""
        self._check(batch, pcm, n_in, out, torch.uint8, 0, sizes, 0, valid, last)
        if s16 is not None:
            assert s16.dtype == torch.uint8 and s16.is_contiguous() and s16_counts is not None and s16_counts.is_contiguous()
        self._call("chunk", dptr(pcm), pcm.stride(0) if pcm is not None else 0, int(n_in), dptr(valid), dptr(s16),
                   s16.shape[1] if s16 is not None else 0, dptr(s16_counts), batch, dptr(last), dptr(out), out.shape[1], dptr(sizes),
                   sizes.shape[1])

    @staticmethod
    def slot_frames(host_out: np.ndarray, host_sizes: np.ndarray, b: int) -> List[bytes]:
        """Slot ``b``'s frames of a call, in order, from the host copies of ``out`` and ``sizes``."""
        frames = []
        for off, n in host_sizes[b]:
            if n <= 0:
                break
            frames.append(host_out[b, int(off):int(off) + int(n)].tobytes())
        return frames


def flac_encode(samples: np.ndarray, sample_rate: int, device: torch.device) -> bytes:
    """A whole utterance as one FLAC file, framed on ``device`` in one call with ``last`` set: float32 samples are quantised as
    rint(clip(x, -1, 1) * 32767), int16 ones taken as they are.  The STREAMINFO carries the true total, the smallest and largest
    frame and the MD5 of the samples (``SmolTTS.__call__``).  Waits for the result."""
    from . import flac

    x = np.asarray(samples).reshape(-1)
    is_f32 = x.dtype != np.int16
    x = np.ascontiguousarray(x, dtype=np.float32 if is_f32 else np.int16)
    s16 = flac.quantize(x) if is_f32 else x
    with _held(FlacEncoder, device, None) as fe:
        fe.reset_slots([0], [sample_rate], [FLAC_F32 if is_f32 else FLAC_S16])
        last = torch.ones(1, dtype=torch.int32, device=device)
        if is_f32:
            frames = _whole_row(fe, x, lambda row, n, out, sizes: fe.chunk(1, out, sizes, pcm=row, n_in=n, last=last))
        else:  # (the int16 row read as the resampler's bytes, all of it final)
            frames = _whole_row(fe, x, lambda row, n, out, sizes: fe.chunk(
                1, out, sizes, s16=row.view(torch.uint8), s16_counts=torch.tensor([[n, 0]], dtype=torch.int32, device=device), last=last))
    return flac.file_from_frames(frames, s16, sample_rate)
