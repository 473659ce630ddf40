"""Output formats of the streaming transport (host side): the format parser and the host mu-law.

A streamed ``output_format`` is ``pcm_<rate>`` (16-bit little-endian PCM) at 8000 / 16000 / 22050 / 44100 / 48000 Hz or
``ulaw_8000`` (G.711 mu-law); ``pcm_24000`` is the codec's own float32 stream and is not converted.  The conversion of streamed
chunks runs on the GPU (``stages.Resampler``, csrc/resample.hip); the host mu-law here serves the blocking route, which
resamples whole signals on the host.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .abi import RESAMPLE_OFF as ENC_OFF, RESAMPLE_S16 as ENC_S16, RESAMPLE_ULAW as ENC_ULAW

STREAM_RATES = (8000, 16000, 22050, 44100, 48000)
STREAM_FORMATS = tuple(f"pcm_{r}" for r in STREAM_RATES) + ("ulaw_8000",)
NATIVE_FORMAT = "pcm_24000"


def parse_stream_format(fmt: str) -> Tuple[int, int]:
    """``"pcm_16000"`` -> (16000, ENC_S16), ``"ulaw_8000"`` -> (8000, ENC_ULAW), ``"pcm_24000"`` -> (24000, ENC_OFF)."""
    if fmt == NATIVE_FORMAT:
        return 24000, ENC_OFF
    if fmt in STREAM_FORMATS:
        kind, rate = fmt.split("_")
        return int(rate), ENC_ULAW if kind == "ulaw" else ENC_S16
    raise ValueError(f"unsupported stream output_format {fmt!r}: supported are {', '.join((NATIVE_FORMAT,) + STREAM_FORMATS)}")


CONTAINERS = ("flac",)


def check_container(container, output_format=None):
    """A stream's ``container`` (None, or ``"flac"``: lossless FLAC framing of its 16-bit samples, flac.py) for ``output_format``
    (None / ``pcm_<rate>``; FLAC frames PCM only).  Returns it; ``ValueError`` for anything else."""
    if container is None:
        return None
    if container not in CONTAINERS:
        raise ValueError(f"unsupported container {container!r}: supported are {', '.join(CONTAINERS)}")
    if output_format is not None and parse_stream_format(output_format)[1] == ENC_ULAW:
        raise ValueError(f"container {container!r} frames 16-bit PCM, not {output_format}")
    return container


def lin2ulaw(s16: np.ndarray) -> np.ndarray:
    """G.711 mu-law of 16-bit samples: Sun's ``linear2ulaw`` on the full 16-bit value (bias 0x84, clip 32635), no 14-bit cut."""
    s = np.asarray(s16, dtype=np.int32)
    mag = np.minimum(np.abs(s), 32635) + 0x84
    seg = np.frexp(mag)[1].astype(np.int32) - 8  # floor(log2(mag)) - 7
    mant = (mag >> (seg + 3)) & 0xF
    sign = np.where(s < 0, 0x80, 0)
    return (~(sign | (seg << 4) | mant) & 0xFF).astype(np.uint8)
