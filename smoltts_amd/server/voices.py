"""Uploaded voice samples: RIFF WAV decoding and the resampling to the codec's 24 kHz, on the host (a one-off cost per voice, not a
request path).  Used by ``POST /v1/voices/add`` (app.py), which takes JSON with base64 WAV since the image has no multipart parser."""
from __future__ import annotations

import base64
import binascii
import secrets
import struct
from math import gcd
from typing import Tuple

import numpy as np

ACCEPTED_RATES = (8000, 16000, 22050, 24000, 44100, 48000)
CODEC_RATE = 24000
WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 1, 3, 0xFFFE


def new_voice_id() -> str:
    """``cv_`` + 20 hex digits: never a preset name, never a numeric string."""
    return "cv_" + secrets.token_hex(10)


def parse_wav(data: bytes) -> Tuple[np.ndarray, int]:
    """RIFF WAV bytes -> (float64 mono samples in [-1, 1), sample rate).  16-bit integer PCM (format 1) or 32-bit float (format 3),
    either also inside WAVE_FORMAT_EXTENSIBLE; any channel count, averaged.  ``ValueError`` for anything else."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    fmt = None
    pcm = None
    off = 12
    while off + 8 <= len(data):
        cid, size = data[off: off + 4], struct.unpack("<I", data[off + 4: off + 8])[0]
        body = data[off + 8: off + 8 + size]
        if len(body) < size and cid != b"data":
            raise ValueError(f"truncated {cid!r} chunk")
        if cid == b"fmt ":
            if size < 16:
                raise ValueError("fmt chunk too short")
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == WAVE_FORMAT_EXTENSIBLE:
                if size < 40:
                    raise ValueError("WAVE_FORMAT_EXTENSIBLE fmt chunk too short")
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]  # the sub-format GUID starts with the format code
        elif cid == b"data":
            pcm = body
            break
        off += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError("WAV without fmt or data chunk")
    code, channels, rate, _, block_align, bits = fmt
    if channels < 1:
        raise ValueError("WAV with no channels")
    if code == WAVE_FORMAT_PCM and bits == 16:
        dtype, scale = np.dtype("<i2"), 1.0 / 32768.0
    elif code == WAVE_FORMAT_IEEE_FLOAT and bits == 32:
        dtype, scale = np.dtype("<f4"), 1.0
    else:
        raise ValueError(f"unsupported WAV sample format {code} with {bits} bits (16-bit PCM or 32-bit float)")
    if block_align != channels * dtype.itemsize:
        raise ValueError("WAV block alignment does not match its format")
    if rate not in ACCEPTED_RATES:
        raise ValueError(f"unsupported sample rate {rate} Hz (one of {', '.join(map(str, ACCEPTED_RATES))})")
    n = len(pcm) // block_align
    if n == 0:
        raise ValueError("WAV without samples")
    x = np.frombuffer(pcm[: n * block_align], dtype=dtype).astype(np.float64).reshape(n, channels) * scale
    x = x.mean(axis=1)
    if not np.all(np.isfinite(x)):
        raise ValueError("WAV samples are not finite")
    return x, int(rate)


def to_codec_rate(x: np.ndarray, rate: int) -> np.ndarray:
    """Mono samples at ``rate`` -> float32 at 24 kHz: ``scipy.signal.resample_poly`` (default filter, float64)."""
    if rate != CODEC_RATE:
        from scipy.signal import resample_poly

        g = gcd(CODEC_RATE, rate)
        x = resample_poly(np.asarray(x, np.float64), CODEC_RATE // g, rate // g)
    return np.asarray(x, dtype=np.float32)


def decode_sample_audio(b64: str) -> np.ndarray:
    """A sample's base64 WAV -> float32 PCM at 24 kHz (``ValueError`` for malformed input)."""
    try:
        data = base64.b64decode(b64, validate=True)
    except (binascii.Error, ValueError, TypeError) as e:
        raise ValueError(f"audio is not valid base64: {e}") from None
    return to_codec_rate(*parse_wav(data))
