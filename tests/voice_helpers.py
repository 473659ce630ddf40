"""Stand-ins for the cloned-voice tests without a GPU: a pool worker scheduler that keeps a voice registry, and WAV writers.
Module-level so that worker processes can import it."""
import os
import struct

import numpy as np

from pool_helpers import EchoScheduler, _Req


class VoiceEchoScheduler(EchoScheduler):
    """EchoScheduler with a voice registry: a request yields len(text) chunks [device, chunk index, voice known?, positions]."""

    def __init__(self, delay: float = 0.0):
        super().__init__(delay)
        self.voices = {}
        self.encoded = 0

    def encode_speaker(self, samples, system_prompt=None):
        self.encoded += 1
        if any(not s.get("text") for s in samples):
            raise ValueError("Sample must contain both 'text' and 'audio'")
        n = sum(int(np.asarray(s["audio"]).size) for s in samples)
        return np.full((9, 3 + n % 5), 7, np.int32)  # a grid whose length depends on the audio

    def add_voice(self, voice_id, samples=None, grid=None, system_prompt=None, name=None):
        if grid is None:
            grid = self.encode_speaker(samples, system_prompt)
        self.voices[voice_id] = np.asarray(grid)
        return {"voice_id": voice_id, "prompt_positions": int(grid.shape[1])}

    def remove_voice(self, voice_id):
        del self.voices[voice_id]

    def submit(self, text, voice="heart", stream=False, max_new_tokens=None, **kw):
        if text == "__die__" or text == "__cancels__" or text == "__raise__":
            return super().submit(text, voice, stream, max_new_tokens)
        r = _Req()
        known = voice in self.voices
        P = int(self.voices[voice].shape[1]) if known else 0
        for i in range(len(text)):
            r.out.put(np.array([float(self.device), i, float(known), P], np.float32))
        r.out.put(None)
        return r


def make_voice_echo(delay: float = 0.0):
    return VoiceEchoScheduler(delay)


def wav_bytes(samples: np.ndarray, rate: int, kind: str = "pcm16", extensible: bool = False) -> bytes:
    """RIFF WAV of ``samples`` ((n,) or (n, channels)) as 16-bit PCM or 32-bit float, plain or WAVE_FORMAT_EXTENSIBLE."""
    x = np.asarray(samples)
    if x.ndim == 1:
        x = x[:, None]
    ch = x.shape[1]
    if kind == "pcm16":
        code, bits, data = 1, 16, x.astype("<i2").tobytes()
    else:
        code, bits, data = 3, 32, x.astype("<f4").tobytes()
    block = ch * bits // 8
    if extensible:
        guid = struct.pack("<H", code) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * block, block, bits, 22, bits, 0) + guid
    else:
        fmt = struct.pack("<HHIIHH", code, ch, rate, rate * block, block, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 4) + b"INFO" + \
        b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body
