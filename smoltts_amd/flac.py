"""FLAC framing of streamed speech: the bitstream contract and its numpy model, the parity oracle of ``csrc/flac.hip``.

RFC 9639, inside the streamable subset: mono, 16 bits per sample, no wasted bits, no LPC subframes.  Every decision is an
integer function of the int16 samples, so the kernel writes the same bytes as this model.

- Frames use the variable-blocksize strategy (sync 0xFFF9): the coded number is the sample number of the block's first sample.
- A subframe is CONSTANT (only when every sample is equal), FIXED of order 0..min(4, n - 1) with a partitioned Rice residual
  (coding method 00, partition order p in 0..8 with n % 2^p == 0 and (n >> p) > order, one parameter k in 0..14 per partition
  minimising 4 + sum((u >> k) + 1 + k), u the zigzag of the residual), or VERBATIM: the fewest bits win, ties in that order
  (and to the smaller k, then the smaller p).
- A stream slot holds back at most 15 samples: with 16 or more pending (or at its last call, with any pending) it emits all of
  them as ceil(P / 4096) blocks sized as evenly as possible, the first P mod m one sample longer.
"""
from __future__ import annotations

import hashlib
from typing import List, Optional, Tuple

import numpy as np

MIN_BLOCK, MAX_BLOCK, HOLD = 16, 4096, 15
RATE_CODES = {8000: 0b0100, 16000: 0b0101, 22050: 0b0110, 24000: 0b0111, 44100: 0b1001, 48000: 0b1010}
BLOCK_CODES = {192: 0b0001, 576: 0b0010, 1152: 0b0011, 2304: 0b0100, 256: 0b1000, 512: 0b1001, 1024: 0b1010, 2048: 0b1011,
               4096: 0b1100}
FIXED_COEFS = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))  # prediction of x[i] from x[i-1], x[i-2], ...


def crc8(data: bytes) -> int:
    """CRC-8 of the frame header: polynomial 0x07, init 0."""
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(data: bytes) -> int:
    """CRC-16 of a frame: polynomial 0x8005, init 0."""
    crc = 0
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ _CRC16[(crc >> 8) ^ b]
    return crc


def coded_number(v: int) -> bytes:
    """The UTF-8-like code of a frame's sample number (up to 36 bits)."""
    if v < 0x80:
        return bytes([v])
    for nbytes, limit in ((2, 1 << 11), (3, 1 << 16), (4, 1 << 21), (5, 1 << 26), (6, 1 << 31), (7, 1 << 36)):
        if v < limit:
            break
    else:
        raise ValueError(f"sample number {v} needs more than 36 bits")
    out = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(nbytes - 1)][::-1]
    lead = (0xFF << (8 - nbytes)) & 0xFF if nbytes < 7 else 0xFE
    return bytes([lead | (v >> (6 * (nbytes - 1)))] + out)


def streaminfo(rate: int, min_block: int = MIN_BLOCK, max_block: int = MAX_BLOCK, min_frame: int = 0, max_frame: int = 0,
               total: int = 0, md5: bytes = bytes(16)) -> bytes:
    """The 34-byte STREAMINFO body: mono, 16 bits; zeros stand for unknown frame sizes, total and MD5."""
    v = min_block << 16 | max_block
    v = v << 24 | min_frame
    v = v << 24 | max_frame
    v = v << 20 | rate
    v = v << 3 | 0          # channels - 1
    v = v << 5 | 15         # bits per sample - 1
    v = v << 36 | total
    return v.to_bytes(18, "big") + bytes(md5)


def stream_header(rate: int, info: Optional[bytes] = None) -> bytes:
    """``fLaC`` and one STREAMINFO block with the last-metadata-block flag set (``info``: its body; default a stream's)."""
    if rate not in RATE_CODES:
        raise ValueError(f"FLAC framing supports the rates {sorted(RATE_CODES)}, not {rate}")
    info = streaminfo(rate) if info is None else info
    return b"fLaC" + bytes([0x80, 0, 0, len(info)]) + info


class _Bits:
    """Big-endian bit writer (whole bytes leave the accumulator as soon as they are complete)."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value: int, width: int) -> None:
        self.acc = (self.acc << width) | (value & ((1 << width) - 1))
        self.n += width
        if self.n >= 64:
            whole = self.n // 8 * 8
            self.out += (self.acc >> (self.n - whole)).to_bytes(whole // 8, "big")
            self.n -= whole
            self.acc &= (1 << self.n) - 1

    def bytes(self) -> bytes:
        pad = -self.n % 8
        return bytes(self.out) + (self.acc << pad).to_bytes((self.n + pad) // 8, "big")


def residual(x: np.ndarray, order: int) -> np.ndarray:
    """FIXED residual of ``order`` for samples [order, n) (int64)."""
    x = x.astype(np.int64)
    r = x[order:].copy()
    for j, c in enumerate(FIXED_COEFS[order]):
        r -= c * x[order - 1 - j: len(x) - 1 - j]
    return r


def _rice_plan(u: np.ndarray, n: int, order: int) -> Tuple[int, int, List[int]]:
    """(bits of the residual section after its 6-bit header, p, [k per partition]) of the cheapest partition order."""
    best = None
    cs = np.concatenate([np.zeros((1, 15), np.int64), np.cumsum(u[:, None] >> np.arange(15)[None, :], axis=0)])  # cs[i, k] = sum_{j<i} u[j] >> k
    for p in range(9):
        if n % (1 << p) or (n >> p) <= order:
            break
        s = n >> p
        bits, ks = 0, []
        for q in range(1 << p):
            lo, hi = max(q * s - order, 0), (q + 1) * s - order
            sums = cs[hi] - cs[lo]
            cnt = hi - lo
            costs = [4 + cnt * (k + 1) + int(sums[k]) for k in range(15)]
            k = int(np.argmin(costs))
            bits += costs[k]
            ks.append(k)
        if best is None or bits < best[0]:
            best = (bits, p, ks)
    return best


def encode_frame(x: np.ndarray, first_sample: int, rate: int) -> bytes:
    """One frame of int16 samples ``x`` (1 to 4096) whose first sample has number ``first_sample``."""
    x = np.asarray(x, dtype=np.int16)
    n = int(x.size)
    assert 1 <= n <= MAX_BLOCK
    if n in BLOCK_CODES:
        bcode, bext = BLOCK_CODES[n], b""
    elif n <= 256:
        bcode, bext = 0b0110, bytes([n - 1])
    else:
        bcode, bext = 0b0111, (n - 1).to_bytes(2, "big")
    head = bytes([0xFF, 0xF9, bcode << 4 | RATE_CODES[rate], 0b0000_100_0]) + coded_number(first_sample) + bext
    head += bytes([crc8(head)])
    # candidates: (bits, rank, kind)
    xi = x.astype(np.int64)
    cands = []
    if np.all(xi == xi[0]):
        cands.append((8 + 16, 0, ("const",)))
    for o in range(min(4, n - 1) + 1):
        r = residual(x, o)
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        bits, p, ks = _rice_plan(u, n, o)
        cands.append((8 + 16 * o + 6 + bits, 1 + o, ("fixed", o, p, ks, u)))
    cands.append((8 + 16 * n, 6, ("verbatim",)))
    kind = min(cands, key=lambda c: (c[0], c[1]))[2]
    b = _Bits()
    for byte in head:
        b.put(byte, 8)
    if kind[0] == "const":
        b.put(0b000000 << 1, 8)
        b.put(int(xi[0]), 16)
    elif kind[0] == "verbatim":
        b.put(0b000001 << 1, 8)
        for v in xi:
            b.put(int(v), 16)
    else:
        _, o, p, ks, u = kind
        b.put((0b001000 | o) << 1, 8)
        for v in xi[:o]:
            b.put(int(v), 16)
        b.put(0, 2)
        b.put(p, 4)
        s = n >> p
        for q, k in enumerate(ks):
            b.put(k, 4)
            for uu in u[max(q * s - o, 0): (q + 1) * s - o]:
                uu = int(uu)
                b.put(1, (uu >> k) + 1)
                b.put(uu, k)
    frame = b.bytes()
    return frame + crc16(frame).to_bytes(2, "big")


def block_sizes(pending: int, last: bool) -> List[int]:
    """Sizes of the blocks a slot with ``pending`` samples emits (empty: it holds them)."""
    if pending >= MIN_BLOCK or (last and pending > 0):
        m = -(-pending // MAX_BLOCK)
        base, extra = divmod(pending, m)
        return [base + 1] * extra + [base] * (m - extra)
    return []


class StreamEncoder:
    """The per-slot state machine of a FLAC stream: ``feed(s16, last)`` -> the bytes of the frames this call completes (the stream
    header is not included: ``stream_header``)."""

    def __init__(self, rate: int):
        if rate not in RATE_CODES:
            raise ValueError(f"FLAC framing supports the rates {sorted(RATE_CODES)}, not {rate}")
        self.rate, self.pos = rate, 0
        self.pending = np.zeros(0, np.int16)

    def feed(self, s16: np.ndarray, last: bool = False) -> bytes:
        return b"".join(self.feed_frames(s16, last))

    def feed_frames(self, s16: np.ndarray, last: bool = False) -> List[bytes]:
        """``feed``, one bytes object per frame."""
        x = np.concatenate([self.pending, np.asarray(s16, dtype=np.int16).reshape(-1)])
        sizes = block_sizes(int(x.size), last)
        if not sizes:
            self.pending = x
            return []
        out, at = [], 0
        for n in sizes:
            out.append(encode_frame(x[at:at + n], self.pos + at, self.rate))
            at += n
        self.pos += at
        self.pending = np.zeros(0, np.int16)
        return out


def quantize(pcm: np.ndarray) -> np.ndarray:
    """float32 PCM -> int16 codes: rint(clip(x, -1, 1) * 32767) (the blocking route's and tsm.py's rule)."""
    return np.rint(np.clip(np.asarray(pcm, dtype=np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)


def encode_file(s16: np.ndarray, rate: int) -> bytes:
    """A whole FLAC file of int16 samples in one call: the stream's frames behind a STREAMINFO with the true total, minimum and
    maximum frame size and the MD5 of the samples as little-endian int16."""
    s16 = np.asarray(s16, dtype=np.int16).reshape(-1)
    return file_from_frames(StreamEncoder(rate).feed_frames(s16, last=True), s16, rate)


def file_from_frames(frames: List[bytes], s16: np.ndarray, rate: int) -> bytes:
    """The file of a one-call stream's ``frames`` (bytes each) of the samples ``s16``: STREAMINFO filled in."""
    sizes = [len(f) for f in frames]
    info = streaminfo(rate, min_block=MIN_BLOCK, max_block=MAX_BLOCK, min_frame=min(sizes, default=0),
                      max_frame=max(sizes, default=0), total=int(s16.size),
                      md5=hashlib.md5(np.asarray(s16, dtype="<i2").tobytes()).digest())
    return stream_header(rate, info) + b"".join(frames)
