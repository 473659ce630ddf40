"""An independent FLAC decoder for the tests, written from RFC 9639 (it does not use smoltts_amd.flac).

It reads the stream header (STREAMINFO, other metadata blocks skipped) and frames of either blocking strategy with independent
channels: CONSTANT, VERBATIM, FIXED and LPC subframes, wasted bits, partitioned Rice residuals with 4- and 5-bit parameters and
the escape code.  Both CRCs are verified; every frame is returned with what its header said, so tests can check the framing."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


class FlacError(ValueError):
    pass


class BitReader:
    def __init__(self, data: bytes, pos: int = 0):
        self.data, self.pos = data, pos  # pos in bits

    def u(self, n: int) -> int:
        if n == 0:
            return 0
        end = self.pos + n
        if end > 8 * len(self.data):
            raise FlacError("read past the end of the data")
        first, last = self.pos // 8, (end - 1) // 8
        v = int.from_bytes(self.data[first:last + 1], "big")
        v >>= (8 * (last + 1) - end)
        self.pos = end
        return v & ((1 << n) - 1)

    def s(self, n: int) -> int:
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self) -> int:
        q = 0
        while self.u(1) == 0:
            q += 1
        return q

    def align(self) -> None:
        self.pos = -(-self.pos // 8) * 8


@dataclass
class StreamInfo:
    min_block: int
    max_block: int
    min_frame: int
    max_frame: int
    rate: int
    channels: int
    bits: int
    total: int
    md5: bytes


@dataclass
class Frame:
    offset: int         # byte offset of the frame in the stream
    length: int         # bytes, CRC-16 included
    variable: bool      # blocking strategy bit
    number: int         # coded number: sample number (variable) or frame number (fixed)
    block_size: int
    rate: int
    bits: int
    kinds: List[str] = field(default_factory=list)  # per channel: constant / verbatim / fixed<o> / lpc<o>
    partition_orders: List[int] = field(default_factory=list)
    samples: Optional[np.ndarray] = None            # [channels, block_size] int64


@dataclass
class Decoded:
    info: StreamInfo
    frames: List[Frame]
    samples: np.ndarray  # [channels, total] int64


RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


def read_utf8(br: BitReader) -> int:
    b0 = br.u(8)
    if b0 < 0x80:
        return b0
    n = 0
    while n < 8 and b0 & (0x80 >> n):
        n += 1
    if n == 1 or n > 7:
        raise FlacError(f"bad coded-number lead byte {b0:#x}")
    v = b0 & ((1 << (7 - n)) - 1) if n < 7 else 0
    for _ in range(n - 1):
        c = br.u(8)
        if c >> 6 != 2:
            raise FlacError("bad coded-number continuation byte")
        v = (v << 6) | (c & 0x3F)
    return v


def parse_streaminfo(body: bytes) -> StreamInfo:
    br = BitReader(body)
    return StreamInfo(min_block=br.u(16), max_block=br.u(16), min_frame=br.u(24), max_frame=br.u(24), rate=br.u(20),
                      channels=br.u(3) + 1, bits=br.u(5) + 1, total=br.u(36), md5=bytes(body[18:34]))


def residual(br: BitReader, n: int, order: int) -> List[int]:
    method = br.u(2)
    if method > 1:
        raise FlacError(f"reserved residual coding method {method}")
    pbits, esc = (4, 15) if method == 0 else (5, 31)
    porder = br.u(4)
    if n % (1 << porder):
        raise FlacError("block size not divisible by the partition count")
    s = n >> porder
    if s <= order and porder > 0 or s < order:
        raise FlacError("partition shorter than the predictor order")
    out = []
    for q in range(1 << porder):
        cnt = s - order if q == 0 else s
        k = br.u(pbits)
        if k == esc:
            w = br.u(5)
            out.extend(br.s(w) if w else 0 for _ in range(cnt))
            continue
        for _ in range(cnt):
            u = (br.unary() << k) | br.u(k)
            out.append((u >> 1) ^ -(u & 1))
    return out, porder


FIXED = ([], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1])


def subframe(br: BitReader, n: int, bits: int, fr: Frame) -> np.ndarray:
    if br.u(1):
        raise FlacError("subframe padding bit set")
    t = br.u(6)
    wasted = 0
    if br.u(1):
        wasted = br.unary() + 1
    bits -= wasted
    porder = -1
    if t == 0:
        fr.kinds.append("constant")
        x = [br.s(bits)] * n
    elif t == 1:
        fr.kinds.append("verbatim")
        x = [br.s(bits) for _ in range(n)]
    elif 8 <= t <= 12:
        o = t - 8
        fr.kinds.append(f"fixed{o}")
        x = [br.s(bits) for _ in range(o)]
        res, porder = residual(br, n, o)
        for r in res:
            x.append(r + sum(c * x[-1 - j] for j, c in enumerate(FIXED[o])))
    elif t >= 32:
        o = t - 31
        fr.kinds.append(f"lpc{o}")
        x = [br.s(bits) for _ in range(o)]
        prec = br.u(4) + 1
        if prec == 16:
            raise FlacError("invalid LPC precision")
        shift = br.s(5)
        if shift < 0:
            raise FlacError("negative LPC shift")
        coefs = [br.s(prec) for _ in range(o)]
        res, porder = residual(br, n, o)
        for r in res:
            x.append(r + (sum(c * x[-1 - j] for j, c in enumerate(coefs)) >> shift))
    else:
        raise FlacError(f"reserved subframe type {t}")
    fr.partition_orders.append(porder)
    return np.asarray(x, dtype=np.int64) << wasted


def decode_frame(data: bytes, off: int, info: Optional[StreamInfo]) -> Frame:
    br = BitReader(data, 8 * off)
    sync = br.u(15)
    if sync != 0x7FFC:
        raise FlacError(f"no frame sync at byte {off}")
    variable = bool(br.u(1))
    bcode, rcode = br.u(4), br.u(4)
    chan, scode = br.u(4), br.u(3)
    if br.u(1):
        raise FlacError("reserved header bit set")
    number = read_utf8(br)
    if bcode == 0:
        raise FlacError("reserved block size code")
    elif bcode == 1:
        n = 192
    elif bcode <= 5:
        n = 576 << (bcode - 2)
    elif bcode == 6:
        n = br.u(8) + 1
    elif bcode == 7:
        n = br.u(16) + 1
    else:
        n = 256 << (bcode - 8)
    if rcode == 0:
        rate = info.rate if info else 0
    elif rcode == 12:
        rate = br.u(8) * 1000
    elif rcode == 13:
        rate = br.u(16)
    elif rcode == 14:
        rate = br.u(16) * 10
    elif rcode == 15:
        raise FlacError("forbidden sample rate code")
    else:
        rate = RATES[rcode]
    bits = info.bits if scode == 0 and info else SIZES.get(scode)
    if bits is None:
        raise FlacError("reserved sample size code")
    hend = br.pos // 8
    if crc8(data[off:hend]) != br.u(8):
        raise FlacError(f"header CRC-8 mismatch at byte {off}")
    if chan > 7:
        raise FlacError("only independent channels are supported")
    fr = Frame(offset=off, length=0, variable=variable, number=number, block_size=n, rate=rate, bits=bits)
    chans = [subframe(br, n, bits, fr) for _ in range(chan + 1)]
    br.align()
    end = br.pos // 8
    want = br.u(16)
    if crc16(data[off:end]) != want:
        raise FlacError(f"frame CRC-16 mismatch at byte {off}")
    fr.length = end + 2 - off
    fr.samples = np.stack(chans)
    return fr


def decode(data: bytes) -> Decoded:
    """A whole FLAC stream: header, then frames to the end of ``data``."""
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    off, info = 4, None
    while True:
        hdr = data[off:off + 4]
        if len(hdr) < 4:
            raise FlacError("truncated metadata")
        last, typ, length = hdr[0] >> 7, hdr[0] & 0x7F, int.from_bytes(hdr[1:4], "big")
        if typ == 0:
            if length != 34:
                raise FlacError("STREAMINFO must be 34 bytes")
            info = parse_streaminfo(data[off + 4:off + 38])
        off += 4 + length
        if last:
            break
    if info is None:
        raise FlacError("no STREAMINFO")
    frames = []
    while off < len(data):
        fr = decode_frame(data, off, info)
        frames.append(fr)
        off += fr.length
    samples = np.concatenate([f.samples for f in frames], axis=1) if frames else np.zeros((info.channels, 0), np.int64)
    return Decoded(info, frames, samples)


def decode_mono16(data: bytes) -> np.ndarray:
    """The samples of a mono 16-bit stream as int16, after checking the framing the project promises: variable blocking with
    contiguous sample numbers, 16 bits, mono."""
    d = decode(data)
    assert d.info.channels == 1 and d.info.bits == 16
    at = 0
    for f in d.frames:
        assert f.variable and f.number == at and f.bits == 16 and f.rate == d.info.rate
        at += f.block_size
    return d.samples[0].astype(np.int16)
