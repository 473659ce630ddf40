"""Device plumbing shared by the engine modules: PyTorch-ROCm is used only as a container for device memory and streams."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .abi import SmolttsError


def _require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise SmolttsError("no HIP device visible; smoltts_amd runs on MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


_UPLOAD_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def upload_stream(device: torch.device) -> "torch.cuda.Stream":
    """The side stream of ``upload`` for this device, created (and the pinned allocator warmed) on first use; engines call
    this when they are built so that no request pays for it."""
    up = _UPLOAD_STREAMS.get(device.index)
    if up is None:
        up = _UPLOAD_STREAMS[device.index] = torch.cuda.Stream(device)
        # torch caches pinned blocks per power-of-two size class, and the first block of a class costs a hipHostMalloc (ms):
        # take a few of every class up to 1 MiB now
        warm = [[torch.empty(1 << k, dtype=torch.uint8).pin_memory() for _ in range(4)] for k in range(8, 21)]
        # ... and put one copy and one event through the stream: its hardware queue is only created by the first submission
        with torch.cuda.stream(up):
            warm[0][0].to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(up)
        torch.cuda.current_stream(device).wait_event(ev)
        up.synchronize()
        del warm
    return up


def upload(arrays: Sequence[np.ndarray], device: torch.device) -> List[torch.Tensor]:
    """Host arrays -> device tensors usable on the current stream, without waiting for the work already queued on it.
    A plain ``tensor.to(device)`` from pageable memory is stream-ordered *and* blocks the host, i.e. it waits for everything
    the stream still has to do (a serving loop has a tick of frame graphs pending there); here the copies leave pinned memory on
    a side stream that is otherwise idle, and the current stream merely waits for their event."""
    cur = torch.cuda.current_stream(device)
    up = upload_stream(device)
    outs = []
    with torch.cuda.stream(up):
        for a in arrays:
            t = torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)
            t.record_stream(cur)  # allocated under the side stream, consumed on the current one
            outs.append(t)
        ev = torch.cuda.Event()
        ev.record(up)
    cur.wait_event(ev)
    return outs


def current_stream_ptr() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def dptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


def _alloc_slab(nbytes: int, device, settle: bool = False) -> torch.Tensor:
    """A zeroed, 256-byte aligned slab.  The zero fill is queued on the current stream.  ``settle``: wait for it here -- for a slab
    that a C create call then initialises with plain hipMemcpy / hipMemset / a null-stream kernel, which are not ordered against
    a non-blocking current stream (a serving thread's frame stream with ticks queued) and would otherwise be overwritten by a
    late zero fill."""
    slab = torch.zeros(nbytes + 256, dtype=torch.uint8, device=device)
    if settle:
        torch.cuda.current_stream(device).synchronize()
    shift = (-slab.data_ptr()) % 256
    return slab[shift: shift + nbytes]


class ClosesOnDel:
    """Base of the objects that own a C handle: ``close()`` when collected, whatever it raises."""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
