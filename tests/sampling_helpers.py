"""A stand-in scheduler for the CPU test of the pool's sampling message: it answers every request with what it received.
Module-level so that worker processes can import it."""
import os
import queue

import numpy as np


class RecordingScheduler:
    """Chunk 0: [device, temperature, fast_temperature, min_p, 0]; chunk 1: [seed >> 32, seed & 0xffffffff] (float64 rows).
    A request without sampling answers -1 in the fields."""

    def __init__(self):
        self.device = os.environ.get("HIP_VISIBLE_DEVICES", "?")

    def submit(self, text, voice="heart", stream=False, max_new_tokens=None, sampling=None):
        q = queue.Queue()
        if sampling is None:
            q.put(np.array([float(self.device), -1, -1, -1, 0], np.float64))
            q.put(np.array([-1, -1], np.float64))
        else:
            seed = -1 if sampling.seed is None else int(sampling.seed)
            vals = [-1.0 if v is None else float(v) for v in (sampling.temperature, sampling.fast_temperature, sampling.min_p)]
            q.put(np.array([float(self.device), *vals, 0], np.float64))
            q.put(np.array([seed >> 32, seed & 0xFFFFFFFF] if seed >= 0 else [-1, -1], np.float64))
        q.put(None)
        return q

    def iter_chunks(self, q):
        while True:
            item = q.get()
            if item is None:
                return
            yield item

    def cancel(self, q):
        pass

    def close(self, drain=False):
        pass


def make_recorder():
    return RecordingScheduler()
