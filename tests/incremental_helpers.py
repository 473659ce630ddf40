"""Stand-ins for the CPU tests of text fed in pieces: a model whose ``stream`` takes an iterator of text (module-level, so that
the pool's worker processes can import the scheduler)."""
import queue
import threading

import numpy as np


class PullingTTS:
    """``stream(text_iter)`` yields one chunk per piece of text it pulls: 4 float32 samples [pieces so far, len(piece), 0 or 1 for
    a flush mark, 0]; it records the call's keyword arguments."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []

    def stream(self, text, voice="heart", **kw):
        from smoltts_amd.longform import FLUSH

        self.calls.append({"voice": voice, **kw})
        assert not isinstance(text, str)
        for i, piece in enumerate(text):
            flush = piece is FLUSH
            if not flush and "<break time=\"9s\"" in piece:
                raise ValueError("break time outside [0, 3] s")
            yield np.array([i + 1, 0 if flush else len(piece), float(flush), 0], np.float32)


class _Req:
    def __init__(self):
        self.out = queue.Queue()
        self.cancelled = False
        self.log = []

    def _say(self, what, n=0):
        self.log.append(what)
        self.out.put(np.array([len(self.log), n], np.float32))

    def feed(self, text):
        if "__bad__" in text:
            raise ValueError("bad break tag")
        self._say("feed", len(text))

    def flush(self):
        self._say("flush")

    def close(self):
        self._say("close")
        self.out.put(None)


class EchoIncrementalScheduler:
    """``submit_incremental`` answers every text call with a chunk [calls so far, len(text)]; ``close`` ends the stream, ``cancel``
    ends it with a chunk [-1, -1] in front."""

    def submit_incremental(self, voice="heart", max_new_tokens=None, **kw):
        r = _Req()
        r.out.put(np.array([len(voice), len(kw)], np.float32))
        return r

    def iter_chunks(self, r):
        while True:
            item = r.out.get()
            if item is None:
                return
            if isinstance(item, Exception):
                raise item
            yield item

    def cancel(self, r):
        r.cancelled = True
        r.out.put(np.array([-1, -1], np.float32))
        r.out.put(None)

    def close(self):
        pass


def make_echo_incremental():
    return EchoIncrementalScheduler()
