"""Request-level data parallelism for serving: one worker *process* per GPU behind one front-end.

Utterances share no state, so a node's GPUs are N independent replicas: every worker process sees exactly one GPU
(``HIP_VISIBLE_DEVICES``), loads its own copy of the weights, and runs its own ``BatchScheduler``; the front-end hands
each request to the worker with the fewest requests in flight and relays the audio.  There is no exchange between the
workers — nothing a collective could carry — and the front-end never touches a GPU.  ``GpuPool`` has the client
interface of ``BatchScheduler`` (submit / synthesize / iter_chunks / cancel / close), so the HTTP handlers do not care
which of the two they talk to.

The reference serves from a single process and a single device (server.py:48-59); this is the part of the scaling story
that the single Python host would otherwise cap.
"""
from __future__ import annotations

import itertools
import multiprocessing as mp
import os
import queue
import threading
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np


@dataclass
class _PoolRequest:
    rid: int
    worker: int
    out: "queue.Queue" = field(default_factory=queue.Queue)  # np.ndarray chunks, then None (or an Exception)
    cancelled: bool = False
    closed: bool = False
    sampling: object = None  # config.RequestSampling as sent to the worker (seed resolved here), or None
    loudness_gain_db: Optional[float] = None  # a blocking request with a loudness: the gain applied (known at its end)
    trimmed_s: float = 0.0  # a blocking request that trims silence: the seconds cut (known at its end)
    watermark: bool = False  # the audio carries the workers' watermark
    finish_reason: Optional[str] = None  # "stop" / "length" (config.finish_reason), known at the request's end
    # scores of a request that asked for them (RequestSampling.logprobs / best_of), known at its end; all takes of a best_of
    # request run on the one worker the request went to, and ``sampling`` then carries the winner's seed
    logprobs: object = None
    mean_logprob: Optional[float] = None
    takes: object = None
    best_of: int = 1
    alignment: object = None  # align.Alignment of a request that asked for timestamps, known at its end
    peak_reduction_db: Optional[float] = None  # a blocking request with a peak_limit_db: -20 log10(min g) (known at its end)


# what a worker reports at a request's end, by ``_PoolRequest`` attribute, with the value of a request that has none
END_REPORT = {"loudness_gain_db": None, "trimmed_s": 0.0, "finish_reason": None, "alignment": None, "peak_reduction_db": None}


@dataclass
class _PoolIncrementalRequest(_PoolRequest):
    """``GpuPool.submit_incremental``'s handle: the text calls travel to the worker that owns the request, in order."""
    pool: object = None

    def feed(self, text) -> None:
        self.pool._inc(self, "feed", text)

    def flush(self) -> None:
        self.pool._inc(self, "flush")

    def close(self) -> None:
        self.pool._inc(self, "close")

    def cancel(self) -> None:
        self.pool.cancel(self)

    def __iter__(self):
        return self.pool.iter_chunks(self)


def visible_device(index: int, inherited: Optional[str]) -> str:
    """The ``HIP_VISIBLE_DEVICES`` value of the worker for GPU ``index``: an entry of the mask this process runs under, if
    there is one (indices are relative to it), else the index itself."""
    if inherited:
        ids = [x.strip() for x in inherited.split(",") if x.strip()]
        if index >= len(ids):
            raise ValueError(f"device {index} is outside HIP_VISIBLE_DEVICES={inherited!r}")
        return ids[index]
    return str(index)


class _Sender:
    """The worker's end of its result pipe; several pump threads share it."""

    def __init__(self, conn):
        self.conn, self.lock = conn, threading.Lock()

    def put(self, msg) -> None:
        with self.lock:
            self.conn.send(msg)


def _worker_main(device: str, factory: Callable[[], object], req_q, res_conn) -> None:
    """Worker process: build the scheduler on its GPU, then serve messages until told to close.  ``factory()`` returns an
    object with the BatchScheduler client interface (it is called here, after the device mask is in place and before
    anything has touched the GPU)."""
    os.environ["HIP_VISIBLE_DEVICES"] = device
    res_q = _Sender(res_conn)
    try:
        sched = factory()
    except BaseException as e:  # the front-end must hear about a worker that cannot start
        res_q.put((None, "fatal", f"{type(e).__name__}: {e}"))
        return
    res_q.put((None, "ready", device))
    live: Dict[int, object] = {}
    lock = threading.Lock()

    def pump(rid: int, req) -> None:
        try:
            if getattr(req, "live_timestamps", False):  # a stream with timestamps: each chunk travels with its part
                for chunk, part in sched.timed_chunks(req):
                    res_q.put((rid, "chunk", (np.ascontiguousarray(chunk), part)))
            else:
                for chunk in sched.iter_chunks(req):
                    res_q.put((rid, "chunk", np.ascontiguousarray(chunk)))  # float32, or int16 / uint8 for a streamed output_format
            scores = None
            if getattr(req, "logprobs", None) is not None:
                scores = {"logprobs": np.asarray(req.logprobs), "mean_logprob": req.mean_logprob, "takes": req.takes, "best_of": req.best_of,
                          "seed": req.sampling.seed}
            end = {k: getattr(req, k, d) for k, d in END_REPORT.items()}  # (a stand-in scheduler's request may lack some)
            res_q.put((rid, "end", dict(end, scores=scores)))
        except Exception as e:
            res_q.put((rid, "error", (type(e).__name__, str(e))))
        finally:
            with lock:
                live.pop(rid, None)

    def control(msg) -> None:  # voice registry: the scheduler call blocks until its worker thread has done the GPU part
        kind, rid = msg[:2]
        try:
            if kind == "encode_voice":
                out = sched.encode_speaker(msg[2], system_prompt=msg[3])
            elif kind == "add_voice":
                out = sched.add_voice(msg[2], grid=msg[3], name=msg[4])
            elif kind == "align_recording":
                out = sched.align_recording(msg[2], msg[3], voice=msg[4], speaker=msg[5], rate=24000)
            else:
                sched.remove_voice(msg[2])
                out = None
            res_q.put((rid, "result", out))
        except Exception as e:
            res_q.put((rid, "error", (type(e).__name__, str(e))))

    try:
        while True:
            msg = req_q.get()
            if msg[0] == "close":
                break
            if msg[0] in ("encode_voice", "add_voice", "remove_voice", "align_recording"):
                threading.Thread(target=control, args=(msg,), name=f"smoltts-voice-{msg[1]}", daemon=True).start()
                continue
            if msg[0] == "submit":
                _, rid, text, voice, stream, max_new_tokens = msg[:6]
                extra = msg[6] if len(msg) > 6 else {}  # (output_format / sampling / speed, only when set)
                try:
                    req = sched.submit(text, voice, stream=stream, max_new_tokens=max_new_tokens, **extra)
                except Exception as e:  # a refused request is that request's error; the worker goes on serving
                    res_q.put((rid, "error", (type(e).__name__, str(e))))
                    continue
                with lock:
                    live[rid] = req
                threading.Thread(target=pump, args=(rid, req), name=f"smoltts-pump-{rid}", daemon=True).start()
            elif msg[0] == "submit_incremental":
                _, rid, voice, max_new_tokens, extra = msg
                try:
                    req = sched.submit_incremental(voice, max_new_tokens=max_new_tokens, **extra)
                except Exception as e:
                    res_q.put((rid, "error", (type(e).__name__, str(e))))
                    continue
                with lock:
                    live[rid] = req
                threading.Thread(target=pump, args=(rid, req), name=f"smoltts-pump-{rid}", daemon=True).start()
            elif msg[0] in ("feed", "flush", "close_text"):
                with lock:
                    req = live.get(msg[1])
                if req is None:
                    continue
                try:
                    req.feed(msg[2]) if msg[0] == "feed" else (req.flush() if msg[0] == "flush" else req.close())
                except Exception as e:  # text the engine refuses (a bad break tag): the request ends with that error
                    res_q.put((msg[1], "error", (type(e).__name__, str(e))))
                    sched.cancel(req)
            elif msg[0] == "cancel":
                with lock:
                    req = live.get(msg[1])
                if req is not None:
                    sched.cancel(req)
    finally:
        try:
            sched.close(drain=True)  # a BatchScheduler finishes what it has accepted
        except TypeError:
            sched.close()


class GpuPool:
    def __init__(self, factory: Callable[[], object], devices: Sequence[int], start_method: str = "spawn", ready_timeout: float = 600.0,
                 respawn: bool = True, generation_settings=None, watermark=None, alignment_heads=None):
        """``factory``: picklable, called once in every worker to build its scheduler.  ``devices``: GPU indices, one
        worker each (an index may repeat: two replicas on one GPU).  ``start_method``: "spawn" or "forkserver" — never
        "fork": a forked copy of a process that has used the GPU is not usable.  ``respawn``: a worker that dies is replaced
        (same GPU); its requests in flight are failed, later ones are served again by all workers.
        ``generation_settings``: what the workers' schedulers are configured with; then every request's sampling is resolved
        here (``RequestSampling.resolve``) and sent along, so that a request samples the same on any worker.  Without it only a
        request that names a ``sampling`` carries one (its seed drawn here when missing).
        ``watermark`` (a ``watermark.Watermark``; None: none): the key the factory gives every worker's scheduler; the pool
        itself marks nothing, it decides here whether a request is marked (``BatchScheduler.submit``'s rule) and says so."""
        from ..watermark import Watermark

        if watermark is not None and not isinstance(watermark, Watermark):
            raise ValueError("watermark must be a smoltts_amd.watermark.Watermark or None")
        self.watermark = watermark
        from ..align import check_heads

        # what the workers' schedulers were built with (the factory's business): lets the front end refuse ``timestamps`` itself
        self.alignment_heads = check_heads(alignment_heads)
        if start_method not in ("spawn", "forkserver"):
            raise ValueError("start_method must be 'spawn' or 'forkserver'")
        if not devices:
            raise ValueError("no devices")
        self._ctx = mp.get_context(start_method)
        self._factory, self._ready_timeout, self._respawn = factory, ready_timeout, respawn
        self._settings = generation_settings
        inherited = os.environ.get("HIP_VISIBLE_DEVICES")
        self._devices = [visible_device(d, inherited) for d in devices]
        started = [self._start_worker(i) for i in range(len(devices))]
        self._procs = [p for p, _, _ in started]
        self._req_qs = [q for _, q, _ in started]
        self._res = [r for _, _, r in started]  # one result pipe per worker: no shared lock, EOF when a worker dies
        self._lock = threading.Lock()
        self._reqs: Dict[int, _PoolRequest] = {}
        self._load: List[int] = [0] * len(devices)
        self._dead: List[bool] = [False] * len(devices)  # set (under the lock) by a worker's dispatcher when its pipe ends
        self._restarts: List[int] = [0] * len(devices)
        self._ids = itertools.count()
        self._closing = False
        self._voices: Dict[str, tuple] = {}  # registered voice id -> (speaker grid, name): replayed to a worker that replaces a dead one
        self._voice_lock = threading.Lock()  # one registry change at a time
        for i, conn in enumerate(self._res):  # all workers up (weights loaded, kernels resident) before the first request is taken
            why = self._await_ready(conn, i)
            if why is not None:
                self._kill()
                raise RuntimeError(why)
        self._threads = [threading.Thread(target=self._dispatch, args=(i,), name=f"smoltts-pool-dispatch-{i}", daemon=True)
                         for i in range(len(devices))]
        for t in self._threads:
            t.start()

    def _start_worker(self, w: int):
        q = self._ctx.Queue()
        r, wr = self._ctx.Pipe(duplex=False)
        p = self._ctx.Process(target=_worker_main, args=(self._devices[w], self._factory, q, wr), daemon=True, name=f"smoltts-gpu-worker-{w}")
        p.start()
        wr.close()  # the worker holds the write end now
        return p, q, r

    def _await_ready(self, conn, w: int) -> Optional[str]:
        """None once worker ``w`` has reported ready, else why it did not."""
        try:
            if not conn.poll(self._ready_timeout):
                return "GPU workers did not come up in time"
            _, kind, payload = conn.recv()
        except (EOFError, OSError):
            return f"GPU worker failed to start: worker {w} exited during start-up"
        return None if kind == "ready" else f"GPU worker failed to start: {payload}"

    # ------------------------------------------------------------------ client side (the BatchScheduler interface)
    def submit(self, text: str, voice: str = "heart", stream: bool = False, max_new_tokens: Optional[int] = None,
               output_format: Optional[str] = None, sampling=None, live_timestamps: bool = False, **options) -> _PoolRequest:
        """As ``BatchScheduler.submit`` (the segments of one request run in one slot of one worker).  The options are parsed
        here, so that a bad request is refused before a worker sees it, and travel to the worker as the parsed value's own
        keywords (``SpeechOptions.given``), ``live_timestamps`` beside them; ``timed_chunks`` relays the parts with the chunks."""
        from ..request import parse_request

        p = parse_request(text, stream, output_format, **options)
        marked = self._marks(p.watermark)
        sampling = self._resolve_sampling(sampling)
        if live_timestamps:
            from ..align import check_live_timestamps

            check_live_timestamps(p, stream, bool(self.alignment_heads), 1 if sampling is None else sampling.takes)
        if p.timestamps:
            if not self.alignment_heads:
                raise ValueError("timestamps need alignment_heads: rank a checkpoint's heads with `python -m smoltts_amd.align rank`")
            if sampling is not None and sampling.takes > 1:
                raise ValueError("timestamps cannot be combined with best_of")
        if sampling is not None and sampling.takes > 1 and (stream or p.plan is not None):
            from ..config import MAX_BEST_OF, check_best_of

            check_best_of(sampling, MAX_BEST_OF, stream=stream, segmented=p.plan is not None)  # (the worker checks the rest)
        req = self._new_request(sampling)
        req.watermark = marked
        w = req.worker
        msg = ("submit", req.rid, text, voice, stream, max_new_tokens)
        extra = dict(p.given(), **({} if sampling is None else {"sampling": sampling}))
        if live_timestamps:
            extra["live_timestamps"] = True
        self._req_qs[w].put(msg + (extra,) if extra else msg)
        return req

    def submit_incremental(self, voice: str = "heart", max_new_tokens: Optional[int] = None, output_format: Optional[str] = None,
                           sampling=None, segment=True, idle_timeout_s: float = 10.0, flush_after_s: Optional[float] = None,
                           **options) -> _PoolIncrementalRequest:
        """As ``BatchScheduler.submit_incremental``: the request lives in one slot of one worker, and ``feed`` / ``flush`` /
        ``close`` / ``cancel`` of the handle go to that worker over its queue, in the order they were called.  Text the worker
        refuses (a bad break tag) ends the stream with that ``ValueError`` instead of raising from ``feed``."""
        from ..longform import segment_options
        from ..request import parse_request

        p = parse_request("", True, output_format, **options)
        opts = segment_options(True if segment is None or segment is False else segment)
        marked = self._marks(p.watermark)
        sampling = self._resolve_sampling(sampling)
        req = self._new_request(sampling, _PoolIncrementalRequest, pool=self)
        req.watermark = marked
        extra = dict(p.given(), segment=opts, idle_timeout_s=idle_timeout_s)
        if sampling is not None:
            extra["sampling"] = sampling
        if flush_after_s is not None:
            extra["flush_after_s"] = flush_after_s
        self._req_qs[req.worker].put(("submit_incremental", req.rid, voice, max_new_tokens, extra))
        return req

    def _marks(self, asked: Optional[bool]) -> bool:
        if asked and self.watermark is None:
            raise ValueError("watermark asked for, and the pool has no watermark key")
        return self.watermark is not None if asked is None else bool(asked)

    def _inc(self, req: _PoolIncrementalRequest, what: str, text=None) -> None:
        if req.closed or req.cancelled:
            if what == "feed":
                raise ValueError("the request has ended")
            return
        self._req_qs[req.worker].put(("feed", req.rid, text) if what == "feed" else ("flush" if what == "flush" else "close_text", req.rid))

    def _resolve_sampling(self, sampling):
        """A request's sampling as it travels: the seed is drawn here, the same on whichever worker serves it."""
        if sampling is not None or self._settings is not None:
            import dataclasses

            from ..config import RequestSampling

            sampling = sampling if sampling is not None else RequestSampling()
            if self._settings is not None:
                sampling = sampling.resolve(self._settings)
            elif sampling.seed is None:
                sampling = dataclasses.replace(sampling, seed=int.from_bytes(os.urandom(8), "little"))
        return sampling

    def _new_request(self, sampling, cls=_PoolRequest, **kw) -> _PoolRequest:
        """A request in the books of the worker with the fewest in flight."""
        with self._lock:
            if self._closing:
                raise RuntimeError("pool closed")
            alive = [i for i, p in enumerate(self._procs) if not self._dead[i] and p.is_alive()]
            if not alive:
                raise RuntimeError("no GPU worker is alive")
            w = min(alive, key=lambda i: self._load[i])
            req = cls(next(self._ids), w, sampling=sampling, **kw)
            self._reqs[req.rid] = req
            self._load[w] += 1
        return req

    def synthesize(self, text: str, voice: str = "heart", max_new_tokens: Optional[int] = None) -> np.ndarray:
        return np.concatenate(list(self.iter_chunks(self.submit(text, voice, False, max_new_tokens))) or [np.zeros(0, np.float32)])

    def iter_chunks(self, req: _PoolRequest):
        pairs = self.timed_chunks(req)
        try:
            for chunk, _ in pairs:
                if len(chunk):
                    yield chunk
        finally:
            pairs.close()

    def timed_chunks(self, req: _PoolRequest):
        """As ``BatchScheduler.timed_chunks``: ``(chunk, align.AlignmentPart or None)``."""
        ended = False
        try:
            while True:
                item = req.out.get()
                if item is None or isinstance(item, Exception):
                    ended = True
                    if item is None:
                        return
                    raise item
                yield item if isinstance(item, tuple) else (item, None)
        finally:
            if not ended:
                self.cancel(req)

    def cancel(self, req: _PoolRequest) -> None:
        if not req.cancelled and not req.closed:
            req.cancelled = True
            self._req_qs[req.worker].put(("cancel", req.rid))

    # ------------------------------------------------------------------ registered voices (the parent stays off the GPU)
    def add_voice(self, voice_id: str, samples=None, grid=None, system_prompt: Optional[str] = None, name: Optional[str] = None) -> dict:
        """``BatchScheduler.add_voice`` on every worker: one worker encodes ``samples`` into a speaker grid, then the grid goes
        to all of them, and the call returns once every one has acknowledged -- a request submitted afterwards finds the voice
        wherever it lands.  The grid is kept here and replayed to a worker that replaces a dead one."""
        if (samples is None) == (grid is None):
            raise ValueError("pass samples or grid")
        with self._voice_lock:
            if grid is None:
                w = self._pick_worker()
                grid = self._await_control(self._control(w, ("encode_voice", samples, system_prompt)))
            grid = np.ascontiguousarray(np.asarray(grid, dtype=np.int32))
            reqs = [self._control(w, ("add_voice", voice_id, grid, name)) for w in self._alive()]
            results = []
            try:
                for r in reqs:
                    results.append(self._await_control(r))
            except BaseException:
                for w in self._alive():  # a partial registration is taken back where it was made
                    try:
                        self._await_control(self._control(w, ("remove_voice", voice_id)))
                    except Exception:
                        pass
                raise
            self._voices[voice_id] = (grid, name)
            return results[0]

    def align_recording(self, audio, text: str, voice: str = "heart", speaker=None, rate: int = 24000):
        """``BatchScheduler.align_recording`` on the least loaded worker -> its ``align.RecordingAlignment``.  Refused here, before
        a worker sees the request (``ValueError``): a pool without ``alignment_heads``, an empty text, audio shorter than one
        frame.  The parent has no tokenizer, so a recording too long for the context behind its prompt is refused by the
        worker's scheduler, before its GPU work, and that ``ValueError`` is relayed."""
        from ..align import no_heads_error
        from .voices import to_codec_rate

        if not self.alignment_heads:
            raise no_heads_error()
        if not isinstance(text, str) or not text.strip():
            raise ValueError("forced alignment needs a text")
        pcm = to_codec_rate(np.asarray(audio, dtype=np.float64).reshape(-1), int(rate))
        if pcm.size < 1920:
            raise ValueError("the audio holds no full frame (1920 samples at 24 kHz)")
        if speaker is not None:
            speaker = np.ascontiguousarray(np.asarray(speaker, dtype=np.int32))
        return self._await_control(self._control(self._pick_worker(), ("align_recording", pcm, text, voice, speaker)))

    def remove_voice(self, voice_id: str) -> None:
        """Forget a registered voice on every worker (``KeyError`` if there is none)."""
        with self._voice_lock:
            if voice_id not in self._voices:
                raise KeyError(voice_id)
            del self._voices[voice_id]
            for r in [self._control(w, ("remove_voice", voice_id)) for w in self._alive()]:
                try:
                    self._await_control(r)
                except KeyError:
                    pass

    def voices(self) -> Dict[str, dict]:
        """Registered voices: id -> {"name", "prompt_positions"}."""
        with self._voice_lock:
            return {k: {"name": n, "prompt_positions": int(g.shape[1])} for k, (g, n) in self._voices.items()}

    def _alive(self) -> List[int]:
        with self._lock:
            return [i for i, p in enumerate(self._procs) if not self._dead[i] and p.is_alive()]

    def _pick_worker(self) -> int:
        alive = self._alive()
        if not alive:
            raise RuntimeError("no GPU worker is alive")
        with self._lock:
            return min(alive, key=lambda i: self._load[i])

    def _control(self, w: int, msg: tuple) -> _PoolRequest:
        """Send a registry message to worker ``w``; its answer arrives through the request books like a request's end."""
        with self._lock:
            if self._closing:
                raise RuntimeError("pool closed")
            req = _PoolRequest(next(self._ids), w)
            self._reqs[req.rid] = req
            self._load[w] += 1
        self._req_qs[w].put((msg[0], req.rid) + tuple(msg[1:]))
        return req

    @staticmethod
    def _await_control(req: _PoolRequest):
        item = req.out.get()
        if isinstance(item, BaseException):
            raise item
        return item[1]

    def stats(self) -> dict:
        """Front-end view (``GET /v1/stats``): workers alive and requests in flight per worker."""
        with self._lock:
            return {"workers": len(self._procs), "alive": sum(1 for i, p in enumerate(self._procs) if not self._dead[i] and p.is_alive()),
                    "in_flight": list(self._load), "restarts": list(self._restarts)}

    def loads(self) -> List[int]:
        """Requests in flight per worker."""
        with self._lock:
            return list(self._load)

    def close(self) -> None:
        with self._lock:
            self._closing = True
        for q in self._req_qs:
            q.put(("close",))
        for p in self._procs:
            p.join(timeout=60)
        self._kill()
        for t in self._threads:  # every dispatcher sees the end of its pipe once its worker is gone
            t.join(timeout=10)
        self._fail_open(RuntimeError("pool closed"))

    # ------------------------------------------------------------------ front-end internals
    def _finish(self, req: _PoolRequest, end) -> None:
        with self._lock:
            if req.closed:
                return
            req.closed = True
            self._reqs.pop(req.rid, None)
            self._load[req.worker] -= 1
        req.out.put(end)

    def _fail_open(self, e: Exception, worker: Optional[int] = None) -> None:
        with self._lock:
            reqs = [r for r in self._reqs.values() if worker is None or r.worker == worker]
        for r in reqs:
            self._finish(r, e)

    def _dispatch(self, w: int) -> None:
        """Relay worker ``w``'s output to the waiting clients; the end of its pipe means the worker is gone."""
        conn = self._res[w]
        while True:
            try:
                rid, kind, payload = conn.recv()
            except (EOFError, OSError):
                with self._lock:
                    self._dead[w] = True  # from here on submit() avoids this worker; what it holds is failed just below
                if self._closing:
                    return
                self._procs[w].join(timeout=5)
                self._fail_open(RuntimeError(f"GPU worker {w} died (exit code {self._procs[w].exitcode})"), worker=w)
                conn = self._replace(w)
                if conn is None:
                    return
                continue
            with self._lock:
                req = self._reqs.get(rid)
            if req is None:
                continue
            if kind == "chunk":
                if not req.cancelled:
                    req.out.put(payload)
            elif kind == "end":
                scores = payload.pop("scores")
                for k, v in payload.items():
                    setattr(req, k, v)
                if scores is not None:
                    import dataclasses

                    req.logprobs, req.mean_logprob, req.takes, req.best_of = (scores[k] for k in ("logprobs", "mean_logprob", "takes", "best_of"))
                    if req.sampling is not None and req.best_of > 1:  # the winner's entry: its seed replays the chosen audio
                        req.sampling = dataclasses.replace(req.sampling, seed=scores["seed"], best_of=None, logprobs=True)
                self._finish(req, None)
            elif kind == "result":  # a registry message's answer
                self._finish(req, ("result", payload))
            elif kind == "error":
                name, msg = payload  # a refused request (ValueError) stays one: the HTTP layer answers 400 for it, 500 for the rest
                self._finish(req, _remote_error(name, msg))

    def _replay_voices(self, w: int, q, conn) -> bool:
        """Register the known voices on the new worker ``w`` (its pipe read here, before its dispatcher takes over)."""
        for k, (grid, name) in list(self._voices.items()):
            rid = next(self._ids)
            q.put(("add_voice", rid, k, grid, name))
            while True:
                try:
                    got, kind, _ = conn.recv()
                except (EOFError, OSError):
                    return False
                if got == rid:
                    break
            if kind != "result":
                return False
        return True

    def _replace(self, w: int):
        """Start a new worker in place of the dead one; its result pipe, or None (not wanted, closing, or it keeps dying)."""
        if not self._respawn or self._restarts[w] >= 3:
            return None
        self._restarts[w] += 1
        p, q, r = self._start_worker(w)
        if self._await_ready(r, w) is not None or self._closing or not self._replay_voices(w, q, r):
            if p.is_alive():
                p.terminate()
            return None
        with self._lock:
            self._procs[w], self._req_qs[w], self._res[w] = p, q, r
            self._dead[w] = False
        return r

    def _kill(self) -> None:
        for p in self._procs:
            if p.is_alive():
                p.terminate()  # the exact children this pool started
        for p in self._procs:
            p.join(timeout=10)


def _remote_error(name: str, msg: str) -> Exception:
    """A worker's exception, by kind: ValueError (and a missing encoder, one of them) stays a refusal, KeyError an unknown voice."""
    if name == "NoEncoderError":
        from .. import NoEncoderError

        return NoEncoderError(msg)
    if name == "KeyError":
        return KeyError(msg)
    return ValueError(msg) if name == "ValueError" else RuntimeError(f"{name}: {msg}")


# ---------------------------------------------------------------------- factories (picklable: module-level callables)
def scheduler_from_settings(settings):
    """What a worker of ``smoltts-server --gpus N`` builds: the model from the settings file (a ``ServerSettings`` or the
    dict it is made from), and its scheduler."""
    from .. import SmolTTS
    from .scheduler import BatchScheduler
    from .settings import ServerSettings

    st = settings if isinstance(settings, ServerSettings) else ServerSettings(**settings)
    model = SmolTTS(checkpoint_dir=str(st.get_checkpoint_dir()), mimi_checkpoint=st.mimi_checkpoint, weight_format=st.weight_format)
    return BatchScheduler(model, max_batch=st.max_batch, generation_settings=st.generation.to_settings(), codec_products=st.codec_products,
                          watermark=st.watermark.to_watermark() if st.watermark is not None else None,
                          min_frames_per_byte=st.min_frames_per_byte, max_frames_per_byte=st.max_frames_per_byte,
                          alignment_heads=st.alignment_heads, timestamp_lag_frames=st.timestamp_lag_frames)


def synthetic_scheduler(model: str = "tiny", seed: int = 21, mimi_seed: int = 5, max_batch: int = 4, frames_per_tick: int = 2,
                        max_new_tokens: int = 64, mimi_encoder: bool = False, watermark=None, alignment_heads=None,
                        timestamp_lag_frames: int = 6):
    """Seeded random weights at the named shapes (tests, rehearsals without a checkpoint); greedy.  ``mimi_encoder``: the codec
    also carries (seeded) encoder weights, so that voices can be cloned."""
    from .. import SmolTTS
    from ..codec.synthetic import synthetic_mimi_encoder_state, synthetic_mimi_state
    from ..config import GenerationSettings
    from ..synthetic import named_config, synthetic_lm_state
    from .scheduler import BatchScheduler

    cfg = named_config(model)
    mst = synthetic_mimi_state(seed=mimi_seed)
    if mimi_encoder:
        mst = {**mst, **synthetic_mimi_encoder_state(seed=mimi_seed)}
    tts = SmolTTS(state=synthetic_lm_state(cfg, seed=seed), config=cfg, mimi_state=mst)
    return BatchScheduler(tts, max_batch=max_batch, frames_per_tick=frames_per_tick,
                          generation_settings=GenerationSettings.greedy(max_new_tokens=max_new_tokens), watermark=watermark,
                          alignment_heads=alignment_heads, timestamp_lag_frames=timestamp_lag_frames)
