"""Streamed character timestamps through the serving side on the tiny synthetic model, four heads in two layers:
the scheduler's live streams against the numpy model over the same rows, the pool and the route on a real worker.  The synthetic
heads track nothing: this tests the plumbing, not the accuracy."""
import threading

import numpy as np
import pytest

from smoltts_amd import align

pytestmark = pytest.mark.gpu

HEADS = [(0, 1), (0, 3), (1, 2), (1, 4)]
TICK, CAP, LAG = 2, 24, 3
TEXTS = ["first request", "the second one, longer", "third", "and a fourth text"]


def _scheduler(lag=LAG, heads=HEADS, max_batch=2):
    from smoltts_amd.server.pool import synthetic_scheduler

    return synthetic_scheduler("tiny", 21, 5, max_batch, TICK, CAP, alignment_heads=heads, timestamp_lag_frames=lag)


def _live(sched, text, **kw):
    req = sched.submit(text, "sky", stream=True, live_timestamps=True, **kw)
    pairs = list(sched.timed_chunks(req))
    return req, pairs


def _audio(pairs):
    return np.concatenate([np.asarray(c).reshape(-1) for c, _ in pairs])


def _same(a, b):
    return a.characters == b.characters and a.start_s == b.start_s and a.end_s == b.end_s


@pytest.fixture(scope="module")
def sched():
    s = _scheduler()
    yield s
    s.close()


@pytest.fixture(scope="module")
def alone(sched):
    """Each text as a live stream on its own, and as a blocking request with ``timestamps`` (whose rows the request keeps)."""
    out = {}
    for t in TEXTS:
        req, pairs = _live(sched, t)
        blocking = sched.submit(t, "sky", timestamps=True)
        pcm = np.concatenate(list(sched.iter_chunks(blocking)))
        out[t] = (req, pairs, blocking, pcm)
    return out


def test_a_live_stream_hands_out_the_models_parts_over_its_rows(sched, alone):
    tok = sched.tts.tokenizer
    early = 0
    for t in TEXTS:
        req, pairs, blocking, _ = alone[t]
        rows = np.concatenate(blocking.al)  # the rows of the same greedy frames: [frames, heads, 2]
        F = _audio(pairs).size // 1920
        assert F == rows.shape[0] == CAP + 1 and rows.shape[1] == len(HEADS) and (rows[:, :, 0] >= 0).all()
        ids = blocking.align_ids
        sf, al = align.StreamFit(len(ids), LAG), align.StreamAligner(t, ids, tok)
        want = []
        for f0 in range(0, F, TICK):  # a tick's frames, then the host's look
            sf.push_rows(rows[f0:min(f0 + TICK, F)])
            want.append(al.update(np.asarray(sf.starts)) if f0 + TICK < F else al.finish(sf.finish(F), al.duration(F)))
        got = [p for _, p in pairs]
        assert len(got) == len(want), t
        for k, (g, w) in enumerate(zip(got, want)):
            assert (g is None) == (w is None) and (g is None or _same(g, w)), (t, k, g, w)
        early += sum(1 for p in want[:-1] if p is not None)
        assert _same(req.alignment, al.alignment()) and req.alignment.characters == list(t)
        assert req.alignment.start_s[0] == 0.0 and req.alignment.end_s[-1] == al.duration(F) == F * 1920 / 24000
        assert all(a <= b for a, b in zip(req.alignment.start_s, req.alignment.start_s[1:]))
    print("parts handed out before the end:", early)


def test_with_a_lag_of_the_whole_utterance_the_stream_equals_the_blocking_alignment(alone):
    """``timestamp_lag_frames`` at the session's max_frames: nothing commits early.  A blocking request keeps only the frames whose
    slow id is semantic, and the synthetic model emits others; "hello there" and "good morning" at 13 frames are requests whose
    frames are all semantic, so both routes deliver the same audio and their alignments must be the same.  For the other
    texts the stream is held to the blocking fit (``align.align``) over the rows of the frames the stream delivers."""
    late = _scheduler(lag=CAP + 1)
    try:
        assert late.timestamp_lag_frames == late.session.max_frames
        for t in ("hello there", "good morning"):
            req, pairs = _live(late, t, max_new_tokens=12)
            blocking = late.submit(t, "sky", timestamps=True, max_new_tokens=12)
            pcm = np.concatenate(list(late.iter_chunks(blocking)))
            assert pcm.size == _audio(pairs).size == 13 * 1920  # the premise: every frame is audio on both routes
            assert [p is not None for _, p in pairs].count(True) == 1  # one part, at the end
            assert _same(req.alignment, blocking.alignment), t
        for t in TEXTS[:2]:
            req, pairs = _live(late, t)
            _, first, blocking, _ = alone[t]
            assert np.array_equal(_audio(pairs), _audio(first))
            rows = np.concatenate(blocking.al)
            F = rows.shape[0]
            want = align.align(t, blocking.align_ids, rows[:, :, 0], rows[:, :, 1], late.tts.tokenizer, duration_s=F * 1920 / 24000)
            assert _audio(pairs).size == F * 1920 and _same(req.alignment, want), t
    finally:
        late.close()


def test_more_requests_than_slots_each_gets_the_parts_it_gets_alone(sched, alone):
    out = {}

    def run(i, t):
        if i % 2 == 0:
            out[i] = _live(sched, t)
        else:
            req = sched.submit(t, "sky", stream=True)
            out[i] = (req, list(sched.timed_chunks(req)))

    order = TEXTS + TEXTS[::-1]
    threads = [threading.Thread(target=run, args=(i, t)) for i, t in enumerate(order)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for i, t in enumerate(order):
        req, pairs = out[i]
        first_req, first, _, _ = alone[t]
        assert np.array_equal(_audio(pairs), _audio(first)), (i, t)
        if i % 2:
            assert req.alignment is None and all(p is None for _, p in pairs)
            continue
        assert _same(req.alignment, first_req.alignment), (i, t)
        mine, theirs = [p for _, p in pairs if p is not None], [p for _, p in first if p is not None]
        assert len(mine) == len(theirs) and all(_same(a, b) for a, b in zip(mine, theirs)), (i, t)
    # the slots a live stream held were switched off behind it when their next tenant came without the option
    req = sched.submit(TEXTS[0], "sky", stream=True)
    list(sched.iter_chunks(req))
    req = sched.submit(TEXTS[1], "sky", stream=True)
    list(sched.iter_chunks(req))


def test_the_option_changes_no_audio_and_a_scheduler_that_never_saw_it_keeps_its_form(sched, alone):
    for t in TEXTS[:2]:
        req, pairs, _, _ = alone[t]
        plain = sched.submit(t, "sky", stream=True)
        chunks = list(sched.iter_chunks(plain))
        assert np.array_equal(np.concatenate(chunks), _audio(pairs)) and len(chunks) == len(pairs)
        assert plain.frame_counts == req.frame_counts and plain.finish_reason == req.finish_reason and plain.alignment is None
        fast, fp = _live(sched, t, speed=1.5, output_format="pcm_16000")
        plain = sched.submit(t, "sky", stream=True, speed=1.5, output_format="pcm_16000")
        assert np.array_equal(np.concatenate(list(sched.iter_chunks(plain))), _audio(fp))
        total = (CAP + 1) * 1920 / 24000 / 1.5  # nominal: the frames' samples over the rate, over the speed
        assert fast.alignment.end_s[-1] == total and max(fast.alignment.end_s) <= total
    fresh = _scheduler()
    try:
        form = fresh.session.graph_form()
        for t in TEXTS[:3]:
            list(fresh.iter_chunks(fresh.submit(t, "sky", stream=True)))
        assert fresh.session.graph_form() == form and form & 32 == 0 and not fresh._fit_on and not fresh._slot_align
        assert int(fresh._fitter.committed.sum()) == 0  # the fitter was never launched
        _live(fresh, TEXTS[0])
        list(fresh.iter_chunks(fresh.submit(TEXTS[1], "sky", stream=True)))
        list(fresh.iter_chunks(fresh.submit(TEXTS[2], "sky", stream=True)))
        assert fresh.session.graph_form() == form and not fresh._fit_on and not fresh._slot_align
    finally:
        fresh.close()


def test_every_refusal_at_the_scheduler(sched):
    from smoltts_amd.config import RequestSampling

    for kw in (dict(stream=False), dict(stream=True, segment=True), dict(stream=True, trim_silence=True), dict(stream=True, max_pause_s=0.5),
               dict(stream=True, timestamps=True), dict(stream=True, sampling=RequestSampling(temperature=0.8, best_of=2))):
        with pytest.raises(ValueError):
            sched.submit(TEXTS[0], "sky", live_timestamps=True, **kw)
    with pytest.raises(TypeError):
        sched.submit_incremental("sky", live_timestamps=True)
    bare = _scheduler(heads=None)
    try:
        with pytest.raises(ValueError, match="alignment_heads"):
            bare.submit("hello", "sky", stream=True, live_timestamps=True)
        assert bare._fitter is None
    finally:
        bare.close()
    with pytest.raises(ValueError):
        _scheduler(lag=0)


def test_the_facade_streams_the_same_audio_with_parts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    tts = SmolTTS(state=synthetic_lm_state(cfg, seed=11), config=cfg, mimi_state=synthetic_mimi_state(seed=2), alignment_heads=HEADS)
    gs = GenerationSettings.greedy(max_new_tokens=CAP)
    text = "Hé, timestamps!"
    for overlap in (True, False):
        plain = np.concatenate(list(tts.stream(text, "sky", generation_settings=gs, sampling=RequestSampling(), overlap=overlap)))
        pairs = list(tts.stream_with_timestamps(text, "sky", generation_settings=gs, overlap=overlap, timestamp_lag_frames=LAG))
        assert np.array_equal(_audio(pairs), plain)
        a = tts.last_alignment
        assert a.characters == list(text) == [c for _, p in pairs if p is not None for c in p.characters]
        assert a.start_s[0] == 0.0 and a.end_s[-1] == plain.size / 24000
        assert all(x <= y for x, y in zip(a.start_s, a.start_s[1:])) and all(s <= e for s, e in zip(a.start_s, a.end_s))
        assert sum(1 for _, p in pairs[:-1] if p is not None) >= 1  # parts do come before the end
    for kw in (dict(segment=True), dict(trim_silence=True), dict(timestamp_lag_frames=0)):
        with pytest.raises(ValueError):
            list(tts.stream_with_timestamps(text, "sky", generation_settings=gs, **kw))
    tts.lm.close()


def test_the_pool_relays_the_parts_and_the_route_serves_them():
    import base64
    import functools
    import json

    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.pool import GpuPool, synthetic_scheduler

    pool = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, TICK, CAP, alignment_heads=HEADS, timestamp_lag_frames=LAG),
                   devices=[0], start_method="forkserver", alignment_heads=HEADS)
    try:
        text = "through the pool"
        req, pairs = _live(pool, text)
        parts = [p for _, p in pairs if p is not None]
        assert len(parts) > 1 and [c for p in parts for c in p.characters] == list(text) == req.alignment.characters
        assert req.alignment.start_s == [s for p in parts for s in p.start_s] and req.alignment.end_s == [e for p in parts for e in p.end_s]
        plain = pool.submit(text, "sky", stream=True)
        assert np.array_equal(np.concatenate(list(pool.iter_chunks(plain))), _audio(pairs)) and plain.alignment is None
        for kw in (dict(stream=False), dict(stream=True, segment=True), dict(stream=True, trim_silence=True)):
            with pytest.raises(ValueError):
                pool.submit(text, "sky", live_timestamps=True, **kw)
        client = TestClient(create_app(None, {}, scheduler=pool))
        r = client.post("/v1/text-to-speech/sky/stream/with-timestamps?output_format=pcm_24000", json={"text": text})
        assert r.status_code == 200
        objs = [json.loads(l) for l in r.text.splitlines()]
        assert [o["alignment"] for o in objs if o["alignment"] is not None] == [p.to_json() for p in parts]
        assert all(o["alignment"] == o["normalized_alignment"] for o in objs)
        audio = b"".join(base64.b64decode(o["audio_base64"]) for o in objs)
        assert audio == client.post("/v1/text-to-speech/sky/stream?output_format=pcm_24000", json={"text": text}).content
        assert client.post("/v1/text-to-speech/sky/stream/with-timestamps", json={"text": text, "trim_silence": True}).status_code == 400
    finally:
        pool.close()
    no_heads = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, TICK, CAP), devices=[0], start_method="forkserver")
    try:
        with pytest.raises(ValueError, match="alignment_heads"):
            no_heads.submit("x", "sky", stream=True, live_timestamps=True)
        r = TestClient(create_app(None, {}, scheduler=no_heads)).post("/v1/text-to-speech/sky/stream/with-timestamps", json={"text": "x"})
        assert r.status_code == 501 and "align rank" in r.json()["detail"]
    finally:
        no_heads.close()
