"""best_of on the GPU through the façade: every take is the plain scored request with its seed, only the winner is decoded, and
the winner is the one config.rank_takes names."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TEXT, VOICE, CAP = "three takes of one short line", "heart", 12
SEED = 2**64 - 2  # the takes' seeds wrap: 2^64 - 2, 2^64 - 1, 0.  That the three takes differ is asserted below, on their codes.


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


@pytest.fixture(scope="module")
def settings():
    from smoltts_amd.config import GenerationSettings

    return GenerationSettings.greedy(max_new_tokens=CAP)


def _request(**kw):
    from smoltts_amd.config import RequestSampling

    # a small bias lets <|im_end|> win now and then, so that takes end for either reason
    return RequestSampling(temperature=0.9, eos_bias=6.0, min_frames=2, **kw)


@pytest.fixture(scope="module")
def best_of_call(tts, settings):
    pcm = tts(TEXT, VOICE, generation_settings=settings, sampling=_request(seed=SEED, best_of=3))
    return pcm, [dict(t) for t in tts.last_takes], tts.last_logprobs.copy(), tts.last_mean_logprob, tts.last_sampling[0], tts.last_finish_reason


def test_every_take_is_the_plain_scored_request_with_its_seed(tts, settings, best_of_call):
    from smoltts_amd.config import mean_logprob, rank_takes, take_seed

    pcm, takes, lp, mean, entry, reason = best_of_call
    assert [t["seed"] for t in takes] == [take_seed(SEED, k) for k in range(3)] == [2**64 - 2, 2**64 - 1, 0]
    assert len({t["codes"].tobytes() for t in takes}) == 3  # the three takes differ
    plains = []
    for k, t in enumerate(takes):
        codes = tts.generate_codes([TEXT], [VOICE], settings, sampling=_request(seed=t["seed"], logprobs=True))[0]
        plain = tts.last_logprobs_all[0]
        plains.append(plain.copy())
        assert np.array_equal(codes, t["codes"]), k
        assert len(plain) == t["frames"] == tts.last_stats["frames"] and tts.last_finish_reason == t["finish_reason"], k
        assert abs(mean_logprob(plain) - t["mean_logprob"]) <= 1e-12 and float(plain.min()) == t["min_logprob"], k
        print(f"take {k}: seed {t['seed']}, {t['frames']} frames, {t['finish_reason']}, mean {t['mean_logprob']:.4f}, chosen {t['chosen']}")
    order = rank_takes([(t["finish_reason"], t["mean_logprob"]) for t in takes])
    assert [t["chosen"] for t in takes] == [k == order[0] for k in range(3)]
    win = takes[order[0]]
    assert entry.seed == win["seed"] and entry.best_of is None and reason == win["finish_reason"]
    assert mean == win["mean_logprob"] and np.array_equal(lp, plains[order[0]])
    # the returned audio: the plain request with the winner's seed, bit for bit
    again = tts(TEXT, VOICE, generation_settings=settings, sampling=_request(seed=win["seed"]))
    assert again.dtype == pcm.dtype and np.array_equal(again, pcm)
    assert tts.last_takes is None and tts.last_logprobs is None  # a plain call asks for no scores
    # best_of=1 is the request without it, and take 0
    one = tts(TEXT, VOICE, generation_settings=settings, sampling=_request(seed=SEED, best_of=1, logprobs=True))
    assert tts.last_takes is None and abs(tts.last_mean_logprob - takes[0]["mean_logprob"]) <= 1e-12
    assert np.array_equal(one, tts(TEXT, VOICE, generation_settings=settings, sampling=_request(seed=SEED)))


def test_a_take_cut_at_the_cap_loses_to_one_that_stopped(tts):
    """The ranking path on two real takes: a nearly greedy take cut by max_new_tokens below its natural length (a high mean) and
    a hot take that is made to stop (a lower mean)."""
    from smoltts_amd.config import GenerationSettings, RequestSampling, rank_takes

    tts(TEXT, VOICE, generation_settings=GenerationSettings.greedy(max_new_tokens=CAP), sampling=RequestSampling(temperature=0.05, seed=3, eos_bias=-100.0, logprobs=True))
    natural = len(tts.last_logprobs)
    tts(TEXT, VOICE, generation_settings=GenerationSettings.greedy(max_new_tokens=4), sampling=RequestSampling(temperature=0.05, seed=3, eos_bias=-100.0, logprobs=True))
    cut = (tts.last_finish_reason, tts.last_mean_logprob)
    assert cut[0] == "length" and len(tts.last_logprobs) == 5 < natural
    tts(TEXT, VOICE, generation_settings=GenerationSettings.greedy(max_new_tokens=CAP), sampling=RequestSampling(temperature=1.5, seed=4, min_frames=6, eos_bias=100.0, logprobs=True))
    stopped = (tts.last_finish_reason, tts.last_mean_logprob)
    print(f"cut take: {cut}, stopped take: {stopped}")
    assert stopped[0] == "stop" and stopped[1] < cut[1]
    assert rank_takes([cut, stopped]) == [1, 0] and rank_takes([stopped, cut]) == [0, 1]


def test_stream_fills_the_scores_once_consumed(tts, settings):
    from smoltts_amd.config import RequestSampling, mean_logprob

    req = RequestSampling(temperature=0.9, seed=11, logprobs=True)
    tts(TEXT, VOICE, generation_settings=settings, sampling=req)
    want = tts.last_logprobs.copy()
    gen = tts.stream(TEXT, VOICE, generation_settings=settings, sampling=req)
    next(gen)
    assert tts.last_logprobs is None
    list(gen)
    assert np.array_equal(tts.last_logprobs, want) and tts.last_mean_logprob == mean_logprob(want)


def test_refusals(tts, settings):
    from smoltts_amd.config import RequestSampling

    with pytest.raises(ValueError, match="blocking"):
        next(tts.stream(TEXT, VOICE, generation_settings=settings, sampling=_request(seed=1, best_of=2)))
    with pytest.raises(ValueError, match="segmented"):
        tts("The first sentence of a long text. The second sentence follows it. And a third one ends it.", VOICE, generation_settings=settings,
            sampling=_request(seed=1, best_of=2), segment={"max_bytes": 40, "pause_s": 0.1})
    with pytest.raises(ValueError, match="sampled slow token"):
        tts(TEXT, VOICE, generation_settings=settings, sampling=RequestSampling(temperature=0.0, best_of=2))


# ---------------------------------------------------------------------------------------------------- scheduler and routes
def _scheduler(tts, max_batch, cap=CAP):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    return BatchScheduler(tts, max_batch=max_batch, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=cap))


def _all(sched, req):
    chunks = list(sched.iter_chunks(req))
    return np.concatenate(chunks) if chunks else np.zeros(0, np.float32)


STREAMS = ("a first plain stream beside the takes", "and a second one")


def test_scheduler_runs_the_takes_beside_plain_streams(tts, settings, best_of_call):
    from smoltts_amd.config import rank_takes

    _, want_takes, want_lp, want_mean, _, _ = best_of_call
    sched = _scheduler(tts, 6)
    try:
        alone = [sched.submit(t, VOICE, stream=True) for t in STREAMS]
        alone = [_all(sched, r) for r in alone]
        streams = [sched.submit(STREAMS[0], VOICE, stream=True)]
        req = sched.submit(TEXT, VOICE, sampling=_request(seed=SEED, best_of=3))
        streams.append(sched.submit(STREAMS[1], VOICE, stream=True))
        pcm = _all(sched, req)
        beside = [_all(sched, r) for r in streams]
        win = next(t for t in req.takes if t["chosen"])
        plain = sched.submit(TEXT, VOICE, sampling=_request(seed=win["seed"], logprobs=True))
        plain_pcm = _all(sched, plain)
        singles = [sched.submit(TEXT, VOICE, sampling=_request(seed=t["seed"], logprobs=True)) for t in req.takes]
        for r in singles:
            _all(sched, r)
    finally:
        sched.close()
    assert len(req.takes) == 3 and req.best_of == 3
    for got, one, want in zip(req.takes, singles, want_takes):
        # each take is the plain scored request with its seed on this scheduler ...
        assert got["frames"] == len(one.logprobs) == one.frame_counts[0] and got["finish_reason"] == one.finish_reason
        assert abs(got["mean_logprob"] - one.mean_logprob) <= 1e-12 and got["min_logprob"] == float(one.logprobs.min())
        # ... and the façade's take: the same ids (its batch of three may run other GEMM variants than this six-slot session, so
        # the logits, and with them the scores, agree to rounding only)
        assert {k: got[k] for k in ("seed", "frames", "finish_reason", "chosen")} == {k: want[k] for k in ("seed", "frames", "finish_reason", "chosen")}
        assert abs(got["mean_logprob"] - want["mean_logprob"]) <= 1e-4
    order = rank_takes([(t["finish_reason"], t["mean_logprob"]) for t in req.takes])
    assert req.takes[order[0]]["chosen"] and req.sampling.seed == win["seed"] and req.finish_reason == win["finish_reason"]
    assert req.logprobs.shape == want_lp.shape and req.mean_logprob == plain.mean_logprob == win["mean_logprob"]
    assert np.array_equal(plain.logprobs, req.logprobs) and plain.takes is None
    assert pcm.size > 0 and np.array_equal(pcm, plain_pcm)  # only the winner was decoded: the plain request's audio
    for a, b in zip(alone, beside):
        assert a.size > 0 and np.array_equal(a, b)  # the streams beside the takes: the bytes they have without them


def test_scheduler_refuses_more_takes_than_slots_and_admits_takes_as_slots_come_free(tts):
    sched = _scheduler(tts, 2)
    try:
        with pytest.raises(ValueError, match="exceeds the 2 slots"):
            sched.submit(TEXT, VOICE, sampling=_request(seed=SEED, best_of=3))
        with pytest.raises(ValueError, match="blocking"):
            sched.submit(TEXT, VOICE, stream=True, sampling=_request(seed=SEED, best_of=2))
    finally:
        sched.close()
    sched = _scheduler(tts, 4)
    try:
        stream = sched.submit(STREAMS[0], VOICE, stream=True)
        block = sched.submit(STREAMS[1], VOICE)
        req = sched.submit(TEXT, VOICE, sampling=_request(seed=SEED, best_of=3))
        assert _all(sched, req).size > 0 and _all(sched, stream).size > 0 and _all(sched, block).size > 0
        assert len({t.first_tick for t in req.take_reqs}) > 1  # two slots were free: the third take came in behind a tenant
        assert sched.stats()["active"] == 0
    finally:
        sched.close()


def test_cancelling_the_parent_frees_every_slot(tts):
    from smoltts_amd.config import RequestSampling

    sched = _scheduler(tts, 4, cap=400)
    try:
        req = sched.submit(TEXT, VOICE, sampling=RequestSampling(temperature=0.9, seed=1, eos_bias=-100.0, best_of=3))
        first = sched.submit(STREAMS[0], VOICE, stream=True, max_new_tokens=6)
        _all(sched, first)  # (the takes are in their slots by now, far from their cap)
        sched.cancel(req)
        assert list(sched.iter_chunks(req)) == []  # the end marker, and no audio
        assert all(t.closed for t in req.take_reqs) and sched.stats()["active"] == 0
        after = sched.submit(STREAMS[1], VOICE, max_new_tokens=6)
        assert _all(sched, after).size > 0
    finally:
        sched.close()


def test_routes(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    body = {"input": TEXT, "temperature": 0.9, "eos_bias": 6.0, "min_frames": 2}
    sched = _scheduler(tts, 4)
    try:
        for client in (TestClient(create_app(tts, scheduler=sched)), TestClient(create_app(tts))):
            a = client.post("/v1/audio/speech", json=dict(body, seed=SEED, best_of=3))
            assert a.status_code == 200 and a.headers["X-Best-Of"] == "3" and float(a.headers["X-Mean-Logprob"]) < 0 and a.headers["X-Seed"]
            b = client.post("/v1/audio/speech", json=dict(body, seed=int(a.headers["X-Seed"])))
            assert b.status_code == 200 and b.content == a.content and "X-Best-Of" not in b.headers
            c = client.post("/v1/audio/speech", json=dict(body, seed=int(a.headers["X-Seed"]), logprobs=True))
            assert c.headers["X-Mean-Logprob"] == a.headers["X-Mean-Logprob"] and c.headers["X-Best-Of"] == "1"
            e = client.post("/v1/text-to-speech/3", json={"text": TEXT, "temperature": 0.9, "seed": 5, "best_of": 2})
            assert e.status_code == 200 and e.headers["X-Best-Of"] == "2"
            assert client.post("/v1/audio/speech", json=dict(body, best_of=2, response_format="pcm")).status_code == 400  # a streaming route
            assert client.post("/v1/text-to-speech/3/stream", json={"text": TEXT, "temperature": 0.9, "best_of": 2}).status_code == 400
            assert client.post("/v1/audio/speech", json={"input": TEXT, "temperature": 0.0, "best_of": 2}).status_code == 400  # greedy
            assert client.post("/v1/audio/speech", json=dict(body, best_of=5)).status_code == 400  # above max_best_of = 4
    finally:
        sched.close()


def test_pool_runs_all_takes_on_one_worker_and_reports_them(best_of_call):
    """(This test is about the worker processes: the takes and their scores travel back with the request's end.)"""
    import functools

    from smoltts_amd.server.pool import GpuPool, synthetic_scheduler

    pcm, want_takes, _, _, _, _ = best_of_call
    pool = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 4, 2, CAP), devices=[0, 0], start_method="forkserver")
    try:
        req = pool.submit(TEXT, VOICE, sampling=_request(seed=SEED, best_of=3))
        got = _all(pool, req)
        plain = pool.submit(TEXT, VOICE, sampling=_request(seed=req.sampling.seed, logprobs=True))
        again = _all(pool, plain)
        with pytest.raises(ValueError, match="blocking"):
            pool.submit(TEXT, VOICE, stream=True, sampling=_request(seed=SEED, best_of=2))
        refused = pool.submit(TEXT, VOICE, sampling=_request(seed=SEED, best_of=5))  # more takes than a worker has slots
        with pytest.raises(Exception, match="exceeds the 4 slots"):
            _all(pool, refused)
    finally:
        pool.close()
    win = next(t for t in req.takes if t["chosen"])
    assert req.best_of == 3 and [t["seed"] for t in req.takes] == [t["seed"] for t in want_takes]
    assert [(t["frames"], t["finish_reason"], t["chosen"]) for t in req.takes] == [(t["frames"], t["finish_reason"], t["chosen"]) for t in want_takes]
    assert req.sampling.seed == win["seed"] and req.sampling.best_of is None and req.mean_logprob == win["mean_logprob"]
    assert len(req.logprobs) == win["frames"] and req.finish_reason == win["finish_reason"]
    assert plain.takes is None and plain.best_of == 1 and np.array_equal(plain.logprobs, req.logprobs)
    assert got.shape == pcm.shape and np.array_equal(got, again)
