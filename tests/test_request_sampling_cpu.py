"""Per-request sampling without a GPU: the RequestSampling schema and its resolution, the route fields and X-Seed, the pool's
submit message, and the host model of the device's request key."""
import functools

import numpy as np
import pytest

from sampling_helpers import make_recorder


class _SamplingTTS:
    """Stand-in façade that records the sampling it was called with."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []

    def _settings(self, generation_settings):
        from smoltts_amd.config import GenerationSettings

        return generation_settings or GenerationSettings()

    def __call__(self, text, voice="heart", sampling=None):
        self.calls.append(sampling)
        return np.linspace(-0.5, 0.5, 1920, dtype=np.float32)

    def stream(self, text, voice="heart", sampling=None):
        self.calls.append(sampling)
        for i in range(2):
            yield np.full(1920, 0.1 * i, dtype=np.float32)


class _SamplingScheduler:
    """Stand-in BatchScheduler: resolves like the real one against its settings and answers with one chunk."""

    def __init__(self, settings):
        self.settings, self.calls = settings, []

    def submit(self, text, voice="heart", stream=False, max_new_tokens=None, output_format=None, sampling=None):
        import queue

        from smoltts_amd.config import RequestSampling

        class R:
            pass

        r = R()
        r.sampling = (sampling if sampling is not None else RequestSampling()).resolve(self.settings)
        r.out = queue.Queue()
        r.out.put(np.zeros(1920, np.float32))
        r.out.put(None)
        self.calls.append((sampling, r.sampling))
        return r

    def iter_chunks(self, r):
        while True:
            item = r.out.get()
            if item is None:
                return
            yield item


def _client(model=None, scheduler=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    return TestClient(create_app(model, scheduler=scheduler))


ROUTES = [("/v1/audio/speech", "input"), ("/v1/text-to-speech/0", "text"), ("/v1/text-to-speech/0/stream", "text")]


def test_request_sampling_defaults_and_ranges():
    from smoltts_amd.config import GenerationSettings, RequestSampling

    r = RequestSampling()
    assert (r.temperature, r.fast_temperature, r.min_p, r.seed) == (None, None, None, None)
    for bad in (dict(temperature=-0.1), dict(fast_temperature=float("inf")), dict(temperature=float("nan")), dict(min_p=1.0),
                dict(min_p=-0.01), dict(seed=-1), dict(seed=2**64)):
        with pytest.raises(ValueError):
            RequestSampling(**bad)
    base = GenerationSettings(default_temp=0.5, default_fast_temp=None, min_p=0.1, min_p_mode="reference")
    res = RequestSampling(seed=7).resolve(base)
    assert (res.temperature, res.fast_temperature, res.min_p, res.seed) == (0.5, 0.0, 0.0, 7)
    res = RequestSampling(temperature=0.8, fast_temperature=0.6).resolve(base)
    assert res.temperature == 0.8 and res.fast_temperature == 0.6 and res.seed is not None and 0 <= res.seed < 2**64
    greedy = RequestSampling(temperature=0.0).resolve(GenerationSettings.greedy())
    assert not greedy.is_sampled and greedy.seed is None  # a greedy request draws no seed
    assert res.resolve(base) == res  # resolving again (pool parent, then worker) changes nothing


def test_min_p_follows_min_p_mode():
    from smoltts_amd.config import GenerationSettings, RequestSampling

    ref = GenerationSettings(default_temp=0.5, min_p=0.1, min_p_mode="reference")
    intended = GenerationSettings(default_temp=0.5, min_p=0.1, min_p_mode="intended")
    assert RequestSampling(min_p=0.3, seed=1).resolve(ref).min_p == 0.0  # the reference's rule removes nothing
    assert RequestSampling(min_p=0.3, seed=1).resolve(intended).min_p == pytest.approx(0.3)
    assert RequestSampling(seed=1).resolve(intended).min_p == pytest.approx(0.1)  # the settings' own value, same rule
    r = RequestSampling(min_p=0.3, seed=1).resolve(intended)
    assert r.resolve(intended) == r


@pytest.mark.parametrize("route,field", ROUTES)
def test_routes_refuse_out_of_range_fields(route, field):
    client = _client(_SamplingTTS())
    for bad in ({"seed": -1}, {"seed": 2**64}, {"temperature": -1}, {"fast_temperature": -0.5}, {"min_p": 1.0}, {"min_p": -0.1},
                {"temperature": "x"}):
        r = client.post(route, json={field: "hi", **bad})
        assert r.status_code == 422, (route, bad)


@pytest.mark.parametrize("route,field", ROUTES)
def test_supplied_seed_reaches_the_model_and_is_echoed(route, field):
    tts = _SamplingTTS()
    client = _client(tts)
    r = client.post(route, json={field: "hi", "seed": 2**64 - 1, "temperature": 0.8, "min_p": 0.2})
    assert r.status_code == 200 and r.headers["X-Seed"] == str(2**64 - 1)
    s = tts.calls[-1]
    assert s.seed == 2**64 - 1 and s.temperature == 0.8 and s.fast_temperature == 0.7  # the façade's default fast temperature
    # no field at all: the façade is called exactly as before, and no header is invented
    r = client.post(route, json={field: "hi"})
    assert r.status_code == 200 and "X-Seed" not in r.headers and tts.calls[-1] is None


@pytest.mark.parametrize("route,field", ROUTES)
def test_scheduler_routes_seed_unseeded_and_greedy(route, field):
    from smoltts_amd.config import GenerationSettings

    sched = _SamplingScheduler(GenerationSettings(default_temp=0.5, default_fast_temp=0.0, min_p=0.1))
    client = _client(_SamplingTTS(), scheduler=sched)
    r = client.post(route, json={field: "hi", "seed": 42})
    assert r.status_code == 200 and r.headers["X-Seed"] == "42"
    assert sched.calls[-1][0].seed == 42 and sched.calls[-1][1].seed == 42  # unchanged on the way in
    r = client.post(route, json={field: "hi"})  # unseeded on a sampled server: the drawn seed is echoed
    assert r.status_code == 200 and r.headers["X-Seed"] == str(sched.calls[-1][1].seed)
    r2 = client.post(route, json={field: "hi"})
    assert r2.headers["X-Seed"] != r.headers["X-Seed"]
    r = client.post(route, json={field: "hi", "temperature": 0, "seed": 5})  # greedy: no X-Seed
    assert r.status_code == 200 and "X-Seed" not in r.headers
    greedy = _SamplingScheduler(GenerationSettings.greedy())
    r = _client(_SamplingTTS(), scheduler=greedy).post(route, json={field: "hi"})
    assert r.status_code == 200 and "X-Seed" not in r.headers


def test_pool_message_carries_sampling_resolved_in_the_parent(monkeypatch):
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.server.pool import GpuPool

    monkeypatch.delenv("HIP_VISIBLE_DEVICES", raising=False)
    gs = GenerationSettings(default_temp=0.5, default_fast_temp=0.0, min_p=0.1)
    pool = GpuPool(functools.partial(make_recorder), devices=[0, 1], ready_timeout=120, generation_settings=gs)
    try:
        for i in range(4):
            req = pool.submit("abc", "sky", sampling=RequestSampling(temperature=0.9) if i % 2 else None)
            got = list(pool.iter_chunks(req))
            assert req.sampling is not None and req.sampling.seed is not None
            t, ft, mp, seed = got[0][1:5]
            # the worker received the parent's resolved values, its seed included
            assert (t, ft, mp) == pytest.approx((req.sampling.temperature, req.sampling.fast_temperature, req.sampling.min_p))
            assert int(got[1][0]) == req.sampling.seed >> 32 and int(got[1][1]) == req.sampling.seed & 0xFFFFFFFF
            assert req.sampling.temperature == (0.9 if i % 2 else 0.5)
    finally:
        pool.close()
    # without the settings only a request that names a sampling carries one, its seed drawn in the parent
    pool = GpuPool(functools.partial(make_recorder), devices=[0], ready_timeout=120)
    try:
        req = pool.submit("abc", sampling=RequestSampling(temperature=0.9))
        got = list(pool.iter_chunks(req))
        assert req.sampling.seed is not None and int(got[1][1]) == req.sampling.seed & 0xFFFFFFFF
        req = pool.submit("abc")
        got = list(pool.iter_chunks(req))
        assert req.sampling is None and got[0][1] == -1
    finally:
        pool.close()


# (seed, frame, step, column, float32 bits of uniform01(seed, 0, frame, step, column)) computed with the device arithmetic
KEY_VECTORS = [
    (0, 0, 0, 0, 0x3E54AEB6),
    (1, 0, 1, 5, 0x3F57F2FE),
    (2, 3, 8, 2047, 0x3F0042D2),
    (2**64 - 1, 7, 2, 1, 0x38AE3000),
    (12345678901234567, 100, 0, 4095, 0x3D2CDF38),
]


def test_request_key_model_matches_fixed_vectors():
    from smoltts_amd.sampling import mix32, request_uniforms, uniform01

    assert [int(mix32(x)) for x in (0, 1, 0xDEADBEEF)] == [0, 1753845952, 3861431939]
    for seed, frame, step, col, bits in KEY_VECTORS:
        u = uniform01(seed, 0, frame, step, [col])
        assert u.dtype == np.float32 and int(u.view(np.uint32)[0]) == bits
        assert request_uniforms(seed, frame, step, col + 1)[col] == u[0]
    u = request_uniforms(3, 0, 0, 1 << 16)
    assert (u > 0).all() and (u < 1).all() and abs(float(u.mean()) - 0.5) < 0.01


def test_gumbel_pick_model():
    from smoltts_amd.sampling import gumbel_pick

    rng = np.random.default_rng(0)
    x = rng.standard_normal(64).astype(np.float32)
    assert gumbel_pick(x, 0.0, 0.0, 1, 0, 0) == int(np.argmax(x))
    assert gumbel_pick(x, 1e-4, 0.0, 1, 0, 0) == int(np.argmax(x))  # a tiny temperature is the argmax
    assert gumbel_pick(x, 1.0, 0.999, 9, 4, 1) == int(np.argmax(x))  # min_p close to 1 keeps only the top token
    picks = {gumbel_pick(x, 2.0, 0.0, s, 0, 0) for s in range(50)}
    assert len(picks) > 5
