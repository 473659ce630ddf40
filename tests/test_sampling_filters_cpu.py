"""Per-request top_k / top_p / repetition penalty without a GPU: the numpy model (sampling.filtered_keys) against brute force,
the RequestSampling fields, the settings and the route bodies, and the fixture rows of the GPU test against the top_p margin."""
import numpy as np
import pytest

from filters_helpers import R, SHAPES, STEPS, make_rows, row_args, row_temp


def _rows(n=24, V=257, seed=3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, V)) * 3.0).astype(np.float32)
    x[:, 7] = x[:, 11]  # ties
    x[0, :5] = x[0].max()  # a tie on the maximum
    return x


@pytest.mark.parametrize("top_k", [1, 2, 5, 50, 256, 257, 1000])
def test_top_k_keeps_what_np_sort_keeps(top_k):
    from smoltts_amd.sampling import filtered_keys

    for r, x in enumerate(_rows()):
        keys = filtered_keys(x, 0.8, 0.0, 5, r, 0, top_k=top_k)
        want = x >= np.sort(x)[::-1][min(top_k, x.shape[0]) - 1]
        assert np.array_equal(np.isfinite(keys), want)
        assert want.sum() >= min(top_k, x.shape[0])


@pytest.mark.parametrize("top_p", [1e-6, 0.3, 0.5, 0.9, 0.999])
@pytest.mark.parametrize("top_k", [0, 20])
def test_top_p_keeps_what_sort_and_cumsum_keeps(top_p, top_k):
    from smoltts_amd.sampling import filtered_keys

    temp = 0.7
    for r, x in enumerate(_rows()):
        keys = filtered_keys(x, temp, 0.0, 5, r, 1, top_k=top_k, top_p=top_p)
        alive = x >= np.sort(x)[::-1][top_k - 1] if top_k else np.ones(x.shape[0], bool)
        z = ((x - x.max()) * np.float32(1.0 / np.float32(temp))).astype(np.float32)
        p = np.where(alive, np.exp(z.astype(np.float64)), 0.0)
        order = np.argsort(-z, kind="stable")
        want = np.zeros(x.shape[0], bool)
        total, tp = p.sum(), float(np.float32(top_p))
        for j in order:  # brute force: the mass of the strictly more probable kept columns
            want[j] = alive[j] and p[z > z[j]].sum() < tp * total
        assert np.array_equal(np.isfinite(keys), want), (r, top_p)
        assert want[np.argmax(x)]
        kept = p[want].sum() / total
        assert kept >= tp * (1 - 1e-12) or want.sum() == alive.sum()  # the nucleus reaches top_p


def test_penalty_values_and_order_of_the_steps():
    from smoltts_amd.sampling import filtered_keys, filtered_pick, gumbel_keys, penalised_row

    x = np.array([2.0, -1.0, 0.5, 0.0, 3.0, -4.0, 1.0, 2.5], np.float32)
    got = penalised_row(x, 1.2, [0, 1, 3, 0, 99, -1])  # duplicates once; out-of-range ids ignored
    inv = np.float32(1.0) / np.float32(1.2)
    want = x.copy()
    want[0], want[1], want[3] = np.float32(2.0) * inv, np.float32(-1.0) * np.float32(1.2), np.float32(0.0) * np.float32(1.2)
    assert np.array_equal(got, want) and got.dtype == np.float32
    assert np.array_equal(penalised_row(x, 1.0, [0, 1]), x) and np.array_equal(penalised_row(x, 3.0, []), x)
    # the maximum used afterwards is the penalised row's, and top_k counts the penalised values
    assert filtered_pick(x, 0.9, 0.0, 1, 0, 0, top_k=1, penalty=3.0, history=[4]) == 7
    keys = filtered_keys(x, 0.9, 0.0, 1, 0, 0, top_k=2, penalty=3.0, history=[4])
    assert set(np.flatnonzero(np.isfinite(keys))) == {0, 7}
    # all off: the unfiltered keys, bit for bit; a greedy row ignores everything
    rows = _rows(4)
    for r, row in enumerate(rows):
        assert np.array_equal(filtered_keys(row, 0.7, 0.05, 9, r, 2), gumbel_keys(row, 0.7, 0.05, 9, r, 2))
        assert filtered_pick(row, 0.0, 0.0, 9, r, 0, top_k=1, top_p=0.1, penalty=3.0, history=[int(np.argmax(row))]) == int(np.argmax(row))


def test_top_p_edge_names_the_flipping_column():
    from smoltts_amd.sampling import filter_keep, top_p_edge

    x = _rows()[3]
    _, z, keep = filter_keep(x, 0.7, top_p=0.6)
    j, dist = top_p_edge(x, 0.7, top_p=0.6)
    p = np.exp(z.astype(np.float64))
    above = p[z > z[j]].sum() / p.sum()
    assert dist == pytest.approx(abs(above - float(np.float32(0.6))) / float(np.float32(0.6)))
    # the edge is the last kept or the first dropped column
    last_kept, first_dropped = np.flatnonzero(keep)[np.argmin(z[keep])], np.flatnonzero(~keep)[np.argmax(z[~keep])]
    assert j in (last_kept, first_dropped)
    assert top_p_edge(x, 0.7, top_p=1.0) == (-1, float("inf"))


@pytest.mark.parametrize("V", SHAPES)
def test_fixture_rows_stay_clear_of_the_top_p_margin(V):
    """The GPU test excuses a row only inside TOP_P_EDGE_MARGIN and caps the excused rows at 3 per shape: the committed seeds
    must leave the model alone inside that cap."""
    from smoltts_amd.sampling import TOP_P_EDGE_MARGIN, top_p_edge

    fx = make_rows(V)
    inside = 0
    for r in range(R):
        near = False
        for step in STEPS:
            t = row_temp(fx, r, step)
            if t > 0:
                a = row_args(fx, r, step)
                near |= top_p_edge(fx["logits"][r], t, a["top_k"], a["top_p"], a["penalty"], a["history"])[1] < TOP_P_EDGE_MARGIN
        inside += near
    assert inside <= 3


def test_request_sampling_filter_fields_and_resolve():
    from smoltts_amd.config import GenerationSettings, RequestSampling

    r = RequestSampling()
    assert (r.top_p, r.top_k, r.repetition_penalty, r.repetition_window) == (None, None, None, None)
    for bad in (dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")), dict(top_k=-1), dict(top_k=1.5), dict(repetition_penalty=0.99),
                dict(repetition_penalty=10.5), dict(repetition_penalty=float("nan")), dict(repetition_window=0), dict(repetition_window=65),
                dict(repetition_window=2.0)):
        with pytest.raises(ValueError):
            RequestSampling(**bad)
    with pytest.raises(ValueError):
        GenerationSettings(top_p=0.0)
    base = GenerationSettings(default_temp=0.5, default_fast_temp=0.5)
    res = RequestSampling(seed=7).resolve(base)
    assert (res.top_p, res.top_k, res.repetition_penalty, res.repetition_window) == (1.0, 0, 1.0, 16) and not res.filters_on
    served = GenerationSettings(default_temp=0.5, top_p=0.8, top_k=40, repetition_penalty=1.2, repetition_window=8)
    res = RequestSampling(seed=7, top_k=5).resolve(served)
    assert (res.top_p, res.top_k, res.repetition_penalty, res.repetition_window) == (0.8, 5, 1.2, 8) and res.filters_on
    assert res.resolve(base) == res  # resolving again (pool parent, then worker) changes nothing
    assert RequestSampling(seed=1, top_p=1.0, top_k=0, repetition_penalty=1.0).resolve(served).filters_on is False
    for on in (dict(top_p=0.5), dict(top_k=1), dict(repetition_penalty=1.1)):
        assert RequestSampling(seed=1, **on).resolve(base).filters_on


def test_server_settings_carry_the_filter_defaults():
    from smoltts_amd.server.settings import GenerationBlock, ServerSettings

    gs = GenerationBlock().to_settings()
    assert (gs.top_p, gs.top_k, gs.repetition_penalty, gs.repetition_window) == (1.0, 0, 1.0, 16)
    s = ServerSettings(checkpoint_dir="x", generation=dict(top_p=0.7, top_k=30, repetition_penalty=1.5, repetition_window=32))
    gs = s.generation.to_settings()
    assert (gs.top_p, gs.top_k, gs.repetition_penalty, gs.repetition_window) == (0.7, 30, 1.5, 32)
    for bad in (dict(top_p=0), dict(top_k=-1), dict(repetition_penalty=11), dict(repetition_window=0)):
        with pytest.raises(ValueError):
            GenerationBlock(**bad)


class _TTS:
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
        yield np.zeros(1920, np.float32)


ROUTES = [("/v1/audio/speech", "input"), ("/v1/text-to-speech/0", "text"), ("/v1/text-to-speech/0/stream", "text")]


@pytest.mark.parametrize("route,field", ROUTES)
def test_route_bodies_carry_the_filter_fields(route, field):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    tts = _TTS()
    client = TestClient(create_app(tts))
    r = client.post(route, json={field: "hi", "top_p": 0.8, "top_k": 40, "repetition_penalty": 1.2, "repetition_window": 8})
    assert r.status_code == 200
    s = tts.calls[-1]
    assert (s.top_p, s.top_k, s.repetition_penalty, s.repetition_window) == (0.8, 40, 1.2, 8)
    r = client.post(route, json={field: "hi", "top_k": 3})  # one field alone makes a sampling; the others take the settings (off)
    assert r.status_code == 200 and tts.calls[-1].top_k == 3 and tts.calls[-1].top_p in (None, 1.0)
    r = client.post(route, json={field: "hi", "temperature": 0, "fast_temperature": 0, "top_p": 0.5})  # greedy: accepted, no effect
    assert r.status_code == 200 and "X-Seed" not in r.headers
    r = client.post(route, json={field: "hi"})
    assert r.status_code == 200 and tts.calls[-1] is None
    for bad in (dict(top_p=0), dict(top_p=1.5), dict(top_k=-1), dict(top_k=2.5), dict(repetition_penalty=0.5), dict(repetition_penalty=11),
                dict(repetition_window=0), dict(repetition_window=65), dict(top_p="much")):
        assert client.post(route, json={field: "hi", **bad}).status_code in (400, 422), bad
