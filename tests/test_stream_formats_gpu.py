"""Streamed output formats on the GPU: the resample kernel behind the codec (engine.Resampler), SmolTTS.stream(output_format=),
the scheduler's mixed-format passes and the stream route, against scipy.signal.resample_poly of the float32 stream."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMATS = ["pcm_24000", "pcm_8000", "pcm_16000", "pcm_22050", "pcm_44100", "pcm_48000", "ulaw_8000"]
RATIO = {8000: (1, 3), 16000: (2, 3), 22050: (147, 160), 44100: (147, 80), 48000: (2, 1)}


def _rate(fmt):
    return int(fmt.split("_")[1])


def _want_s16(x24, rate):
    from scipy import signal

    up, down = RATIO[rate]
    y = signal.resample_poly(np.asarray(x24, np.float64), up, down)
    return np.rint(np.clip(y, -1.0, 1.0) * 32767).astype(np.int16)


# The scheduler decodes a stream in tick-sized codec passes, SmolTTS.stream one frame per call: their float PCM agrees to ~1e-7
# (test_scheduler_gpu.py), not bit for bit, and the int16 rounding turns that into an occasional one-code difference.
ACROSS_CODEC_CHUNKS = 0.995


def _close_s16(got, want, what, frac=0.999):
    assert got.dtype == np.int16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and np.mean(d == 0) >= frac, (what, int(d.max()), float(np.mean(d == 0)))


def _close_bytes(got, want, what, frac=0.999):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.mean(got == want) >= frac, (what, float(np.mean(got == want)))


def _n_final(n, up, down, half):
    t = up * n - 1 - half
    return 0 if t < 0 else t // down + 1


@pytest.fixture(scope="module")
def codec():
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.engine import MimiEngine

    return MimiEngine(synthetic_mimi_state(seed=3), max_positions=256)


def _decode(codec, codes, chunk_frames=4):
    """codes [B, F, 8] -> the codec's fp32 PCM [B, 1920 F] on the device."""
    from smoltts_amd.engine import MimiSession

    ms = MimiSession(codec, max_batch=codes.shape[0], max_chunk_frames=chunk_frames)
    pcm = ms.decode(codes)
    torch.cuda.synchronize()
    ms.close()
    return pcm


def _convert(pcm, chunk_frames, formats):
    """Convert the device PCM in place, chunk_frames frames per call; -> (per slot the concatenated outputs incl. the last tail,
    per call the (finals, tail) counts)."""
    from smoltts_amd.engine import Resampler

    B, T = pcm.shape
    rs = Resampler(pcm.device, B, chunk_frames * 1920)
    rs.reset_slots(list(range(B)), formats)
    outs = [[] for _ in range(B)]
    counts = []
    for s0 in range(0, T, chunk_frames * 1920):
        n = min(chunk_frames * 1920, T - s0)
        out, cnt = rs.new_outputs(B)
        rs.chunk(pcm[:, s0: s0 + n], n, out, cnt)
        oh, ch = out.cpu().numpy(), cnt.cpu().numpy()
        counts.append(ch.copy())
        for b in range(B):
            if rs.formats[b][1]:
                outs[b].append(rs.slot_bytes(oh, ch, b, tail=s0 + n >= T))
    rs.close()
    return [np.concatenate(o) if o else None for o in outs], counts


def test_engine_resampler_formats_counts_and_chunking(codec):
    from smoltts_amd import engine
    from smoltts_amd.formats import lin2ulaw

    rng = np.random.default_rng(0)
    F = 16
    one = torch.from_numpy(rng.integers(0, 2048, size=(1, F, 8)).astype(np.int32))
    codes = one.expand(len(FORMATS), F, 8).contiguous().cuda()  # identical codes in every slot
    pcm_d = _decode(codec, codes)
    runs = {cf: _convert(pcm_d, cf, FORMATS) for cf in (1, 4, 16)}
    res, counts = runs[1]
    pcm = pcm_d.cpu().numpy()
    for b, fmt in enumerate(FORMATS):
        rate = _rate(fmt)
        if rate == 24000:
            assert res[b] is None and all((c[b] == 0).all() for c in counts)  # off: nothing
            continue
        for cf in (4, 16):  # chunking is invisible
            assert np.array_equal(runs[cf][0][b], res[b]), (fmt, cf)
        _, up, down, half = engine.resample_design(rate)
        want = _want_s16(pcm[b], rate)
        if fmt.startswith("ulaw"):
            assert res[b].dtype == np.uint8
            _close_bytes(res[b], lin2ulaw(want), fmt)
        else:
            _close_s16(res[b], want, fmt)
        for cf in (1, 4, 16):  # per-call counts
            n_prev = 0
            for c in runs[cf][1]:
                n = n_prev + 1920 * cf
                fin = _n_final(n, up, down, half)
                assert c[b, 0] == fin - _n_final(n_prev, up, down, half) and c[b, 1] == -(-n * up // down) - fin, (fmt, cf)
                assert c[b, 1] <= 20
                n_prev = n
    assert counts[0][1].tolist() == [630, 10]  # 8 kHz, one frame per call: 630 first, then 640 per frame, 10 at the end
    assert counts[1][1].tolist() == [640, 10]


def test_engine_resampler_mulaw_exact_and_slot_reset_isolated(codec):
    """Every slot reads the same fp32 row: the mu-law slot equals the formula on the 8 kHz slot exactly; restarting one slot's
    stream mid-way does not change any other slot's bytes."""
    from smoltts_amd.engine import Resampler
    from smoltts_amd.formats import lin2ulaw

    B, n_calls, n_in = len(FORMATS), 6, 4 * 1920
    rng = np.random.default_rng(1)
    x = torch.from_numpy((0.6 * np.sin(np.arange(n_calls * n_in) * 0.013) + 0.3 * rng.standard_normal(n_calls * n_in)).astype(np.float32))
    x = x.cuda()[None].expand(B, -1).contiguous()

    def run(reset_slot=None):
        rs = Resampler(x.device, B, n_in)
        rs.reset_slots(list(range(B)), FORMATS)
        outs = [[] for _ in range(B)]
        for k in range(n_calls):
            if reset_slot is not None and k == 3:
                rs.reset_slots([reset_slot], [FORMATS[reset_slot]])
            out, cnt = rs.new_outputs(B)
            rs.chunk(x[:, k * n_in:(k + 1) * n_in], n_in, out, cnt)
            oh, ch = out.cpu().numpy(), cnt.cpu().numpy()
            for b in range(1, B):
                outs[b].append(rs.slot_bytes(oh, ch, b, tail=k == n_calls - 1))
        rs.close()
        return [None] + [np.concatenate(o) for o in outs[1:]]

    base = run()
    assert np.array_equal(base[6], lin2ulaw(base[1]))
    _close_s16(base[1], _want_s16(x[0].cpu().numpy(), 8000), "pcm_8000")
    other = run(reset_slot=3)
    for b in range(1, B):
        if b != 3:
            assert np.array_equal(other[b], base[b]), FORMATS[b]
    assert not np.array_equal(other[3], base[3])  # (the restarted slot began a new stream)


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


@pytest.mark.parametrize("overlap", [True, False])
def test_facade_stream_output_format(tts, overlap):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.formats import lin2ulaw

    gs = GenerationSettings.greedy(max_new_tokens=12)
    ref = np.concatenate(list(tts.stream("a formatted stream", "sky", generation_settings=gs, overlap=overlap)))
    for fmt in FORMATS[1:]:
        chunks = list(tts.stream("a formatted stream", "sky", generation_settings=gs, overlap=overlap, output_format=fmt))
        got = np.concatenate(chunks)
        want = _want_s16(ref, _rate(fmt))
        if fmt.startswith("ulaw"):
            assert all(c.dtype == np.uint8 for c in chunks)
            _close_bytes(got, lin2ulaw(want), fmt)
        else:
            assert all(c.dtype == np.int16 for c in chunks)
            _close_s16(got, want, fmt)
    with pytest.raises(ValueError):
        next(tts.stream("x", "sky", generation_settings=gs, output_format="flac_8000"))


def test_scheduler_mixed_formats_match_the_facade(tts):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    reqs = [("first streamed request", "heart", 9, "pcm_8000"), ("second one, a bit longer", "sky", 13, "ulaw_8000"),
            ("third stays float", "nova", 7, None), ("fourth at forty four", "bella", 10, "pcm_44100"),
            ("fifth refills a slot", "liam", 8, "pcm_48000"), ("sixth refills too", "heart", 6, "pcm_22050")]
    want = []
    for text, voice, n, fmt in reqs:
        gs = GenerationSettings.greedy(max_new_tokens=n)
        want.append(np.concatenate(list(tts.stream(text, voice, generation_settings=gs, output_format=fmt))))
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=300))
    got = [None] * len(reqs)
    try:
        # one request is cancelled mid-stream: its slot is refilled, the others do not notice
        victim = sched.submit("this client hangs up early", "sky", stream=True, max_new_tokens=200, output_format="pcm_16000")
        it = sched.iter_chunks(victim)
        first = next(it)
        assert first.dtype == np.int16 and first.size > 0
        it.close()

        def worker(i):
            text, voice, n, fmt = reqs[i]
            r = sched.submit(text, voice, stream=True, max_new_tokens=n, output_format=fmt)
            got[i] = np.concatenate(list(sched.iter_chunks(r)))

        threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(reqs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=180)
    finally:
        sched.close()
    for (text, _, _, fmt), g, w in zip(reqs, got, want):
        assert g is not None, text
        if fmt is None:
            assert g.dtype == np.float32 and g.shape == w.shape and float(np.sqrt(np.mean((g - w) ** 2))) <= 1e-6
        elif fmt.startswith("ulaw"):
            _close_bytes(g, w, fmt, ACROSS_CODEC_CHUNKS)
        else:
            _close_s16(g, w, fmt, ACROSS_CODEC_CHUNKS)


def test_server_stream_ulaw_on_the_scheduler(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler

    want = np.concatenate(list(tts.stream("over the telephone", "7", generation_settings=GenerationSettings.greedy(max_new_tokens=10),
                                          output_format="ulaw_8000")))
    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=10))
    try:
        client = TestClient(create_app(tts, scheduler=sched))
        r = client.post("/v1/text-to-speech/7/stream?output_format=ulaw_8000", json={"text": "over the telephone"})
        assert r.status_code == 200 and r.headers["x-sample-rate"] == "8000"
        _close_bytes(np.frombuffer(r.content, np.uint8), want, "ulaw_8000", ACROSS_CODEC_CHUNKS)
        r = client.post("/v1/text-to-speech/7/stream?output_format=flac_8000", json={"text": "x"})
        assert r.status_code == 422
    finally:
        sched.close()
