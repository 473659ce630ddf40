"""FLAC framing on the GPU (csrc/flac.hip, engine.FlacEncoder / StreamConverter / flac_encode): the kernel's bytes equal the numpy
model's (smoltts_amd/flac.py) call by call, and streams framed as FLAC decode to the samples of the same stream without it."""
import numpy as np
import pytest
import torch

from flac_decode_helpers import decode, decode_mono16

pytestmark = pytest.mark.gpu

RATES = [8000, 16000, 22050, 24000, 44100, 48000]


def _signal(rng, kind, n):
    t = np.arange(n)
    if kind == 0:
        return (0.5 * np.sin(2 * np.pi * 440 * t / 24000)).astype(np.float32)
    if kind == 1:
        return rng.uniform(-1.2, 1.2, n).astype(np.float32)  # beyond full scale: clipped
    if kind == 2:
        return np.zeros(n, np.float32)
    return np.clip(np.cumsum(rng.normal(0, 0.01, n)), -1, 1).astype(np.float32)


def test_kernel_equals_model_call_by_call():
    """32 slots in one launch per pass: fp32 slots at 24 kHz and int16 slots at every rate, off slots, random pass sizes (0, under
    16, large, more than one block), a slot restarted mid-way and last calls; every slot's bytes equal flac.StreamEncoder's."""
    from smoltts_amd import flac
    from smoltts_amd.engine import FLAC_F32, FLAC_OFF, FLAC_S16, FlacEncoder

    rng = np.random.default_rng(5)
    dev = torch.device("cuda:0")
    B, NMAX = 32, 9000
    fe = FlacEncoder(dev, B)
    src = [FLAC_OFF if b % 8 == 7 else (FLAC_F32 if b % 2 == 0 else FLAC_S16) for b in range(B)]
    rate = [24000 if s == FLAC_F32 else RATES[b % len(RATES)] for b, s in enumerate(src)]
    kind = [b % 4 for b in range(B)]
    fe.reset_slots(list(range(B)), rate, src)
    model = [flac.StreamEncoder(r) for r in rate]
    pos = [0] * B
    ended = [False] * B
    for call in range(7):
        if call == 4:  # slot 2 starts a new stream at 16 kHz from int16
            fe.reset_slots([2], [16000], [FLAC_S16])
            src[2], rate[2], model[2], pos[2], ended[2] = FLAC_S16, 16000, flac.StreamEncoder(16000), 0, False
        n_in = int(rng.choice([0, 5, 15, 16, 1920, 7680, NMAX]))
        pcm = np.zeros((B, max(n_in, 1)), np.float32)
        valid = np.zeros(B, np.int32)
        s16 = np.zeros((B, 2 * NMAX + 64), np.uint8)
        counts = np.zeros((B, 2), np.int32)
        last = np.zeros(B, np.int32)
        feeds = {}
        for b in range(B):
            if src[b] == FLAC_OFF or ended[b]:
                continue
            is_last = call == 6 or rng.random() < 0.1
            if src[b] == FLAC_F32:
                v = int(rng.integers(0, n_in + 1))
                x = _signal(rng, kind[b], pos[b] + v)[pos[b]:]
                pcm[b, :v] = x
                valid[b] = v
                feeds[b] = flac.quantize(x)
            else:
                fin = int(rng.integers(0, NMAX - 40))
                tail = int(rng.integers(0, 30))
                x = flac.quantize(_signal(rng, kind[b], pos[b] + fin + tail)[pos[b]:])
                s16[b, :2 * (fin + tail)] = x.view(np.uint8)
                counts[b] = (fin, tail)
                feeds[b] = x if is_last else x[:fin]
                v = fin
            pos[b] += v
            last[b] = is_last
            ended[b] = is_last
        out, sizes = fe.new_outputs(B, max(n_in, NMAX + 32))
        d = [torch.from_numpy(a).to(dev) for a in (pcm, valid, s16, counts, last)]
        fe.chunk(B, out, sizes, pcm=d[0], n_in=n_in, valid=d[1], s16=d[2], s16_counts=d[3], last=d[4])
        ho, hs = out.cpu().numpy(), sizes.cpu().numpy()
        for b in range(B):
            got = b"".join(FlacEncoder.slot_frames(ho, hs, b))
            want = model[b].feed(feeds[b], bool(last[b])) if b in feeds else b""
            assert got == want, (call, b, src[b], rate[b], len(got), len(want))
    fe.close()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096, 4097, 12345])
def test_flac_encode_equals_model(n):
    from smoltts_amd import flac
    from smoltts_amd.engine import flac_encode

    rng = np.random.default_rng(n)
    x = (0.4 * np.sin(np.arange(n) * 0.05) + rng.normal(0, 0.01, n)).astype(np.float32)
    got = flac_encode(x, 24000, torch.device("cuda:0"))
    assert got == flac.encode_file(flac.quantize(x), 24000)
    d = decode(got)
    assert np.array_equal(d.samples[0].astype(np.int16), flac.quantize(x))
    assert d.info.total == n and d.info.max_frame == max(f.length for f in d.frames)
    s16 = flac.quantize(x[::-1].copy())
    got16 = flac_encode(s16, 48000, torch.device("cuda:0"))
    assert got16 == flac.encode_file(s16, 48000)


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


def _pcm16(chunks, fmt):
    """The int16 samples of a stream without FLAC: the converted chunks, or the float32 of pcm_24000 quantised."""
    from smoltts_amd import flac

    x = np.concatenate(chunks)
    return flac.quantize(x) if fmt == "pcm_24000" else x


def _flac_samples(chunks, rate):
    data = b"".join(np.asarray(c, np.uint8).tobytes() for c in chunks)
    d = decode(data)
    assert d.info.rate == rate
    return decode_mono16(data)


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("speed", [None, 0.5])
def test_facade_stream_flac_equals_its_pcm(tts, overlap, speed):
    from smoltts_amd.config import GenerationSettings

    gs = GenerationSettings.greedy(max_new_tokens=14)
    for fmt in ["pcm_24000", "pcm_8000", "pcm_16000", "pcm_22050", "pcm_44100", "pcm_48000"]:
        kw = dict(generation_settings=gs, overlap=overlap, speed=speed, output_format=fmt)
        want = _pcm16(list(tts.stream("a lossless stream", "sky", **kw)), fmt)
        chunks = list(tts.stream("a lossless stream", "sky", container="flac", **kw))
        assert all(c.dtype == np.uint8 for c in chunks) and bytes(chunks[0][:4]) == b"fLaC"
        got = _flac_samples(chunks, int(fmt.split("_")[1]))
        assert got.shape == want.shape and np.array_equal(got, want), (fmt, overlap, speed)


def test_scheduler_flac_beside_other_formats_in_one_tick(tts):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    # (text, voice, frames, format, speed): every FLAC request has a pcm twin in the same batch
    reqs = [("one", "heart", 9, "pcm_24000", None), ("two", "sky", 12, "pcm_16000", None), ("three", "nova", 7, "pcm_48000", 0.5),
            ("four", "bella", 10, "pcm_24000", 1.5)]
    sched = BatchScheduler(tts, max_batch=12, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=300))
    try:
        hs = []
        for t, v, n, f, s in reqs:
            fmt = None if f == "pcm_24000" else f
            hs.append((sched.submit(t, v, stream=True, max_new_tokens=n, output_format=fmt, speed=s, container="flac"),
                       sched.submit(t, v, stream=True, max_new_tokens=n, output_format=fmt, speed=s)))
        others = [sched.submit("mu", "liam", stream=True, max_new_tokens=8, output_format="ulaw_8000"),
                  sched.submit("float", "heart", stream=True, max_new_tokens=6),
                  sched.submit("blocking", "sky", max_new_tokens=5)]
        got = [(list(sched.iter_chunks(a)), list(sched.iter_chunks(b))) for a, b in hs]
        for o in others:
            assert len(list(sched.iter_chunks(o)))
    finally:
        sched.close()
    for (t, v, n, f, s), (fl, twin) in zip(reqs, got):
        want = _pcm16(twin, f)
        assert np.array_equal(_flac_samples(fl, int(f.split("_")[1])), want), t


def test_openai_flac_and_pcm_on_the_scheduler(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd import flac
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler

    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=10))
    try:
        client = TestClient(create_app(tts, scheduler=sched))
        r_pcm = client.post("/v1/audio/speech", json={"input": "over the wire", "voice": "7", "response_format": "pcm"})
        r_flac = client.post("/v1/audio/speech", json={"input": "over the wire", "voice": "7", "response_format": "flac", "speed": 0.5})
        r_flac1 = client.post("/v1/audio/speech", json={"input": "over the wire", "voice": "7", "response_format": "flac"})
        r_long = client.post("/v1/audio/speech", json={"input": "word " * 5000, "response_format": "flac"})
    finally:
        sched.close()
    assert r_pcm.status_code == 200 and r_flac.status_code == 200 and r_flac1.status_code == 200
    assert r_flac.headers["content-type"] == "audio/flac"
    pcm = np.frombuffer(r_pcm.content, "<i2")
    assert np.array_equal(decode_mono16(r_flac1.content), pcm)
    assert decode_mono16(r_flac.content).size > 1.9 * pcm.size
    assert len(r_flac1.content) < len(r_pcm.content) * 1.01 + len(flac.stream_header(24000))
    assert r_long.status_code == 400


def test_pool_streams_flac():
    import functools

    from smoltts_amd.server.pool import GpuPool, synthetic_scheduler

    pool = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, 2, 16), devices=[0], start_method="forkserver")
    try:
        a = pool.submit("through the pool", "sky", stream=True, max_new_tokens=9, container="flac", output_format="pcm_22050")
        fl = list(pool.iter_chunks(a))
        b = pool.submit("through the pool", "sky", stream=True, max_new_tokens=9, output_format="pcm_22050")
        twin = list(pool.iter_chunks(b))
    finally:
        pool.close()
    assert np.array_equal(_flac_samples(fl, 22050), np.concatenate(twin))
