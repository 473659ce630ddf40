"""Per-request speaking speed on the GPU: the time-stretch kernel (engine.TimeStretcher) against the numpy model tsm.Stretcher,
chained with the resampler, and speed through SmolTTS (blocking and stream) and the BatchScheduler (blocking and streamed, with
formats, cloned voices and seeds)."""
import numpy as np
import pytest
import torch

from smoltts_amd import tsm

pytestmark = pytest.mark.gpu

SPEEDS = [0.25, 0.5, 0.8, 1.25, 2.0, 4.0]
RATIO = {8000: (1, 3), 16000: (2, 3), 48000: (2, 1)}


def _voiced(n, seed=0, f0=150.0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.03 * np.sin(2 * np.pi * 3 * t))) / 24000.0
    x = sum(0.3 / k * np.sin(k * ph) for k in range(1, 6)) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.5 * t))
    return (x + 0.01 * rng.standard_normal(n)).astype(np.float32)


def _want_s16(x24, rate):
    from scipy import signal

    up, down = RATIO[rate]
    y = signal.resample_poly(np.asarray(x24, np.float64), up, down)
    return np.rint(np.clip(y, -1.0, 1.0) * 32767).astype(np.int16)


def _close_s16(got, want, what, frac=0.999):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and np.mean(d == 0) >= frac, (what, int(d.max()), float(np.mean(d == 0)))


def _run_kernel(x, sq, calls):
    """calls: [(n_in, valid, last)] over x -> (per-call outputs, per-call slot states) from a one-slot TimeStretcher."""
    from smoltts_amd.engine import TimeStretcher

    dev = torch.device("cuda", 0)
    ts = TimeStretcher(dev, 1)
    ts.reset_slots([0], [sq])
    outs, states, i = [], [], 0
    for n_in, valid, last in calls:
        row = np.zeros(max(n_in, 1), np.float32)
        row[valid:n_in] = 1e3  # garbage past the valid samples must not be read
        seg = x[i:i + valid]  # (zeros past the end of x)
        row[:seg.size] = seg
        i += valid
        pcm = torch.from_numpy(row)[None].to(dev)
        out, cnt = ts.new_outputs(1, n_in)
        ts.chunk(pcm, n_in, out, cnt, valid=torch.tensor([valid], dtype=torch.int32, device=dev),
                 last=torch.tensor([int(last)], dtype=torch.int32, device=dev))
        c = int(cnt.cpu()[0])
        outs.append(out[0, :c].cpu().numpy())
        states.append(ts.slot_state(0))
    ts.close()
    return outs, states


@pytest.mark.parametrize("speed", SPEEDS)
def test_kernel_matches_the_model(speed):
    sq = tsm.speed_q(speed)
    x = _voiced(17000, int(speed * 8))
    rng = np.random.default_rng(5)
    plans = {}
    for size in (1920, 7680, 15360):
        n = -(-x.size // size)
        plans[str(size)] = [(size, min(size, x.size - size * j), j == n - 1) for j in range(n)]
    plans["whole"] = [(x.size, x.size, True)]
    cut, used = [], 0  # valid cut short mid-call, the stream ended mid-way, two calls after the end
    while used < 9000:
        v = int(rng.integers(0, 7680))
        cut.append((7680, v, False))
        used += v
    cut[-1] = (7680, cut[-1][1], True)
    plans["cut"] = cut + [(7680, 5000, False), (7680, 7680, True)]
    for name, calls in plans.items():
        model = tsm.Stretcher(sq)
        consumed = 0
        outs, states = _run_kernel(x, sq, calls)
        for j, (n_in, valid, last) in enumerate(calls):
            want = model.push(x[consumed:consumed + valid], last=last) if not model.ended else np.zeros(0, np.float32)
            consumed += valid
            got = outs[j]
            assert got.shape == want.shape, (name, j, got.shape, want.shape)
            if got.size:
                assert float(np.abs(got - want).max()) <= 1e-6, (name, j)
            st = states[j]
            assert st["k"] == model.k and st["n_out"] == model.n_out and st["ended"] == int(model.ended), (name, j, st)
            if model.k:
                assert st["p_prev"] == model.positions[model.k - 1], (name, j)
        if name != "cut":
            assert model.n_out == tsm.out_length(x.size, sq)


def test_32_slots_mixed_speeds_off_slots_and_formats():
    from smoltts_amd.engine import Resampler, TimeStretcher
    from smoltts_amd.formats import lin2ulaw

    B, tick = 32, 7680
    speeds = [SPEEDS[b % 6] if b % 7 != 3 else 1.0 for b in range(B)]
    formats = [["pcm_24000", "pcm_16000", "ulaw_8000", "pcm_48000"][b % 4] for b in range(B)]
    lens = [9000 + 1777 * b for b in range(B)]
    xs = [_voiced(n, 100 + b) for b, n in enumerate(lens)]
    dev = torch.device("cuda", 0)
    ts = TimeStretcher(dev, B)
    ts.reset_slots(list(range(B)), [tsm.speed_q(s) for s in speeds])
    rs = Resampler(dev, B, ts.out_samples(tick))
    rs.reset_slots(list(range(B)), formats)
    models = [tsm.Stretcher(tsm.speed_q(s)) if s != 1.0 else None for s in speeds]
    got_ts = [[] for _ in range(B)]
    got_rs = [[] for _ in range(B)]
    n_calls = -(-max(lens) // tick)
    for j in range(n_calls):
        pcm = np.zeros((B, tick), np.float32)
        valid = np.zeros(B, np.int32)
        last = np.zeros(B, np.int32)
        for b in range(B):
            seg = xs[b][j * tick:(j + 1) * tick]
            pcm[b, :seg.size] = seg
            valid[b] = seg.size
            last[b] = int(seg.size > 0 and (j + 1) * tick >= lens[b])
        pcm_d = torch.from_numpy(pcm).to(dev)
        out, cnt = ts.new_outputs(B, tick)
        ts.chunk(pcm_d, tick, out, cnt, valid=torch.from_numpy(valid).to(dev), last=torch.from_numpy(last).to(dev))
        ro, rc = rs.new_outputs(B)
        rs.chunk(out, out.shape[1], ro, rc, valid=cnt)
        out_h, cnt_h, ro_h, rc_h = out.cpu().numpy(), cnt.cpu().numpy(), ro.cpu().numpy(), rc.cpu().numpy()
        for b in range(B):
            if models[b] is None:
                assert cnt_h[b] == 0 and rc_h[b, 0] == 0
                continue
            if valid[b] or last[b]:
                want = models[b].push(xs[b][j * tick: j * tick + valid[b]], last=bool(last[b]))
                assert cnt_h[b] == want.size, (b, j)
                assert want.size == 0 or float(np.abs(out_h[b, :want.size] - want).max()) <= 1e-6, (b, j)
            else:
                assert cnt_h[b] == 0
            got_ts[b].append(out_h[b, :cnt_h[b]])
            if formats[b] != "pcm_24000":
                got_rs[b].append(rs.slot_bytes(ro_h, rc_h, b, tail=bool(last[b])))
    for b in range(B):
        if models[b] is None:
            continue
        y = np.concatenate(got_ts[b])
        assert y.size == tsm.out_length(lens[b], tsm.speed_q(speeds[b]))
        if formats[b] != "pcm_24000":
            got = np.concatenate(got_rs[b])
            want = _want_s16(tsm.stretch(xs[b], speeds[b]), int(formats[b].split("_")[1]))
            if formats[b] == "ulaw_8000":
                assert np.mean(got == lin2ulaw(want)) >= 0.999, b
            else:
                _close_s16(got, want, (b, formats[b]))
    ts.close()
    rs.close()


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


class _Launches:
    """Counts TimeStretcher.chunk calls (monkeypatched)."""

    def __init__(self, monkeypatch):
        from smoltts_amd import engine

        self.n = 0
        real = engine.TimeStretcher.chunk

        def chunk(ts, *a, **k):
            self.n += 1
            return real(ts, *a, **k)

        monkeypatch.setattr(engine.TimeStretcher, "chunk", chunk)


@pytest.mark.parametrize("overlap", [True, False])
def test_facade_stream_and_call_with_speed(tts, overlap, monkeypatch):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.formats import lin2ulaw

    gs = GenerationSettings.greedy(max_new_tokens=14)
    text, voice = "a stretched stream", "sky"
    ref = np.concatenate(list(tts.stream(text, voice, generation_settings=gs, overlap=overlap)))
    launches = _Launches(monkeypatch)
    same = np.concatenate(list(tts.stream(text, voice, generation_settings=gs, overlap=overlap, speed=1.0)))
    assert np.array_equal(same, ref) and launches.n == 0
    for speed, fmt in ((1.5, None), (0.5, "pcm_16000"), (2.0, "ulaw_8000"), (0.8, "pcm_48000")):
        chunks = list(tts.stream(text, voice, generation_settings=gs, overlap=overlap, speed=speed, output_format=fmt))
        assert all(c.size for c in chunks)
        want = tsm.stretch(ref, speed)
        got = np.concatenate(chunks)
        if fmt is None:
            assert got.dtype == np.float32 and got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-6
        elif fmt == "ulaw_8000":
            assert np.mean(got == lin2ulaw(_want_s16(want, 8000))) >= 0.999
        else:
            _close_s16(got, _want_s16(want, int(fmt.split("_")[1])), fmt)
    assert launches.n > 0
    block = tts(text, voice, generation_settings=gs)
    n0 = launches.n
    assert np.array_equal(tts(text, voice, generation_settings=gs, speed=1.0), block) and launches.n == n0
    got = tts(text, voice, generation_settings=gs, speed=2.0)
    want = tsm.stretch(block, 2.0)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-6
    with pytest.raises(ValueError):
        tts(text, voice, generation_settings=gs, speed=5.0)


def test_scheduler_speeds_and_formats(tts, monkeypatch):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.formats import lin2ulaw
    from smoltts_amd.server.scheduler import BatchScheduler

    reqs = [("first at one and a half", "heart", 9, 1.5, None), ("second slow and narrow", "sky", 12, 0.5, "pcm_16000"),
            ("third on the telephone", "nova", 7, 2.0, "ulaw_8000"), ("fourth stays plain", "bella", 10, None, "pcm_16000"),
            ("fifth refills a slot", "liam", 8, 4.0, None), ("sixth slow float", "heart", 6, 0.25, None)]
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=300))
    try:
        # the references: the same requests without speed or format, float32 from this scheduler
        base = {t: np.concatenate(list(sched.iter_chunks(sched.submit(t, v, stream=True, max_new_tokens=n)))) for t, v, n, _, _ in reqs}
        plain_block = np.concatenate(list(sched.iter_chunks(sched.submit("a blocking one", "sky", max_new_tokens=11))))
        launches = _Launches(monkeypatch)
        again = np.concatenate(list(sched.iter_chunks(sched.submit(reqs[0][0], "heart", stream=True, max_new_tokens=9, speed=1.0))))
        assert np.array_equal(again, base[reqs[0][0]]) and launches.n == 0 and sched._stream_conv.ts is None
        handles = [sched.submit(t, v, stream=True, max_new_tokens=n, speed=s, output_format=f) for t, v, n, s, f in reqs]
        blocking = sched.submit("a blocking one", "sky", max_new_tokens=11, speed=0.8)
        got = [np.concatenate(list(sched.iter_chunks(h))) for h in handles]
        got_block = np.concatenate(list(sched.iter_chunks(blocking)))
    finally:
        sched.close()
    for (t, v, n, s, f), g in zip(reqs, got):
        want = tsm.stretch(base[t], s) if s else base[t]
        if f is None:
            assert g.dtype == np.float32 and g.shape == want.shape and float(np.abs(g - want).max()) <= 1e-6, t
        elif f == "ulaw_8000":
            assert np.mean(g == lin2ulaw(_want_s16(want, 8000))) >= 0.999, t
        else:
            _close_s16(g, _want_s16(want, int(f.split("_")[1])), t)
    want = tsm.stretch(plain_block, 0.8)
    assert got_block.shape == want.shape and float(np.abs(got_block - want).max()) <= 1e-6
    assert launches.n > 0


def test_cloned_voice_seed_and_speed_same_bytes_in_two_slots(tts):
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.server.scheduler import BatchScheduler

    pe = tts.prompt_encoder
    spk = np.concatenate([pe.encode_text_turn("user", "a reference line for the voice"),
                          pe.encode_text_turn("assistant", "and its answer")], axis=1).astype(np.int32)
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=300))
    samp = RequestSampling(temperature=0.8, fast_temperature=0.6, min_p=0.0, seed=4242)
    try:
        sched.add_voice("cv_speed", grid=spk)
        # both at once: two slots, the same seed, voice and speed
        a, b = [sched.submit("the cloned voice, faster", "cv_speed", stream=True, max_new_tokens=12, sampling=samp, speed=1.5,
                             output_format="pcm_16000") for _ in range(2)]
        first = np.concatenate(list(sched.iter_chunks(a)))
        second = np.concatenate(list(sched.iter_chunks(b)))
    finally:
        sched.close()
    assert a.slot != b.slot
    assert first.dtype == np.int16 and first.size > 0 and np.array_equal(first, second)


def test_scheduler_blocking_speeds_in_flight_together(tts):
    """Several blocking utterances with speeds finish close together: their stretches are queued on a side stream and handed
    over when done, each equal to the model's stretch of the same request without a speed; one cancelled request ends quietly."""
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    reqs = [(f"blocking request number {i}", ["heart", "sky", "nova"][i % 3], 6 + i, s)
            for i, s in enumerate([0.25, 0.5, 1.5, 2.0, 4.0, 0.8])]
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=300))
    try:
        base = [np.concatenate(list(sched.iter_chunks(sched.submit(t, v, max_new_tokens=n)))) for t, v, n, _ in reqs]
        victim = sched.submit("a blocking request whose client leaves", "sky", max_new_tokens=20, speed=0.5)
        handles = [sched.submit(t, v, max_new_tokens=n, speed=s) for t, v, n, s in reqs]
        sched.cancel(victim)
        got = [list(sched.iter_chunks(h)) for h in handles]
        assert list(sched.iter_chunks(victim)) == []
        assert not sched._stretches
    finally:
        sched.close()
    for (t, v, n, s), b, g in zip(reqs, base, got):
        assert len(g) == 1, t  # one chunk: the stretched utterance
        want = tsm.stretch(b, s)
        assert g[0].shape == want.shape and float(np.abs(g[0] - want).max()) <= 1e-6, t
