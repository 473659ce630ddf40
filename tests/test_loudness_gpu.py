"""The loudness stage on the device against its numpy model (``smoltts_amd/loudness.py``): the stream kernel sample for sample and
state for state, the whole-utterance helpers, the stage inside ``StreamConverter`` beside and in front of the other stages, the
front ends on the tiny checkpoint, and the stage's bad-argument cases."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import engine, loudness as L  # noqa: E402


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _speechlike(seed, seconds, level):
    """Shaped noise in bursts and pauses, with a slow swell, so that blocks fall on both sides of both gates."""
    rng = np.random.default_rng(seed)
    n = int(seconds * L.FS)
    x = rng.standard_normal(n)
    x = np.convolve(x, np.ones(8) / 8, mode="same")
    t = np.arange(n) / L.FS
    env = (np.sin(2 * np.pi * 0.7 * t + seed) > -0.3) * (0.4 + 0.6 * np.abs(np.sin(2 * np.pi * 0.11 * t)))
    return (level * env * x).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_state(dev_state, model, what):
    m = model.state()
    for k in ("pos", "ka", "kb"):
        assert dev_state[k] == m[k], (what, k, dev_state[k], m[k])
    assert _bits(dev_state["peak"]) == _bits(m["peak"]), what
    assert np.array_equal(dev_state["filter"].view(np.uint64), m["filter"].view(np.uint64)), what
    assert np.array_equal(dev_state["ring"].view(np.uint64), m["ring"].view(np.uint64)), what
    assert dev_state["ptarget"] == model.ptarget


# ------------------------------------------------------------------------------- the kernel against the model
def test_stream_kernel_equals_the_model_bit_for_bit(device):
    B = 6
    targets = [-20.0, -16.0, -30.0, -23.0, None, -12.5]
    starts = [0.0, 6.0, -3.5, 20.0, 0.0, -20.0]
    levels = [0.05, 0.3, 0.01, 0.9, 0.1, 0.002]
    sig = [_speechlike(b, 9.0, levels[b]) for b in range(B)]
    sig[3][5000:5100] = 1.0  # a full-scale click: the peak cap binds against the +20 dB start
    rng = np.random.default_rng(7)
    ln = engine.LoudnessNormalizer(device, B)
    try:
        ln.reset_slots(list(range(B)), targets, starts)
        models = [None if t is None else L.StreamState(t, s) for t, s in zip(targets, starts)]
        cursor = [0] * B
        compared = 0
        for call in range(40):
            frames = int(rng.integers(1, 5))
            n_in = frames * 1920
            batch = B if call % 5 else int(rng.integers(2, B))  # some calls leave the last slots out: they carry their state
            if call == 17:  # slot 1 starts a new stream mid-run, the others go on
                ln.reset_slots([1], [-18.0], [-2.0])
                models[1] = L.StreamState(-18.0, -2.0)
            valid = rng.integers(0, n_in + 1, size=B).astype(np.int32)
            valid[call % B] = n_in
            if call % 7 == 0:
                valid[(call + 1) % B] = 0
            pcm = np.zeros((batch, n_in), np.float32)
            for b in range(batch):
                valid[b] = min(valid[b], sig[b].size - cursor[b])
                pcm[b, :valid[b]] = sig[b][cursor[b]: cursor[b] + valid[b]]
            pcm_d = torch.from_numpy(pcm).to(device)
            valid_d = torch.from_numpy(valid[:batch].copy()).to(device)
            out, counts = ln.new_outputs(batch, n_in)
            ln.chunk(pcm_d, n_in, out, counts, valid=valid_d)
            out, counts = out.cpu().numpy(), counts.cpu().numpy()
            for b in range(batch):
                if models[b] is None:
                    assert counts[b] == 0
                    continue
                want = models[b].process(pcm[b, :valid[b]])
                assert counts[b] == valid[b]
                assert np.array_equal(_bits(out[b, :valid[b]]), _bits(want)), (call, b)
                cursor[b] += int(valid[b])
                compared += int(valid[b])
            if call in (3, 16, 17, 39):
                for b in range(B):
                    st = ln.slot_state(b)
                    if models[b] is None:
                        assert st["on"] == 0
                    else:
                        _assert_state(st, models[b], (call, b))
        assert compared > 300000
        # the run moved knots, passed both gates and hit the cap: the comparison above covered all of it
        assert any(len(set(m.knots)) > 10 for m in models if m is not None)
        assert min(models[3].knots) < L.knot_of_db(20.0)
    finally:
        ln.close()


def test_one_sample_calls_and_a_seam_wide_row(device):
    """Calls of a single sample, then one call as wide as a row behind the seam (more than one round of 256 sub-blocks)."""
    x = _speechlike(11, 4.0, 0.08)
    ln = engine.LoudnessNormalizer(device, 2)
    try:
        ln.reset_slots([0, 1], [-20.0, -20.0])
        m = L.StreamState(-20.0)
        for i in range(700):
            row = torch.from_numpy(np.stack([x[i:i + 1], x[i:i + 1]])).to(device)
            out, counts = ln.new_outputs(2, 1)
            ln.chunk(row, 1, out, counts)
            assert np.array_equal(_bits(out.cpu().numpy()[1]), _bits(m.process(x[i:i + 1])))
        wide = 7680 + 24240 + 36000
        row = torch.from_numpy(np.stack([x[700:700 + wide]] * 2)).to(device)
        out, counts = ln.new_outputs(2, wide)
        ln.chunk(row, wide, out, counts)
        want = m.process(x[700:700 + wide])
        assert np.array_equal(_bits(out.cpu().numpy()[1]), _bits(want)) and counts.cpu().tolist() == [wide, wide]
        _assert_state(ln.slot_state(1), m, "wide")
        _assert_state(ln.slot_state(0), m, "wide, slot 0")
    finally:
        ln.close()


# ------------------------------------------------------------------------------- whole utterances
@pytest.mark.parametrize("seconds, level", [(6.3, 0.05), (2.0, 0.5), (31.0, 0.02), (0.3, 0.1), (1.0, 0.0)])
def test_whole_utterance_helpers_equal_the_model(device, seconds, level):
    x = _speechlike(3, seconds, level)
    lufs, peak = engine.measure_loudness(x, device)
    want_lufs, want_peak = L.measure(x)
    assert peak == want_peak
    if np.isinf(want_lufs):
        assert lufs == want_lufs
    else:
        assert abs(lufs - want_lufs) <= 1e-9
    for target in (-20.0, -8.0):
        y, g = engine.loudness_normalize(x, target, device, with_gain=True)
        want, want_g = L.normalize(x, target)
        assert g == want_g
        assert np.array_equal(_bits(y), _bits(want))
    assert engine.measure_loudness(np.zeros(0, np.float32), device) == (float("-inf"), 0.0)


# ------------------------------------------------------------------------------- bad arguments
def test_loudness_stage_refuses_bad_arguments(device):
    lib = engine.load_library()
    ln = engine.LoudnessNormalizer(device, 2)
    stream = engine.current_stream_ptr()
    try:
        tab = L.tables().packed()
        h = C.c_void_p()
        need = lib.smoltts_loudness_bytes(2)
        assert lib.smoltts_loudness_bytes(0) == 0 and need > 0
        slab = engine._alloc_slab(need, device, settle=True)
        assert lib.smoltts_loudness_create(engine.dptr(slab), need - 256, 2, tab.ctypes.data, tab.size, C.byref(h)) != 0
        assert lib.smoltts_loudness_create(engine.dptr(slab), need, 2, tab.ctypes.data, tab.size - 1, C.byref(h)) != 0
        assert lib.smoltts_loudness_create(engine.dptr(slab), need, 2, None, tab.size, C.byref(h)) != 0
        assert lib.smoltts_loudness_create(engine.dptr(slab) + 8, need, 2, tab.ctypes.data, tab.size, C.byref(h)) != 0
        with pytest.raises(engine.SmolttsError, match="slab has"):
            engine.check(lib.smoltts_loudness_create(engine.dptr(slab), 256, 2, tab.ctypes.data, tab.size, C.byref(h)), "create")

        one, pw, kn = (C.c_int32 * 1)(0), (C.c_double * 1)(0.01), (C.c_int32 * 1)(0)
        assert lib.smoltts_loudness_reset_slots(ln.handle, (C.c_int32 * 1)(2), pw, kn, 1, stream) != 0   # slot out of range
        assert lib.smoltts_loudness_reset_slots(ln.handle, (C.c_int32 * 1)(-1), pw, kn, 1, stream) != 0
        assert lib.smoltts_loudness_reset_slots(ln.handle, one, (C.c_double * 1)(1.5), kn, 1, stream) != 0
        assert lib.smoltts_loudness_reset_slots(ln.handle, one, (C.c_double * 1)(float("nan")), kn, 1, stream) != 0
        assert lib.smoltts_loudness_reset_slots(ln.handle, one, pw, (C.c_int32 * 1)(1281), 1, stream) != 0
        assert lib.smoltts_loudness_reset_slots(ln.handle, one, pw, kn, 0, stream) != 0
        assert lib.smoltts_loudness_reset_slots(ln.handle, one, None, kn, 1, stream) != 0
        assert lib.smoltts_loudness_reset_slots(ln.handle, one, pw, None, 1, stream) == 0  # (no start knots: 0 dB)

        pcm = torch.zeros(2, 1920, device=device)
        out, counts = ln.new_outputs(2, 1920)
        args = dict(pcm=engine.dptr(pcm), stride=1920, batch=2, n_in=1920, out=engine.dptr(out), ostride=1920, counts=engine.dptr(counts))

        def chunk(**kw):
            a = dict(args, **kw)
            return lib.smoltts_loudness_chunk(ln.handle, a["pcm"], a["stride"], a["batch"], a["n_in"], None, a["out"], a["ostride"],
                                              a["counts"], stream)

        assert chunk(batch=3) != 0 and chunk(batch=0) != 0
        assert chunk(n_in=-1) != 0 and chunk(stride=1000) != 0
        assert chunk(ostride=1919) != 0
        assert chunk(pcm=None) != 0 and chunk(out=None) != 0 and chunk(counts=None) != 0
        assert lib.smoltts_loudness_chunk(None, args["pcm"], 1920, 2, 1920, None, args["out"], 1920, args["counts"], stream) != 0
        with pytest.raises(engine.SmolttsError, match="out_stride"):
            engine.check(chunk(ostride=10), "chunk")
        assert chunk() == 0

        hops, res = torch.zeros(4, dtype=torch.float64, device=device), torch.zeros(4, dtype=torch.float64, device=device)
        assert lib.smoltts_loudness_measure(ln.handle, engine.dptr(pcm), 1920 * 2, engine.dptr(hops), 0, engine.dptr(res), stream) != 0
        assert lib.smoltts_loudness_measure(ln.handle, engine.dptr(pcm), -1, engine.dptr(hops), 4, engine.dptr(res), stream) != 0
        assert lib.smoltts_loudness_measure(ln.handle, None, 10, engine.dptr(hops), 4, engine.dptr(res), stream) != 0
        assert lib.smoltts_loudness_scale(engine.dptr(pcm), 10, -1.0, engine.dptr(out), stream) != 0
        assert lib.smoltts_loudness_scale(engine.dptr(pcm), 10, float("nan"), engine.dptr(out), stream) != 0
        assert lib.smoltts_loudness_scale(None, 10, 1.0, engine.dptr(out), stream) != 0
        ints, vals = (C.c_int64 * 4)(), np.zeros(531)
        assert lib.smoltts_loudness_slot_state(ln.handle, 2, ints, vals.ctypes.data, stream) != 0
        assert lib.smoltts_loudness_slot_state(ln.handle, 0, None, vals.ctypes.data, stream) != 0
        torch.cuda.synchronize()
    finally:
        ln.close()


# ------------------------------------------------------------------------------- through the converter
def test_slots_without_loudness_keep_their_bytes_beside_one_with_it(device):
    """Two converters fed the same rows: in one, slot 0 also asks for loudness.  Slot 1 (pcm_16000, a speed) and slot 2 (FLAC)
    give the same bytes in both; slot 0's float32 equals the model, and its converted bytes the resampler fed the model's."""
    x = np.stack([_speechlike(20 + b, 2.0, 0.1) for b in range(3)])
    outs = []
    for with_loudness in (True, False):
        conv = engine.StreamConverter(device, 3, 1920)
        try:
            conv.reset_slots([0, 1, 2], ["pcm_16000", "pcm_16000", None], [None, 80000, None], [None, None, "flac"],
                             [-18.0 if with_loudness else None, None, None], [2.0 if with_loudness else None, None, None])
            assert (conv.ln is not None) == with_loudness
            got = [[], [], []]
            n = x.shape[1] // 1920
            for f in range(n):
                pcm = torch.from_numpy(x[:, f * 1920:(f + 1) * 1920].copy()).to(device)
                valid = torch.full((3,), 1920, dtype=torch.int32, device=device)
                last = torch.full((3,), int(f == n - 1), dtype=torch.int32, device=device)
                p = conv.run(pcm, 1920, valid, last)
                assert ("loudness" in p.plan.stages) == with_loudness
                p.to_host(torch.cuda.current_stream())
                torch.cuda.synchronize()
                for b in range(3):
                    got[b].append(p.chunk(b, f == n - 1))
            outs.append([np.concatenate(g) for g in got])
        finally:
            conv.close()
    (a0, a1, a2), (b0, b1, b2) = outs
    assert a1.tobytes() == b1.tobytes() and a2.tobytes() == b2.tobytes() and a0.tobytes() != b0.tobytes()
    want = L.stream_normalize(x[0, : 1920 * (x.shape[1] // 1920)], -18.0, 2.0)
    rs = engine.Resampler(device, 1, want.size)
    try:
        rs.reset_slots([0], ["pcm_16000"])
        out, counts = rs.new_outputs(1, want.size)
        rs.chunk(torch.from_numpy(want).to(device)[None], want.size, out, counts)
        ref = rs.slot_bytes(out.cpu().numpy(), counts.cpu().numpy(), 0, tail=True)
    finally:
        rs.close()
    assert a0.shape == ref.shape and int(np.abs(a0.astype(np.int32) - ref.astype(np.int32)).max()) <= 1


# ------------------------------------------------------------------------------- end to end on the tiny checkpoint
@pytest.fixture(scope="module")
def tts(device):
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


TEXT = 'The first sentence is here. A second one follows it! <break time="0.5s"/> And then a third, which ends the text.'
OPTS = {"max_bytes": 40, "pause_s": 0.2}


def _at_target_or_ceiling(y, target):
    lufs, peak = L.measure(y)
    print(f"measured {lufs:.6f} LUFS, peak {peak:.6f}")
    return abs(lufs - target) <= 1e-4 or abs(peak - L.tables().ceiling) <= 1e-6


def test_facade_blocking_and_stream(tts):
    from smoltts_amd import seam, tsm
    from smoltts_amd.config import GenerationSettings

    from flac_decode_helpers import decode_mono16

    gs = GenerationSettings.greedy(max_new_tokens=14)
    plain = tts("Level this sentence, please.", "nova", generation_settings=gs)
    assert L.measure(plain)[0] > -70.0, "the tiny checkpoint's audio must be measurable for this test to say anything"
    got = tts("Level this sentence, please.", "nova", generation_settings=gs, loudness=-20.0)
    want, g = L.normalize(plain, -20.0)
    assert np.array_equal(_bits(got), _bits(want)) and tts.last_loudness_gain_db == L.gain_db(g)
    assert _at_target_or_ceiling(got, -20.0)
    again = tts("Level this sentence, please.", "nova", generation_settings=gs, loudness=None)
    assert np.array_equal(_bits(again), _bits(plain))  # no field: the path without the feature
    # segmented and stretched: behind the seam join, in front of the stretch
    joined = tts(TEXT, "sky", generation_settings=gs, segment=OPTS)
    got = tts(TEXT, "sky", generation_settings=gs, segment=OPTS, loudness=-24.0, speed=1.25)
    want = tsm.stretch(L.normalize(joined, -24.0)[0], 1.25)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-6
    assert _at_target_or_ceiling(tts(TEXT, "sky", generation_settings=gs, segment=OPTS, loudness=-24.0), -24.0)

    # streams: the model applied to the stream's own float PCM
    ref = np.concatenate(list(tts.stream("Level this sentence, please.", "nova", generation_settings=gs)))
    chunks = list(tts.stream("Level this sentence, please.", "nova", generation_settings=gs, loudness=-20.0, loudness_start_gain_db=4.0))
    assert all(c.size == 1920 for c in chunks)  # every frame's samples leave with the frame
    assert np.array_equal(_bits(np.concatenate(chunks)), _bits(L.stream_normalize(ref, -20.0, 4.0)))
    # segmented, stretched, converted and framed: seam -> loudness -> stretch -> resample -> flac
    ref = np.concatenate(list(tts.stream(TEXT, "sky", generation_settings=gs, segment=OPTS)))
    data = b"".join(c.tobytes() for c in tts.stream(TEXT, "sky", generation_settings=gs, segment=OPTS, loudness=-22.0, speed=1.5,
                                                     output_format="pcm_16000", container="flac"))
    assert data[:4] == b"fLaC" and data.count(b"fLaC") == 1
    samples = np.asarray(decode_mono16(data), np.int16)
    chain = tsm.stretch(L.stream_normalize(ref, -22.0), 1.5)
    rs = engine.Resampler(tts.lm.device, 1, chain.size)
    try:
        rs.reset_slots([0], ["pcm_16000"])
        out, counts = rs.new_outputs(1, chain.size)
        rs.chunk(torch.from_numpy(chain).to(tts.lm.device)[None], chain.size, out, counts)
        want = rs.slot_bytes(out.cpu().numpy(), counts.cpu().numpy(), 0, tail=True)
    finally:
        rs.close()
    assert samples.shape == want.shape and int(np.abs(samples.astype(np.int32) - want.astype(np.int32)).max()) <= 1


def test_scheduler_and_speech_route(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler

    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=14))
    try:
        text = "Level this sentence, please."
        def run(**kw):
            return np.concatenate(list(sched.iter_chunks(sched.submit(text, "nova", **kw))))

        # before any request has named a loudness: the routes as they were (a stream's float PCM and a blocking utterance's come
        # from different codec passes, so each is compared with its own kind)
        plain, raw0 = run(), run(stream=True)
        assert sched._stream_conv.ln is None
        req = sched.submit(text, "nova", loudness=-20.0)
        block = np.concatenate(list(sched.iter_chunks(req)))
        want, g = L.normalize(plain, -20.0)
        assert np.array_equal(_bits(block), _bits(want)) and req.loudness_gain_db == L.gain_db(g)
        assert _at_target_or_ceiling(block, -20.0)
        stream = run(stream=True, loudness=-20.0, loudness_start_gain_db=-3.0)
        assert sched._stream_conv.ln is not None
        assert np.array_equal(_bits(stream), _bits(L.stream_normalize(raw0, -20.0, -3.0)))
        # the field omitted, now that the stage exists, alone and beside streams that name it: the same bytes as before
        assert np.array_equal(_bits(run(stream=True)), _bits(raw0)) and np.array_equal(_bits(run()), _bits(plain))
        reqs = [sched.submit(text, "nova", stream=True, loudness=-20.0), sched.submit(text, "nova", stream=True),
                sched.submit(text, "nova", stream=True, loudness=-30.0, output_format="pcm_16000")]
        a, b, c16 = [np.concatenate(list(sched.iter_chunks(r))) for r in reqs]
        assert np.array_equal(_bits(a), _bits(L.stream_normalize(b, -20.0))) and c16.dtype == np.int16 and c16.size
        with pytest.raises(ValueError, match="loudness"):
            sched.submit(text, "nova", loudness=-3.0)

        c = TestClient(create_app(tts, scheduler=sched))
        r0 = c.post("/v1/audio/speech", json={"input": text, "voice": "nova"})
        r1 = c.post("/v1/audio/speech", json={"input": text, "voice": "nova", "loudness": -20})
        assert r0.status_code == 200 and r1.status_code == 200 and "x-loudness-gain-db" not in r0.headers
        assert r1.headers["x-loudness-gain-db"] == f"{L.gain_db(g):.2f}" and r1.content != r0.content
        from smoltts_amd.server.wav import pcm_to_wav_bytes

        assert r0.content == pcm_to_wav_bytes(plain, 24000) and r1.content == pcm_to_wav_bytes(want, 24000)
        assert c.post("/v1/audio/speech", json={"input": text, "voice": "nova", "loudness": -50}).status_code == 400
    finally:
        sched.close()
