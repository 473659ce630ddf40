"""Long texts as chained segments on the GPU: the seam kernel against the numpy model, and the façade's segmented call and
stream against their definitions (chained prompts, segment seeds, the seam model of each segment's audio)."""
import numpy as np
import pytest

from smoltts_amd import seam
from smoltts_amd.seam import D, FINAL, FIRST, H, SeamState

pytestmark = pytest.mark.gpu


def _speech(n, rng, amp=0.3):
    x = rng.uniform(-amp, amp, n).astype(np.float32)
    x[::40] = amp
    return x


def _quiet(n, rng):
    return rng.uniform(-0.5, 0.5, n).astype(np.float32) * np.float32(2 ** -9)


def _segment(rng):
    parts = []
    for _ in range(int(rng.integers(1, 4))):
        parts.append(_quiet(int(rng.choice([0, 100, 240, 3000, H - 7, H + 2000, D + 5000])), rng))
        parts.append(_speech(int(rng.integers(1, 5000)), rng))
    parts.append(_quiet(int(rng.choice([0, 239, 4800, H + 3000])), rng))
    return np.concatenate(parts)


def test_seam_kernel_matches_model_across_slots_and_chunkings():
    import torch

    from smoltts_amd.engine import SEAM_OFF, SeamJoiner

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    B, n_row = 6, 4 * 1920
    on = [0, 1, 2, 4, 5]  # slot 3 stays off
    plans = {}
    for b in on:
        nseg = int(rng.integers(1, 4)) if b != 5 else 1
        segs = [_segment(rng) for _ in range(nseg)]
        pauses = [int(rng.choice([0, 2400, 6000, 72000])) for _ in range(nseg - 1)]
        plans[b] = dict(segs=segs, pauses=pauses, lead=int(rng.choice([0, 1234])), trail=int(rng.choice([0, 777])))
    sj = SeamJoiner(dev, B)
    models = {b: SeamState() for b in on}
    pos = {b: [0, 0] for b in on}  # (segment, offset)
    got = {b: [] for b in on}
    want = {b: [] for b in on}

    def start(b):
        p, (k, _) = plans[b], pos[b]
        final = k == len(p["segs"]) - 1
        pause = p["trail"] if final else p["pauses"][k]
        flags = (FIRST if k == 0 else 0) | (FINAL if final else 0)
        sj.start_segments([b], [pause], [flags], [p["lead"]])
        models[b].start(pause, flags, p["lead"])

    for b in on:
        start(b)
    sj.start_segments([3], [0], [SEAM_OFF])
    calls = 0
    while any(pos[b][0] < len(plans[b]["segs"]) for b in on):
        batch = int(rng.integers(1, B + 1))  # slots past the batch carry their state
        pcm = np.zeros((batch, n_row), np.float32)
        valid = np.zeros(batch, np.int32)
        end = np.zeros(batch, np.int32)
        live = [b for b in on if b < batch and pos[b][0] < len(plans[b]["segs"])]
        for b in live:
            k, off = pos[b]
            x = plans[b]["segs"][k]
            n = int(min(x.size - off, rng.integers(1, n_row + 1)))
            if rng.random() < 0.5:
                n = min(x.size - off, int(rng.integers(1, 4)) * 1920)
            pcm[b, :n] = x[off:off + n]
            pcm[b, n:] = 7.0  # past valid: never read
            valid[b] = n
            end[b] = off + n == x.size
        pcm_d, valid_d, end_d = (torch.from_numpy(a).to(dev) for a in (pcm, valid, end))
        out, counts = sj.new_outputs(batch, n_row)
        sj.chunk(pcm_d, n_row, out, counts, valid=valid_d, seg_end=end_d)
        out_h, counts_h = out.cpu().numpy(), counts.cpu().numpy()
        calls += 1
        assert counts_h[3] == 0 if batch > 3 else True
        for b in live:
            k, off = pos[b]
            y = models[b].push(pcm[b, :valid[b]], end=bool(end[b]))
            assert counts_h[b] == y.size, (b, calls)
            np.testing.assert_array_equal(out_h[b, :y.size], y)
            got[b].append(out_h[b, :y.size].copy())
            want[b].append(y)
            pos[b][1] += int(valid[b])
            if end[b]:
                pos[b] = [k + 1, 0]
                if k + 1 < len(plans[b]["segs"]):
                    start(b)
            else:
                st = sj.slot_state(b)
                m = models[b]
                assert (st["n_in"], st["judged"], st["ec"], st["head"], st["open"]) == (m.n_in, m.judged, m.ec, int(m.head), 1)
    for b in on:
        p = plans[b]
        whole = seam.join(p["segs"], p["pauses"], lead=p["lead"], trail=p["trail"])
        np.testing.assert_array_equal(np.concatenate(got[b]), whole)
        assert sj.slot_state(b)["open"] == 0
    sj.close()


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


TEXT = 'The first sentence is here. A second one follows it! <break time="0.5s"/> And then a third, which ends the text.'
OPTS = {"max_bytes": 40, "pause_s": 0.2}


def _raw_stream(tts, prompt, gs, sampling):
    """One prompt streamed on its own as float32 (what a segment's codec output is)."""
    from smoltts_amd.engine import LMSession, MimiSession
    from smoltts_amd.generate import _apply_sampling, _apply_slot_sampling, stream_pcm

    max_new = gs.max_new_tokens
    T = int(prompt.shape[1])
    sess = LMSession(tts.lm, 1, max_seq=min(tts.config.max_seq_len, T + max_new + 2), max_rows=T, max_frames=max_new + 1)
    _apply_sampling(sess, gs)
    if sampling is not None:
        _apply_slot_sampling(sess, [0], [r.resolve(gs) for r in sampling])
    ms = MimiSession(tts.codec, max_batch=1, max_chunk_frames=1)
    try:
        return np.concatenate(list(stream_pcm(sess, ms, prompt)))
    finally:
        ms.close()
        sess.close()


@pytest.mark.parametrize("seeded", [False, True])
def test_facade_segmented_call_and_stream(tts, seeded):
    import dataclasses

    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.longform import chain_prompt, segment_seed, split_text, voice_prefix
    from smoltts_amd.seam import pause_samples

    gs = GenerationSettings.greedy(max_new_tokens=10)
    sampling = RequestSampling(temperature=0.8, fast_temperature=0.8, seed=1234) if seeded else None
    segs = split_text(TEXT, OPTS["max_bytes"])
    assert len(segs) == 3
    pcm = tts(TEXT, "nova", generation_settings=gs, sampling=sampling, segment=OPTS)
    info = tts.last_segments
    assert [i["text"] for i in info] == [s.text for s in segs]
    pre = voice_prefix(tts.prompt_encoder, "nova")
    pieces = []
    for k, it in enumerate(info):
        prev = (info[k - 1]["text"], info[k - 1]["codes"]) if k else (None, None)
        prompt = chain_prompt(tts.prompt_encoder, pre, it["text"], *prev, max_new_tokens=10, max_seq=tts.config.max_seq_len)
        np.testing.assert_array_equal(it["prompt"], prompt)
        samp_k = [dataclasses.replace(sampling, seed=segment_seed(1234, k))] if seeded else None
        codes = tts.generate_prompt_codes([prompt], gs, samp_k)[0]
        np.testing.assert_array_equal(it["codes"], codes)
        if seeded:
            assert it["seed"] == segment_seed(1234, k)
        pieces.append(tts.decode_codes(codes))
    if seeded:  # segment 0 of a segmented request is the plain request
        np.testing.assert_array_equal(info[0]["codes"], tts.generate_codes([segs[0].text], ["nova"], gs, sampling=sampling)[0])
    pauses = [pause_samples(s.pause_after_s if s.pause_after_s is not None else 0.2) for s in segs[:-1]]
    want = seam.join(pieces, pauses)
    np.testing.assert_array_equal(pcm, want)

    # the stream: the seam model of each segment's own stream, in one float32 stream
    chunks = list(tts.stream(TEXT, "nova", generation_settings=gs, sampling=sampling, segment=OPTS))
    sinfo = tts.last_segments
    raws = []
    for k, it in enumerate(sinfo):
        np.testing.assert_array_equal(it["codes"], info[k]["codes"])
        samp_k = [dataclasses.replace(sampling, seed=segment_seed(1234, k))] if seeded else None
        raws.append(_raw_stream(tts, it["prompt"], gs, samp_k))
    np.testing.assert_array_equal(np.concatenate(chunks), seam.join(raws, pauses))


def test_facade_segmented_formats_speed_and_flac(tts):
    from smoltts_amd import tsm
    from smoltts_amd.config import GenerationSettings

    from flac_decode_helpers import decode_mono16

    gs = GenerationSettings.greedy(max_new_tokens=10)
    ref = np.concatenate(list(tts.stream(TEXT, "sky", generation_settings=gs, segment=OPTS)))
    fl = list(tts.stream(TEXT, "sky", generation_settings=gs, segment=OPTS, container="flac"))
    data = b"".join(c.tobytes() for c in fl)
    assert data[:4] == b"fLaC" and data.count(b"fLaC") == 1
    samples = decode_mono16(data)
    q = np.rint(np.clip(ref, -1, 1) * np.float32(32767)).astype(np.int16)
    np.testing.assert_array_equal(np.asarray(samples, np.int16), q)
    sped = np.concatenate(list(tts.stream(TEXT, "sky", generation_settings=gs, segment=OPTS, speed=1.5)))
    want = tsm.stretch(ref, 1.5)
    assert sped.shape == want.shape and float(np.abs(sped - want).max()) <= 1e-6
    import torch

    from smoltts_amd.engine import Resampler

    for fmt in ("pcm_16000", "ulaw_8000"):  # the joined float32 converted in one call: what the stream's chunks add up to
        got = np.concatenate(list(tts.stream(TEXT, "sky", generation_settings=gs, segment=OPTS, output_format=fmt)))
        rs = Resampler(tts.lm.device, 1, ref.size)
        rs.reset_slots([0], [fmt])
        out, counts = rs.new_outputs(1, ref.size)
        rs.chunk(torch.from_numpy(ref).to(tts.lm.device)[None], ref.size, out, counts)
        want = rs.slot_bytes(out.cpu().numpy(), counts.cpu().numpy(), 0, tail=True)
        rs.close()
        assert got.dtype == want.dtype and got.shape == want.shape
        assert int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max(initial=0)) <= (1 if fmt == "pcm_16000" else 255)
        if fmt == "ulaw_8000":
            assert np.mean(got == want) >= 0.999
    block = tts(TEXT, "sky", generation_settings=gs, segment=OPTS, speed=2.0)
    assert block.size == tsm.out_length(tts(TEXT, "sky", generation_settings=gs, segment=OPTS).size, tsm.speed_q(2.0))


def test_short_text_takes_the_plain_path(tts, monkeypatch):
    from smoltts_amd import engine
    from smoltts_amd.config import GenerationSettings

    calls = []
    real = engine.SeamJoiner.chunk
    monkeypatch.setattr(engine.SeamJoiner, "chunk", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    gs = GenerationSettings.greedy(max_new_tokens=8)
    text = "A short request."
    np.testing.assert_array_equal(tts(text, "heart", generation_settings=gs, segment=True), tts(text, "heart", generation_settings=gs))
    a = np.concatenate(list(tts.stream(text, "heart", generation_settings=gs, segment=True)))
    np.testing.assert_array_equal(a, np.concatenate(list(tts.stream(text, "heart", generation_settings=gs))))
    assert not calls


def test_server_long_text(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app

    tts_gs = tts._settings
    tts._settings = lambda g=None: g or GenerationSettings.greedy(max_new_tokens=6)
    try:
        text = " ".join(f"Sentence number {i} of a rather long text." for i in range(70))
        assert 2800 <= len(text) <= 3200
        seg = TestClient(create_app(tts, {"long_text": "segment", "segment_max_bytes": 300}))
        r = seg.post("/v1/audio/speech", json={"input": text, "voice": "heart"})
        assert r.status_code == 200 and r.content[:4] == b"RIFF"
        r = seg.post("/v1/audio/speech", json={"input": text, "voice": "heart", "response_format": "flac"})
        assert r.status_code == 200 and r.content[:4] == b"fLaC"
        assert seg.get("/v1/stats").json()["segments"] == 2 * len(__import__("smoltts_amd.longform").longform.split_text(text, 300))
    finally:
        tts._settings = tts_gs
