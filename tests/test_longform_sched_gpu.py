"""Long texts in the batched scheduler (GPU): segmented requests keep their slot from segment to segment, next to ordinary
requests, and give what the façade gives; the seam kernel's stream-end release; the server's long_text mode behind a scheduler."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TEXT = 'The first sentence is here. A second one follows it! <break time="0.5s"/> And then a third, which ends the text.'
OPTS = {"max_bytes": 40, "pause_s": 0.2}


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


def _s16_close(got, want):
    got, want = np.asarray(got, np.int32), np.asarray(want, np.int32)
    assert got.shape == want.shape and int(np.abs(got - want).max(initial=0)) <= 1


def test_seam_kernel_releases_held_run_at_stream_end():
    import torch

    from smoltts_amd.engine import SeamJoiner
    from smoltts_amd.seam import SeamState

    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-0.3, 0.3, 5000), rng.uniform(-1, 1, 9000) * 2 ** -10]).astype(np.float32)
    dev = torch.device("cuda", 0)
    sj = SeamJoiner(dev, 2)
    sj.start_segments([0, 1], [6000, 6000], [0, 0])  # middle segments: their tails are held
    m = SeamState()
    m.start(6000, 0)
    got, want = [], []
    for a, b in ((0, 4000), (4000, 11000), (11000, x.size)):
        last = b == x.size
        pcm = torch.from_numpy(np.stack([x[a:b], x[a:b]])).to(dev)
        out, cnt = sj.new_outputs(2, b - a)
        sj.chunk(pcm, b - a, out, cnt, last=torch.tensor([int(last), 0], dtype=torch.int32, device=dev))
        c = int(cnt.cpu()[0])
        got.append(out[0, :c].cpu().numpy())
        want.append(m.push(x[a:b], last=last))
    np.testing.assert_array_equal(np.concatenate(got), np.concatenate(want))
    np.testing.assert_array_equal(np.concatenate(got), x)  # a stream that ends in a middle segment keeps its tail
    assert sj.slot_state(0)["open"] == 0 and sj.slot_state(1)["open"] == 1
    sj.close()


@pytest.mark.parametrize("side", [True, False])
def test_scheduler_segmented_next_to_ordinary_requests(tts, side):
    from flac_decode_helpers import decode_mono16

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    gs = GenerationSettings.greedy(max_new_tokens=10)
    ref = np.concatenate(list(tts.stream(TEXT, "nova", generation_settings=gs, segment=OPTS)))
    ref16 = np.concatenate(list(tts.stream(TEXT, "nova", generation_settings=gs, segment=OPTS, output_format="pcm_16000")))
    ref_block = tts(TEXT, "nova", generation_settings=gs, segment=OPTS)
    ref_sped = tts(TEXT, "nova", generation_settings=gs, segment=OPTS, speed=1.5)
    plain = np.concatenate(list(tts.stream("an ordinary request", "sky", generation_settings=gs)))
    plain_block = tts("another ordinary one", "bella", generation_settings=gs)
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=gs, side_prefill=side,
                           side_prefill_min_active=1)
    try:
        reqs = {
            "f32": sched.submit(TEXT, "nova", stream=True, segment=OPTS),
            "plain": sched.submit("an ordinary request", "sky", stream=True),
            "s16": sched.submit(TEXT, "nova", stream=True, output_format="pcm_16000", segment=OPTS),
            "flac": sched.submit(TEXT, "nova", stream=True, container="flac", segment=OPTS),
            "block": sched.submit(TEXT, "nova", segment=OPTS),
            "plain_block": sched.submit("another ordinary one", "bella"),
            "sped": sched.submit(TEXT, "nova", segment=OPTS, speed=1.5),
        }
        out = {k: list(sched.iter_chunks(r)) for k, r in reqs.items()}
        st = sched.stats()
    finally:
        sched.close()
    f32 = np.concatenate(out["f32"])
    assert f32.shape == ref.shape and float(np.abs(f32 - ref).max()) <= 1e-4
    _s16_close(np.concatenate(out["s16"]), ref16)
    data = b"".join(c.tobytes() for c in out["flac"])
    assert data.count(b"fLaC") == 1
    _s16_close(decode_mono16(data), np.rint(np.clip(ref, -1, 1) * np.float32(32767)))
    p = np.concatenate(out["plain"])
    assert p.shape == plain.shape and float(np.abs(p - plain).max()) <= 1e-4
    for key, want in (("block", ref_block), ("plain_block", plain_block), ("sped", ref_sped)):
        got = np.concatenate(out[key])
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-4, key
    assert st["segments"] == 5 * 3 and st["completed"] == 7 and st["active"] == 0


def test_scheduler_cancel_mid_segment_frees_the_slot(tts):
    import time

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    gs = GenerationSettings.greedy(max_new_tokens=40)
    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=gs)
    try:
        it = sched.iter_chunks(sched.submit(TEXT, "heart", stream=True, segment=OPTS))
        next(it)
        it.close()  # the client goes away inside the first segment
        deadline = time.time() + 30
        while time.time() < deadline and (sched.stats()["active"] or sched.stats()["cancelled"] == 0):
            time.sleep(0.01)
        st = sched.stats()
        assert st["active"] == 0 and st["cancelled"] == 1
        ok = np.concatenate(list(sched.iter_chunks(sched.submit("after it", "heart", stream=True))))
        assert ok.size > 0
    finally:
        sched.close()


def test_server_long_text_behind_a_scheduler(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.longform import split_text
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler

    text = " ".join(f"Sentence number {i} of a rather long text." for i in range(70))
    assert 2800 <= len(text) <= 3200
    gs = GenerationSettings.greedy(max_new_tokens=6)
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=gs)
    try:
        plain = TestClient(create_app(tts, None, scheduler=sched))
        assert plain.post("/v1/audio/speech", json={"input": text, "voice": "heart"}).status_code == 400
        seg = TestClient(create_app(tts, {"long_text": "segment", "segment_max_bytes": 300}, scheduler=sched))
        r = seg.post("/v1/audio/speech", json={"input": text, "voice": "heart"})
        assert r.status_code == 200 and r.content[:4] == b"RIFF"
        r = seg.post("/v1/audio/speech", json={"input": text, "voice": "heart", "response_format": "flac"})
        assert r.status_code == 200 and r.content[:4] == b"fLaC"
        assert seg.get("/v1/stats").json()["segments"] == 2 * len(split_text(text, 300))
    finally:
        sched.close()
