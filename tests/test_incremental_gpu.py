"""Text fed in pieces, in the batched scheduler and the façade (GPU; tiny model, synthetic codec): the stream is the whole text's,
a late close ends it as the seam model says, a parked slot leaves the others alone, and timeouts and cancels free it."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S1, S2, S3 = "The first sentence is here.", "A second one follows it!", "And then a third, which ends the text."
TEXT = f'{S1} {S2} <break time="0.5s"/> {S3}'
OPTS = {"max_bytes": 40, "pause_s": 0.2}
FIRST_PART = f"{S1} {S2} "  # settles segment 1 (sentence 2 does not fit beside it) and nothing else


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


def _scheduler(tts, max_new_tokens=10, max_batch=3):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    return BatchScheduler(tts, max_batch=max_batch, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=max_new_tokens),
                          side_prefill_min_active=1)


def _bytes(chunks) -> bytes:
    return b"".join(np.ascontiguousarray(c).tobytes() for c in chunks)


def _until(cond, what, timeout=30.0):
    deadline = time.time() + timeout
    while not cond():
        assert time.time() < deadline, f"timed out waiting for {what}"
        time.sleep(0.001)


def test_fed_text_streams_the_bytes_of_the_whole_text(tts):
    from smoltts_amd.config import RequestSampling

    sched = _scheduler(tts)
    try:
        assert [s.text for s in __import__("smoltts_amd.longform", fromlist=["x"]).split_text(TEXT, 40)] == [S1, S2, S3]
        # greedy float32: every piece and the close arrive before the first segment has been admitted
        want = _bytes(sched.iter_chunks(sched.submit(TEXT, "nova", stream=True, segment=OPTS)))
        r = sched.submit_incremental("nova", segment=OPTS)
        data = TEXT.encode()
        for a in range(0, len(data), 7):
            r.feed(data[a:a + 7])
        r.close()
        got = _bytes(r)
        assert len(got) == len(want) > 0 and got == want
        # seeded, faster, 16 kHz, FLAC: the text grows while the request is speaking
        kw = dict(sampling=RequestSampling(temperature=0.8, fast_temperature=0.8, seed=1234), speed=1.25, output_format="pcm_16000",
                  container="flac", segment=OPTS)
        want = _bytes(sched.iter_chunks(sched.submit(TEXT, "nova", stream=True, **kw)))
        r = sched.submit_incremental("nova", **kw)
        r.feed(FIRST_PART)
        chunks = iter(r)
        head = next(chunks)  # segment 1 is speaking (or has ended: its seam is the same either way)
        r.feed(TEXT[len(FIRST_PART):])
        r.close()           # ... and both arrive before segment 2, which has yet to be admitted, can end
        got = _bytes([head, *chunks])
        assert got[:4] == b"fLaC" and got.count(b"fLaC") == 1
        assert len(got) == len(want) and got == want
        st = sched.stats()
        assert st["segments"] == 4 * 3 and st["completed"] == 4 and st["active"] == st["parked"] == 0
    finally:
        sched.close()


def _raw_stream(tts, prompt, gs):
    """One prompt streamed on its own as float32 (what a segment's codec output is)."""
    from smoltts_amd.engine import LMSession, MimiSession
    from smoltts_amd.generate import _apply_sampling, stream_pcm

    T = int(prompt.shape[1])
    sess = LMSession(tts.lm, 1, max_seq=min(tts.config.max_seq_len, T + gs.max_new_tokens + 2), max_rows=T, max_frames=gs.max_new_tokens + 1)
    _apply_sampling(sess, gs)
    ms = MimiSession(tts.codec, max_batch=1, max_chunk_frames=1)
    try:
        return np.concatenate(list(stream_pcm(sess, ms, prompt)))
    finally:
        ms.close()
        sess.close()


def test_close_behind_the_last_segments_start_ends_the_stream_as_the_seam_model_does(tts):
    """The last segment is opened while text may still follow (not FINAL); the close that then arrives with no text ends the
    stream with the seam's ``last`` marker.  The reference is ``seam.SeamState`` over each segment's own stream from the façade;
    the bound is the 1e-4 the scheduler's codec passes are held to against the façade's (test_longform_sched_gpu.py)."""
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.seam import FIRST, SeamState, pause_samples

    gs = GenerationSettings.greedy(max_new_tokens=60)
    list(tts.stream(TEXT, "nova", generation_settings=gs, segment=OPTS))
    raws = [_raw_stream(tts, it["prompt"], gs) for it in tts.last_segments]
    model, want = SeamState(), []
    for k, (raw, pause) in enumerate(zip(raws, (0.2, 0.5, 0.2))):  # (segment 3 was opened with a seam's default pause behind it)
        model.start(pause_samples(pause), FIRST if k == 0 else 0)
        want.append(model.push(raw, end=True, last=k == 2))
    want = np.concatenate(want)
    sched = _scheduler(tts, max_new_tokens=60)
    try:
        r = sched.submit_incremental("nova", segment=OPTS)
        r.feed(TEXT)
        r.flush()  # segment 3 is handed over, the text is still open
        _until(lambda: sched.stats()["segments"] >= 2, "segment 3's turn")
        r.close()  # no text behind it: segment 3 (30 ticks long) turns out to be the last while it is speaking
        got = np.concatenate(list(r))
        st = sched.stats()
    finally:
        sched.close()
    print("late close: samples", got.size, want.size, "max |diff|", float(np.abs(got - want).max()) if got.shape == want.shape else None)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-4
    assert st["segments"] == 3 and st["completed"] == 1 and st["parked"] == 0


def test_a_parked_slot_leaves_the_others_alone_and_goes_on_when_fed(tts):
    sched = _scheduler(tts)
    try:
        whole = _bytes(sched.iter_chunks(sched.submit(TEXT, "nova", stream=True, segment=OPTS)))
        alone = _bytes(sched.iter_chunks(sched.submit("an ordinary request", "sky", stream=True)))
        a = sched.submit_incremental("nova", segment=OPTS)
        a.feed(FIRST_PART)
        _until(lambda: sched.stats()["parked"] == 1, "the park")  # segment 1 is through, segment 2 is not settled yet
        ticks = sched.stats()["ticks"]
        beside = _bytes(sched.iter_chunks(sched.submit("an ordinary request", "sky", stream=True)))
        st = sched.stats()
        assert st["parked"] == 1 and st["active"] == 0 and st["ticks"] > ticks
        assert beside == alone
        a.feed(TEXT[len(FIRST_PART):])
        a.close()
        got = _bytes(a)
        assert len(got) == len(whole) and got == whole
        assert sched.stats()["parked"] == 0 and sched.stats()["completed"] == 4
    finally:
        sched.close()


def test_idle_timeout_and_cancel_free_a_parked_slot(tts):
    sched = _scheduler(tts, max_batch=2)
    try:
        two = _bytes(sched.iter_chunks(sched.submit(f"{S1} {S2}", "nova", stream=True, segment=OPTS)))
        a = sched.submit_incremental("nova", segment=OPTS, idle_timeout_s=0.2)
        a.feed(FIRST_PART)
        got = _bytes(a)  # nobody closes it: the timeout does, and the buffered sentence is the last segment
        assert got == two
        st = sched.stats()
        assert st["idle_timeouts"] == 1 and st["parked"] == 0 and st["active"] == 0
        with pytest.raises(ValueError, match="closed"):
            a.feed("too late")
        b = sched.submit_incremental("nova", segment=OPTS)
        b.feed(FIRST_PART)
        chunks = iter(b)
        next(chunks)
        _until(lambda: sched.stats()["parked"] == 1, "the park")
        b.cancel()
        _until(lambda: sched.stats()["cancelled"] == 1, "the cancel")
        assert sched.stats()["parked"] == 0
        assert sorted(sched._free) == [0, 1]  # both slots are free again
        list(chunks)  # (the chunks that were out before the cancel, then the end)
        both = [sched.submit("after it", v, stream=True) for v in ("heart", "sky")]
        assert all(len(_bytes(sched.iter_chunks(r))) > 0 for r in both)
        # a request that is closed without anything to speak is refused, one that never gets text holds no slot
        c = sched.submit_incremental("nova")
        c.feed("  ")
        c.close()
        with pytest.raises(ValueError, match="nothing to speak"):
            list(c)
    finally:
        sched.close()


def test_close_of_a_parked_stream_flushes_its_stages(tts):
    """The text is closed, with nothing more to say, after its last segment has ended as a middle segment: the stream is that
    segment with its seam's pause behind it (``seam.SeamState`` over the scheduler's own plain stream of the sentence), and the
    FLAC encoder's last frame still comes out."""
    from flac_decode_helpers import decode_mono16

    from smoltts_amd.seam import FIRST, SeamState, pause_samples

    sched = _scheduler(tts)
    try:
        plain = np.concatenate(list(sched.iter_chunks(sched.submit(S1, "nova", stream=True))))
        model = SeamState()
        model.start(pause_samples(0.2), FIRST)
        want = model.push(plain, end=True)
        assert want.size >= plain.size
        got = {}
        for key, kw in (("f32", {}), ("flac", {"container": "flac"})):
            r = sched.submit_incremental("nova", segment=OPTS, **kw)
            r.feed(S1)
            r.flush()
            chunks = iter(r)
            head = next(chunks)
            _until(lambda: sched.stats()["parked"] == 1, "the park")
            r.close()
            got[key] = [head, *chunks]
        st = sched.stats()
    finally:
        sched.close()
    f32 = np.concatenate(got["f32"])
    assert f32.shape == want.shape and float(np.abs(f32 - want).max()) <= 1e-4
    pcm16 = decode_mono16(_bytes(got["flac"]))
    ref16 = np.rint(np.clip(want, -1, 1) * np.float32(32767)).astype(np.int32)
    assert pcm16.shape == ref16.shape and int(np.abs(np.asarray(pcm16, np.int32) - ref16).max(initial=0)) <= 1
    assert st["parked"] == 0 and st["active"] == 0 and st["completed"] == 3


def test_facade_streams_from_a_generator_what_it_streams_from_the_text(tts):
    from smoltts_amd.config import GenerationSettings

    gs = GenerationSettings.greedy(max_new_tokens=10)
    want = np.concatenate(list(tts.stream(TEXT, "nova", generation_settings=gs, segment=OPTS)))
    pulled = []

    def pieces():
        for a in range(0, len(TEXT), 9):
            pulled.append(a)
            yield TEXT[a:a + 9]

    chunks = tts.stream(pieces(), "nova", generation_settings=gs, segment=OPTS)
    first = next(chunks)
    assert len(pulled) * 9 < len(TEXT)  # it speaks before it has pulled the whole text
    got = np.concatenate([first, *chunks])
    np.testing.assert_array_equal(got, want)
    assert [s["text"] for s in tts.last_segments] == [S1, S2, S3]
    flac = _bytes(tts.stream(iter([TEXT[:50], TEXT[50:]]), "nova", generation_settings=gs, segment=OPTS, container="flac", speed=1.25))
    assert flac == _bytes(tts.stream(TEXT, "nova", generation_settings=gs, segment=OPTS, container="flac", speed=1.25))
