"""Every audio option on at once, through the public keyword interface only, on the tiny checkpoint: the façade and the
scheduler speak the same request and must deliver the same bytes and report the same values, so an option that one of them
drops on the way from its keywords to the stages shows here whichever option it is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import watermark as W  # noqa: E402

KEY = W.Watermark(0x0123456789ABCDEF, -26.0)
TEXT = "The first sentence is here. A second one follows it!"
SEG = {"max_bytes": 30}  # two segments
STREAM_KW = dict(output_format="pcm_16000", container="flac", speed=1.25, loudness=-20.0, loudness_start_gain_db=-3.0,
                 trim_silence=True, max_pause_s=0.2, peak_limit_db=-6.0, watermark=True, segment=SEG)
BLOCK_KW = dict(speed=1.25, loudness=-10.0, trim_silence=True, max_pause_s=0.2, peak_limit_db=-6.0, watermark=True, segment=SEG)
FRAMES = 12


def _bytes(chunks) -> bytes:
    return b"".join(np.ascontiguousarray(c).tobytes() for c in chunks)


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5), watermark=KEY)


@pytest.fixture(scope="module")
def sched(tts):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    # (one frame a tick: the stages then see the calls the façade's frame-by-frame stream gives them.  With two frames a tick
    # this request's stream has the façade's length and not its bytes, and its FLAC frames are cut elsewhere)
    s = BatchScheduler(tts, max_batch=2, frames_per_tick=1, generation_settings=GenerationSettings.greedy(max_new_tokens=FRAMES),
                       watermark=KEY)
    yield s
    s.close()


def _sampling():
    from smoltts_amd.config import RequestSampling

    return RequestSampling(temperature=0.8, fast_temperature=0.8, seed=1234)


def test_stream_with_every_option_is_the_same_bytes_from_both_front_ends(tts, sched):
    from smoltts_amd.config import GenerationSettings

    gs = GenerationSettings.greedy(max_new_tokens=FRAMES)
    want = _bytes(tts.stream(TEXT, "nova", generation_settings=gs, sampling=_sampling(), **STREAM_KW))
    assert len(tts.last_segments) == 2 and want[:4] == b"fLaC" and want.count(b"fLaC") == 1
    bare = _bytes(tts.stream(TEXT, "nova", generation_settings=gs, sampling=_sampling(), watermark=False))
    assert len(bare) > 0 and want != bare  # (both paths dropping every option would agree too)
    other = sched.submit("an ordinary request", "sky", stream=True, watermark=False)  # a plain stream in the other slot
    req = sched.submit(TEXT, "nova", stream=True, sampling=_sampling(), **STREAM_KW)
    got = _bytes(sched.iter_chunks(req))
    assert len(_bytes(sched.iter_chunks(other))) > 0
    print(f"stream: {len(want)} bytes from the façade, {len(got)} from the scheduler, {len(bare)} without the options")
    assert got == want


def test_blocking_with_every_option_is_the_same_audio_and_the_same_report(tts, sched):
    from smoltts_amd.config import GenerationSettings

    gs = GenerationSettings.greedy(max_new_tokens=FRAMES)
    want = tts(TEXT, "nova", generation_settings=gs, sampling=_sampling(), **BLOCK_KW)
    report = (tts.last_loudness_gain_db, tts.last_trimmed_s, tts.last_peak_reduction_db, tts.last_finish_reason)
    assert len(tts.last_segments) == 2 and want.size > 0
    bare = tts(TEXT, "nova", generation_settings=gs, sampling=_sampling(), watermark=False)
    assert not np.array_equal(want, bare)
    req = sched.submit(TEXT, "nova", sampling=_sampling(), **BLOCK_KW)
    got = np.concatenate(list(sched.iter_chunks(req)))
    print(f"blocking: {want.size} samples ({bare.size} without the options); gain dB, trimmed s, reduction dB, reason: "
          f"{report} from the façade, {(req.loudness_gain_db, req.trimmed_s, req.peak_reduction_db, req.finish_reason)} from the scheduler")
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert req.watermark is True
    assert (req.loudness_gain_db, req.trimmed_s, req.peak_reduction_db, req.finish_reason) == report
    assert req.loudness_gain_db is not None and req.peak_reduction_db is not None and req.finish_reason in ("stop", "length")
