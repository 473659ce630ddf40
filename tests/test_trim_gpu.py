"""Silence trimming on the GPU: the trim kernel against its numpy model (``trim.TrimState``) call by call over slots, segments
and chunkings, and the front ends on the tiny checkpoint: ``SmolTTS`` (blocking, streamed, segmented, with a speed and a format),
``BatchScheduler`` (a trimmed request beside an untrimmed one) and the HTTP route.  Samples are only copied or dropped: every
float32 comparison is exact."""
import itertools

import numpy as np
import pytest

from smoltts_amd import seam, trim
from smoltts_amd.seam import BLOCK, FINAL, FIRST, THRESH

pytestmark = pytest.mark.gpu

ALL_FLAGS = (FIRST | FINAL, 0, FIRST, FINAL)
TEXT = 'The first sentence is here. A second one follows it! <break time="0.5s"/> And then a third, which ends the text.'
OPTS = {"max_bytes": 40, "pause_s": 0.2}
SHORT = "A short request, trimmed."


def _speech(n, rng, amp=0.3):
    x = rng.uniform(-amp, amp, n).astype(np.float32)
    x[::40] = amp
    return x


def _quiet(n, rng, amp=2.0 ** -9):
    return rng.uniform(-0.5, 0.5, n).astype(np.float32) * np.float32(amp)


def _segment(rng, mid):
    """Speech between silent runs on every side of the rule's boundaries (2, 10, 11 and 200 blocks, HOLD + TAIL_KEEP), and parts
    at ``mid``: silence for a threshold above it only."""
    runs = [0, 100, 240, 480, 720, 2160, 2400, 2640, 2880, 5000, 47760, 48240, 50640, 50880, 53000]
    parts = []
    for _ in range(int(rng.integers(1, 4))):
        parts.append(_quiet(int(rng.choice(runs)), rng))
        parts.append(_speech(int(rng.integers(1, 3000)), rng))
        if rng.random() < 0.4:
            parts += [_quiet(int(rng.choice([480, 3000])), rng, mid), _speech(int(rng.integers(1, 500)), rng)]
    parts.append(_quiet(int(rng.choice([0, 239, 1200, 2400, 2640, 4800, 50641, 53000])), rng))
    x = np.concatenate(parts)
    if rng.random() < 0.3 and x.size > 5000:
        x[int(rng.integers(0, x.size))] = np.nan  # (not silence, wherever it falls)
    return x


def test_trim_kernel_matches_model_across_slots_and_chunkings():
    import torch

    from smoltts_amd.engine import SEAM_OFF, SilenceTrimmer

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    B, n_row = 6, 4 * 1920
    on = [0, 1, 2, 4, 5]  # slot 3 stays off
    # (trim, P, thr): every cap, with and without the ends, one threshold that is not the default
    params = {0: (True, 0, THRESH), 1: (True, 10, THRESH), 2: (False, 11, trim.threshold(-40.0)), 4: (True, 200, THRESH),
              5: (True, 11, trim.threshold(-40.0))}
    plans = {}
    for i, b in enumerate(on):
        nseg = 1 + (i + 2) % 3  # 3, 1, 2, 3, 1 segments
        flags = [ALL_FLAGS[(i + k) % 4] for k in range(nseg)]
        plans[b] = dict(segs=[_segment(rng, 0.006) for _ in range(nseg)], flags=flags)
    assert {f for p in plans.values() for f in p["flags"]} == set(ALL_FLAGS)
    st = SilenceTrimmer(dev, B)
    models = {b: trim.TrimState() for b in on}
    pos = {b: [0, 0] for b in on}  # (segment, offset)
    got = {b: [[] for _ in plans[b]["segs"]] for b in on}

    def start(b):
        k = pos[b][0]
        t, P, thr = params[b]
        st.start_segments([b], [plans[b]["flags"][k]], [t], [P], [thr])
        models[b].start(plans[b]["flags"][k], t, P, thr)

    st.start_segments(on, [plans[b]["flags"][0] for b in on], [params[b][0] for b in on], [params[b][1] for b in on],
                      [params[b][2] for b in on])  # (several slots in one call)
    for b in on:
        models[b].start(plans[b]["flags"][0], *params[b])
    st.start_segments([3], [SEAM_OFF], [1], [0], [THRESH])
    calls = 0
    while any(pos[b][0] < len(plans[b]["segs"]) for b in on):
        batch = int(rng.integers(1, B + 1))  # slots past the batch carry their state
        pcm = np.zeros((batch, n_row), np.float32)
        valid = np.zeros(batch, np.int32)
        end = np.zeros((2, batch), np.int32)  # seg_end, last
        live = [b for b in on if b < batch and pos[b][0] < len(plans[b]["segs"])]
        for b in live:
            k, off = pos[b]
            x = plans[b]["segs"][k]
            n = int(min(x.size - off, rng.choice([0, 1, 100, 239, 240, 241, int(rng.integers(1, n_row + 1)), n_row])))
            if rng.random() < 0.5:
                n = min(x.size - off, int(rng.integers(1, 5)) * 1920)
            pcm[b, :n] = x[off:off + n]
            pcm[b, n:] = 7.0  # past valid: never read
            valid[b] = n
            end[int(rng.integers(0, 2)), b] = off + n == x.size  # the segment's end comes as seg_end or as last
        pcm_d, valid_d, end_d = (torch.from_numpy(a).to(dev) for a in (pcm, valid, end))
        out, counts = st.new_outputs(batch, n_row)
        out.fill_(-9.0)
        st.chunk(pcm_d, n_row, out, counts, valid=valid_d, seg_end=end_d[0], last=end_d[1])
        out_h, counts_h = out.cpu().numpy(), counts.cpu().numpy()
        calls += 1
        assert counts_h[3] == 0 if batch > 3 else True
        for b in live:
            k, off = pos[b]
            ended = bool(end[:, b].any())
            y = models[b].push(pcm[b, :valid[b]], end=bool(end[0, b]), last=bool(end[1, b]))
            assert counts_h[b] == y.size, (b, calls)
            np.testing.assert_array_equal(out_h[b, :y.size], y)
            assert np.all(out_h[b, y.size:] == -9.0)  # nothing written past the count
            got[b][k].append(y)
            pos[b][1] += int(valid[b])
            s = st.slot_state(b)
            assert {n: s[n] for n in trim.TrimState.COUNTERS} == models[b].state(), (b, calls)
            assert s["open"] == (0 if ended else 1) and s["held"] <= trim.HOLD * BLOCK
            if ended:
                pos[b] = [k + 1, 0]
                if k + 1 < len(plans[b]["segs"]):
                    start(b)
    for b in on:
        for k, x in enumerate(plans[b]["segs"]):
            np.testing.assert_array_equal(np.concatenate(got[b][k]), trim.trim(x, plans[b]["flags"][k], *params[b]))
    dropped = {b: sum(x.size for x in plans[b]["segs"]) - sum(y.size for g in got[b] for y in g) for b in on}
    assert all(d > 0 for d in dropped.values()), dropped  # every slot's rule cut something
    st.close()


def test_trim_pcm_whole_rows_and_bad_arguments():
    import torch

    from smoltts_amd.engine import SilenceTrimmer, SmolttsError, trim_pcm

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    # longer than one call takes (trim.MAX_CALL): the row goes through in pieces
    x = np.concatenate([_quiet(30000, rng), _speech(50000, rng), _quiet(60000, rng), _speech(7, rng), _quiet(70001, rng)])
    assert x.size > 3 * trim.MAX_CALL
    for flags, on, P in itertools.product(ALL_FLAGS, (False, True), (0, 10, 200)):
        np.testing.assert_array_equal(trim_pcm(x, flags, dev, on, P), trim.trim(x, flags, on, P))
    np.testing.assert_array_equal(trim_pcm(x[:0], FIRST | FINAL, dev), x[:0])
    np.testing.assert_array_equal(trim_pcm(x[:100], FIRST | FINAL, dev, thr=0.5), x[:100])
    st = SilenceTrimmer(dev, 2)
    assert st.out_samples(1920) == 1920 + (trim.HOLD + 1) * BLOCK and st.out_samples(trim.MAX_CALL + 1) == 0
    for bad in (dict(pauses=[9]), dict(pauses=[201]), dict(thrs=[0.0]), dict(thrs=[1.5]), dict(flags=[8]), dict(slots=[2])):
        kw = dict(slots=[0], flags=[3], trims=[1], pauses=[0], thrs=[THRESH])
        kw.update(bad)
        with pytest.raises(SmolttsError):
            st.start_segments(**kw)
    st.close()


# ------------------------------------------------------------------------------- the front ends on the tiny checkpoint
@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    # (this codec's audio starts quieter than it goes on, below -6 dBFS: the threshold the tests take from it is one a request may name)
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=3))


def _median_db(raw):
    """The median of the per-block max-abs of ``raw`` in dBFS, inside the range a request may name: synthetic audio may have no
    block under 2^-8, and about half of its blocks are silence by this threshold."""
    n = raw.size // BLOCK * BLOCK
    m = float(np.median(np.abs(raw[:n]).reshape(-1, BLOCK).max(axis=1)))
    return float(np.clip(20.0 * np.log10(m), -72.0, -6.0))


def _cuts(raw, want):
    """The condition on the reference: the model drops something and keeps something."""
    print(f"the model keeps {want.size} of {raw.size} samples")
    return 0 < want.size < raw.size


def test_facade_blocking_and_stream(tts):
    from smoltts_amd.config import GenerationSettings

    gs = GenerationSettings.greedy(max_new_tokens=10)
    raw = np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs)))
    block = tts(SHORT, "nova", generation_settings=gs)
    assert tts.last_trimmed_s == 0.0
    db = _median_db(raw)
    kw = dict(trim_silence=True, max_pause_s=0.1, silence_threshold_db=db)
    want = trim.trim(raw, FIRST | FINAL, True, 10, trim.threshold(db))
    assert _cuts(raw, want)
    chunks = list(tts.stream(SHORT, "nova", generation_settings=gs, **kw))
    np.testing.assert_array_equal(np.concatenate(chunks), want)
    assert all(c.dtype == np.float32 and c.size % BLOCK == 0 for c in chunks[:-1])
    want_b = trim.trim(block, FIRST | FINAL, True, 10, trim.threshold(db))
    np.testing.assert_array_equal(tts(SHORT, "nova", generation_settings=gs, **kw), want_b)
    assert tts.last_trimmed_s == pytest.approx((block.size - want_b.size) / 24000.0) and tts.last_trimmed_s > 0
    # each option on its own
    np.testing.assert_array_equal(tts(SHORT, "nova", generation_settings=gs, trim_silence=True, silence_threshold_db=db),
                                  trim.trim(block, FIRST | FINAL, True, 0, trim.threshold(db)))
    np.testing.assert_array_equal(np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs, max_pause_s=0.1, silence_threshold_db=db))),
                                  trim.trim(raw, FIRST | FINAL, False, 10, trim.threshold(db)))
    with pytest.raises(ValueError, match="max_pause_s"):
        tts(SHORT, "nova", generation_settings=gs, max_pause_s=3.0)
    with pytest.raises(ValueError, match="silence_threshold_db"):
        list(tts.stream(SHORT, "nova", generation_settings=gs, silence_threshold_db=-30.0))


def test_facade_segmented(tts):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.longform import split_text
    from smoltts_amd.seam import pause_samples, segment_flags

    from test_longform_gpu import _raw_stream

    gs = GenerationSettings.greedy(max_new_tokens=10)
    segs = split_text(TEXT, OPTS["max_bytes"])
    pauses = [pause_samples(s.pause_after_s if s.pause_after_s is not None else 0.2) for s in segs[:-1]]
    tts(TEXT, "nova", generation_settings=gs, segment=OPTS)
    pieces = [tts.decode_codes(it["codes"]) for it in tts.last_segments]
    assert len(pieces) == 3
    db = _median_db(np.concatenate(pieces))
    thr = trim.threshold(db)
    kw = dict(trim_silence=True, max_pause_s=0.1, silence_threshold_db=db)
    trimmed = [trim.trim(x, segment_flags(k, 3), True, 10, thr) for k, x in enumerate(pieces)]
    assert _cuts(np.concatenate(pieces), np.concatenate(trimmed))
    got = tts(TEXT, "nova", generation_settings=gs, segment=OPTS, **kw)
    np.testing.assert_array_equal(got, seam.join(trimmed, pauses))
    assert tts.last_trimmed_s == pytest.approx(sum(x.size - y.size for x, y in zip(pieces, trimmed)) / 24000.0)
    # the stream: each segment's own stream trimmed with its flags, then the seam
    chunks = list(tts.stream(TEXT, "nova", generation_settings=gs, segment=OPTS, **kw))
    raws = [_raw_stream(tts, it["prompt"], gs, None) for it in tts.last_segments]
    want = seam.join([trim.trim(x, segment_flags(k, 3), True, 10, thr) for k, x in enumerate(raws)], pauses)
    np.testing.assert_array_equal(np.concatenate(chunks), want)


def test_facade_trim_with_speed_and_format(tts):
    import torch

    from smoltts_amd import tsm
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.engine import Resampler

    gs = GenerationSettings.greedy(max_new_tokens=10)
    raw = np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs)))
    db = _median_db(raw)
    kw = dict(trim_silence=True, max_pause_s=0.1, silence_threshold_db=db)
    ref = trim.trim(raw, FIRST | FINAL, True, 10, trim.threshold(db))
    assert _cuts(raw, ref)
    sped = np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs, speed=1.5, **kw)))
    want = tsm.stretch(ref, 1.5)
    assert sped.shape == want.shape and float(np.abs(sped - want).max()) <= 1e-6
    got = np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs, speed=1.5, output_format="pcm_16000", **kw)))
    rs = Resampler(tts.lm.device, 1, sped.size)  # the stretched float32 converted in one call: what the stream's chunks add up to
    rs.reset_slots([0], ["pcm_16000"])
    out, counts = rs.new_outputs(1, sped.size)
    rs.chunk(torch.from_numpy(sped).to(tts.lm.device)[None], sped.size, out, counts)
    want16 = rs.slot_bytes(out.cpu().numpy(), counts.cpu().numpy(), 0, tail=True)
    rs.close()
    assert got.dtype == want16.dtype == np.int16 and got.shape == want16.shape
    assert int(np.abs(got.astype(np.int32) - want16.astype(np.int32)).max(initial=0)) <= 1


def test_requests_without_the_options_make_no_trim_stage(tts, monkeypatch):
    from smoltts_amd import engine
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    made = []
    real = engine.SilenceTrimmer.__init__
    monkeypatch.setattr(engine.SilenceTrimmer, "__init__", lambda self, *a, **k: (made.append(1), real(self, *a, **k))[1])
    gs = GenerationSettings.greedy(max_new_tokens=8)
    tts._finish.held.pop(engine.SilenceTrimmer, None)
    a = tts(SHORT, "heart", generation_settings=gs)
    b = np.concatenate(list(tts.stream(SHORT, "heart", generation_settings=gs, trim_silence=False, max_pause_s=None)))
    tts(TEXT, "heart", generation_settings=gs, segment=OPTS)
    list(tts.stream(TEXT, "heart", generation_settings=gs, segment=OPTS, speed=1.25))
    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=gs)
    try:
        np.testing.assert_array_equal(np.concatenate(list(sched.iter_chunks(sched.submit(SHORT, "heart")))), a)
        c = np.concatenate(list(sched.iter_chunks(sched.submit(SHORT, "heart", stream=True))))
        assert c.size > 0 and b.size > 0 and sched._stream_conv.tr is None and sched._finisher.held.get(engine.SilenceTrimmer) is None
    finally:
        sched.close()
    assert not made and tts._finish.held.get(engine.SilenceTrimmer) is None
    tts(SHORT, "heart", generation_settings=gs, trim_silence=True)
    assert made == [1]


def test_scheduler_and_http(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=10))
    try:
        def run(reqs):
            return [np.concatenate(list(sched.iter_chunks(r)) or [np.zeros(0, np.float32)]) for r in reqs]

        raw0, plain = run([sched.submit(SHORT, "nova", stream=True), sched.submit(SHORT, "nova")])
        assert sched._stream_conv.tr is None
        db = _median_db(raw0)
        thr = trim.threshold(db)
        kw = dict(trim_silence=True, max_pause_s=0.1, silence_threshold_db=db)
        want = trim.trim(raw0, FIRST | FINAL, True, 10, thr)
        assert _cuts(raw0, want)
        # side by side in one batch: the untrimmed stream's bytes are unchanged, the trimmed one is the model's
        reqs = [sched.submit(SHORT, "nova", stream=True, **kw), sched.submit(SHORT, "nova", stream=True),
                sched.submit(SHORT, "nova", stream=True, output_format="pcm_16000"), sched.submit(SHORT, "nova", **kw)]
        a, b, c16, blk = run(reqs)
        np.testing.assert_array_equal(b, raw0)
        np.testing.assert_array_equal(a, want)
        want_b = trim.trim(plain, FIRST | FINAL, True, 10, thr)
        np.testing.assert_array_equal(blk, want_b)
        assert reqs[3].trimmed_s == pytest.approx((plain.size - want_b.size) / 24000.0) and sched._stream_conv.tr is not None
        c16_alone, = run([sched.submit(SHORT, "nova", stream=True, output_format="pcm_16000")])
        np.testing.assert_array_equal(c16, c16_alone)
        # a segmented stream: each segment trimmed with its flags in front of the seam
        seg0, = run([sched.submit(TEXT, "nova", stream=True, segment=OPTS)])
        seg, = run([sched.submit(TEXT, "nova", stream=True, segment=OPTS, max_pause_s=0.1, silence_threshold_db=db)])
        assert seg.size <= seg0.size
        with pytest.raises(ValueError, match="trim_silence"):
            sched.submit(SHORT, "nova", trim_silence="yes")

        c = TestClient(create_app(tts, scheduler=sched))
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova"})
        assert r.status_code == 200 and "x-silence-trimmed-ms" not in r.headers and r.content == pcm_to_wav_bytes(plain, 24000)
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova", **kw})
        assert r.status_code == 200 and r.content == pcm_to_wav_bytes(want_b, 24000)
        assert r.headers["x-silence-trimmed-ms"] == f"{1e3 * (plain.size - want_b.size) / 24000.0:.0f}"
        r = c.post("/v1/text-to-speech/nova", json={"text": SHORT, **kw})
        assert r.status_code == 200 and r.content == pcm_to_wav_bytes(want_b, 24000) and "x-silence-trimmed-ms" in r.headers
        r = c.post("/v1/text-to-speech/nova/stream", json={"text": SHORT, **kw})
        assert r.status_code == 200 and r.content == want.tobytes()
        assert c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova", "max_pause_s": 5}).status_code == 400
        assert c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova", "silence_threshold_db": -30}).status_code == 400
        # the server's defaults, and a body that switches them off
        c = TestClient(create_app(tts, settings={"trim_silence": True, "max_pause_s": 0.1}, scheduler=sched))
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova", "silence_threshold_db": db})
        assert r.status_code == 200 and r.content == pcm_to_wav_bytes(want_b, 24000)
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova", "trim_silence": None, "max_pause_s": None})
        assert r.status_code == 200 and r.content == pcm_to_wav_bytes(plain, 24000) and "x-silence-trimmed-ms" not in r.headers
    finally:
        sched.close()
