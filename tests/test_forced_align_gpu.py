"""Forced alignment: ``smoltts_k_score_rows``, ``LMSession.measure_rows`` and the front ends above them, on
the tiny and 70m synthetic configs.

1. The row-scoring kernel against ``sampling.pick_logprob`` on the same fp32 rows, |error| <= ``LOGPROB_MARGIN``: widths 1024 and
   1027, 1 and 33 rows, targets at the maximum, far below it (mass 0, finite score) and at a -inf column (-inf); a row with target
   -1 keeps the sentinel written in front of the launch.
2. The grid of a greedy run of 20 frames, measured in one call in a one-slot session, in chunks of 16 rows, and in slot 2 of a
   3-slot session whose other slots decode in between: the same (m, s1) rows and the same scores, bit for bit; fp32 and bf16 KV.
3. ... and those bits are the ones the decode frames recorded for the same run (alignment rows and scores of a session whose frame 0
   is a decode row, as in the scheduler).
4. Rows with a frame index < 0 leave the -1 fill in place; a scheduler that measured a recording in its scratch session serves the
   ids, PCM and alignments of one that never did, and its serving session's graph form does not change.
5. ``SmolTTS.align_recording`` on the PCM the model generated, the scheduler beside two speaking requests, the pool and the route."""
import base64
import functools

import numpy as np
import pytest
import torch

from lm_strict_helpers import make_oracles, random_grid

pytestmark = pytest.mark.gpu

T0, F = 21, 20  # prompt columns, frames: 40 rows; in chunks of 16 the calls hold 16 and 4 rows (a chunk ends in front of the first
#                 scored row, T0 - 1), then 16 and 4
WINDOW = (1, T0 - 1)
PAIRS = {"tiny": [(0, 1), (1, 4)], "smoltts_byte_70m": [(3, 2), (9, 7)]}
SENTINEL = -12345.0


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("n_cols", [1024, 1027])
@pytest.mark.parametrize("n_rows", [1, 33])
def test_score_rows_matches_pick_logprob(n_cols, n_rows):
    from smoltts_amd import ops
    from smoltts_amd.sampling import LOGPROB_MARGIN, pick_logprob

    rng = np.random.default_rng(n_cols * 100 + n_rows)
    for case in ("max", "far", "neg_inf", "random", "skipped"):
        x = (rng.standard_normal((n_rows, n_cols)) * 4.0).astype(np.float32)
        tgt = rng.integers(0, n_cols, size=n_rows).astype(np.int32)
        for r in range(n_rows):
            if case == "max":
                tgt[r] = int(np.argmax(x[r]))
            elif case == "far":  # more than 30 below the maximum: mass 0, the score stays finite
                x[r, tgt[r]] = x[r].max() - np.float32(31.0 + r)
            elif case == "neg_inf":
                x[r, tgt[r]] = -np.inf
        if case == "skipped":
            tgt[::2] = -1
            if n_rows > 2:
                tgt[1] = n_cols  # outside the row: writes nothing either
        out = torch.full((n_rows,), SENTINEL, dtype=torch.float32, device="cuda")
        ops.score_rows(torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda(), out)
        got = out.cpu().numpy()
        for r in range(n_rows):
            if not 0 <= tgt[r] < n_cols:
                assert got[r:r + 1].view(np.uint32)[0] == np.float32(SENTINEL).view(np.uint32), (case, r)
                continue
            want = pick_logprob(x[r], int(tgt[r]))
            if case == "neg_inf":
                assert got[r] == -np.inf and want == -np.inf, (case, r, got[r], want)
            else:
                assert np.isfinite(got[r]) and abs(float(got[r]) - want) <= LOGPROB_MARGIN, (case, n_cols, r, float(got[r]), want)
            if case == "far":
                assert got[r] < -30.0


def test_score_rows_reads_a_row_inside_a_wider_buffer():
    from smoltts_amd import ops
    from smoltts_amd.sampling import LOGPROB_MARGIN, pick_logprob

    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 1030)) * 3.0).astype(np.float32)  # ld 1030: no 16-byte rows, the kernel's scalar path
    tgt = np.asarray([0, 1026, 513], np.int32)
    out = torch.zeros(3, dtype=torch.float32, device="cuda")
    ops.score_rows(torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda(), out, n_cols=1027)
    for r in range(3):
        assert abs(float(out[r]) - pick_logprob(x[r, :1027], int(tgt[r]))) <= LOGPROB_MARGIN


# ---------------------------------------------------------------------------------------------------- 2. / 3. the session
class _Model:
    def __init__(self, cfgname):
        from smoltts_amd.config import NumericsMode, TokenConfig
        from smoltts_amd.engine import LMEngine
        from smoltts_amd.tokenizer import load_tokenizer

        self.name = cfgname
        self.cfg, state, _o32, _o64 = make_oracles(cfgname, 3)
        self.eng = LMEngine(self.cfg, state, TokenConfig.from_tokenizer(load_tokenizer(), self.cfg), NumericsMode.torch_reference())
        gen = torch.Generator().manual_seed(23)
        self.prompt = random_grid(self.cfg, T0, gen)
        self.others = [random_grid(self.cfg, 9, gen), random_grid(self.cfg, 30, gen)]
        self.pairs = PAIRS[cfgname]
        self.runs = {}

    def run(self, kv):
        """The greedy run (its frame 0 a decode row), its grid, and the grid measured in the three ways -- once per kv dtype."""
        if kv not in self.runs:
            self.runs[kv] = _measure_all(self, kv)
        return self.runs[kv]


@pytest.fixture(scope="module", params=["tiny", "smoltts_byte_70m"])
def model(request):
    m = _Model(request.param)
    yield m
    m.eng.close()


def _session(m, B, kv, score=False):
    from smoltts_amd.engine import LMSession

    s = LMSession(m.eng, B, max_seq=128, max_rows=256, max_frames=F + 4, kv_dtype=kv)
    s.set_slot_sampling(list(range(B)), [0.0] * B, [0.0] * B, [0.0] * B, [0] * B)
    s.set_align_heads(m.pairs)
    if score:
        s.set_slot_score([0], [True])
    return s


def _measure_all(m, kv):
    out = {}
    # the run itself: greedy, deferred frame 0 (a decode row, measured and scored like the others: what the scheduler does)
    s = _session(m, 1, kv, score=True)
    s.set_slot_align([0], [WINDOW[0]], [WINDOW[1]])
    s.prefill([m.prompt], stop_on_eos=False, defer_frame0=True)
    s.decode(F)
    codes, n, _, _ = s.fetch()
    assert n[0] == F
    out["decode"] = (s.fetch_alignment(0, F + 4).copy(), s.fetch_logprobs()[0, :F].copy())
    s.close()
    # the columns whose rows produced frames 0 .. F - 1, the frame of each row and the id it emitted
    grid = np.concatenate([m.prompt, codes[0, :F - 1].T], axis=1).astype(np.int32)
    T = grid.shape[1]
    frame_of_row = np.full(T, -1, np.int32)
    frame_of_row[T0 - 1:] = np.arange(F)
    targets = np.full(T, -1, np.int32)
    targets[T0 - 1:] = codes[0, :F, 0]
    out["grid"] = (grid, frame_of_row, targets)
    for name, chunk in (("one call", None), ("chunks of 16", 16)):
        s = _session(m, 1, kv)
        s.set_slot_align([0], [WINDOW[0]], [WINDOW[1]])
        form = s.graph_form()
        lp = s.measure_rows(grid, 0, frame_of_row, targets, chunk)
        assert s.graph_form() == form
        out[name] = (s.fetch_alignment(0, F + 4).copy(), lp[T0 - 1:].copy())
        assert np.isnan(lp[:T0 - 1]).all()
        if chunk is None:  # 4. every other frame only: the skipped frames keep the -1 fill, the measured ones their bits
            s.set_slot_align([0], [WINDOW[0]], [WINDOW[1]])  # (resets the slot's rows)
            s.measure_rows(grid, 0, np.where(frame_of_row % 2 == 0, frame_of_row, -1), np.full(T, -1, np.int32))
            out["even frames"] = s.fetch_alignment(0, F + 4).copy()
        s.close()
    # slot 2 of a 3-slot session whose slots 0 and 1 decode meanwhile
    s = _session(m, 3, kv)
    s.set_slot_align([2], [WINDOW[0]], [WINDOW[1]])
    s.prefill(m.others, slots=[0, 1], stop_on_eos=False, defer_frame0=True)
    s.decode(1)
    it = s.iter_measure_rows(grid, 2, frame_of_row, targets, 16)
    between = 0
    while True:
        try:
            next(it)
            s.decode(2)
            between += 1
        except StopIteration as done:
            lp = done.value.cpu().numpy()
            break
    s.decode(2)
    _, n, _, _ = s.fetch()
    assert between >= 2 and n[0] == n[1] == 1 + 2 * (between + 1) and n[2] == 0  # the others spoke, the measured slot emitted nothing
    out["slot 2 of 3"] = (s.fetch_alignment(2, F + 4).copy(), lp[T0 - 1:].copy())
    s.close()
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kv", ["fp32", "bf16"])
def test_the_same_bits_however_the_rows_are_fed(model, kv):
    run = model.run(kv)
    rows, lp = run["one call"]
    assert (rows[:F, :, 0] >= 0).all() and (rows[:F, :, 0] <= 1 + 1e-6).all() and np.isfinite(lp).all() and (lp <= 0).all()
    assert (rows[F:, :, 0] == -1).all() and (rows[F:, :, 1] == 0).all()  # nothing behind the last frame
    for name in ("chunks of 16", "slot 2 of 3"):
        r, l = run[name]
        assert np.array_equal(_bits(r), _bits(rows)), f"{model.name} {kv} {name}: the alignment rows differ from one call's"
        assert np.array_equal(_bits(l), _bits(lp)), f"{model.name} {kv} {name}: the scores differ from one call's"
    even = run["even frames"]
    assert np.array_equal(_bits(even[:F:2]), _bits(rows[:F:2]))
    assert (even[1:F:2, :, 0] == -1).all() and (even[1:F:2, :, 1] == 0).all()  # rows with row_frame < 0 wrote nothing


@pytest.mark.parametrize("kv", ["fp32", "bf16"])
def test_the_measured_rows_are_the_ones_the_decode_frames_recorded(model, kv):
    """Measured on the MI355X before this assertion was written: on both configs, with fp32 and bf16 KV and in every
    chunking, the teacher-forced (m, s1) rows and scores equal the decode frames' bit for bit."""
    run = model.run(kv)
    rows_d, lp_d = run["decode"]
    for name in ("one call", "chunks of 16", "slot 2 of 3"):
        r, l = run[name]
        d_rows = float(np.abs(r[:F].astype(np.float64) - rows_d[:F]).max())
        d_lp = float(np.abs(l.astype(np.float64) - lp_d).max())
        print(f"{model.name} {kv} {name}: largest |rows - decode| = {d_rows:.3e} (m, s1), {d_lp:.3e} (logprob)")
    for name in ("one call", "chunks of 16", "slot 2 of 3"):
        r, l = run[name]
        assert np.array_equal(_bits(r[:F]), _bits(rows_d[:F])), f"{model.name} {kv} {name}: alignment rows differ from the decode frames'"
        assert np.array_equal(_bits(l), _bits(lp_d)), f"{model.name} {kv} {name}: scores differ from the decode frames'"


# ---------------------------------------------------------------------------------------------------- 4. / 5. the front ends
HEADS = [(0, 1), (1, 4)]
TEXT, OTHER = "align these words", "other words, same"  # the same length


def _check(ra, text, n_samples):
    a = ra.alignment
    F = n_samples // 1920
    assert a.characters == list(text) and len(a.start_s) == len(a.end_s) == len(text)
    assert a.start_s[0] == 0.0 and a.end_s[-1] == pytest.approx(F * 1920 / 24000)
    assert all(s <= e for s, e in zip(a.start_s, a.end_s)) and all(x <= y for x, y in zip(a.start_s, a.start_s[1:]))
    assert ra.logprobs.shape == (F,) and ra.logprobs.dtype == np.float32 and np.isfinite(ra.logprobs).all()
    assert np.isfinite(ra.loss) and ra.loss == pytest.approx(-float(ra.logprobs.astype(np.float64).mean())) and np.isfinite(ra.end_logprob)
    assert [w.text for w in ra.words] == text.split()
    j = ra.to_json()
    assert set(j) == {"characters", "words", "loss"} and [c["text"] for c in j["characters"]] == list(text)
    assert all(set(w) == {"text", "start", "end", "loss"} for w in j["words"])


def _same(x, y):
    assert x.alignment.start_s == y.alignment.start_s and x.alignment.end_s == y.alignment.end_s
    assert np.array_equal(_bits(x.logprobs), _bits(y.logprobs)) and x.loss == y.loss and x.end_logprob == y.end_logprob
    assert np.array_equal(x.alignment.mass, y.alignment.mass) and np.array_equal(x.alignment.centroid, y.alignment.centroid, equal_nan=True)
    assert x.words == y.words


def test_the_facade_aligns_the_audio_the_model_generated():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_encoder_state, synthetic_mimi_state
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    mst = {**synthetic_mimi_state(seed=2), **synthetic_mimi_encoder_state(seed=2)}
    tts = SmolTTS(state=synthetic_lm_state(cfg, seed=11), config=cfg, mimi_state=mst, alignment_heads=HEADS)
    pcm = tts(TEXT, "sky", generation_settings=GenerationSettings.greedy(max_new_tokens=12))
    assert pcm.size >= 2 * 1920
    ra = tts.align_recording(pcm, TEXT, "sky")
    _check(ra, TEXT, pcm.size)
    _same(ra, tts.align_recording(pcm, TEXT, "sky"))  # the call repeats itself
    # the ranking tool's measurement on the same recording: every head of the model, teacher-forced, through rank_heads
    from smoltts_amd.align import measure_heads_recorded, rank_heads

    rg = tts.recording_grid(pcm, TEXT, "sky")
    every = [(l, h) for l in range(cfg.n_layer) for h in range(cfg.n_head)]
    runs = measure_heads_recorded(tts.lm, [rg.grid], [rg.window], [rg.frame_of_row], every)
    assert len(runs) == 1 and runs[0]["m"].shape == (rg.n_frames, len(every)) and runs[0]["n_tokens"] == len(TEXT)
    assert (runs[0]["m"] >= 0).all() and (runs[0]["m"] <= 1 + 1e-6).all()
    chosen = [every.index(p) for p in HEADS]
    assert np.array_equal(runs[0]["m"][:, chosen].astype(np.float64).sum(axis=1), ra.alignment.mass)  # a head's row does not depend on the others chosen
    assert sorted((r.layer, r.head) for r in rank_heads(runs)) == every
    other = tts.align_recording(pcm, OTHER, "sky")
    _check(other, OTHER, pcm.size)
    assert other.loss != ra.loss  # the score sees the transcript
    half = tts.align_recording(pcm[::2], TEXT, "sky", rate=12000)  # resampled as a voice sample is
    assert half.logprobs.shape[0] in (pcm.size // 1920, pcm.size // 1920 - 1)
    with pytest.raises(ValueError, match="text"):
        tts.align_recording(pcm, "  ", "sky")
    with pytest.raises(ValueError, match="full frame"):
        tts.align_recording(pcm[:1000], TEXT, "sky")
    with pytest.raises(ValueError, match=r"context allows \d+\.\d+ s"):
        tts.align_recording(np.zeros(1920 * (cfg.max_seq_len + 1), np.float32), TEXT, "sky")
    bare = SmolTTS(state=synthetic_lm_state(cfg, seed=11), config=cfg, mimi_state=mst)
    with pytest.raises(ValueError, match="align rank"):
        bare.align_recording(pcm, TEXT, "sky")


def _scheduler(max_batch=3):
    from smoltts_amd.server.pool import synthetic_scheduler

    return synthetic_scheduler("tiny", 21, 5, max_batch, 2, 12, mimi_encoder=True, alignment_heads=HEADS)


def _blocking(sched, text, **kw):
    req = sched.submit(text, "sky", **kw)
    pcm = np.concatenate(list(sched.iter_chunks(req)) or [np.zeros(0, np.float32)])
    return req, pcm


def test_the_scheduler_measures_between_ticks_and_leaves_its_serving_session_alone():
    from smoltts_amd.codec.synthetic import synthetic_pcm

    texts = ["first request", "the second one, longer", "third"]
    noise = synthetic_pcm(10 * 1920 + 700, seed=3)  # any audio is a recording: 10 frames and a rest that is cut
    served = {}
    for measures in (True, False):  # a scheduler that measured first, and one that never did
        sched = _scheduler()
        try:
            if measures:
                form = sched.session.graph_form()
                first = sched.align_recording(noise, TEXT, "sky")
                _check(first, TEXT, noise.size)
                assert sched.session.graph_form() == form and not sched.session.align_slots and not sched._slot_align
                assert sched._scratch is not None and sched._scratch.alignment is not None  # a buffer of its own
            out = [_blocking(sched, t, timestamps=True) for t in texts]
            served[measures] = [(pcm, r.alignment) for r, pcm in out]
            if measures:  # the same answer while two requests speak
                reqs = [sched.submit(t, "sky") for t in texts[:2]]
                busy = sched.align_recording(noise, TEXT, "sky")
                for r in reqs:
                    assert sum(c.size for c in sched.iter_chunks(r)) > 0
                _same(busy, first)
                pcm = served[True][0][0]
                own = sched.align_recording(pcm, texts[0], "sky")  # ... and of what the model itself said
                _check(own, texts[0], pcm.size)
                with pytest.raises(ValueError, match=r"context allows \d+\.\d+ s"):
                    sched.align_recording(np.zeros(1920 * 14, np.float32), TEXT, "sky")  # max_frames is 13 here
                with pytest.raises(ValueError, match="full frame"):
                    sched.align_recording(noise[:100], TEXT, "sky")
                with pytest.raises(ValueError, match="text"):
                    sched.align_recording(noise, "", "sky")
        finally:
            sched.close()
    for (pcm_a, al_a), (pcm_b, al_b) in zip(served[True], served[False]):
        assert np.array_equal(pcm_a, pcm_b)
        assert al_a.start_s == al_b.start_s and al_a.end_s == al_b.end_s
        assert np.array_equal(al_a.mass, al_b.mass) and np.array_equal(al_a.centroid, al_b.centroid, equal_nan=True)


def _float_wav(pcm, rate=24000):
    import struct

    data = np.asarray(pcm, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + \
        b"data" + struct.pack("<I", len(data)) + data


def test_the_pool_relays_and_the_route_answers():
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.codec.synthetic import synthetic_pcm
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.pool import GpuPool, synthetic_scheduler

    noise = synthetic_pcm(8 * 1920, seed=4)
    pool = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, 2, 12, mimi_encoder=True, alignment_heads=HEADS), devices=[0],
                   start_method="forkserver", alignment_heads=HEADS)
    try:
        ra = pool.align_recording(noise, TEXT, "sky")
        _check(ra, TEXT, noise.size)
        with pytest.raises(ValueError, match="full frame"):
            pool.align_recording(noise[:10], TEXT, "sky")
        with pytest.raises(ValueError, match="text"):
            pool.align_recording(noise, "", "sky")
        with pytest.raises(ValueError, match="context allows"):
            pool.align_recording(np.zeros(1920 * 14, np.float32), TEXT, "sky")
        client = TestClient(create_app(None, {}, scheduler=pool))
        body = {"audio": base64.b64encode(_float_wav(noise)).decode("ascii"), "text": TEXT, "voice": "sky"}
        r = client.post("/v1/forced-alignment", json=body)
        assert r.status_code == 200, r.text
        assert r.json() == ra.to_json()
        long = dict(body, audio=base64.b64encode(_float_wav(np.zeros(1920 * 14, np.float32))).decode("ascii"))
        r = client.post("/v1/forced-alignment", json=long)
        assert r.status_code == 400 and "context allows" in r.json()["detail"]
        assert client.post("/v1/forced-alignment", json=dict(body, audio="AAAA")).status_code == 400
        assert client.post("/v1/forced-alignment", json=dict(body, text=" ")).status_code == 400
    finally:
        pool.close()

    class NoHeads:  # a scheduler without alignment_heads: the route answers before it looks at the body
        alignment_heads = []

    r = TestClient(create_app(None, {}, scheduler=NoHeads())).post("/v1/forced-alignment", json=body)
    assert r.status_code == 501 and "align rank" in r.json()["detail"]
