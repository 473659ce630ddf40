"""Cloned-voice prefixes on the GPU: the speaker turns' KV rows computed once (smoltts_session_save_prefix) and copied into the slots
of later requests (smoltts_session_install_prefix), whose own turns are prefilled from position P on.  The kernel is checked byte
for byte against the rows a direct chunked prefill writes; the session's ids against the direct path and the CPU oracle; the
scheduler's audio against the façade, which prefills the whole prompt every time."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 8


def _setup(name, seed=13):
    from smoltts_amd.config import TokenConfig
    from smoltts_amd.engine import LMEngine
    from smoltts_amd.prompt import PromptEncoder
    from smoltts_amd.synthetic import named_config, synthetic_lm_state
    from smoltts_amd.tokenizer import load_tokenizer

    cfg = named_config(name)
    tok = load_tokenizer()
    tc = TokenConfig.from_tokenizer(tok, cfg)
    state = synthetic_lm_state(cfg, seed=seed)
    return cfg, state, LMEngine(cfg, state, tc), PromptEncoder(tok, tc.semantic_start_id, cfg.num_codebooks, cfg.duplicate_code_0)


def _speaker(pe, cfg, frames, seed, text="a reference line"):
    """A speaker grid as create_speaker builds it (user turn + Mimi codes + <|im_end|>), from random codes."""
    codes = np.random.default_rng(seed).integers(0, cfg.codebook_size, size=(cfg.num_codebooks, frames))
    return np.concatenate([pe.encode_text_turn("user", text), pe.encode_vq(codes)], axis=1).astype(np.int32)


def _chunks(sess, grid, slot):
    """The speaker grid alone into ``slot`` as non-final chunks (what a registration computes)."""
    for a in range(0, grid.shape[1], CHUNK):
        sess.prefill([grid[:, a: a + CHUNK]], [slot], pos0=[a], final=False)


def _prefix(eng, grid, kv, max_seq):
    from smoltts_amd.engine import LMSession

    s = LMSession(eng, 1, max_seq=max_seq, max_rows=CHUNK, max_frames=1, kv_dtype=kv)
    _chunks(s, grid, 0)
    pk = s.save_prefix(0, grid.shape[1])
    torch.cuda.synchronize()
    s.close()
    return pk


@pytest.mark.parametrize("kv", ["fp32", "bf16"])
def test_install_writes_the_rows_of_a_direct_prefill_byte_for_byte(kv):
    from smoltts_amd.engine import LMSession, PrefixHeader, SmolttsError

    cfg, state, eng, pe = _setup("tiny")
    grids = [_speaker(pe, cfg, 4, 1), _speaker(pe, cfg, 30, 2, "a longer reference line spanning many chunks"), _speaker(pe, cfg, 1, 3, "x")]
    P = [g.shape[1] for g in grids]
    assert len(set(P)) == 3 and max(P) > 3 * CHUNK
    slots = [0, 1, 3]
    direct = LMSession(eng, 4, max_seq=256, max_rows=64, max_frames=4, kv_dtype=kv)
    for g, b in zip(grids, slots):
        _chunks(direct, g, b)
    prefixes = [_prefix(eng, g, kv, 256) for g in grids]
    assert [p.n_positions for p in prefixes] == P
    sess = LMSession(eng, 4, max_seq=256, max_rows=64, max_frames=4, kv_dtype=kv)
    canary = []
    for t in sess.kv_cache():
        u = t.view(torch.uint8)
        u.copy_(torch.randint(0, 256, u.shape, dtype=torch.uint8, device=u.device))
        canary.append(u.clone())
    sess.install_prefix(prefixes, slots)  # one launch
    torch.cuda.synchronize()
    want = [t.view(torch.uint8) for t in direct.kv_cache()]
    got = [t.view(torch.uint8) for t in sess.kv_cache()]
    for w, g, c in zip(want, got, canary):
        for p, b in zip(P, slots):
            assert torch.equal(g[:, b, :, :p], w[:, b, :, :p]), f"slot {b}: installed rows differ from the direct prefill"
            assert torch.equal(g[:, b, :, p:], c[:, b, :, p:]), f"slot {b}: rows >= P touched"
        assert torch.equal(g[:, 2], c[:, 2]), "an unlisted slot was touched"
    # errors: mismatched dtype / layout, P too large, bad slots, a prefix that was never saved
    other = "bf16" if kv == "fp32" else "fp32"
    with pytest.raises(SmolttsError, match="kv format"):
        LMSession(eng, 2, max_seq=256, max_rows=64, max_frames=4, kv_dtype=other).install_prefix([prefixes[0]], [0])
    bad = _prefix(eng, grids[0], kv, 256)
    h = PrefixHeader()
    for f, _ in PrefixHeader._fields_:
        setattr(h, f, getattr(bad.header, f))
    h.n_layer += 1
    bad.header = h
    with pytest.raises(SmolttsError, match="layers"):
        sess.install_prefix([bad], [2])
    with pytest.raises(SmolttsError, match="max_seq"):
        LMSession(eng, 2, max_seq=P[1], max_rows=64, max_frames=4, kv_dtype=kv).install_prefix([prefixes[1]], [0])
    for s_bad in ([4], [-1]):
        with pytest.raises(SmolttsError, match="slot"):
            sess.install_prefix([prefixes[0]], s_bad)
    with pytest.raises(SmolttsError, match="twice"):
        sess.install_prefix([prefixes[0], prefixes[2]], [2, 2])
    with pytest.raises(SmolttsError):
        sess.save_prefix(4, 3)
    with pytest.raises(SmolttsError):
        sess.save_prefix(0, 256)
    torch.cuda.synchronize()
    got2 = [t.view(torch.uint8) for t in sess.kv_cache()]
    for g, g2 in zip(got, got2):
        assert torch.equal(g, g2), "a refused install changed the cache"


def _serve(eng, presets, suffixes, P, prefix, side: bool, F=12):
    """Slots 0, 1: preset prompts, speaking; slots 2, 3 then take two requests for the cloned voice -- their own turns prefilled
    at pos0 = P on top of the installed prefix (``prefix`` given) or of a direct chunked prefill of the speaker grid (``prefix`` is
    the grid) -- in line or beside the frames."""
    from smoltts_amd.engine import LMSession

    s = LMSession(eng, max_batch=4, max_seq=512, max_rows=512, max_frames=40)
    s.prefill(presets, slots=[0, 1], stop_on_eos=False, defer_frame0=True)
    s.decode(3)
    cached = not isinstance(prefix, np.ndarray)
    if not cached:
        for b in (2, 3):
            _chunks(s, prefix, b)
    kw = {"prefixes": [prefix, prefix]} if cached else {"pos0": [P, P]}
    if side:
        h = s.side_park(suffixes, [2, 3], **kw)
        s.decode(2)
        other = torch.cuda.Stream()
        with torch.cuda.stream(other):
            s.side_run(h)
        s.side_start(h, stop_on_eos=False)
    else:
        s.decode(2)
        s.prefill_chunked(suffixes, slots=[2, 3], stop_on_eos=False, chunk=CHUNK, between=lambda: s.decode(1), defer_frame0=True, **kw)
    s.decode(F)
    codes, n, done, margin = s.fetch()
    s.close()
    return codes, n, margin


@pytest.mark.parametrize("name", ["tiny", "smoltts_byte_70m"])
@pytest.mark.parametrize("side", [False, True])
def test_cached_prefix_gives_the_ids_of_the_direct_prefill_and_the_oracle(name, side):
    from oracle.lm_oracle import LMOracle, OracleLMConfig

    cfg, state, eng, pe = _setup(name)
    grid = _speaker(pe, cfg, 20, 7, "the cloned speaker's transcript")
    P = grid.shape[1]
    presets = [pe.build_prompt("the first tenant", "heart"), pe.build_prompt("a second one, speaking meanwhile", "nova")]
    texts = ["a cloned voice speaks", "and a second request for the same voice, with a longer text"]
    full = [pe.build_prompt(t, "cv", grid) for t in texts]
    suffixes = [f[:, P:] for f in full]
    assert all(np.array_equal(f[:, :P], grid) for f in full) and max(x.shape[1] for x in suffixes) > CHUNK
    pk = _prefix(eng, grid, "fp32", 512)
    a, na, ma = _serve(eng, presets, suffixes, P, pk, side)
    b, nb, mb = _serve(eng, presets, suffixes, P, grid, side)
    assert np.array_equal(na, nb)
    for slot in range(4):
        assert np.array_equal(a[slot, :na[slot]], b[slot, :nb[slot]]), f"slot {slot}: cached and direct prefix paths differ"
    F = 12
    assert list(na[2:]) == [F, F]
    orc = LMOracle(OracleLMConfig.from_dict(cfg.__dict__), state)
    logs = orc.generate([torch.from_numpy(f) for f in full], max_frames=F, stop_on_eos=False)
    for i, slot in enumerate((2, 3)):
        want = np.array(logs[i].grid)[:F]
        if not np.array_equal(a[slot, :F], want):  # allowed only at a near-tie (test_batch_invariance_gpu.py's rule)
            assert float(ma[slot]) < 1e-5, f"{name} slot {slot}: ids differ from the oracle although the smallest top-2 gap is {ma[slot]:.2e}"
    eng.close()


# ------------------------------------------------------------------ scheduler
@pytest.fixture(scope="module")
def clone_tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_encoder_state, synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    mst = {**synthetic_mimi_state(seed=5), **synthetic_mimi_encoder_state(seed=5)}
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=mst)


def _samples():
    from smoltts_amd.codec.synthetic import synthetic_pcm

    return ({"A": [{"text": "a first reference line", "audio": synthetic_pcm(1920 * 3 + 500, 1)}],
             "B": [{"text": "another speaker", "audio": synthetic_pcm(1920 * 2, 2)},
                   {"text": "and a second sample", "audio": synthetic_pcm(1920 * 2 + 100, 3)}]})


def _rms(g, w):
    return float(np.sqrt(np.mean((g.astype(np.float64) - w) ** 2))) if g.size else 0.0


def test_scheduler_serves_cloned_voices_like_the_facade(clone_tts):
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.server.scheduler import BatchScheduler

    tts = clone_tts
    smp = _samples()
    grids = {k: tts.create_speaker(v) for k, v in smp.items()}
    tts.add_voice("cv_facade_a", grids["A"])
    tts.add_voice("cv_facade_b", grids["B"])
    seeded = RequestSampling(temperature=0.8, fast_temperature=0.6, min_p=0.0, seed=4242)
    # (text, voice, frames, stream, output_format, sampling)
    reqs = [("first request", "heart", 6, False, None, None), ("cloned voice speaks", "A", 9, True, None, None),
            ("a blocking clone", "B", 7, False, None, None), ("formatted clone", "A", 8, True, "pcm_16000", None),
            ("seeded clone", "B", 10, False, None, seeded), ("preset streams", "sky", 5, True, None, None),
            ("another for b", "B", 6, True, None, None), ("last in line, voice a", "A", 5, False, None, None)]
    fac = {"A": "cv_facade_a", "B": "cv_facade_b"}
    want = []
    for text, voice, n, stream, fmt, sampling in reqs:
        gs = GenerationSettings.greedy(max_new_tokens=n)
        v = fac.get(voice, voice)
        kw = {"sampling": sampling} if sampling is not None else {}
        if stream:
            want.append(np.concatenate(list(tts.stream(text, v, generation_settings=gs, output_format=fmt, **kw))))
        else:
            want.append(tts(text, v, generation_settings=gs, **kw))
    # the façade's registered voice is the speaker= prompt
    assert np.array_equal(want[2], tts("a blocking clone", None, speaker=grids["B"], generation_settings=GenerationSettings.greedy(max_new_tokens=7)))
    sched = BatchScheduler(tts, max_batch=3, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=16),
                           prefill_chunk=8)
    try:
        ids = {}
        for k in ("A", "B"):
            vid = f"cv_sched_{k.lower()}"
            res = sched.add_voice(vid, samples=smp[k])
            assert res == {"voice_id": vid, "prompt_positions": grids[k].shape[1]}
            ids[k] = vid
        assert sched.stats()["voices"] == 2
        victim = sched.submit("this client hangs up early", ids["A"], stream=True, max_new_tokens=16)
        subs = [sched.submit(text, ids.get(voice, voice), stream=stream, max_new_tokens=n, output_format=fmt,
                             **({"sampling": s} if s is not None else {})) for text, voice, n, stream, fmt, s in reqs]
        sched.remove_voice(ids["B"])  # requests already submitted for it keep its prefix
        with pytest.raises(KeyError):
            sched.remove_voice(ids["B"])
        got = [None] * len(reqs)

        def collect(i):
            got[i] = np.concatenate(list(sched.iter_chunks(subs[i])) or [np.zeros(0, np.float32)])

        it = sched.iter_chunks(victim)
        next(it)
        it.close()  # cancels it
        threads = [threading.Thread(target=collect, args=(i,)) for i in range(len(reqs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        st = sched.stats()
    finally:
        sched.close()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g is not None and g.shape == w.shape and g.dtype == w.dtype, (i, None if g is None else (g.shape, g.dtype), w.shape)
        if reqs[i][4] is None:
            assert _rms(g, w) <= 1e-6, i
        else:  # int16 after the resampler: the codec chunks differ in the last bits (test_stream_formats_gpu.py)
            d = np.abs(g.astype(np.int32) - w.astype(np.int32))
            assert d.max() <= 1 and np.mean(d == 0) >= 0.995, i
    assert st["voices"] == 1 and st["prefix_installs"] >= 6 and st["cancelled"] >= 1


def test_cloned_arrival_among_speaking_slots_takes_the_side_path(clone_tts):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    tts = clone_tts
    grid = tts.create_speaker(_samples()["A"])
    P = grid.shape[1]
    want = tts("arrives while others speak", None, speaker=grid, generation_settings=GenerationSettings.greedy(max_new_tokens=8))
    sched = BatchScheduler(tts, max_batch=3, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=80),
                           prefill_chunk=8, side_prefill_min_active=2)
    calls = []
    s = sched.session
    for name in ("side_park", "prefill", "prefill_chunked", "install_prefix"):
        orig = getattr(s, name)

        def spy(*a, _orig=orig, _name=name, **k):
            calls.append((_name, a, k))
            return _orig(*a, **k)

        setattr(s, name, spy)
    try:
        assert sched.add_voice("cv_x", grid=grid)["prompt_positions"] == P
        talkers = [sched.submit(f"a long preset talker {i}", v, stream=True, max_new_tokens=80) for i, v in enumerate(("heart", "sky"))]
        its = [sched.iter_chunks(r) for r in talkers]
        for it in its:
            next(it)  # both speaking
        mark = len(calls)
        r = sched.submit("arrives while others speak", "cv_x", max_new_tokens=8)
        got = np.concatenate(list(sched.iter_chunks(r)))
        for it in its:
            it.close()
        new = calls[mark:]
    finally:
        sched.close()
    assert got.shape == want.shape and _rms(got, want) <= 1e-6
    parks = [c for c in new if c[0] == "side_park"]
    assert len(parks) == 1 and parks[0][2]["pos0"] == [P] and parks[0][2]["prefixes"][0] is not None
    assert parks[0][1][0][0].shape[1] == tts._get_prompt("arrives while others speak", "x").shape[1] - 5  # own turns only
    assert not [c for c in new if c[0] in ("prefill", "prefill_chunked")], "the arrival was prefilled in line"


def test_scheduler_limits_use_the_prefix(clone_tts):
    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.scheduler import BatchScheduler

    tts = clone_tts
    pe, cfg = tts.prompt_encoder, tts.config
    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=16),
                           prefill_chunk=8)
    try:
        t_min = pe.build_prompt("", "x").shape[1] - 5  # an empty request's own turns
        P = cfg.max_seq_len - t_min - 16 - 2 - 4       # room for 4 text tokens
        overhead = pe.encode_text_turn("user", "r").shape[1] + pe.tokenize_text("<|im_end|>\n").shape[1]
        big = _speaker(pe, cfg, P - overhead, 9, "r")
        assert big.shape[1] == P
        with pytest.raises(ValueError, match="max_seq_len"):
            sched.add_voice("cv_huge", grid=_speaker(pe, cfg, P + 10, 9, "r"))
        sched.add_voice("cv_big", grid=big)
        with pytest.raises(ValueError, match="max_seq_len"):
            sched.synthesize("this text is far too long for what is left of the context", "cv_big")
        assert sched.synthesize("ok", "cv_big", max_new_tokens=4).shape[0] % 1920 == 0
        assert sched.synthesize("still alive").shape[0] % 1920 == 0
    finally:
        sched.close()
