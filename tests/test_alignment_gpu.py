"""The alignment rows of a session (``LMSession.set_align_heads`` / ``set_slot_align``): what the decode frames write about where
chosen heads of the slow attention look, on the tiny and 70m synthetic configs.

1. The option changes no id -- greedy and sampled, every slot of a mixed batch, with single-frame graphs, 4-frame graphs and
   SMOLTTS_NO_GRAPH=1 -- and the rows are the same bits in the three launch modes.
2. The rows of two heads in two layers against a float64 oracle whose blocks record q (``make_oracles(..., block_cls=)``),
   teacher-forced on the emitted grid: (m, s1) of the same formula over the oracle's keys, within FACTOR x the fp32 oracle's own
   error in max and rms, per layer and component (the form tests/test_lm_strict_gpu.py uses).
3. Frames the session did not measure read m = -1: frame 0 behind ``prefill`` (a prefill row), everything behind a slot's last
   frame, every frame of a slot whose window is off.
4. A slot re-used by a new tenant with another window gets the new window, and with every window off the form loses bit 5."""
import os

import numpy as np
import pytest
import torch

from lm_strict_helpers import FACTOR, make_oracles, random_grid, rms

pytestmark = pytest.mark.gpu

CAP = 10
TS = (5, 40, 17, 70)
PAIRS = {"tiny": [(0, 1), (1, 4)], "smoltts_byte_70m": [(3, 2), (9, 7)]}
GREEDY = [(0.0, 0.0, 0.0, 0)] * 4
SAMPLED = [(0.9, 0.8, 0.0, 11), (0.0, 0.0, 0.0, 0), (0.8, 0.0, 0.05, 12), (0.7, 0.7, 0.0, 13)]
ON = (True, False, True, False)  # the mixed batch: slots 0 and 2 measure


def _rec_block():
    from oracle.lm_oracle import _Block

    class RecBlock(_Block):
        """The oracle's block, keeping the q of its last ``qkv`` call (after RoPE): [1, S, H, 64] of a teacher-forced pass."""

        def qkv(self, x, cs):
            q, k, v = super().qkv(x, cs)
            self.last_q = q
            return q, k, v

    return RecBlock


class _Model:
    def __init__(self, cfgname):
        from smoltts_amd.config import NumericsMode, TokenConfig
        from smoltts_amd.engine import LMEngine
        from smoltts_amd.tokenizer import load_tokenizer

        rec = _rec_block()
        self.name = cfgname
        self.cfg, state, _plain32, self.o64, self.o32 = make_oracles(cfgname, 3, block_cls=rec)
        for L in self.o64.layers:
            L.__class__ = rec
        self.eng = LMEngine(self.cfg, state, TokenConfig.from_tokenizer(load_tokenizer(), self.cfg), NumericsMode.torch_reference())
        gen = torch.Generator().manual_seed(17)
        self.prompts = [random_grid(self.cfg, T, gen) for T in TS]
        self.pairs = PAIRS[cfgname]


@pytest.fixture(scope="module", params=["tiny", "smoltts_byte_70m"])
def model(request):
    m = _Model(request.param)
    yield m
    m.eng.close()


def _window(T):
    return (1, T - 1) if T > 6 else (0, T)


def _session(m, entries, on, per_graph, B=4):
    from smoltts_amd.engine import LMSession

    s = LMSession(m.eng, B, max_seq=128, max_rows=256, max_frames=CAP)
    s.set_frames_per_graph(per_graph)
    s.set_slot_sampling(list(range(len(entries))), *[list(x) for x in zip(*entries)])
    if on is not None:
        s.set_align_heads(m.pairs)
        wins = [_window(T) if o else (0, 0) for T, o in zip(TS, on)]
        s.set_slot_align(list(range(len(on))), [w[0] for w in wins], [w[1] for w in wins])
    return s


def _run(m, entries, on, per_graph=1, no_graph=False, defer=False):
    """(codes [4, CAP, H], n_frames, rows [4, CAP, pairs, 2] or None) of one whole run: a prefill and CAP - 1 decode frames."""
    old = os.environ.get("SMOLTTS_NO_GRAPH")
    if no_graph:
        os.environ["SMOLTTS_NO_GRAPH"] = "1"
    try:
        s = _session(m, entries, on, per_graph)
        s.prefill(m.prompts, stop_on_eos=False, defer_frame0=defer)
        s.decode(CAP if defer else CAP - 1)
        codes, n, _, _ = s.fetch()
        rows = None if on is None else s.alignment.cpu().numpy().copy()
        form = s.graph_form()
        s.close()
    finally:
        if no_graph:
            os.environ.pop("SMOLTTS_NO_GRAPH")
            if old is not None:
                os.environ["SMOLTTS_NO_GRAPH"] = old
    assert (n == CAP).all(), n
    assert bool(form & 32) == (on is not None and any(on))
    return codes.copy(), n.copy(), rows


@pytest.mark.parametrize("entries", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_the_option_changes_no_id_and_the_rows_do_not_depend_on_the_launch_mode(model, entries):
    base, _, _ = _run(model, entries, None)
    if entries is SAMPLED:
        greedy, _, _ = _run(model, GREEDY, None)
        assert not np.array_equal(greedy[0], base[0])  # the sampled entries do sample
    rows = {}
    for mode, kw in (("one frame per graph", dict(per_graph=1)), ("four frames per graph", dict(per_graph=4)),
                     ("no graph", dict(no_graph=True))):
        codes, _, rows[mode] = _run(model, entries, ON, **kw)
        assert np.array_equal(codes, base), f"{model.name} {mode}: the ids differ with the option on"
    first = rows["one frame per graph"]
    for mode, r in rows.items():
        assert np.array_equal(r.view(np.uint32), first.view(np.uint32)), f"{model.name} {mode}: the rows differ from the single-frame graphs'"
    # 3. what was not measured reads m = -1: the slots whose window is off, and frame 0, which came out of the prefill's tail
    for b, o in enumerate(ON):
        if not o:
            assert (first[b, :, :, 0] == -1).all() and (first[b, :, :, 1] == 0).all(), b
        else:
            assert (first[b, 0, :, 0] == -1).all(), b
            assert (first[b, 1:, :, 0] >= 0).all() and (first[b, 1:, :, 0] <= 1 + 1e-6).all(), (b, first[b, :, :, 0])
    all_on, _, rows_all = _run(model, entries, (True,) * 4)
    assert np.array_equal(all_on, base)
    for b, o in enumerate(ON):  # a slot's rows do not depend on what the other slots asked for
        if o:
            assert np.array_equal(rows_all[b].view(np.uint32), first[b].view(np.uint32)), b


def _formula(q, K, pos, t0, t1, dtype):
    sc = (K[:pos + 1].astype(dtype) @ q.astype(dtype)) * dtype(0.125)
    e = np.exp(sc - sc.max())
    p = e / e.sum(dtype=dtype)
    lo, hi = max(t0, 0), min(t1, pos + 1)
    if hi <= lo:
        return dtype(0), dtype(0)
    return p[lo:hi].sum(dtype=dtype), (p[lo:hi] * (np.arange(lo, hi) - t0).astype(dtype)).sum(dtype=dtype)


def test_rows_match_the_float64_oracle_within_the_fp32_oracle_noise(model):
    m = model
    codes, n, rows = _run(m, GREEDY, (True,) * 4, per_graph=4, defer=True)  # deferred frame 0: a decode row, measured like the others
    assert (rows[:, :, :, 0] >= 0).all()
    G = m.cfg.n_head // m.cfg.n_local_heads
    own, diff = {}, {}
    for b, T in enumerate(TS):
        grid = np.concatenate([m.prompts[b], codes[b, :CAP - 1].T], axis=1)  # the columns whose rows the frames 0 .. CAP - 1 were picked at
        t0, t1 = _window(T)
        ref = {}
        for orc, dt in ((m.o32, np.float32), (m.o64, np.float64)):
            orc.teacher_forced(torch.as_tensor(grid).long())
            ref[dt] = np.zeros((CAP, len(m.pairs), 2), dt)
            for i, (l, h) in enumerate(m.pairs):
                q = orc.layers[l].last_q[0, :, h].numpy()
                K = orc.tf_K[l][:, h // G].numpy()
                for f in range(CAP):
                    ref[dt][f, i] = _formula(q[T - 1 + f], K, T - 1 + f, t0, t1, dt)
        for i, (l, _h) in enumerate(m.pairs):
            for comp in (0, 1):
                own.setdefault((l, comp), []).append(ref[np.float32][:, i, comp].astype(np.float64) - ref[np.float64][:, i, comp])
                diff.setdefault((l, comp), []).append(rows[b, :, i, comp].astype(np.float64) - ref[np.float64][:, i, comp])
    fails = []
    for key in own:
        o, d = np.concatenate(own[key]), np.concatenate(diff[key])
        e_ref, r_ref, e, r = float(np.abs(o).max()), rms(o), float(np.abs(d).max()), rms(d)
        assert e_ref > 0.0, key
        line = (f"{m.name} layer {key[0]} {'m' if key[1] == 0 else 's1'}: max err {e:.3e} = {e / e_ref:.2f} x E_ref ({e_ref:.3e}), "
                f"rms {r:.3e} = {r / r_ref:.2f} x R_ref ({r_ref:.3e})")
        print(line)
        if e > FACTOR * e_ref or r > FACTOR * r_ref:
            fails.append(line + f", bound {FACTOR:g}")
    assert not fails, "\n".join(fails)


def test_a_new_tenant_gets_its_own_window_and_all_off_drops_the_form(model):
    from smoltts_amd.engine import LMSession

    m = model
    s = _session(m, GREEDY, (True,) * 4, per_graph=4)
    s.prefill(m.prompts, stop_on_eos=False, defer_frame0=True)
    s.decode(CAP)
    s.fetch()
    assert s.graph_form() & 32
    # slot 1's next tenant: prompt 3 with a window of its own, the other slots are through and keep theirs
    new_win = (3, 50)
    s.set_slot_align([1], [new_win[0]], [new_win[1]])
    s.prefill([m.prompts[3]], slots=[1], stop_on_eos=False, defer_frame0=True)
    s.decode(CAP)
    codes, n, _, _ = s.fetch()
    got = s.alignment[1].cpu().numpy().copy()
    # the same tenant alone in slot 0 of a fresh one-slot session
    f = LMSession(m.eng, 1, max_seq=128, max_rows=256, max_frames=CAP)
    f.set_slot_sampling([0], [0.0], [0.0], [0.0], [0])
    f.set_align_heads(m.pairs)
    f.set_slot_align([0], [new_win[0]], [new_win[1]])
    f.prefill([m.prompts[3]], stop_on_eos=False, defer_frame0=True)
    f.decode(CAP)
    fcodes, _, _, _ = f.fetch()
    want = f.alignment[0].cpu().numpy().copy()
    f.close()
    assert np.array_equal(codes[1], fcodes[0])
    assert (want[:, :, 0] >= 0).all() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    old = s.alignment[3].cpu().numpy()
    assert not np.array_equal(got, old)  # (the previous holder of that prompt measured another window)
    # every window off: the form has lost bit 5, and the frames write nothing
    s.set_slot_align([0, 1, 2, 3], [0] * 4, [0] * 4)
    assert s.graph_form() & 32 == 0 and not s.align_slots
    s.prefill([m.prompts[0]], slots=[2], stop_on_eos=False, defer_frame0=True)
    s.decode(CAP)
    s.fetch()
    rows = s.alignment.cpu().numpy()
    assert (rows[:, :, :, 0] == -1).all() and (rows[:, :, :, 1] == 0).all()
    s.close()


# ---------------------------------------------------------------------------------------------------- the front end
@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=11), config=cfg, mimi_state=synthetic_mimi_state(seed=2), alignment_heads=[(1, 4), (0, 1)])


def test_the_facade_returns_the_same_audio_and_an_alignment_of_the_text(tts):
    from smoltts_amd.align import window_of
    from smoltts_amd.config import GenerationSettings, RequestSampling

    text = "Hé, timestamps!"
    gs = GenerationSettings.greedy(max_new_tokens=12)
    for sampling in (None, RequestSampling(temperature=0.8, seed=5)):
        plain = tts(text, "sky", generation_settings=gs, sampling=sampling)
        assert tts.last_alignment is None
        pcm = tts(text, "sky", generation_settings=gs, sampling=sampling, timestamps=True)
        assert np.array_equal(pcm, plain)  # the option changes no sample
        a = tts.last_alignment
        assert a.characters == list(text) and len(a.start_s) == len(a.end_s) == len(text)
        assert a.start_s[0] == 0.0 and a.end_s[-1] == pytest.approx(pcm.size / 24000)
        assert all(s <= e for s, e in zip(a.start_s, a.end_s)) and all(x <= y for x, y in zip(a.start_s, a.start_s[1:]))
        F = pcm.size // 1920
        assert a.mass.shape == (F,) and a.mass[0] == -1 and (a.mass[1:] >= 0).all() and (a.mass[1:] <= 2 + 1e-5).all()
    t0, t1 = window_of(tts._get_prompt(text, "sky")[0], tts.tokenizer)
    assert t1 - t0 == len(text)  # latin-1 text: one token per character
    fast = tts(text, "sky", generation_settings=gs, timestamps=True, speed=1.5)
    b = tts.last_alignment
    assert b.end_s[-1] == pytest.approx(fast.size / 24000) and max(b.end_s) <= fast.size / 24000 + 1e-9
    for kw in (dict(segment=True), dict(trim_silence=True), dict(max_pause_s=0.5)):
        with pytest.raises(ValueError):
            tts(text, "sky", generation_settings=gs, timestamps=True, **kw)
    with pytest.raises(ValueError):
        tts(text, "sky", generation_settings=gs, timestamps=True, sampling=RequestSampling(temperature=0.8, best_of=2))


def test_measure_heads_and_the_ranking_run_on_a_model(tts):
    from smoltts_amd.align import measure_heads, rank_heads, window_of

    prompts = [tts._get_prompt(t, "sky") for t in ("first text", "a second, longer text")]
    windows = [window_of(p[0], tts.tokenizer) for p in prompts]
    pairs = [(l, h) for l in range(2) for h in range(6)]
    runs = measure_heads(tts.lm, prompts, windows, pairs, max_frames=10)
    assert len(runs) == 2 and runs[0]["m"].shape[1] == 12 and runs[0]["n_tokens"] == len("first text")
    ranked = rank_heads(runs)
    assert sorted((r.layer, r.head) for r in ranked) == pairs and all(0 <= r.mean_mass <= 1 + 1e-6 for r in ranked)


# ---------------------------------------------------------------------------------------------------- the serving side
HEADS = [(0, 1), (1, 4)]


def _scheduler(heads=HEADS, max_batch=2):
    from smoltts_amd.server.pool import synthetic_scheduler

    return synthetic_scheduler("tiny", 21, 5, max_batch, 2, 12, alignment_heads=heads)


def _blocking(sched, text, **kw):
    req = sched.submit(text, "sky", **kw)
    pcm = np.concatenate(list(sched.iter_chunks(req)) or [np.zeros(0, np.float32)])
    return req, pcm


def _check_alignment(a, text, pcm):
    assert a.characters == list(text) and len(a.start_s) == len(a.end_s) == len(text)
    assert a.start_s[0] == 0.0 and a.end_s[-1] == pytest.approx(pcm.size / 24000)
    assert all(s <= e for s, e in zip(a.start_s, a.end_s)) and all(x <= y for x, y in zip(a.start_s, a.start_s[1:]))


def test_the_scheduler_serves_alignments_and_hands_no_window_to_the_next_tenant():
    texts = ["first request", "the second one, longer", "third", "and a fourth text"]
    sched = _scheduler()
    try:
        alone = {}
        for t in texts:  # one at a time: each in a slot of its own turn
            req, pcm = _blocking(sched, t, timestamps=True)
            _check_alignment(req.alignment, t, pcm)
            F = pcm.size // 1920
            assert req.alignment.mass.shape == (F,) and (req.alignment.mass >= 0).all()  # frame 0 is a decode row here: measured
            plain, pcm0 = _blocking(sched, t)
            assert plain.alignment is None and np.array_equal(pcm, pcm0)  # the option changes no sample
            alone[t] = req.alignment
        assert not sched._slot_align and not sched.session.align_slots  # every window was switched off behind its tenant
        assert sched.session.graph_form() & 32 == 0
        # together, more requests than slots, every other one without the option: a slot changes tenant with and without a window,
        # and each alignment is the one the request gets alone (same bits in any slot of any batch)
        import threading

        out = {}

        def run(i, t):
            out[i] = _blocking(sched, t, **({"timestamps": True} if i % 2 == 0 else {}))

        order = texts + texts[::-1]
        threads = [threading.Thread(target=run, args=(i, t)) for i, t in enumerate(order)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for i, t in enumerate(order):
            req, pcm = out[i]
            if i % 2:
                assert req.alignment is None
                continue
            _check_alignment(req.alignment, t, pcm)
            assert np.array_equal(req.alignment.mass, alone[t].mass) and np.array_equal(req.alignment.centroid, alone[t].centroid, equal_nan=True), (i, t)
            assert req.alignment.start_s == alone[t].start_s and req.alignment.end_s == alone[t].end_s
        assert not sched._slot_align
        fast, pcm = _blocking(sched, texts[0], timestamps=True, speed=1.5)
        _check_alignment(fast.alignment, texts[0], pcm)
        # refusals, before anything is queued
        from smoltts_amd.config import RequestSampling

        for kw in (dict(segment=True), dict(trim_silence=True), dict(max_pause_s=0.5), dict(stream=True),
                   dict(sampling=RequestSampling(temperature=0.8, best_of=2))):
            with pytest.raises(ValueError):
                sched.submit(texts[0], "sky", timestamps=True, **kw)
    finally:
        sched.close()
    bare = _scheduler(heads=None)
    try:
        with pytest.raises(ValueError, match="alignment_heads"):
            bare.submit("hello", "sky", timestamps=True)
        assert bare.session.alignment is None
    finally:
        bare.close()


def test_the_pool_relays_the_alignment_and_the_route_serves_it():
    import base64
    import functools

    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.pool import GpuPool, synthetic_scheduler

    pool = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, 2, 12, alignment_heads=HEADS), devices=[0],
                   start_method="forkserver", alignment_heads=HEADS)
    try:
        text = "through the pool"
        req, pcm = _blocking(pool, text, timestamps=True)
        _check_alignment(req.alignment, text, pcm)
        plain, pcm0 = _blocking(pool, text)
        assert plain.alignment is None and np.array_equal(pcm, pcm0)
        with pytest.raises(ValueError):
            pool.submit(text, "sky", timestamps=True, segment=True)
        client = TestClient(create_app(None, {}, scheduler=pool))
        r = client.post("/v1/text-to-speech/sky/with-timestamps?output_format=pcm_24000", json={"text": text})
        assert r.status_code == 200
        j = r.json()
        assert j["alignment"] == req.alignment.to_json() == j["normalized_alignment"]
        assert base64.b64decode(j["audio_base64"]) == client.post("/v1/text-to-speech/sky?output_format=pcm_24000", json={"text": text}).content
        assert client.post("/v1/text-to-speech/sky/with-timestamps", json={"text": text, "trim_silence": True}).status_code == 400
    finally:
        pool.close()
    no_heads = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, 2, 12), devices=[0], start_method="forkserver")
    try:
        with pytest.raises(ValueError, match="alignment_heads"):
            no_heads.submit("x", "sky", timestamps=True)
        r = TestClient(create_app(None, {}, scheduler=no_heads)).post("/v1/text-to-speech/sky/with-timestamps", json={"text": "x"})
        assert r.status_code == 501 and "align rank" in r.json()["detail"]
    finally:
        no_heads.close()
