"""Per-request sampling on the GPU: the per-row sampler against the host model of its key, slot mode of a session (greedy
slots unchanged, draws independent of the slot, its tenants and its companions), the scheduler against the façade, and the
stream route.  Small models and at most 8 slots, so that the compared runs select the same kernel variants."""
import math
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _chi2_ok(counts, probs, n):
    keep = probs * n >= 5
    exp = probs[keep] * n
    chi2 = float(((counts[keep] - exp) ** 2 / exp).sum())
    dof = int(keep.sum()) - 1
    return chi2 < dof + 6 * math.sqrt(2 * dof), chi2, dof  # ~6 sigma


def test_sample_rows_greedy_rows_and_host_model():
    from smoltts_amd import ops
    from smoltts_amd.sampling import gumbel_keys, gumbel_pick

    g = torch.Generator().manual_seed(11)
    R, V = 64, 2048
    logits = (torch.randn(R, V, generator=g) * 3.0).cuda()
    temps = [0.0, 0.3, 0.7, 1.0, 1.5, 0.0, 2.0, 0.9] * (R // 8)
    fasts = [0.5, 0.0, 1.2, 0.0, 0.8, 0.0, 0.6, 1.0] * (R // 8)
    min_ps = [0.0, 0.0, 0.05, 0.2, 0.0, 0.5, 0.01, 0.0] * (R // 8)
    seeds = [int(x) for x in np.random.default_rng(2).integers(0, 2**63, R)]
    seeds[3] = 2**64 - 1
    table = ops.slot_sampling_table(temps, fasts, min_ps, seeds)
    frames = torch.arange(R, dtype=torch.int32, device="cuda") * 3 + 1
    host = logits.cpu().numpy()
    near = 0
    for step, tt in ((0, temps), (3, fasts)):
        ids = ops.sample_rows(logits, table, frames, step=step).cpu().numpy()
        for r in range(R):
            if tt[r] <= 0:
                assert ids[r] == int(torch.argmax(logits[r])), (step, r)
                continue
            mp = min_ps[r]
            want = gumbel_pick(host[r], tt[r], mp, seeds[r], int(frames[r]), step)
            if ids[r] != want:
                k = gumbel_keys(host[r], tt[r], mp, seeds[r], int(frames[r]), step)
                assert abs(k[ids[r]] - k[want]) < 1e-4, (step, r, ids[r], want)  # fp32 logf noise only
                near += 1
    assert near <= 2
    # the picks do not depend on the row order: rows permuted with their entries give the same ids
    perm = torch.randperm(R, generator=g)
    permuted = ops.sample_rows(logits[perm.cuda()].contiguous(), table.view(R, 24)[perm.cuda()].contiguous().view(-1),
                               frames[perm.cuda()].contiguous(), step=0)
    base = ops.sample_rows(logits, table, frames, step=0)
    assert torch.equal(permuted, base[perm.cuda()])


@pytest.mark.parametrize("temp", [0.7, 1.5])
def test_sample_rows_follows_softmax(temp):
    from smoltts_amd import ops

    V, n = 1024, 40000
    row = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 2.0
    logits = row[None].repeat(n, 1).contiguous().cuda()
    # one request per row, its frame number the row index: n independent draws at `temp` (the slow step) and at 2 * temp (depth)
    table = ops.slot_sampling_table([temp] * n, [2 * temp] * n, [0.0] * n, [77] * n)
    frames = torch.arange(n, dtype=torch.int32, device="cuda")
    for step, t in ((0, temp), (1, 2 * temp)):
        ids = ops.sample_rows(logits, table, frames, step=step).cpu().numpy()
        probs = torch.softmax((row / t).double(), 0).numpy()
        ok, chi2, dof = _chi2_ok(np.bincount(ids, minlength=V).astype(np.float64), probs, n)
        assert ok, f"t={t}: chi2 {chi2:.1f} for {dof} dof"


def _engine(model="tiny", seed=21):
    from smoltts_amd.config import TokenConfig
    from smoltts_amd.engine import LMEngine
    from smoltts_amd.prompt import PromptEncoder
    from smoltts_amd.synthetic import named_config, synthetic_lm_state
    from smoltts_amd.tokenizer import load_tokenizer

    cfg = named_config(model)
    tok = load_tokenizer()
    tc = TokenConfig.from_tokenizer(tok, cfg)
    pe = PromptEncoder(tok, tc.semantic_start_id, cfg.num_codebooks, cfg.duplicate_code_0)
    return LMEngine(cfg, synthetic_lm_state(cfg, seed=seed), tc), pe


def _run(eng, prompts, entries=None, frames=12, slots=None):
    """Codes of every prompt (stop_on_eos off: all run `frames` frames); entries: (temp, fast, min_p, seed) per prompt -> slot mode."""
    from smoltts_amd.engine import LMSession

    B = len(prompts)
    s = LMSession(eng, B, max_seq=256, max_rows=256 * B, max_frames=frames)
    if entries is not None:
        s.set_slot_sampling(list(range(B)), *[list(x) for x in zip(*entries)])
    s.prefill(prompts, stop_on_eos=False)
    s.decode(frames - 1)
    codes, n, _, _ = s.fetch()
    s.close()
    assert (n == frames).all()
    return codes[:, :frames].copy()


def test_slot_mode_all_greedy_equals_session_wide_greedy():
    eng, pe = _engine()
    prompts = [pe.build_prompt(t, v) for t, v in (("one", "heart"), ("a second prompt", "sky"), ("3", "nova"))]
    want = _run(eng, prompts)
    got = _run(eng, prompts, entries=[(0.0, 0.0, 0.0, 5)] * 3)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("model", ["tiny", "smoltts_byte_70m"])
def test_slot_draws_do_not_depend_on_slot_or_companions(model):
    eng, pe = _engine(model)
    p = pe.build_prompt("the same prompt in four slots", "heart")
    entries = [(0.0, 0.0, 0.0, 0), (0.8, 0.8, 0.0, 1), (0.8, 0.8, 0.0, 1), (0.8, 0.7, 0.0, 2)]
    got = _run(eng, [p] * 4, entries=entries)
    assert np.array_equal(got[1], got[2])
    assert not np.array_equal(got[1], got[3])
    assert np.array_equal(got[0], _run(eng, [p])[0])  # the greedy slot beside sampled ones = greedy alone
    assert np.array_equal(got[1], _run(eng, [p], entries=[entries[1]])[0])  # = the same request alone


def test_second_tenant_with_the_same_seed_repeats_the_first():
    from smoltts_amd.engine import LMSession

    eng, pe = _engine()
    p = pe.build_prompt("tenant after tenant", "sky")
    q = pe.build_prompt("a neighbour", "nova")
    s = LMSession(eng, 2, max_seq=256, max_rows=512, max_frames=10)
    s.set_slot_sampling([0, 1], [0.9, 0.5], [0.9, 0.0], [0.0, 0.0], [31, 4])
    out = []
    for seed in (31, 31, 32):
        s.set_slot_sampling([0], [0.9], [0.9], [0.0], [seed])
        s.prefill([p, q] if not out else [p], slots=[0, 1] if not out else [0], stop_on_eos=False)
        s.decode(9)
        codes, n, _, _ = s.fetch()
        assert n[0] == 10
        out.append(codes[0, :10].copy())
    s.close()
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0], out[2])


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


def test_scheduler_seeded_request_equals_the_facade_alone(tts):
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.server.scheduler import BatchScheduler

    target = RequestSampling(temperature=0.8, fast_temperature=0.6, min_p=0.0, seed=123456789)
    gs = GenerationSettings.greedy(max_new_tokens=12)
    want_block = tts("the seeded request", "heart", generation_settings=gs, sampling=target)
    want_stream = np.concatenate(list(tts.stream("the seeded request", "heart", generation_settings=gs, sampling=target)))
    # 4 slots, 3 companions with other settings, more requests than slots: refills go through side prefill (min active 1)
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=16),
                           prefill_chunk=8, side_prefill_min_active=1)
    reqs = [("a greedy companion", "sky", None, False), ("a sampled companion", "nova", RequestSampling(temperature=0.6, seed=9), True),
            ("another one", "bella", RequestSampling(temperature=0.9, fast_temperature=0.5), False),
            ("the seeded request", "heart", target, False), ("filler request number five", "liam", RequestSampling(temperature=1.2), False),
            ("the seeded request", "heart", target, True)]
    got = [None] * len(reqs)

    def worker(i):
        text, voice, smp, stream = reqs[i]
        r = sched.submit(text, voice, stream=stream, max_new_tokens=12, sampling=smp)
        got[i] = np.concatenate(list(sched.iter_chunks(r)) or [np.zeros(0, np.float32)])

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(reqs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=180)
    sched.close()
    for i, w in ((3, want_block), (5, want_stream)):
        g = got[i]
        assert g is not None and g.shape == w.shape, (i, None if g is None else g.shape, w.shape)
        assert float(np.sqrt(np.mean((g - w) ** 2))) <= 1e-6, i


def test_stream_route_replays_seeds_on_the_scheduler(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler

    sched = BatchScheduler(tts, max_batch=3, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=10))
    try:
        client = TestClient(create_app(tts, scheduler=sched))
        body = {"text": "replay me", "temperature": 0.8, "fast_temperature": 0.8}
        a = client.post("/v1/text-to-speech/3/stream", json={**body, "seed": 11})
        b = client.post("/v1/text-to-speech/3/stream", json={**body, "seed": 11})
        c = client.post("/v1/text-to-speech/3/stream", json={**body, "seed": 12})
        assert a.status_code == b.status_code == c.status_code == 200
        assert a.headers["X-Seed"] == "11" and len(a.content) > 0
        assert a.content == b.content and a.content != c.content
        d = client.post("/v1/text-to-speech/3/stream", json=body)
        seed = int(d.headers["X-Seed"])
        e = client.post("/v1/text-to-speech/3/stream", json={**body, "seed": seed})
        assert d.content == e.content
        g = client.post("/v1/text-to-speech/3/stream", json={"text": "replay me"})  # greedy server, no fields: no X-Seed
        assert g.status_code == 200 and "X-Seed" not in g.headers
    finally:
        sched.close()
