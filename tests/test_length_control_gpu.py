"""Per-request length control on the GPU (minimum length, end-of-speech bias, finish reason): the in-kernel patch of the slow pick
against the parent's path on host-patched rows (exact, every row), a ragged session whose boundary falls inside a multi-frame
graph, slot and batch invariance, a recycled slot, every entry point that picks, and the front ends with their finish reason."""
import numpy as np
import pytest
import torch

from filters_helpers import R, SHAPES, make_rows

pytestmark = pytest.mark.gpu

BIASES = [0.0, 3.5, -3.5, 1e4, -1e4]


def im_end_columns(V):
    """Column 0, the last column, four consecutive middle columns 4k .. 4k + 3 (one per float4 component) and, on the vector path
    (V % 4 == 0), a column of the second register group (>= 1024)."""
    k = (V // 2) // 4 * 4
    return [0, V - 1, k, k + 1, k + 2, k + 3] + ([1024 + 5 * 4 + 1] if V % 4 == 0 and V > 1024 + 5 * 4 + 1 else [])


def length_rows(fx, im_end):
    """Row r's (min_frames, eos_bias): min_frames off, at, above and below the row's frame counter; every bias; an off entry where
    both are off.  Every second row's im_end logit is moved to just under the row's maximum, so that a bias of 3.5 changes picks."""
    frames = fx["frames"]
    mf = [[0, frames[r], frames[r] + 1, max(frames[r] - 1, 0)][r % 4] for r in range(R)]
    bias = [BIASES[(r // 4 + r // 20) % 5] for r in range(R)]
    logits = fx["logits"].copy()
    for r in range(0, R, 2):
        rest = np.delete(logits[r], im_end)
        logits[r, im_end] = rest.max() - np.float32(1.0)
    return logits, mf, bias


@pytest.fixture(scope="module", params=SHAPES)
def shape_fx(request):
    from smoltts_amd import ops

    V = request.param
    fx = make_rows(V)
    table = ops.slot_sampling_table(fx["temps"], fx["fasts"], fx["min_ps"], fx["seeds"])
    filters = ops.slot_filter_table(fx["top_p"], fx["top_k"], fx["penalty"], fx["window"])
    hist = torch.from_numpy(fx["history"]).cuda()
    hlen = torch.tensor(fx["hist_len"], dtype=torch.int32, device="cuda")
    frames = torch.tensor(fx["frames"], dtype=torch.int32, device="cuda")
    return V, fx, table, filters, hist, hlen, frames


def test_in_kernel_patch_equals_the_parent_on_host_patched_rows(shape_fx):
    """Device: the new entry with the table (min_frames, eos_bias).  Reference: the existing sample_rows / sample_rows_filtered on
    sampling.length_patch of the same row.  Equal for every row (greedy and sampled, filters on and off), no tolerance; greedy
    rows are also np.argmax of the patched row."""
    from smoltts_amd import ops
    from smoltts_amd.sampling import length_patch

    V, fx, table, filters, hist, hlen, frames = shape_fx
    assert any(t <= 0 for t in fx["temps"]) and any(t > 0 for t in fx["temps"])
    changed = 0
    for im_end in im_end_columns(V):
        logits, mf, bias = length_rows(fx, im_end)
        assert {0} < set(mf) and set(bias) == set(BIASES) and any(m == 0 and b == 0 for m, b in zip(mf, bias))
        patched = np.stack([length_patch(logits[r], im_end, fx["frames"][r], mf[r], bias[r]) for r in range(R)])
        dev_rows, ref_rows = torch.from_numpy(logits).cuda(), torch.from_numpy(patched).cuda()
        length = ops.slot_length_table(mf, bias)
        got_f = ops.sample_rows_length(dev_rows, table, length, im_end, frames, step=0, filters=filters, history=hist, history_len=hlen)
        want_f = ops.sample_rows_filtered(ref_rows, table, filters, hist, hlen, frames, step=0)
        got_p = ops.sample_rows_length(dev_rows, table, length, im_end, frames, step=0)
        want_p = ops.sample_rows(ref_rows, table, frames, step=0)
        bad = [(r, int(got_f[r]), int(want_f[r]), int(got_p[r]), int(want_p[r])) for r in range(R) if got_f[r] != want_f[r] or got_p[r] != want_p[r]]
        assert not bad, (V, im_end, bad)
        for r in range(R):
            if fx["temps"][r] <= 0:
                assert int(got_p[r]) == int(got_f[r]) == int(np.argmax(patched[r])), (V, im_end, r)
            if fx["frames"][r] < mf[r]:
                assert int(got_p[r]) != im_end and int(got_f[r]) != im_end, (V, im_end, r)
        changed += int((got_p != ops.sample_rows(dev_rows, table, frames, step=0)).sum())
        # step >= 1 (a depth code) ignores the table entirely
        assert torch.equal(ops.sample_rows_length(dev_rows, table, length, im_end, frames, step=3, filters=filters, history=hist, history_len=hlen),
                           ops.sample_rows_filtered(dev_rows, table, filters, hist, hlen, frames, step=3))
        assert torch.equal(ops.sample_rows_length(dev_rows, table, length, im_end, frames, step=3), ops.sample_rows(dev_rows, table, frames, step=3))
        # an all-off table is the parent's pick
        off = ops.slot_length_table([0] * R, [0.0] * R)
        assert torch.equal(ops.sample_rows_length(dev_rows, table, off, im_end, frames, step=0), ops.sample_rows(dev_rows, table, frames, step=0))
    assert changed > 20  # the entries do change picks here: the equalities above are not vacuous


def test_patch_reaches_the_columns_behind_65536():
    """A row wider than 65536 columns (the scalar path's tail loop of a filtered row), im_end in the tail."""
    from smoltts_amd import ops
    from smoltts_amd.sampling import length_patch

    V, n, im_end = 65536 + 777, 8, 65536 + 401
    rng = np.random.default_rng(7)
    logits = (rng.standard_normal((n, V)) * 3.0).astype(np.float32)
    logits[:, im_end] = logits.max(axis=1) + np.float32(0.5)  # im_end wins every unpatched greedy pick
    temps = [0.0, 0.8] * 4
    mf, bias = [0, 0, 9, 9, 0, 0, 3, 3], [0.0, 0.0, 0.0, 0.0, -1e4, 3.5, 1e4, 1e4]
    frames_h = [5] * n
    table = ops.slot_sampling_table(temps, temps, [0.0] * n, list(range(11, 11 + n)))
    filters = ops.slot_filter_table([0.9] * n, [50] * n, [1.5] * n, [8] * n)
    hist = torch.from_numpy(np.tile(np.arange(64, dtype=np.int32) * 1031 % V, (n, 1))).cuda()
    hist[:, 0] = im_end
    hlen = torch.full((n,), 8, dtype=torch.int32, device="cuda")
    frames = torch.tensor(frames_h, dtype=torch.int32, device="cuda")
    patched = np.stack([length_patch(logits[r], im_end, frames_h[r], mf[r], bias[r]) for r in range(n)])
    dev_rows, ref_rows = torch.from_numpy(logits).cuda(), torch.from_numpy(patched).cuda()
    length = ops.slot_length_table(mf, bias)
    got_f = ops.sample_rows_length(dev_rows, table, length, im_end, frames, step=0, filters=filters, history=hist, history_len=hlen)
    assert torch.equal(got_f, ops.sample_rows_filtered(ref_rows, table, filters, hist, hlen, frames, step=0))
    got_p = ops.sample_rows_length(dev_rows, table, length, im_end, frames, step=0)
    assert torch.equal(got_p, ops.sample_rows(ref_rows, table, frames, step=0))
    assert int(got_p[0]) == im_end and int(got_p[2]) != im_end and int(got_p[4]) != im_end and int(got_p[6]) == im_end
    for r in range(0, n, 2):
        assert int(got_p[r]) == int(np.argmax(patched[r]))


# ---------------------------------------------------------------------------------------------------- session level
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


@pytest.fixture(scope="module")
def eng_pe():
    return _engine()


CAP = 12
TEXTS = (("one", "heart"), ("a second, longer prompt than the first", "sky"), ("3", "nova"), ("the fourth one", "bella"), ("five five five", "liam"))


def _run(eng, prompts, entries, length=None, frames=CAP, per_graph=4, slots=None, commit_picks=True):
    """(codes [B, frames, H], n_frames [B]) of the prompts in slot mode with stop_on_eos; entries: (temp, fast, min_p, seed) per
    prompt; length: (min_frames, eos_bias) or None per prompt (all None: set_slot_length is never called)."""
    from smoltts_amd.engine import LMSession

    B = len(prompts) if slots is None else max(slots) + 1
    slots = list(range(len(prompts))) if slots is None else list(slots)
    s = LMSession(eng, B, max_seq=256, max_rows=256 * B, max_frames=frames)
    if not commit_picks:
        s.use_commit_picks(False)
    s.set_frames_per_graph(per_graph)
    s.set_slot_sampling(slots, *[list(x) for x in zip(*entries)])
    if length is not None:
        on = [i for i in range(len(prompts)) if length[i] is not None]
        s.set_slot_length([slots[i] for i in on], [length[i][0] for i in on], [length[i][1] for i in on])
    s.prefill(prompts, slots=slots, stop_on_eos=True)
    s.decode(frames - 1)
    codes, n, _, _ = s.fetch()
    s.close()
    return codes[slots, :frames].copy(), n[slots].copy()


@pytest.fixture(scope="module")
def prompts5(eng_pe):
    _, pe = eng_pe
    return [pe.build_prompt(t, v) for t, v in TEXTS]


@pytest.fixture(scope="module")
def plain_runs(eng_pe, prompts5):
    """The five prompts in sessions that never call set_slot_length: greedy, and with the slow token of A, D, E sampled."""
    eng, _ = eng_pe
    greedy = [(0.0, 0.0, 0.0, 0)] * 5
    return {"greedy": _run(eng, prompts5, greedy), "sampled": _run(eng, prompts5, SAMPLED)}


SAMPLED = [(0.7, 0.0, 0.0, 101), (0.0, 0.0, 0.0, 0), (0.0, 0.0, 0.0, 0), (0.7, 0.0, 0.0, 104), (0.7, 0.0, 0.0, 105)]
# A: the boundary (frame 5) falls inside the second 4-frame replay (frames 5 .. 8); B never stops; C: the minimum lies above the cap
# (with the bias on, so that only the minimum keeps it running); D and E: off entries
LENGTH = [(5, 1e4), (0, -1e4), (CAP + 10, 1e4), None, None]


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_session_ragged(eng_pe, prompts5, plain_runs, mode):
    eng, _ = eng_pe
    im_end = eng.token_config.im_end_id
    entries = [(0.0, 0.0, 0.0, 0)] * 5 if mode == "greedy" else SAMPLED
    assert len({p.shape[1] for p in prompts5}) > 2  # ragged
    codes, n = _run(eng, prompts5, entries, LENGTH)
    base_codes, base_n = plain_runs[mode]
    assert (base_n == CAP).all() and not (base_codes[:, :, 0] == im_end).any()  # unforced, nothing stops here
    assert n[0] == 6 and codes[0, 5, 0] == im_end and not (codes[0, :5, 0] == im_end).any()
    assert n[1] == CAP and not (codes[1, :, 0] == im_end).any()
    assert n[2] == CAP and not (codes[2, :, 0] == im_end).any()
    for b in (3, 4):  # off entries beside entries that are on: the whole grid as without the table
        assert n[b] == base_n[b] and np.array_equal(codes[b], base_codes[b]), b
    assert np.array_equal(codes[0, :5], base_codes[0, :5])  # A's frames before its forced end are its own


def test_single_frame_graphs_and_the_pick_as_its_own_launch_agree(eng_pe, prompts5):
    eng, _ = eng_pe
    want = _run(eng, prompts5, SAMPLED, LENGTH)
    for kw in (dict(per_graph=1), dict(commit_picks=False)):
        got = _run(eng, prompts5, SAMPLED, LENGTH, **kw)
        assert np.array_equal(got[1], want[1]) and all(np.array_equal(got[0][b, :want[1][b]], want[0][b, :want[1][b]]) for b in range(5)), kw


def test_request_does_not_depend_on_slot_or_companions(eng_pe, prompts5):
    eng, pe = eng_pe
    p = pe.build_prompt("the same length-controlled request", "heart")
    target, tl = (0.7, 0.0, 0.0, 4242), (7, 2.0)
    alone, n_alone = _run(eng, [p], [target], [tl])
    entries = [(0.0, 0.0, 0.0, 0), (0.7, 0.7, 0.0, 1), (1.1, 0.0, 0.0, 2), target, (0.0, 0.6, 0.0, 4)]
    length = [(3, 1e4), None, (0, -5.0), tl, (2, 0.0)]
    among, n_among = _run(eng, prompts5[:3] + [p] + prompts5[4:], entries, length)
    assert n_among[3] == n_alone[0] and np.array_equal(among[3, :n_alone[0]], alone[0, :n_alone[0]])


def test_recycled_slot_does_not_inherit_the_entry(eng_pe, prompts5):
    """A tenant with an entry on, then one without in the same slot (entries written as every front end writes them)."""
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.engine import LMSession
    from smoltts_amd.generate import _apply_slot_sampling

    eng, _ = eng_pe
    im_end = eng.token_config.im_end_id
    gs = GenerationSettings.greedy()
    first = RequestSampling(min_frames=2, eos_bias=100.0).resolve(gs)
    second = RequestSampling(temperature=0.7, seed=9).resolve(gs)
    s = LMSession(eng, 2, max_seq=256, max_rows=512, max_frames=CAP)
    s.set_frames_per_graph(4)
    _apply_slot_sampling(s, [0, 1], [first, RequestSampling().resolve(gs)])
    s.prefill(prompts5[:2], stop_on_eos=True)
    s.decode(CAP - 1)
    codes, n, _, _ = s.fetch()
    assert n[0] == 3 and codes[0, 2, 0] == im_end and 0 in s.length_slots
    _apply_slot_sampling(s, [0], [second])
    assert 0 not in s.length_slots
    s.prefill([prompts5[2]], slots=[0], stop_on_eos=True)
    s.decode(CAP - 1)
    codes, n, _, _ = s.fetch()
    got = codes[0, :n[0]].copy()
    s.close()
    want, wn = _run(eng, [prompts5[2]], [(0.7, 0.0, 0.0, 9)])
    assert n[0] == wn[0] == CAP and np.array_equal(got, want[0])


@pytest.mark.parametrize("entry", ["prefill", "chunked", "deferred", "side"])
@pytest.mark.parametrize("commit_picks", [True, False])
def test_every_entry_point_that_picks(eng_pe, entry, commit_picks):
    """min_frames = 1, eos_bias = +1e4: frame 0's slow id is not im_end, frame 1's is -- after the plain prefill (whose tail picks
    frame 0), the chunked one, the deferred one and the side prefill (whose frame 0 comes out of the first decode frame)."""
    from smoltts_amd.engine import LMSession

    eng, pe = eng_pe
    im_end = eng.token_config.im_end_id
    p = pe.build_prompt("an utterance long enough to be prefilled in several chunks of four columns", "heart")
    s = LMSession(eng, 2, max_seq=256, max_rows=512, max_frames=CAP)
    if not commit_picks:
        s.use_commit_picks(False)
    s.set_frames_per_graph(4)
    s.set_slot_sampling([0, 1], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0, 0])
    s.set_slot_length([1], [1], [1e4])
    if entry == "prefill":
        s.prefill([p], slots=[1], stop_on_eos=True)
    elif entry == "chunked":
        assert p.shape[1] > 8
        s.prefill_chunked([p], slots=[1], stop_on_eos=True, chunk=4)
    elif entry == "deferred":
        s.prefill([p], slots=[1], stop_on_eos=True, defer_frame0=True)
    else:
        h = s.side_park([p], [1])
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            s.side_run(h)
        s.side_start(h, stop_on_eos=True)
    s.decode(5)
    codes, n, done, _ = s.fetch()
    s.close()
    assert n[1] == 2 and done[1] == 1, (entry, n, done)
    assert codes[1, 0, 0] != im_end and codes[1, 1, 0] == im_end


# ---------------------------------------------------------------------------------------------------- front ends
@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


def test_facade_and_scheduler_agree_with_their_finish_reason(tts):
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.server.scheduler import BatchScheduler

    gs = GenerationSettings.greedy(max_new_tokens=12)
    stop = RequestSampling(temperature=0.7, seed=77, min_frames=4, eos_bias=100.0)
    run = RequestSampling(eos_bias=-100.0)
    want_stop = tts("the length-controlled request", "heart", generation_settings=gs, sampling=stop)
    assert tts.last_finish_reason == "stop"
    assert tts.last_stats["frames"] == 5  # frames 0 .. 3, then the forced <|im_end|>
    codes = tts.generate_codes(["the length-controlled request"], ["heart"], gs, sampling=stop)[0]
    assert tts.last_stats["frames"] == 5 and codes.shape[1] <= 4 and want_stop.size == 1920 * codes.shape[1]
    want_run = tts("the length-controlled request", "heart", generation_settings=gs, sampling=run)
    assert tts.last_finish_reason == "length" and tts.last_stats["frames"] == 13
    sched = BatchScheduler(tts, max_batch=3, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=16))
    try:
        # more requests than slots: a slot is handed from a tenant with the entry to one without
        reqs = [sched.submit("the length-controlled request", "heart", max_new_tokens=12, sampling=smp) for smp in (stop, run, None, stop, run)]
        got = [np.concatenate(list(sched.iter_chunks(r)) or [np.zeros(0, np.float32)]) for r in reqs]
    finally:
        sched.close()
    assert [r.finish_reason for r in reqs] == ["stop", "length", "length", "stop", "length"]
    assert [r.frame_counts for r in reqs] == [[5], [13], [13], [5], [13]]  # the façade's frame counts, exactly
    for g, w in ((got[0], want_stop), (got[3], want_stop), (got[1], want_run), (got[4], want_run)):
        assert g.shape == w.shape and (g.size == 0 or float(np.sqrt(np.mean((g - w) ** 2))) <= 1e-6)


def test_segmented_request_sets_the_entry_for_every_segment(tts):
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.server.scheduler import BatchScheduler

    text = "The first sentence of a long text. The second sentence follows it. And a third one ends it."
    gs = GenerationSettings.greedy(max_new_tokens=12)
    smp = RequestSampling(min_frames=3, eos_bias=100.0)
    seg = {"max_bytes": 40, "pause_s": 0.1}
    tts(text, "heart", generation_settings=gs, sampling=smp, segment=seg)
    assert len(tts.last_segments) >= 3 and tts.last_finish_reason == "stop"
    im_end = tts.token_config.im_end_id
    from smoltts_amd.generate import BatchGenerator, resolve_sampling

    for k, s in enumerate(tts.last_segments):  # each segment again, as the call ran it: min_frames frames, then <|im_end|>
        one = resolve_sampling(RequestSampling(min_frames=3, eos_bias=100.0, seed=s["seed"]), gs, 1)
        gen = BatchGenerator(tts.lm, [s["prompt"]], gs, frames_per_sync=16, sampling=one)
        slow = [row[0].semantic_code for row in gen if row[0] is not None]
        gen.close()
        print(f"segment {k}: slow ids {slow}, {s['codes'].shape[1]} audio frames")
        assert len(slow) == 3 + 1 and slow[3] == im_end and im_end not in slow[:3], (k, slow)
        tc = tts.token_config
        assert s["codes"].shape[1] == sum(tc.semantic_start_id <= t <= tc.semantic_end_id for t in slow[:3])  # the call's own frames
    # without the entry on a later segment, that segment would end at its frame 0: the forced end needs every segment's own entry
    tts(text, "heart", generation_settings=gs, sampling=RequestSampling(eos_bias=-100.0), segment=seg)
    assert tts.last_finish_reason == "length"
    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=12))
    try:
        r = sched.submit(text, "heart", sampling=smp, segment=seg)
        list(sched.iter_chunks(r))
        assert r.finish_reason == "stop" and len(r.reasons) == len(tts.last_segments) and set(r.reasons) == {"stop"}
        q = sched.submit(text, "heart", sampling=RequestSampling(min_frames=3, eos_bias=-100.0), segment=seg, max_new_tokens=6)
        list(sched.iter_chunks(q))
        assert q.finish_reason == "length" and set(q.reasons) == {"length"}
    finally:
        sched.close()


# ---------------------------------------------------------------------------------------------------- bounds from the text length
BOUND_TEXT = "Short one. " + "A much longer second sentence that goes on for quite a while before it ends. " + "End."
BOUND_SEG = {"max_bytes": 80, "pause_s": 0.1}
MIN_FPB, MAX_FPB, BOUND_CAP = 0.1, 0.2, 12
PLAIN_TEXT = "A plain utterance of some forty-odd bytes."


def _bounds(texts, cap0=BOUND_CAP, own=0):
    """[(min_frames, cap)] of the texts under the two ratios, by the issue's arithmetic."""
    import math

    out = []
    for t in texts:
        n = len(t.encode("utf-8"))
        cap = max(1, min(cap0, math.ceil(n * MAX_FPB)))
        out.append((min(max(own, math.floor(n * MIN_FPB)), cap - 1), cap))
    return out


@pytest.fixture()
def length_calls(monkeypatch):
    """Every (min_frames list, eos_bias list) a session's set_slot_length is given."""
    from smoltts_amd.lm import LMSession

    calls, real = [], LMSession.set_slot_length

    def spy(self, slots, min_frames, eos_bias):
        calls.append((list(min_frames), list(eos_bias)))
        return real(self, slots, min_frames, eos_bias)

    monkeypatch.setattr(LMSession, "set_slot_length", spy)
    return calls


@pytest.fixture()
def bounded_tts(tts):
    tts.min_frames_per_byte, tts.max_frames_per_byte = MIN_FPB, MAX_FPB
    yield tts
    tts.min_frames_per_byte = tts.max_frames_per_byte = None


def test_facade_applies_the_ratios_to_plain_utterances(bounded_tts, length_calls):
    from smoltts_amd.config import GenerationSettings, RequestSampling

    tts = bounded_tts
    gs = GenerationSettings.greedy(max_new_tokens=BOUND_CAP)
    (lo, cap), = _bounds([PLAIN_TEXT])
    assert 1 < lo < cap - 1 < BOUND_CAP - 1  # both ratios bite
    early, late = RequestSampling(eos_bias=100.0), RequestSampling(eos_bias=-100.0)
    tts(PLAIN_TEXT, "heart", generation_settings=gs, sampling=early)
    assert tts.last_stats["frames"] == lo + 1 and tts.last_finish_reason == "stop"  # <|im_end|> at the first frame the minimum allows
    tts(PLAIN_TEXT, "heart", generation_settings=gs, sampling=late)
    assert tts.last_stats["frames"] == cap + 1 and tts.last_finish_reason == "length"
    assert len(list(tts.stream(PLAIN_TEXT, "heart", generation_settings=gs, sampling=early))) == lo + 1 and tts.last_finish_reason == "stop"
    assert len(list(tts.stream(PLAIN_TEXT, "heart", generation_settings=gs, sampling=late))) == cap + 1 and tts.last_finish_reason == "length"
    # a call without sampling= (session-wide mode until now): the minimum still reaches the device, the cap still holds
    for run in (lambda: tts(PLAIN_TEXT, "heart", generation_settings=gs), lambda: list(tts.stream(PLAIN_TEXT, "heart", generation_settings=gs))):
        length_calls.clear()
        out = run()
        assert length_calls == [([lo], [0.0])], length_calls
        assert (len(out) if isinstance(out, list) else tts.last_stats["frames"]) == cap + 1
    # the request's own minimum where it is the larger
    tts(PLAIN_TEXT, "heart", generation_settings=gs, sampling=RequestSampling(eos_bias=100.0, min_frames=lo + 2))
    assert tts.last_stats["frames"] == lo + 3


def test_facade_applies_the_ratios_to_every_segment(bounded_tts, length_calls):
    from smoltts_amd.config import GenerationSettings, RequestSampling

    tts = bounded_tts
    gs = GenerationSettings.greedy(max_new_tokens=BOUND_CAP)
    early, late = RequestSampling(eos_bias=100.0), RequestSampling(eos_bias=-100.0)
    tts(BOUND_TEXT, "heart", generation_settings=gs, sampling=early, segment=BOUND_SEG)
    want = _bounds([s["text"] for s in tts.last_segments])
    assert len(want) == 3 and len(set(want)) == 3 and want[1][0] > want[0][0] > 0 and want[1][1] > want[0][1] > want[2][1]  # different bounds
    assert [s["frames"] for s in tts.last_segments] == [lo + 1 for lo, _ in want]
    tts(BOUND_TEXT, "heart", generation_settings=gs, sampling=late, segment=BOUND_SEG)
    assert [s["frames"] for s in tts.last_segments] == [cap + 1 for _, cap in want] and tts.last_finish_reason == "length"
    list(tts.stream(BOUND_TEXT, "heart", generation_settings=gs, sampling=early, segment=BOUND_SEG))
    assert [s["frames"] for s in tts.last_segments] == [lo + 1 for lo, _ in want] and tts.last_finish_reason == "stop"
    list(tts.stream(BOUND_TEXT, "heart", generation_settings=gs, sampling=late, segment=BOUND_SEG))
    assert [s["frames"] for s in tts.last_segments] == [cap + 1 for _, cap in want]
    # text that arrives in pieces: the same segments, the same bounds
    list(tts.stream(iter([BOUND_TEXT[:30], BOUND_TEXT[30:]]), "heart", generation_settings=gs, sampling=early, segment=BOUND_SEG))
    assert [s["frames"] for s in tts.last_segments] == [lo + 1 for lo, _ in want]
    # without sampling=: every segment's own minimum is written (a minimum of 0 writes nothing), every segment's cap holds
    for run in (lambda: tts(BOUND_TEXT, "heart", generation_settings=gs, segment=BOUND_SEG),
                lambda: list(tts.stream(BOUND_TEXT, "heart", generation_settings=gs, segment=BOUND_SEG))):
        length_calls.clear()
        run()
        assert length_calls == [([lo], [0.0]) for lo, _ in want if lo > 0], length_calls
        assert [s["frames"] for s in tts.last_segments] == [cap + 1 for _, cap in want]


def test_scheduler_applies_the_ratios_to_every_utterance_and_segment(tts):
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.longform import SegmentPlan, segment_options
    from smoltts_amd.server.scheduler import BatchScheduler

    texts = [s.text for s in SegmentPlan.create(BOUND_TEXT, segment_options(BOUND_SEG)).segs]
    want, (plain,) = _bounds(texts), _bounds([PLAIN_TEXT])
    early, late = RequestSampling(eos_bias=100.0), RequestSampling(eos_bias=-100.0)
    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=BOUND_CAP),
                           min_frames_per_byte=MIN_FPB, max_frames_per_byte=MAX_FPB)
    try:
        jobs = [("seg early", dict(text=BOUND_TEXT, sampling=early, segment=BOUND_SEG), [lo + 1 for lo, _ in want]),
                ("seg late", dict(text=BOUND_TEXT, sampling=late, segment=BOUND_SEG), [cap + 1 for _, cap in want]),
                ("seg early stream", dict(text=BOUND_TEXT, sampling=early, segment=BOUND_SEG, stream=True), [lo + 1 for lo, _ in want]),
                ("seg late stream", dict(text=BOUND_TEXT, sampling=late, segment=BOUND_SEG, stream=True), [cap + 1 for _, cap in want]),
                # the request's own cap of 5 comes back for the second segment after the first one's cap of 2
                ("seg late, own cap", dict(text=BOUND_TEXT, sampling=late, segment=BOUND_SEG, max_new_tokens=5), [c + 1 for _, c in _bounds(texts, cap0=5)]),
                ("seg early, own minimum", dict(text=BOUND_TEXT, sampling=RequestSampling(eos_bias=100.0, min_frames=9), segment=BOUND_SEG),
                 [lo + 1 for lo, _ in _bounds(texts, own=9)]),
                ("plain early", dict(text=PLAIN_TEXT, sampling=early), [plain[0] + 1]), ("plain late", dict(text=PLAIN_TEXT, sampling=late), [plain[1] + 1]),
                ("plain default", dict(text=PLAIN_TEXT), [plain[1] + 1]), ("plain late stream", dict(text=PLAIN_TEXT, sampling=late, stream=True), [plain[1] + 1])]
        reqs = [sched.submit(kw.pop("text"), "heart", **kw) for _, kw, _ in jobs]
        for r in reqs:
            list(sched.iter_chunks(r))
        inc = sched.submit_incremental("heart", sampling=early, segment=BOUND_SEG)
        inc.feed(BOUND_TEXT[:30])
        inc.feed(BOUND_TEXT[30:])
        inc.close()
        list(inc)
    finally:
        sched.close()
    assert _bounds(texts, cap0=5) != want and _bounds(texts, own=9) != want
    for (name, _, frames), r in zip(jobs, reqs):
        assert r.frame_counts == frames, (name, r.frame_counts, frames)
        assert r.finish_reason == ("stop" if "early" in name else "length"), name
    assert inc.frame_counts == [lo + 1 for lo, _ in want] and inc.finish_reason == "stop"


def test_blocking_routes_answer_the_finish_reason(tts):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler

    sched = BatchScheduler(tts, max_batch=3, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=10))
    try:
        client = TestClient(create_app(tts, scheduler=sched))
        a = client.post("/v1/audio/speech", json={"input": "to the cap", "eos_bias": -100})
        b = client.post("/v1/audio/speech", json={"input": "to the cap", "eos_bias": 100, "min_duration_s": 0.2})
        assert a.status_code == b.status_code == 200
        assert a.headers["X-Finish-Reason"] == "length" and b.headers["X-Finish-Reason"] == "stop"
        assert len(b.content) < len(a.content)
        c = client.post("/v1/text-to-speech/3", json={"text": "to the cap", "eos_bias": -100})
        d = client.post("/v1/text-to-speech/3", json={"text": "to the cap", "eos_bias": 100, "min_frames": 3})
        assert c.headers["X-Finish-Reason"] == "length" and d.headers["X-Finish-Reason"] == "stop"
        assert client.post("/v1/audio/speech", json={"input": "x", "min_frames": 3, "min_duration_s": 0.2}).status_code in (400, 422)
        assert client.post("/v1/audio/speech", json={"input": "x", "eos_bias": 101}).status_code in (400, 422)
    finally:
        sched.close()
    model_only = TestClient(create_app(tts))
    gs_cap = tts._settings(None).max_new_tokens
    e = model_only.post("/v1/audio/speech", json={"input": "stop soon", "eos_bias": 100, "min_frames": 2})
    assert e.status_code == 200 and e.headers["X-Finish-Reason"] == "stop" and gs_cap >= 2
