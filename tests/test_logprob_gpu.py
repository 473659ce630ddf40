"""The score of the slow pick on the GPU: the log-probability of every picked id against the numpy model
(sampling.pick_logprob, |error| <= LOGPROB_MARGIN) with ids that equal the unscored picks bit for bit, at the kernel entry over
every path of the row pick, and in a ragged session (frame by frame, four frames per graph, the pick as its own launch, a slot
run to the cap, a recycled slot)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the scalar path; the vector path with 1, 2 and 8 full register groups (the first two with one float4 more); just past the
# vector limit; the tail loop behind 65,536
WIDTHS = (5, 1028, 2052, 8192, 8196, 65836)
SCALES = (0.01, 1.0, 30.0, 1e4)
FILTERS = ("off", "top_k", "top_p", "penalty")
LENGTHS = ("off", "block", "plus", "minus")
TEMP = 0.9
ROWS = list(itertools.product((False, True), FILTERS, LENGTHS, SCALES))  # (sampled, filter, length entry, scale): 128 rows
WORST = {}  # width -> the largest |device - model| seen (printed; DESIGN.md 20 quotes it)


def _im_ends(V):
    return [0, V - 1] + ([65536 + 123] if V > 65536 + 123 else [])


def _fixture(V):
    rng = np.random.default_rng(4000 + V)
    R = len(ROWS)
    logits = np.stack([(rng.standard_normal(V) * s).astype(np.float32) for _, _, _, s in ROWS])
    frames = [r % 7 + 1 for r in range(R)]
    hist = np.zeros((R, 64), np.int32)
    for r in range(R):
        if ROWS[r][1] == "penalty":  # the largest column stays the largest after its division by 1.5: the pick of a peaked row
            order = np.argsort(-logits[r])
            logits[r, order[0]] = np.float32(2.0) * np.abs(logits[r, order[1]])
        hist[r, :8] = np.resize(np.argsort(-logits[r])[:8], 8)  # the row's largest columns: a sampled pick is usually one of them
    return logits, frames, hist


@pytest.fixture(scope="module", params=WIDTHS)
def width_fx(request):
    V = request.param
    return (V,) + _fixture(V)


def _padded(rows, ld_vec):
    """The rows on the device with a row stride that is (ld_vec) or is not a multiple of 4: the kernel's two load paths."""
    R, V = rows.shape
    ld = (V + 3) // 4 * 4 if ld_vec else (V + 3) // 4 * 4 + 1
    buf = torch.zeros((R, ld), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(rows).cuda()
    return buf[:, :V]


@pytest.mark.parametrize("ld_vec", [True, False])
def test_kernel_entry_matches_the_model_and_leaves_the_ids_alone(width_fx, ld_vec):
    from smoltts_amd import ops
    from smoltts_amd.sampling import LOGPROB_MARGIN, length_patch, penalised_row, pick_logprob

    V, logits, frames_h, hist_h = width_fx
    R = len(ROWS)
    temps = [TEMP if smp else 0.0 for smp, _, _, _ in ROWS]
    table = ops.slot_sampling_table(temps, temps, [0.0] * R, [977 * r + 13 for r in range(R)])
    filters = ops.slot_filter_table([0.5 if f == "top_p" else 1.0 for _, f, _, _ in ROWS], [3 if f == "top_k" else 0 for _, f, _, _ in ROWS],
                                    [1.5 if f == "penalty" else 1.0 for _, f, _, _ in ROWS], [64] * R)
    hist = torch.from_numpy(hist_h).cuda()
    hlen = torch.full((R,), 8, dtype=torch.int32, device="cuda")
    frames = torch.tensor(frames_h, dtype=torch.int32, device="cuda")
    mf = [frames_h[r] + 1 if le == "block" else 0 for r, (_, _, le, _) in enumerate(ROWS)]
    bias = [{"plus": 3.5, "minus": -3.5}.get(le, 0.0) for _, _, le, _ in ROWS]
    length = ops.slot_length_table(mf, bias)
    dev = _padded(logits, ld_vec)
    assert (dev.stride(0) % 4 == 0) == ld_vec
    worst, in_hist, not_max = 0.0, 0, 0
    for im_end, with_filters, with_length in itertools.product(_im_ends(V), (True, False), (True, False)):
        if not with_length and im_end != 0:
            continue  # (without the length table im_end means nothing)
        fkw = dict(filters=filters, history=hist, history_len=hlen) if with_filters else {}
        ids, lp = ops.sample_rows_scored(dev, table, length if with_length else None, im_end, frames, step=0, **fkw)
        if with_length:
            want_ids = ops.sample_rows_length(dev, table, length, im_end, frames, step=0, **fkw)
        elif with_filters:
            want_ids = ops.sample_rows_filtered(dev, table, filters, hist, hlen, frames, step=0)
        else:
            want_ids = ops.sample_rows(dev, table, frames, step=0)
        assert torch.equal(ids, want_ids), (V, im_end, with_filters, with_length)
        ids_h, lp_h = ids.cpu().numpy(), lp.cpu().numpy()
        for r, (smp, f, le, scale) in enumerate(ROWS):
            row = length_patch(logits[r], im_end, frames_h[r], mf[r], bias[r]) if with_length else logits[r]
            if smp and with_filters and f == "penalty":
                row = penalised_row(row, 1.5, hist_h[r, :8])
                in_hist += int(ids_h[r] in hist_h[r, :8])
            if np.isnan(row).any():
                continue
            not_max += int(ids_h[r] != int(np.argmax(row)))
            want = pick_logprob(row, int(ids_h[r]))
            err = abs(float(lp_h[r]) - want)
            worst = max(worst, err)
            assert np.isfinite(lp_h[r]) and err <= LOGPROB_MARGIN, (V, ld_vec, im_end, with_filters, with_length, r, ROWS[r], float(lp_h[r]), want)
            if with_length and le == "block":
                assert int(ids_h[r]) != im_end
    assert in_hist > 0 and not_max > 0  # the penalty did reach picked ids, and sampled rows did pick below the maximum
    WORST[(V, ld_vec)] = worst
    print(f"logprob kernel entry: {V} columns, ld_vec={ld_vec}: largest |device - model| = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------- session level
CAP = 12
TEXTS = (("one", "heart"), ("a second, longer prompt than the first", "sky"), ("3", "nova"), ("the fourth one", "bella"), ("five five five", "liam"))
GREEDY = [(0.0, 0.0, 0.0, 0)] * 5
# slot 0 scored and sampled, slot 1 sampled with filters, slot 2 scored and greedy, the rest greedy
SAMPLED = [(0.9, 0.0, 0.0, 101), (0.8, 0.0, 0.0, 102), (0.0, 0.0, 0.0, 0), (0.0, 0.0, 0.0, 0), (0.0, 0.0, 0.0, 0)]
FILTER1 = (0.9, 50, 1.5, 8)  # slot 1's (top_p, top_k, penalty, window)
# slot 0 ends at frame 5: inside the second four-frame replay (frame 0 comes out of the prefill, then frames 1 .. 4, 5 .. 8);
# slot 3's im_end logit carries a bias without ending it
LENGTH = {0: (5, 1e4), 3: (0, -2.0)}
SCORED = (0, 2)
SENTINEL = -777.0


@pytest.fixture(scope="module")
def eng_pe():
    from smoltts_amd.config import TokenConfig
    from smoltts_amd.engine import LMEngine
    from smoltts_amd.prompt import PromptEncoder
    from smoltts_amd.synthetic import named_config, synthetic_lm_state
    from smoltts_amd.tokenizer import load_tokenizer

    cfg = named_config("tiny")
    tok = load_tokenizer()
    tc = TokenConfig.from_tokenizer(tok, cfg)
    pe = PromptEncoder(tok, tc.semantic_start_id, cfg.num_codebooks, cfg.duplicate_code_0)
    return LMEngine(cfg, synthetic_lm_state(cfg, seed=21), tc), pe


@pytest.fixture(scope="module")
def prompts5(eng_pe):
    _, pe = eng_pe
    return [pe.build_prompt(t, v) for t, v in TEXTS]


def _session(eng, entries, score, per_graph=4, commit_picks=True):
    from smoltts_amd.engine import LMSession

    s = LMSession(eng, 5, max_seq=256, max_rows=256 * 5, max_frames=CAP)
    if not commit_picks:
        s.use_commit_picks(False)
    s.set_frames_per_graph(per_graph)
    s.set_slot_sampling(list(range(5)), *[list(x) for x in zip(*entries)])
    if entries is SAMPLED:
        s.set_slot_filters([1], [FILTER1[0]], [FILTER1[1]], [FILTER1[2]], [FILTER1[3]])
    s.set_slot_length(list(LENGTH), [LENGTH[b][0] for b in LENGTH], [LENGTH[b][1] for b in LENGTH])
    if score:
        s.set_slot_score(list(SCORED), [True] * len(SCORED))
    s.logprobs.fill_(SENTINEL)
    return s


def _run(eng, prompts, entries, score, **kw):
    """(codes [5, CAP, H], n_frames [5], logprobs [5, CAP]) of one whole run."""
    s = _session(eng, entries, score, **kw)
    s.prefill(prompts, stop_on_eos=True)
    s.decode(CAP - 1)
    s.decode(4)  # every slot is through: these frames must write nothing
    codes, n, _, _ = s.fetch()
    lp = s.fetch_logprobs()
    s.close()
    return codes.copy(), n.copy(), lp.copy()


@pytest.fixture(scope="module", params=["greedy", "sampled"])
def stepped(request, eng_pe, prompts5):
    """(a): one frame per call, each frame's rows of slow logits kept -> (entries, codes, n, logprobs, rows[f][b])."""
    eng, _ = eng_pe
    entries = GREEDY if request.param == "greedy" else SAMPLED
    s = _session(eng, entries, True, per_graph=1)
    rows = []
    s.prefill(prompts5, stop_on_eos=True)
    for f in range(CAP):
        torch.cuda.current_stream().synchronize()
        rows.append(s.slow_logits.cpu().numpy().copy())
        if f + 1 < CAP:
            s.decode(1)
    codes, n, _, _ = s.fetch()
    lp = s.fetch_logprobs()
    s.close()
    return entries, codes.copy(), n.copy(), lp.copy(), rows


def test_session_scores_match_the_model_frame_by_frame(eng_pe, stepped):
    """(a) Every live row of the scored form, frame 0 out of the prefill tail included: the asked slots and the others."""
    from smoltts_amd.sampling import LOGPROB_MARGIN, length_patch, penalised_row, pick_logprob

    eng, _ = eng_pe
    im_end = eng.token_config.im_end_id
    entries, codes, n, lp, rows = stepped
    assert n[0] == 6 and codes[0, 5, 0] == im_end and (n[1:] == CAP).sum() >= 2  # one slot ends early, some run to max_frames
    worst, checked = 0.0, 0
    for b in range(5):
        for f in range(int(n[b])):
            row = rows[f][b]
            if b in LENGTH:
                row = length_patch(row, im_end, f, *LENGTH[b])
            if entries is SAMPLED and b == 1:
                row = penalised_row(row, FILTER1[2], codes[b, max(0, f - FILTER1[3]):f, 0])
            want = pick_logprob(row, int(codes[b, f, 0]))
            err = abs(float(lp[b, f]) - want)
            worst, checked = max(worst, err), checked + 1
            assert err <= LOGPROB_MARGIN, (b, f, float(lp[b, f]), want)
        assert (lp[b, int(n[b]):] == SENTINEL).all(), b  # (e) nothing behind a slot's last frame
    assert checked == int(n.sum())
    print(f"logprob session: {checked} picks, largest |device - model| = {worst:.3e}")


def test_scoring_changes_no_id(eng_pe, prompts5, stepped):
    """(b) All five slots against a session that never called set_slot_score, whose array stays untouched."""
    eng, _ = eng_pe
    entries, codes, n, _, _ = stepped
    base_codes, base_n, base_lp = _run(eng, prompts5, entries, score=False)
    assert np.array_equal(n, base_n) and all(np.array_equal(codes[b, :n[b]], base_codes[b, :n[b]]) for b in range(5))
    assert (base_lp == SENTINEL).all()
    if entries is SAMPLED:
        greedy_codes, _, _ = _run(eng, prompts5, GREEDY, score=False)
        assert not np.array_equal(greedy_codes[0, :6, 0], codes[0, :6, 0]) or not np.array_equal(greedy_codes[1, :, 0], codes[1, :, 0])


@pytest.mark.parametrize("kw", [dict(per_graph=4), dict(per_graph=4, commit_picks=False), dict(per_graph=1, commit_picks=False)],
                         ids=["four per graph", "four per graph, pick launches", "pick launches"])
def test_graph_replays_and_the_pick_as_its_own_launch_give_the_same_bits(eng_pe, prompts5, stepped, kw):
    """(c), (d), (e): slot 0 ends inside the second replay; the scores are (a)'s bit for bit and nothing lies behind a slot's last
    frame, also after four more frames with every slot through (the slots that ran to max_frames among them)."""
    eng, _ = eng_pe
    entries, codes, n, lp, _ = stepped
    got_codes, got_n, got_lp = _run(eng, prompts5, entries, score=True, **kw)
    assert np.array_equal(got_n, n)
    for b in range(5):
        assert np.array_equal(got_codes[b, :n[b]], codes[b, :n[b]]), b
        assert np.array_equal(got_lp[b, :n[b]].view(np.uint32), lp[b, :n[b]].view(np.uint32)), (b, got_lp[b], lp[b])
        assert (got_lp[b, n[b]:] == SENTINEL).all(), (b, got_lp[b])


def test_recycled_slot_without_the_option_stops_the_scoring(eng_pe, prompts5):
    """(f) Tenants written as every front end writes them: once no live slot scores, the form has lost bit 4 -- nothing is written
    any more -- and the new tenant's ids are those of a session that never scored."""
    from smoltts_amd.config import GenerationSettings, RequestSampling
    from smoltts_amd.engine import LMSession
    from smoltts_amd.generate import _apply_slot_sampling

    eng, _ = eng_pe
    gs = GenerationSettings.greedy()
    never = dict(eos_bias=-100.0)  # (no tenant stops before the cap)
    first = RequestSampling(temperature=0.9, seed=5, logprobs=True, **never).resolve(gs)
    second = RequestSampling(temperature=0.9, seed=9, **never).resolve(gs)
    plain = RequestSampling(**never).resolve(gs)
    runs = {}
    for scored in (True, False):
        s = LMSession(eng, 2, max_seq=256, max_rows=512, max_frames=CAP)
        s.set_frames_per_graph(4)
        s.logprobs.fill_(SENTINEL)
        _apply_slot_sampling(s, [0, 1], [first if scored else RequestSampling(temperature=0.9, seed=5, **never).resolve(gs), plain])
        assert (0 in s.scored_slots) == scored
        s.prefill(prompts5[:2], stop_on_eos=True)
        s.decode(CAP - 1)
        codes, n, _, _ = s.fetch()
        lp = s.fetch_logprobs()
        runs[scored, 1] = codes[:, :CAP].copy()
        assert n[0] == n[1] == CAP
        assert (lp != SENTINEL).all() if scored else (lp == SENTINEL).all()
        s.logprobs.fill_(SENTINEL)
        _apply_slot_sampling(s, [0], [second])
        assert not s.scored_slots
        s.prefill([prompts5[2]], slots=[0], stop_on_eos=True)
        s.decode(CAP - 1)
        codes, n, _, _ = s.fetch()
        assert n[0] == CAP and (s.fetch_logprobs() == SENTINEL).all()
        runs[scored, 2] = codes[0, :CAP].copy()
        s.close()
    assert np.array_equal(runs[True, 1], runs[False, 1]) and np.array_equal(runs[True, 2], runs[False, 2])
