"""The per-slot tables behind more uploads than the pinned ring has areas: 13 rounds of ``set_slot_sampling`` / ``_filters`` /
``_length`` / ``_align`` (52 uploads, the ring holds 8) queued behind a running utterance without a host synchronisation, twelve
of them with entries that differ from the last.  The utterance that follows must be, bit for bit, that of a fresh session which
received the last entries only, and the graph form must be the one those entries imply: the last write wins across the ring's
wraps, on the device and in the host mirror."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 12
B = 5
ROUNDS = 13
TEXTS = (("one", "heart"), ("a second, longer prompt than the first", "sky"), ("3", "nova"), ("the fourth one", "bella"), ("five five five", "liam"))
PAIRS = [(0, 1), (1, 4)]
# the final entries, all five slots in every table: slot 0 sampled and scored, slot 1 sampled with a filter and a window, slot 2 greedy
# with a length entry (it ends at frame 5), slot 3 greedy, scored, with a window, slot 4 with none of them
SAMPLING = [(0.9, 0.0, 0.0, 101), (0.8, 0.0, 0.05, 102), (0.0, 0.0, 0.0, 0), (0.0, 0.0, 0.0, 0), (0.0, 0.0, 0.0, 0)]
FILTERS = [(1.0, 0, 1.0, 0), (0.9, 50, 1.5, 8), (1.0, 0, 1.0, 0), (1.0, 0, 1.0, 0), (1.0, 0, 1.0, 0)]  # (top_p, top_k, penalty, window)
LENGTH = [(0, 0.0), (0, 0.0), (5, 1e4), (0, 0.0), (0, 0.0)]  # (min_frames, eos_bias)
SCORE = [True, False, False, True, False]
WINDOW_ON = [False, True, False, True, False]
FORM = 1 | 4 | 8 | 16 | 32  # slow token sampled (no depth code is), a filter, a length entry, a score flag, a window


def _columns(rows):
    return [list(x) for x in zip(*rows)]


def _windows(prompts):
    return [(1, p.shape[1] - 1) if on else (0, 0) for p, on in zip(prompts, WINDOW_ON)]


def _write_final(s, prompts):
    every = list(range(B))
    s.set_slot_sampling(every, *_columns(SAMPLING))
    s.set_slot_filters(every, *_columns(FILTERS))
    s.set_slot_length(every, *_columns(LENGTH))
    s.set_slot_align(every, *_columns(_windows(prompts)))
    s.set_slot_score(every, SCORE)


def _other_round(s, r, prompts):
    """Round r < ROUNDS: entries that differ from the final ones, over a subset of the slots that changes with r (every slot is
    listed in some round of every table, slot 4 with everything on)."""
    slots = [b for b in range(B) if (b + r) % 3 != 0]
    n = len(slots)
    s.set_slot_sampling(slots, [0.5 + 0.03 * r + 0.01 * b for b in slots], [0.4 if (b + r) % 2 else 0.0 for b in slots], [0.02] * n,
                        [1000 * r + b for b in slots])
    s.set_slot_filters(slots, [0.7 if (b + r) % 2 else 1.0 for b in slots], [5 + r if (b + r) % 2 == 0 else 0 for b in slots],
                       [1.2] * n, [(4 + b) * (r % 2) for b in slots])
    s.set_slot_length(slots, [(r + b) % 4 for b in slots], [0.5 * r - 2.0 if b != 2 else -3.0 for b in slots])
    s.set_slot_align(slots, [b % 2 for b in slots], [(prompts[b].shape[1] - (r + b) % 2) * ((r + b) % 3 != 1) for b in slots])
    if r % 4 == 1:
        s.set_slot_score([4, 1], [True, True])


def _utterance(s, prompts):
    """codes, frame counts, logprobs, alignment rows of the slots with a window, form."""
    form = s.graph_form()
    s.prefill(prompts, stop_on_eos=True)
    s.decode(CAP - 1)
    codes, n, _, _ = s.fetch()
    lp = s.fetch_logprobs()
    rows = {b: s.fetch_alignment(b, int(n[b])).copy() for b in range(B) if WINDOW_ON[b]}
    return codes.copy(), n.copy(), lp.copy(), rows, form


@pytest.fixture(scope="module")
def runs():
    from smoltts_amd.config import TokenConfig
    from smoltts_amd.engine import LMEngine, LMSession
    from smoltts_amd.prompt import PromptEncoder
    from smoltts_amd.synthetic import named_config, synthetic_lm_state
    from smoltts_amd.tokenizer import load_tokenizer

    cfg = named_config("tiny")
    tok = load_tokenizer()
    tc = TokenConfig.from_tokenizer(tok, cfg)
    pe = PromptEncoder(tok, tc.semantic_start_id, cfg.num_codebooks, cfg.duplicate_code_0)
    eng = LMEngine(cfg, synthetic_lm_state(cfg, seed=21), tc)
    prompts = [pe.build_prompt(t, v) for t, v in TEXTS]

    def session():
        s = LMSession(eng, B, max_seq=256, max_rows=256 * B, max_frames=CAP)
        s.set_frames_per_graph(4)
        s.set_align_heads(PAIRS)
        return s

    a = session()
    _other_round(a, 0, prompts)  # (slot mode entered, and its first graphs built, before anything is in flight)
    a.prefill(prompts, stop_on_eos=True)
    a.decode(CAP - 1)
    for r in range(1, ROUNDS):  # behind the frames just queued: no host synchronisation from here to the end of the rounds
        _other_round(a, r, prompts)
    _write_final(a, prompts)
    form_after = a.graph_form()
    got = _utterance(a, prompts)
    slots_a = (set(a.filtered_slots), set(a.length_slots), set(a.scored_slots), set(a.align_slots))
    a.close()
    b = session()
    _write_final(b, prompts)
    want = _utterance(b, prompts)
    slots_b = (set(b.filtered_slots), set(b.length_slots), set(b.scored_slots), set(b.align_slots))
    b.close()
    eng.close()
    return dict(got=got, want=want, form_after=form_after, slots_a=slots_a, slots_b=slots_b)


def test_the_form_is_what_the_final_entries_imply(runs):
    assert runs["form_after"] == FORM
    assert runs["got"][4] == FORM and runs["want"][4] == FORM
    want_slots = ({b for b in range(B) if FILTERS[b] != (1.0, 0, 1.0, 0)}, {b for b in range(B) if LENGTH[b] != (0, 0.0)},
                  {b for b in range(B) if SCORE[b]}, {b for b in range(B) if WINDOW_ON[b]})
    assert runs["slots_a"] == want_slots and runs["slots_b"] == want_slots


def test_the_last_write_wins_across_the_wraps_of_the_ring(runs):
    codes, n, lp, rows, _ = runs["got"]
    wcodes, wn, wlp, wrows, _ = runs["want"]
    assert np.array_equal(n, wn), (n, wn)
    assert n[2] == 6 and (n > 0).all()  # (the final length entry acted: slot 2 could not end before frame 5 and did there)
    for b in range(B):
        assert np.array_equal(codes[b, :n[b]], wcodes[b, :n[b]]), b
        if SCORE[b]:
            assert np.array_equal(lp[b, :n[b]].view(np.uint32), wlp[b, :n[b]].view(np.uint32)), (b, lp[b], wlp[b])
        if WINDOW_ON[b]:
            assert np.array_equal(rows[b].view(np.uint32), wrows[b].view(np.uint32)), b
            assert (rows[b][1:, :, 0] >= 0).all()  # (the decode frames did measure inside the final window)
