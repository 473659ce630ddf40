"""Long texts as chained segments, host side (no GPU): text segmentation, chained prompts, segment seeds, the numpy seam model and
the server's long_text settings with a stand-in model."""
import numpy as np
import pytest

from smoltts_amd.longform import (SEED_STEP, Segment, SegmentOptions, SegmentPlan, chain_prompt, needs_segments, segment_options,
                                  segment_seed, split_text, voice_prefix)
from smoltts_amd import seam
from smoltts_amd.seam import BLOCK, D, H, THRESH, SeamState


def _texts(segs):
    return [s.text for s in segs]


def _norm(text):
    from smoltts_amd.longform import _BREAK

    return " ".join(_BREAK.sub(" ", text).split())


# ---------------------------------------------------------------------------------------------------- split_text
def test_short_text_without_tags_is_one_segment():
    segs = split_text("Hello there. How are you?")
    assert segs == [Segment("Hello there. How are you?", None)]
    assert not needs_segments(segs)


def test_sentences_newlines_and_greedy_packing():
    text = "One two. Three four! Five six? Seven…  Eight.\nNine ten"
    assert _texts(split_text(text, max_bytes=4096)) == ["One two. Three four! Five six? Seven… Eight. Nine ten"]
    assert _texts(split_text(text, max_bytes=20)) == ["One two. Three four!", "Five six? Seven…", "Eight. Nine ten"]
    # a sentence end needs whitespace after it; closing quotes and brackets stay with their sentence
    assert _texts(split_text('He said "Go." (Then left.) v1.2 is out', max_bytes=12)) == ['He said', '"Go."', '(Then left.)', 'v1.2 is out']
    # a newline always cuts a sentence, even without a full stop
    assert _texts(split_text("line one\nline two", max_bytes=9)) == ["line one", "line two"]


def test_long_sentence_cut_at_clause_then_space_then_character():
    s = "alpha beta, gamma delta; epsilon zeta: eta theta"
    segs = _texts(split_text(s, max_bytes=26))
    assert segs == ["alpha beta, gamma delta;", "epsilon zeta: eta theta"]
    assert _texts(split_text("aaaa bbbb cccc dddd", max_bytes=10)) == ["aaaa bbbb", "cccc dddd"]
    assert _texts(split_text("abcdefghij", max_bytes=4)) == ["abcd", "efgh", "ij"]
    # multi-byte text: no cut inside a character, every segment within the limit
    ja = "日本語のテキストはとても長いです" * 3
    out = _texts(split_text(ja, max_bytes=20))
    assert all(len(t.encode()) <= 20 for t in out) and "".join(out) == ja
    assert _texts(split_text("éééééé", max_bytes=5)) == ["éé", "éé", "éé"]


def test_segments_respect_the_limit_and_round_trip():
    rng = np.random.default_rng(0)
    words = ["a", "bb", "ccc,", "dddd.", "ééé", "ff?", "g;", "hhhhhhhhhhhhhhhhhhhhhhh", "—", "\n", "i!", "“j.”", "(k.)"]
    for trial in range(200):
        text = " ".join(rng.choice(words, size=int(rng.integers(1, 80))))
        if trial % 3 == 0:
            text = text.replace(" ", '<break time="0.5s"/>', 2)
        mb = int(rng.integers(8, 60))
        segs = split_text(text, max_bytes=mb)
        assert all(0 < len(s.text.encode()) <= mb for s in segs)
        assert all(s.text == s.text.strip() and "  " not in s.text for s in segs)
        if all(len(w.encode()) <= mb for w in _norm(text).split()):
            assert " ".join(_texts(segs)) == _norm(text)
        else:  # a word cut at a character boundary comes back with a space in it
            assert "".join(_texts(segs)).replace(" ", "") == _norm(text).replace(" ", "")
        assert split_text(text, max_bytes=mb) == segs  # deterministic


def test_break_tags():
    segs = split_text('Hello.<break time="1.5s" /> World. <break time="750ms"/>Again<break time=\'2s\'>', max_bytes=300)
    assert segs == [Segment("Hello.", 1.5), Segment("World.", 0.75), Segment("Again", 2.0)]
    assert needs_segments(segs)
    # consecutive tags add up; tags at the start become silence in front
    segs = split_text('<break time="1s"/><break time="0.5s"/>Hi. <break time="3s"/> <break time="2s" /> there', max_bytes=300)
    assert segs == [Segment("Hi.", 5.0, 1.5), Segment("there", None)]
    # one segment with a tag still needs the seam stage
    assert needs_segments(split_text('Hi <break time="1s"/>'))
    with pytest.raises(ValueError):
        split_text('a <break time="3.5s"/> b')
    with pytest.raises(ValueError):
        split_text('a <break time="3001ms"/> b')
    assert split_text('<break time="1s"/>') == []


def test_segment_options():
    assert segment_options(False) is None and segment_options(None) is None
    assert segment_options(True) == SegmentOptions()
    assert segment_options({"max_bytes": 50, "context": "none"}).max_bytes == 50
    for bad in ({"context": "all"}, {"pause_s": 4.0}, {"max_bytes": 2}):
        with pytest.raises(ValueError):
            segment_options(bad)


# ---------------------------------------------------------------------------------------------------- chain_prompt
@pytest.fixture()
def encoder():
    from smoltts_amd.prompt import PromptEncoder
    from smoltts_amd.tokenizer import load_tokenizer

    return PromptEncoder(load_tokenizer(), 320)


def test_chain_prompt_segment0_is_build_prompt(encoder):
    for voice in ("heart", "nova", "unknown"):
        pre = voice_prefix(encoder, voice)
        np.testing.assert_array_equal(chain_prompt(encoder, pre, "Hello world."), encoder.build_prompt("Hello world.", voice))
    spk = np.arange(27, dtype=np.int32).reshape(9, 3)
    np.testing.assert_array_equal(chain_prompt(encoder, voice_prefix(encoder, "x", spk), "Hi"), encoder.build_prompt("Hi", "x", spk))


def test_chain_prompt_with_context(encoder):
    pre = voice_prefix(encoder, "bella")
    codes = (np.arange(8 * 5, dtype=np.uint32).reshape(8, 5) * 7) % 300
    got = chain_prompt(encoder, pre, "Second.", "First.", codes, max_new_tokens=100, max_seq=2048)
    want = np.concatenate([pre, encoder.encode_text_turn("user", "First."), encoder.encode_vq(codes.astype(np.int64)),
                           encoder.encode_text_turn("user", "Second."), encoder.encode_text_turn("assistant")], axis=1)
    np.testing.assert_array_equal(got, want)
    # the context goes in exactly when P + context + turn + max_new + 2 <= max_seq
    plain = chain_prompt(encoder, pre, "Second.")
    need = want.shape[1] + 100 + 2
    assert chain_prompt(encoder, pre, "Second.", "First.", codes, 100, need).shape == want.shape
    np.testing.assert_array_equal(chain_prompt(encoder, pre, "Second.", "First.", codes, 100, need - 1), plain)


def test_segment_seed():
    assert segment_seed(None, 3) is None
    assert segment_seed(12345, 0) == 12345
    assert segment_seed(12345, 1) == (12345 + 0x9E3779B97F4A7C15) % 2**64
    assert segment_seed(2**64 - 1, 2) == (2**64 - 1 + 2 * SEED_STEP) % 2**64


def test_segment_plan_numbers():
    from smoltts_amd.config import GenerationSettings, RequestSampling

    text = '<break time="0.5s"/> One two. <break time="1s"/> Three four. Five six. <break time="250ms"/>'
    plan = SegmentPlan.create(text, SegmentOptions(max_bytes=12, pause_s=0.2))
    assert [s.text for s in plan.segs] == ["One two.", "Three four.", "Five six."]
    assert plan.pauses == [24000, 4800] and plan.lead == 12000 and plan.trail == 6000
    assert [plan.seam_args(k) for k in range(3)] == [(24000, seam.FIRST, 12000), (4800, 0, 12000), (6000, seam.FINAL, 12000)]
    want = [5, 11400714819323198490, 4354685564936845359]
    assert [plan.sampling(k, RequestSampling(temperature=0.5, seed=5)) for k in range(3)] == [
        RequestSampling(temperature=0.5, seed=s) for s in want]
    gs = GenerationSettings(max_new_tokens=7, seed=5)
    assert [plan.sampling(k, gs) for k in range(3)] == [GenerationSettings(max_new_tokens=7, seed=s) for s in want]
    assert seam.segment_flags(0, 1) == seam.FIRST | seam.FINAL


def test_segment_plan_prompt_follows_the_context_option(encoder):
    pre = voice_prefix(encoder, "heart")
    codes = np.arange(8 * 3, dtype=np.uint32).reshape(8, 3) % 50
    for context in ("previous", "none"):
        plan = SegmentPlan.create("First. Second.", SegmentOptions(max_bytes=8, context=context))
        assert plan.prompt(0, encoder, pre, None, 100, 2048).tolist() == chain_prompt(encoder, pre, "First.").tolist()
        got = plan.prompt(1, encoder, pre, ("First.", codes), 100, 2048)
        want = chain_prompt(encoder, pre, "Second.", *(("First.", codes) if context == "previous" else (None, None)), 100, 2048)
        np.testing.assert_array_equal(got, want)


def test_segment_plan_is_none_exactly_without_segments():
    texts = ["Hello there.", "One. Two. Three.", 'Hi. <break time="1s"/>', '<break time="1s"/> Hi.', "a" * 40, "x\ny",
             'Hi <break time="0s"/> there']
    for opts in (SegmentOptions(), SegmentOptions(max_bytes=8)):
        for t in texts:
            assert (SegmentPlan.create(t, opts) is None) == (not needs_segments(split_text(t, opts.max_bytes))), (t, opts)
    with pytest.raises(ValueError, match="nothing to speak"):
        SegmentPlan.create(' <break time="1s"/> ', SegmentOptions())


# ---------------------------------------------------------------------------------------------------- numpy seam model
def _speech(n, rng, amp=0.3):
    """Samples whose every 240-sample block is well above the threshold."""
    x = rng.uniform(-amp, amp, n).astype(np.float32)
    x[::40] = amp
    return x


def _quiet(n, rng):
    return rng.uniform(-0.5, 0.5, n).astype(np.float32) * np.float32(2 ** -9)  # max|x| < 2^-8 everywhere


def _split(n, rng):
    sizes, left = [], n
    while left > 0:
        k = int(min(left, rng.integers(1, 4 * 1920 + 1)))
        sizes.append(k)
        left -= k
    return sizes or [0]


def test_single_segment_is_identity_for_any_chunking():
    rng = np.random.default_rng(1)
    x = np.concatenate([_quiet(3000, rng), _speech(5000, rng), _quiet(30000, rng)])
    for _ in range(5):
        np.testing.assert_array_equal(seam.join([x], [], chunks=[_split(x.size, rng)]), x)


def test_trailing_silence_becomes_exactly_the_pause():
    rng = np.random.default_rng(2)
    a_sp, b_sp = _speech(4800, rng), _speech(2400, rng)
    for r in (0, 100, 240, 4000, 9000):
        for G in (0, 2400, 6000):
            tail = _quiet(r, rng)
            a = np.concatenate([a_sp, tail])
            y = seam.join([a, b_sp], [G])
            # the tail's r samples are held in whole blocks (the partial last one judged by the same rule): all of them here
            keep = min(r, G)
            want = np.concatenate([a_sp, tail[:keep], np.zeros(G - keep, np.float32), b_sp])
            np.testing.assert_array_equal(y, want)


def test_held_run_is_released_unchanged_when_speech_resumes():
    rng = np.random.default_rng(3)
    a = np.concatenate([_speech(2400, rng), _quiet(4800, rng), _speech(2400, rng)])
    b = _speech(480, rng)
    # (a ends loud: nothing is held at its end, and the seam is the pause alone)
    np.testing.assert_array_equal(seam.join([a, b], [1000]), np.concatenate([a, np.zeros(1000, np.float32), b]))


def test_hold_and_drop_caps():
    rng = np.random.default_rng(4)
    long_tail = _quiet(H + 24 * BLOCK, rng)
    a = np.concatenate([_speech(2400, rng), long_tail])
    b_head = _quiet(D + 10 * BLOCK, rng)
    b = np.concatenate([b_head, _speech(2400, rng)])
    y = seam.join([a, b], [480])
    # only the last H of the tail can go: its first 24 blocks are released; of the head, at most D is dropped
    want = np.concatenate([a[:2400 + 24 * BLOCK], long_tail[24 * BLOCK:24 * BLOCK + 480], b_head[D:], b[b_head.size:]])
    np.testing.assert_array_equal(y, want)


def test_head_drop_stops_at_first_loud_block_and_cuts_stay_quiet():
    rng = np.random.default_rng(5)
    a = _speech(2400, rng)
    b = np.concatenate([_quiet(5 * BLOCK + 17, rng), _speech(2400, rng)])  # the loud block is block 5 (partly quiet)
    y = seam.join([a, b], [0])
    np.testing.assert_array_equal(y, np.concatenate([a, b[5 * BLOCK:]]))
    assert np.max(np.abs(b[5 * BLOCK:5 * BLOCK + 17])) < THRESH


def test_lead_and_trail_and_chunking_independence():
    rng = np.random.default_rng(6)
    segs = []
    for k in range(4):
        parts = []
        for _ in range(int(rng.integers(1, 5))):
            parts.append(_quiet(int(rng.integers(0, 40000)), rng))
            parts.append(_speech(int(rng.integers(1, 6000)), rng))
        parts.append(_quiet(int(rng.integers(0, 40000)), rng))
        segs.append(np.concatenate(parts))
    pauses = [6000, 0, 24000]
    whole = seam.join(segs, pauses, lead=1234, trail=777)
    assert np.all(whole[:1234] == 0) and np.all(whole[-777:] == 0)
    for _ in range(6):
        np.testing.assert_array_equal(seam.join(segs, pauses, lead=1234, trail=777, chunks=[_split(s.size, rng) for s in segs]), whole)


def test_last_flag_releases_the_held_run():
    rng = np.random.default_rng(7)
    st = SeamState()
    st.start(5000, 0)
    x = np.concatenate([_speech(2400, rng), _quiet(4800, rng)])
    y = np.concatenate([st.push(x[:3000]), st.push(x[3000:], last=True)])
    np.testing.assert_array_equal(y, x)


# ---------------------------------------------------------------------------------------------------- server, stand-in model
class _SegModel:
    sampling_rate = 24000

    def __init__(self):
        self.calls = []

    def __call__(self, text, voice="heart", **kw):
        self.calls.append(("call", text, kw))
        return np.linspace(-0.5, 0.5, 1920, dtype=np.float32)

    def stream(self, text, voice="heart", **kw):
        self.calls.append(("stream", text, kw))
        for i in range(2):
            yield np.full(1920, 0.1 * i, dtype=np.float32)


def _client(model, settings=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    return TestClient(create_app(model, settings))


def test_server_passes_segment_only_in_segment_mode():
    m = _SegModel()
    c = _client(m)
    assert c.post("/v1/audio/speech", json={"input": "Hi. There.", "voice": "heart"}).status_code == 200
    assert m.calls[-1] == ("call", "Hi. There.", {})
    assert c.post("/v1/text-to-speech/3/stream", json={"text": "Hi."}).status_code == 200
    assert m.calls[-1] == ("stream", "Hi.", {})
    assert c.get("/v1/stats").json() == {}

    m2 = _SegModel()
    c2 = _client(m2, {"long_text": "segment", "segment_max_bytes": 120, "seam_pause_ms": 400})
    text = 'First sentence. <break time="1s"/> Second one.'
    assert c2.post("/v1/audio/speech", json={"input": text, "voice": "heart"}).status_code == 200
    kind, got, kw = m2.calls[-1]
    assert kind == "call" and got == text  # break tags reach the model
    assert kw == {"segment": {"max_bytes": 120, "pause_s": 0.4}}
    for fmt in ("pcm_24000", "pcm_16000", "ulaw_8000"):
        assert c2.post(f"/v1/text-to-speech/3/stream?output_format={fmt}", json={"text": text}).status_code == 200
        assert m2.calls[-1][0] == "stream" and m2.calls[-1][2]["segment"] == {"max_bytes": 120, "pause_s": 0.4}
    assert c2.post("/v1/audio/speech", json={"input": text, "voice": "heart", "response_format": "flac"}).status_code == 200
    assert m2.calls[-1][2]["container"] == "flac" and "segment" in m2.calls[-1][2]
    assert c2.get("/v1/stats").json() == {"segments": 2 * 5}


def test_server_segment_mode_refuses_over_max_input_chars_and_bad_tags():
    m = _SegModel()
    c = _client(m, {"long_text": "segment", "max_input_chars": 100})
    assert c.post("/v1/audio/speech", json={"input": "a" * 101, "voice": "heart"}).status_code == 400
    assert c.post("/v1/text-to-speech/3/stream", json={"text": "a" * 101}).status_code == 400
    assert c.post("/v1/text-to-speech/3", json={"text": 'a <break time="9s"/> b'}).status_code == 400
    assert c.post("/v1/audio/speech", json={"input": "a" * 100, "voice": "heart"}).status_code == 200
    assert not any(call[1] == "a" * 101 for call in m.calls)


def test_settings_schema_long_text():
    from smoltts_amd.server.settings import ServerSettings

    s = ServerSettings(checkpoint_dir="x")
    assert (s.long_text, s.segment_max_bytes, s.seam_pause_ms, s.max_input_chars) == ("refuse", 300, 250, 5000)
    assert ServerSettings(checkpoint_dir="x", long_text="segment").long_text == "segment"
    with pytest.raises(Exception):
        ServerSettings(checkpoint_dir="x", long_text="always")
