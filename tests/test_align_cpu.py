"""The host side of the character timestamps (smoltts_amd/align.py) and the option's parsing, without a GPU."""
import re

import numpy as np
import pytest

from smoltts_amd import abi, align
from smoltts_amd.prompt import PromptEncoder
from smoltts_amd.request import parse_request
from smoltts_amd.tokenizer import load_tokenizer
from test_host_cpu import ROOT


# ------------------------------------------------------------------------------------------------ the fit
def test_isotonic_step_equals_scipy_on_random_inputs():
    from scipy.optimize import isotonic_regression

    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 200):
        for _ in range(20):
            y = np.cumsum(rng.standard_normal(n)) + rng.standard_normal(n) * 3
            w = rng.uniform(0.05, 2.0, n)
            want = isotonic_regression(y, weights=w).x
            got = align.isotonic(y, w)
            assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(y).max())), n
            assert (np.diff(got) >= 0).all()
    with pytest.raises(ValueError):
        align.isotonic([1.0, 2.0], [1.0, 0.0])


def _staircase(durations, rng, heads=2):
    """Token i held for durations[i] frames by ``heads`` heads of mass 0.3 .. 0.6 each -> (m, s1) [frames, heads], boundaries."""
    tok = np.repeat(np.arange(len(durations)), durations)
    F = tok.size
    m = rng.uniform(0.3, 0.6, (F, heads))
    s1 = m * tok[:, None]
    return m, s1, np.concatenate([[0], np.cumsum(durations)])


def test_a_planted_staircase_is_recovered_to_within_half_a_frame():
    rng = np.random.default_rng(11)
    for trial in range(10):
        durations = rng.integers(2, 7, size=int(rng.integers(3, 25)))
        m, s1, bounds = _staircase(durations, rng)
        F, n = m.shape[0], len(durations)
        # frame 0 out of the prefill; a few frames whose heads look elsewhere: outliers (their centroid is
        # anywhere in the text) of a mass below MIN_MASS, which the fit gives no weight
        m[0] = -1.0
        # (no two of them adjacent: one missing frame moves a boundary by at most half a frame, two in a row by a whole one)
        cand = np.arange(2, F, 3) + rng.integers(0, 2)
        quiet = rng.choice(cand[cand < F], size=max(1, F // 10), replace=False)
        m[quiet] = rng.uniform(0.0, 0.02, (quiet.size, m.shape[1]))
        s1[quiet] = m[quiet] * rng.uniform(0, n, (quiet.size, 1))
        ft = align.fit(m, s1, n)
        assert ft.starts[0] == 0.0 and ft.ends[-1] == F
        assert (np.diff(ft.starts) >= 0).all() and np.array_equal(ft.ends[:-1], ft.starts[1:])
        assert np.abs(ft.starts - bounds[:-1]).max() <= 0.5, (trial, ft.starts, bounds)
        assert (ft.mass[0] == -1) and np.isnan(ft.centroid[0]) and np.isnan(ft.centroid[quiet]).all()
    # an outlier of full mass is pooled with its neighbours: it moves a boundary inside its own token's four frames at most, and
    # the times stay monotone and whole
    m, s1, bounds = _staircase([4] * 10, rng)
    s1[13] = m[13] * 0.0
    s1[25] = m[25] * 9.0
    ft = align.fit(m, s1, 10)
    assert (np.diff(ft.starts) >= 0).all() and ft.ends[-1] == 40 and np.abs(ft.starts - bounds[:-1]).max() <= 4.0


def test_unmeasured_or_massless_frames_carry_no_weight():
    m = np.array([[-1.0], [0.5], [align.MIN_MASS / 2], [0.5]])
    s1 = np.array([[0.0], [0.0], [100.0], [0.5]])
    ft = align.fit(m, s1, 2)
    assert np.isnan(ft.centroid[[0, 2]]).all() and ft.centroid[1] == 0.0 and ft.centroid[3] == 1.0
    assert ft.starts[1] == pytest.approx(2.5)  # halfway between the centres of frames 1 and 3
    none = align.fit(np.full((6, 2), -1.0), np.zeros((6, 2)), 3)
    assert np.allclose(none.starts, [0, 2, 4]) and none.ends[-1] == 6


# ------------------------------------------------------------------------------------------------ characters
def test_characters_map_to_their_tokens():
    tok = load_tokenizer()
    text = "aé<|im_end|>b中z"  # latin-1 e-acute: one token; a spelled-out added token; a CJK character the tokenizer drops
    ids = tok.encode(text).ids
    spans = align.token_spans(text, ids, tok)
    assert len(spans) == len(text) and len(ids) == 5
    assert spans[0] == (0, 1) and spans[1] == (1, 2)
    assert spans[2:12] == [(2, 3)] * 10  # every character of <|im_end|> belongs to its one token
    assert spans[12] == (3, 4) and spans[13] == (4, 4) and spans[14] == (4, 5)
    # a byte-level vocabulary: one token per UTF-8 byte, a multi-byte character owns all of its bytes
    text2 = "hé中!"
    ids2 = list(text2.encode("utf-8"))
    assert align.token_spans(text2, ids2) == [(0, 1), (1, 3), (3, 6), (6, 7)]
    with pytest.raises(ValueError):
        align.token_spans("ab", [97, 98, 99])


def test_window_of_finds_the_requests_own_text():
    tok = load_tokenizer()
    enc = PromptEncoder(tok, tok.token_to_id("<|semantic:0|>"), 8, True)
    text = "hello there"
    p = enc.build_prompt(text, "sky")
    t0, t1 = align.window_of(p[0], tok)
    assert list(p[0, t0:t1]) == tok.encode(text).ids and p[0, t1] == tok.token_to_id("<|im_end|>")
    # a cloned voice's speaker turns in front are user turns too: the window is the last one
    speaker = np.concatenate([enc.encode_text_turn("user", "the reference transcript"), enc.encode_vq(np.ones((8, 5), np.int64))], axis=1)
    q = enc.build_prompt(text, "sky", speaker)
    u0, u1 = align.window_of(q[0], tok)
    assert list(q[0, u0:u1]) == tok.encode(text).ids and u0 > speaker.shape[1] and u1 - u0 == len(text)
    with pytest.raises(ValueError):
        align.window_of(enc.encode_text_turn("assistant")[0], tok)


# ------------------------------------------------------------------------------------------------ times
def test_times_are_monotone_end_at_the_duration_and_scale_with_speed():
    rng = np.random.default_rng(3)
    tok = load_tokenizer()
    text = "café au lait"
    ids = tok.encode(text).ids
    m, s1, bounds = _staircase([3] * len(ids), rng)
    F = m.shape[0]
    a = align.align(text, ids, m, s1, tok)
    assert a.characters == list(text) and len(a.start_s) == len(a.end_s) == len(text)
    assert a.start_s[0] == 0.0 and a.end_s[-1] == pytest.approx(F * 0.08)
    assert all(s <= e for s, e in zip(a.start_s, a.end_s)) and all(x <= y for x, y in zip(a.start_s, a.start_s[1:]))
    assert np.allclose(a.start_s, bounds[:-1] * 0.08, atol=0.04 + 1e-9)
    j = a.to_json()
    assert set(j) == {"characters", "character_start_times_seconds", "character_end_times_seconds"} and j["characters"] == list(text)
    # at speed 1.5 the delivered audio is a little shorter than nominal: times are divided by the speed, the end is the duration
    fast = align.align(text, ids, m, s1, tok, speed=1.5, duration_s=F * 0.08 / 1.5 - 0.01)
    assert np.allclose(fast.start_s, np.asarray(a.start_s) / 1.5) and fast.end_s[-1] == pytest.approx(F * 0.08 / 1.5 - 0.01)
    assert max(fast.end_s) <= F * 0.08 / 1.5 - 0.01 + 1e-12
    assert align.FRAME_S == 1920 / 24000


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw,word", [(dict(segment=True), "segment"), (dict(segment={}), "segment"),
                                     (dict(trim_silence=True), "trim_silence"), (dict(max_pause_s=0.5), "max_pause_s"),
                                     (dict(pieces=True), "pieces"), (dict(stream=True), "blocking")])
def test_timestamps_are_refused_where_a_frames_place_in_the_output_is_not_known(kw, word):
    with pytest.raises(ValueError, match=word):
        parse_request("Some text. And more.", timestamps=True, **kw)
    assert parse_request("Some text. And more.", **kw).timestamps is False  # (the other option alone stays accepted)


def test_timestamps_parse_and_need_configured_heads():
    assert parse_request("x", timestamps=True).timestamps is True and parse_request("x").timestamps is False
    assert parse_request("x", timestamps=True, speed=1.25, loudness=-20.0).timestamps is True
    with pytest.raises(ValueError):
        parse_request("x", timestamps="yes")
    assert align.check_heads(None) == [] and align.check_heads([[3, 1], (0, 2)]) == [(0, 2), (3, 1)]
    for bad in ([[0]], [[0, 1], [0, 1]], [[-1, 0]], [[0.5, 1]], [[i, 0] for i in range(17)], ["ab"]):
        with pytest.raises(ValueError):
            align.check_heads(bad)

    class Cfg:
        n_layer, n_head = 2, 6

    with pytest.raises(ValueError):
        align.check_heads([[2, 0]], Cfg)
    with pytest.raises(ValueError):
        align.check_heads([[0, 6]], Cfg)
    # the front end refuses the option without heads before it touches the GPU
    from smoltts_amd import SmolTTS

    tts = SmolTTS.__new__(SmolTTS)
    tts.alignment_heads, tts.watermark = [], None
    with pytest.raises(ValueError, match="alignment_heads"):
        tts("hello", timestamps=True)


# ------------------------------------------------------------------------------------------------ ranking
def test_rank_heads_puts_a_planted_diagonal_head_first():
    rng = np.random.default_rng(8)
    pairs = [(l, h) for l in range(2) for h in range(4)]
    planted = 5
    runs = []
    for n in (12, 30):
        F = 3 * n
        m = rng.uniform(0.0, 0.5, (F, len(pairs)))
        s1 = m * rng.uniform(0, n - 1, (F, len(pairs)))  # random heads: a random place of the text every frame
        m[:, planted] = rng.uniform(0.3, 0.5, F)
        s1[:, planted] = m[:, planted] * np.clip(np.arange(F) / 3.0 + rng.normal(0, 0.2, F), 0, n - 1)
        m[0] = -1.0
        runs.append({"pairs": pairs, "m": m, "s1": s1, "n_tokens": n})
    ranked = align.rank_heads(runs)
    assert len(ranked) == len(pairs) and (ranked[0].layer, ranked[0].head) == pairs[planted]
    assert ranked[0].monotone > 0.6 and ranked[0].coverage > 0.9 and ranked[0].score > 2 * ranked[1].score
    assert all(0 <= r.monotone <= 1 and 0 <= r.coverage <= 1 for r in ranked)


# ------------------------------------------------------------------------------------------------ ABI
def test_the_header_the_table_and_the_version_agree():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "smoltts_hip.h").read_text(), flags=re.S)
    assert re.search(r"#define\s+SMOLTTS_ABI_VERSION\s+9\b", header) and abi.ABI_VERSION == 9
    assert re.search(r"#define\s+SMOLTTS_MAX_ALIGN_HEADS\s+16\b", header) and abi.MAX_ALIGN_HEADS == 16
    for name in ("smoltts_session_set_align_heads", "smoltts_session_set_slot_align", "smoltts_session_alignment",
                 "smoltts_session_align_bytes", "smoltts_session_graph_form", "smoltts_k_attention_align"):
        assert name in abi.SIGNATURES and re.search(r"\b" + name + r"\s*\(", header), name
    engine = (ROOT / "smoltts_amd" / "csrc" / "lm_engine.hip").read_text()
    assert re.search(r"constexpr int GRAPH_FORMS = 64;", engine)


# ------------------------------------------------------------------------------------------------ the route
class _FakeTTS:
    """The stand-in engine of tests/test_server_cpu.py with the alignment side of ``SmolTTS``: one frame per character."""
    sampling_rate = 24000

    def __init__(self, heads):
        self.alignment_heads = heads
        self.last_alignment = None
        self.calls = []

    def __call__(self, text, voice="heart", **kw):
        self.calls.append(kw)
        parse_request(text, **{k: v for k, v in kw.items() if k != "sampling"})  # refuses what the real front end refuses
        if len(text) > 1000:
            raise ValueError("prompt + max_new_tokens exceed max_seq_len")
        F = max(1, len(text))
        pcm = np.linspace(-0.5, 0.5, int(1920 * F / (kw.get("speed") or 1.0)), dtype=np.float32)
        self.last_alignment = None
        if kw.get("timestamps"):
            m = np.full(F, 0.5)
            ids = load_tokenizer().encode(text).ids
            self.last_alignment = align.align(text, ids, m, m * np.arange(F), load_tokenizer(), speed=kw.get("speed"),
                                              duration_s=pcm.size / 24000)
        return pcm


def _client(heads, settings=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    tts = _FakeTTS(heads)
    return TestClient(create_app(tts, settings)), tts


def test_with_timestamps_route_answers_elevenlabs_json():
    import base64

    client, tts = _client([(0, 1)])
    text = "héllo"
    r = client.post("/v1/text-to-speech/3/with-timestamps?output_format=pcm_24000", json={"text": text})
    assert r.status_code == 200 and r.headers["content-type"].startswith("application/json")
    j = r.json()
    assert set(j) == {"audio_base64", "alignment", "normalized_alignment"} and j["alignment"] == j["normalized_alignment"]
    al = j["alignment"]
    assert set(al) == {"characters", "character_start_times_seconds", "character_end_times_seconds"} and al["characters"] == list(text)
    st, en = al["character_start_times_seconds"], al["character_end_times_seconds"]
    assert len(st) == len(en) == len(text) and st[0] == 0.0 and en[-1] == pytest.approx(len(text) * 0.08)
    assert all(a <= b for a, b in zip(st, en)) and all(a <= b for a, b in zip(st, st[1:]))
    audio = base64.b64decode(j["audio_base64"])
    plain = client.post("/v1/text-to-speech/3?output_format=pcm_24000", json={"text": text})
    assert audio == plain.content and len(audio) == len(text) * 1920 * 2  # the blocking route's audio, in its format
    assert tts.calls[0].get("timestamps") is True and "timestamps" not in tts.calls[1]
    wav = client.post("/v1/text-to-speech/3/with-timestamps", json={"text": text}).json()
    assert base64.b64decode(wav["audio_base64"])[:4] == b"RIFF"
    fast = client.post("/v1/text-to-speech/3/with-timestamps", json={"text": text, "voice_settings": {"speed": 2.0}}).json()["alignment"]
    assert fast["character_end_times_seconds"][-1] == pytest.approx(len(text) * 0.04, abs=1e-3)
    assert client.post("/v1/text-to-speech/3/with-timestamps", json={}).status_code == 422


def test_with_timestamps_route_answers_501_without_heads_and_400_for_what_it_refuses():
    client, tts = _client(None)
    r = client.post("/v1/text-to-speech/3/with-timestamps", json={"text": "abc"})
    assert r.status_code == 501 and "smoltts_amd.align rank" in r.json()["detail"] and not tts.calls
    client, tts = _client(None, {"alignment_heads": [[2, 3]]})  # the server setting alone turns the route on
    assert client.post("/v1/text-to-speech/3/with-timestamps", json={"text": "abc"}).status_code == 200
    client, tts = _client([(0, 1)])
    for body, word in (({"text": "abc", "trim_silence": True}, "trim_silence"), ({"text": "abc", "max_pause_s": 0.5}, "max_pause_s"),
                       ({"text": "abc", "temperature": 0.8, "best_of": 2}, "best_of"), ({"text": "x" * 2000}, "max_seq_len")):
        r = client.post("/v1/text-to-speech/3/with-timestamps", json=body)
        assert r.status_code == 400 and word in r.json()["detail"], (body, r.status_code, r.text)
    # a server that trims by default refuses too (the body can switch the trim off); one that segments long texts speaks the
    # request as one utterance
    client, tts = _client([(0, 1)], {"trim_silence": True})
    assert client.post("/v1/text-to-speech/3/with-timestamps", json={"text": "abc"}).status_code == 400
    assert client.post("/v1/text-to-speech/3/with-timestamps", json={"text": "abc", "trim_silence": None}).status_code == 200
    client, tts = _client([(0, 1)], {"long_text": "segment"})
    assert client.post("/v1/text-to-speech/3/with-timestamps", json={"text": "One. Two."}).status_code == 200
    assert "segment" not in tts.calls[-1]
    assert client.post("/v1/text-to-speech/3", json={"text": "One. Two."}).status_code == 200 and "segment" in tts.calls[-1]


def test_the_server_setting_takes_pairs_only():
    from smoltts_amd.server.settings import ServerSettings

    assert ServerSettings(checkpoint_dir="x").alignment_heads is None
    assert ServerSettings(checkpoint_dir="x", alignment_heads=[[1, 2], [3, 4]]).alignment_heads == [(1, 2), (3, 4)]
    for bad in ([[1]], [[1, 2, 3]], "ab", [[i, 0] for i in range(17)]):
        with pytest.raises(ValueError):
            ServerSettings(checkpoint_dir="x", alignment_heads=bad)
