"""The host side of forced alignment (smoltts_amd/align.py ``recording_grid`` / ``recording``), every refusal
of the front ends, the route with a stand-in engine and the ABI table, without a GPU."""
import base64
import re
import struct

import numpy as np
import pytest

from smoltts_amd import abi, align
from smoltts_amd.config import TokenConfig
from smoltts_amd.prompt import PromptEncoder
from smoltts_amd.synthetic import named_config
from smoltts_amd.tokenizer import load_tokenizer
from test_host_cpu import ROOT


def _parts(cfgname):
    cfg = named_config(cfgname)
    tok = load_tokenizer(None, cfg.codebook_size)
    tc = TokenConfig.from_tokenizer(tok, cfg)
    return cfg, tok, tc, PromptEncoder.from_config(tok, cfg, tc)


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("cfgname,height", [("tiny", 9), ("tiny_nodup", 8)])
def test_the_grid_the_frame_map_and_the_targets(cfgname, height):
    cfg, tok, tc, enc = _parts(cfgname)
    rng = np.random.default_rng(3)
    text, F = "Hé, a text.", 7
    codes = rng.integers(0, cfg.codebook_size, size=(8, F))
    rg = align.recording_grid(enc, tok, tc, text, codes, "sky")
    prompt = enc.build_prompt(text, "sky")
    a0 = prompt.shape[1]
    assert rg.a0 == a0 and rg.n_frames == F and rg.grid.shape == (height, a0 + F) and rg.grid.dtype == np.int32
    assert np.array_equal(rg.grid[:, :a0], prompt)
    # the audio columns are those of encode_vq without its closing turn: the slow id, then the depth rows
    assert np.array_equal(rg.grid[:, a0:], enc.encode_vq(codes)[:, :F])
    assert np.array_equal(rg.grid[0, a0:], codes[0] + tc.semantic_start_id)
    assert np.array_equal(rg.grid[1:, a0:], codes if cfgname == "tiny" else codes[1:])
    assert rg.grid[0, a0 - 1] == tok.token_to_id("\n")  # the assistant header's last token produces frame 0
    # row a0 - 1 + f produces frame f and should emit the slow id of column a0 + f; the last audio column should emit <|im_end|>
    want_f = np.full(a0 + F, -1)
    want_f[a0 - 1: a0 - 1 + F] = np.arange(F)
    assert np.array_equal(rg.frame_of_row, want_f) and rg.frame_of_row[rg.end_row] == -1
    assert (rg.targets[:a0 - 1] == -1).all()
    assert np.array_equal(rg.targets[a0 - 1: a0 - 1 + F], rg.grid[0, a0:])
    assert rg.end_row == a0 + F - 1 and rg.targets[rg.end_row] == tc.im_end_id
    # the window is the transcript's tokens in the user turn
    t0, t1 = rg.window
    assert (t0, t1) == align.window_of(prompt[0], tok) and t1 - t0 == len(text)  # (this vocabulary: a token per latin-1 character)
    assert align.token_spans(text, rg.grid[0, t0:t1], tok)[-1][1] == t1 - t0


def test_a_cloned_speakers_turns_stand_in_front():
    cfg, tok, tc, enc = _parts("tiny")
    rng = np.random.default_rng(4)
    speaker = np.concatenate([enc.encode_text_turn("user", "a sample"), enc.encode_vq(rng.integers(0, 2048, size=(8, 5)))], axis=1)
    rg = align.recording_grid(enc, tok, tc, "mine", rng.integers(0, 2048, size=(8, 3)), "cv_x", speaker)
    P = speaker.shape[1]
    assert np.array_equal(rg.grid[:, :P], speaker) and rg.window[0] > P and rg.window[1] - rg.window[0] == 4  # the last user turn


# ------------------------------------------------------------------------------------------------ words and scores
def _planted(text, per_char, tok, heads=2, seed=1):
    cfg, _tok, tc, enc = _parts("tiny")
    F = per_char * len(text)
    rng = np.random.default_rng(seed)
    rg = align.recording_grid(enc, tok, tc, text, rng.integers(0, 2048, size=(8, F)), "sky")
    at = np.repeat(np.arange(len(text)), per_char)
    m = rng.uniform(0.3, 0.6, (F, heads))
    rows = np.stack([m, m * at[:, None]], axis=2).astype(np.float32)
    lp = np.full(rg.grid.shape[1], np.nan, np.float32)
    lp[rg.a0 - 1: rg.a0 - 1 + F] = -(1.0 + at)  # frame f of character c scores -(1 + c)
    lp[rg.end_row] = -0.25
    return rg, rows, lp


def test_words_and_their_loss_on_a_planted_diagonal():
    tok = load_tokenizer(None, 2048)
    text, per = "ab  cde f", 4
    rg, rows, lp = _planted(text, per, tok)
    ra = align.recording(text, rg, rows, lp, tok)
    F = per * len(text)
    a = ra.alignment
    assert a.characters == list(text) and a.start_s[0] == 0.0 and a.end_s[-1] == pytest.approx(F * align.FRAME_S)
    assert np.allclose(a.start_s, np.arange(len(text)) * per * align.FRAME_S, atol=0.5 * align.FRAME_S + 1e-9)
    assert [w.text for w in ra.words] == ["ab", "cde", "f"]
    starts = {"ab": 0, "cde": 4, "f": 8}
    for w in ra.words:
        i, j = starts[w.text], starts[w.text] + len(w.text)
        assert w.start == a.start_s[i] and w.end == a.end_s[j - 1] and w.start < w.end
        centres = (np.arange(F) + 0.5) * align.FRAME_S
        inside = (centres >= w.start) & (centres < w.end)
        assert inside.sum() >= per * len(w.text) - 1
        assert w.loss == pytest.approx(float(-lp[rg.a0 - 1: rg.a0 - 1 + F].astype(np.float64)[inside].mean()))
        assert 1 + i - 0.5 <= w.loss <= j + 0.5  # the mean of the planted scores of its own characters, to within a frame
    assert ra.logprobs.shape == (F,) and ra.logprobs.dtype == np.float32 and ra.end_logprob == -0.25
    assert ra.loss == pytest.approx(float(np.mean(1.0 + np.repeat(np.arange(len(text)), per))))  # <|im_end|>'s score stays out
    # a word no frame's centre falls into has no loss
    short = align.Alignment(list("a b"), [0.0, 0.01, 0.01], [0.01, 0.01, 0.16], np.zeros(2), np.zeros(2))
    ws = align.words_of(short, np.asarray([-1.0, -3.0], np.float32))
    assert [(w.text, w.loss) for w in ws] == [("a", None), ("b", 2.0)]


def test_to_json_is_the_forced_alignment_shape():
    tok = load_tokenizer(None, 2048)
    text = "two words"
    rg, rows, lp = _planted(text, 3, tok)
    j = align.recording(text, rg, rows, lp, tok).to_json()
    assert set(j) == {"characters", "words", "loss"} and isinstance(j["loss"], float)
    assert [c["text"] for c in j["characters"]] == list(text) and all(set(c) == {"text", "start", "end"} for c in j["characters"])
    assert [w["text"] for w in j["words"]] == ["two", "words"] and all(set(w) == {"text", "start", "end", "loss"} for w in j["words"])
    assert all(isinstance(c["start"], float) and isinstance(c["end"], float) for c in j["characters"])
    import json

    json.dumps(j)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_host_model():
    cfg, tok, tc, enc = _parts("tiny")
    codes = np.zeros((8, 4), np.int64)
    for bad in ("", "   ", None):
        with pytest.raises(ValueError, match="text"):
            align.recording_grid(enc, tok, tc, bad, codes)
    with pytest.raises(ValueError, match="full frame"):
        align.recording_grid(enc, tok, tc, "x", np.zeros((8, 0), np.int64))
    assert align.recording_limit_frames(40, 512, 1000) == 512 - 1 - 40 and align.recording_limit_frames(40, 512, 13) == 13
    assert align.recording_limit_frames(600, 512, 13) == 0
    align.check_recording_fits(40, 471, 512, 1000)
    with pytest.raises(ValueError, match=r"has 37\.76 s.*allows 37\.68 s"):
        align.check_recording_fits(40, 472, 512, 1000)
    with pytest.raises(ValueError, match=r"allows 1\.04 s"):
        align.check_recording_fits(40, 14, 512, 13)
    assert "align rank" in str(align.no_heads_error())


def test_the_facade_refuses_before_it_touches_the_gpu():
    from smoltts_amd import SmolTTS

    cfg, tok, tc, enc = _parts("tiny")
    tts = SmolTTS.__new__(SmolTTS)
    tts.alignment_heads, tts.voices, tts.config, tts.prompt_encoder, tts.tokenizer, tts.token_config = [], {}, cfg, enc, tok, tc
    pcm = np.zeros(1920 * 3, np.float32)
    with pytest.raises(ValueError, match="align rank"):
        tts.align_recording(pcm, "hello")
    tts.alignment_heads = [(0, 1)]
    with pytest.raises(ValueError, match="text"):
        tts.align_recording(pcm, "")
    with pytest.raises(ValueError, match="full frame"):
        tts.align_recording(pcm[:1919], "hello")
    with pytest.raises(ValueError, match="full frame"):
        tts.align_recording(np.zeros(900, np.float32), "hello", rate=12000)  # 1800 samples at the codec's rate
    with pytest.raises(ValueError, match=r"allows \d+\.\d\d s \(max_seq 512"):
        tts.align_recording(np.zeros(1920 * 512, np.float32), "hello")
    with pytest.raises(ValueError, match="max_frames 5"):
        tts.recording_grid(np.zeros(1920 * 6, np.float32), "hello", max_frames=5)


def test_the_pool_refuses_before_a_worker_sees_the_request():
    from smoltts_amd.server.pool import GpuPool

    pool = GpuPool.__new__(GpuPool)
    pool.alignment_heads = []

    def unreachable(*a, **k):
        raise AssertionError("a worker was asked")

    pool._pick_worker = pool._control = unreachable
    pcm = np.zeros(1920 * 2, np.float32)
    with pytest.raises(ValueError, match="align rank"):
        pool.align_recording(pcm, "hello")
    pool.alignment_heads = [(0, 1)]
    with pytest.raises(ValueError, match="text"):
        pool.align_recording(pcm, " ")
    with pytest.raises(ValueError, match="full frame"):
        pool.align_recording(pcm[:100], "hello")


def test_the_rank_tool_takes_recordings_or_texts(capsys):
    assert align.main(["rank", "--checkpoint", "nowhere"]) == 2
    assert "--texts FILE or --recordings FILE" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the route
def _wav16(pcm, rate=24000):
    data = (np.clip(np.asarray(pcm), -1, 1) * 32767).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + \
        b"data" + struct.pack("<I", len(data)) + data


class _FakeTTS:
    """A stand-in engine with the forced-alignment side of ``SmolTTS``: the characters share the recording evenly."""

    def __init__(self, heads, limit_frames=50):
        self.alignment_heads, self.limit, self.calls = heads, limit_frames, []

    def align_recording(self, audio, text, voice="heart", speaker=None, rate=24000):
        self.calls.append((len(audio), text, voice, rate))
        if not self.alignment_heads:
            raise align.no_heads_error()
        if not text.strip():
            raise ValueError("forced alignment needs a text")
        F = len(audio) * 24000 // rate // 1920
        if F < 1:
            raise ValueError("the audio holds no full frame (1920 samples at 24 kHz)")
        align.check_recording_fits(0, F, self.limit + 1, 1 << 30)
        edges = np.linspace(0.0, F * align.FRAME_S, len(text) + 1)
        al = align.Alignment(list(text), list(edges[:-1]), list(edges[1:]))
        lp = -np.arange(1, F + 1, dtype=np.float32)
        return align.RecordingAlignment(al, align.words_of(al, lp), lp, -0.5, float(-lp.mean()))


def test_the_route_answers_the_json_and_its_refusals():
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    fake = _FakeTTS([(0, 1)])
    client = TestClient(create_app(fake, {}))
    pcm = np.linspace(-0.5, 0.5, 1920 * 6 + 5)
    body = {"audio": base64.b64encode(_wav16(pcm, 24000)).decode("ascii"), "text": "hi there"}
    r = client.post("/v1/forced-alignment", json=body)
    assert r.status_code == 200, r.text
    j = r.json()
    assert set(j) == {"characters", "words", "loss"} and [c["text"] for c in j["characters"]] == list("hi there")
    assert [w["text"] for w in j["words"]] == ["hi", "there"] and j["loss"] == pytest.approx(3.5)
    assert j["characters"][-1]["end"] == pytest.approx(6 * 0.08) and j["words"][0]["start"] == 0.0
    assert fake.calls[-1][1:] == ("hi there", "heart", 24000)
    r = client.post("/v1/forced-alignment", json=dict(body, voice="sky", audio=base64.b64encode(_wav16(pcm[::3], 8000)).decode("ascii")))
    assert r.status_code == 200 and fake.calls[-1][2:] == ("sky", 8000)  # the rates of /v1/voices/add
    # 400: what the call refuses, and audio that cannot be read
    for bad in (dict(body, text="  "), dict(body, audio="!!"), dict(body, audio=base64.b64encode(b"RIFFxxxxWAVE").decode("ascii")),
                dict(body, audio=base64.b64encode(_wav16(pcm[:500])).decode("ascii")),
                dict(body, audio=base64.b64encode(_wav16(np.zeros(1920 * 51))).decode("ascii")),
                dict(body, audio=base64.b64encode(_wav16(pcm, 11025)).decode("ascii"))):
        r = client.post("/v1/forced-alignment", json=bad)
        assert r.status_code == 400, (r.status_code, r.text)
    assert "allows 4.00 s" in client.post("/v1/forced-alignment", json=dict(
        body, audio=base64.b64encode(_wav16(np.zeros(1920 * 51))).decode("ascii"))).json()["detail"]
    assert client.post("/v1/forced-alignment", json={"text": "x"}).status_code == 422  # no audio at all
    # 501 without heads, in the with-timestamps route's words
    bare = TestClient(create_app(_FakeTTS([]), {}))
    r = bare.post("/v1/forced-alignment", json=body)
    assert r.status_code == 501 and "align rank" in r.json()["detail"]
    assert r.json()["detail"] == bare.post("/v1/text-to-speech/sky/with-timestamps", json={"text": "x"}).json()["detail"]


# ------------------------------------------------------------------------------------------------ ABI
def test_the_header_the_table_and_the_version_agree():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "smoltts_hip.h").read_text(), flags=re.S)
    assert re.search(r"#define\s+SMOLTTS_ABI_VERSION\s+9\b", header) and abi.ABI_VERSION == 9
    for name, kinds in (("smoltts_lm_measure_rows", "p p p p p p i p p"), ("smoltts_k_score_rows", "p i i q p p p")):
        assert name in abi.SIGNATURES and abi.SIGNATURES[name][1] == kinds and re.search(r"\b" + name + r"\s*\(", header), name
    engine = (ROOT / "smoltts_amd" / "csrc" / "lm_engine.hip").read_text()
    assert re.search(r"constexpr int GRAPH_FORMS = 64;", engine) and "smoltts_lm_measure_rows" in engine
    from smoltts_amd import lm, ops

    assert callable(ops.score_rows) and callable(lm.LMSession.measure_rows) and callable(lm.LMSession.iter_measure_rows)
