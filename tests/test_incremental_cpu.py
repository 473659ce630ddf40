"""Text fed in pieces (host side, no GPU): the incremental splitter against the whole-text split, the plan that grows, the
``stream-input`` route over a stand-in model, and the pool's forwarding of the text calls to a stand-in worker."""
import asyncio
import json
import random

import numpy as np
import pytest

from smoltts_amd.longform import SegmentOptions, SegmentPlan, split_text

TAGS = ['<break time="0.5s"/>', "<break time='250ms' />", '<BREAK  time = "1s" >', '<break time=".2s"/>', '<break\ttime="0.05s"/ >']
NOT_TAGS = ['<break time="1."/>', "<brea k", "< b", "<break time='1s\"/>", "<break time=\"1s\"", "<breaktime='1s'/>", "a<b>c"]
MARKS = [". ", "! ", "? ", ", ", "; ", ".", '." ', "…) ", "?!» ", "\n", " ", "  ", " : ", "\n\n"]
WIDE = ["é", "ß", "漢字", "🙂", "—", "…", " "]


def _text(rng: random.Random) -> str:
    out = []
    for _ in range(rng.randint(1, 40)):
        r = rng.random()
        if r < 0.45:
            out.append("".join(rng.choice("abcdefg hij") for _ in range(rng.randint(1, 12))))
        elif r < 0.65:
            out.append(rng.choice(MARKS))
        elif r < 0.75:
            out.append(rng.choice(WIDE))
        elif r < 0.85:
            out.append(rng.choice(TAGS))
        elif r < 0.90:
            out.append(rng.choice(NOT_TAGS))
        else:  # a sentence (or a word) longer than the cap
            out.append(" ".join("x" * rng.randint(3, 60) + rng.choice(["", ",", ";"]) for _ in range(rng.randint(1, 8))))
    return "".join(out)


def _fed(text: str, cuts, opts, as_bytes=True):
    """(what the feeds returned, what close returned) for ``text`` cut at the byte positions ``cuts``."""
    from smoltts_amd.longform import IncrementalSplitter

    sp = IncrementalSplitter(opts)
    data = text.encode("utf-8")
    got, prev = [], 0
    for c in list(cuts) + [len(data)]:
        piece = data[prev:c]
        got += sp.feed(piece if as_bytes else piece.decode("utf-8"))
        prev = c
    return got, sp.close()


@pytest.mark.parametrize("block", range(4))
def test_splitter_matches_the_whole_text_split_however_the_text_is_cut(block):
    n_long = n_tagged = n_early = 0
    for seed in range(block * 75, block * 75 + 75):  # 300 texts in all
        rng = random.Random(seed)
        text = _text(rng)
        max_bytes = rng.choice([4, 16, 40, 300, 300])
        opts = SegmentOptions(max_bytes=max_bytes)
        want = split_text(text, max_bytes)
        plan = SegmentPlan.create(text, opts) if want else None
        if plan is not None:
            assert list(plan.segs) == want
        data = text.encode("utf-8")
        n_long += any(len(s.encode()) > 300 for s in text.replace("\n", ". ").split(". "))
        n_tagged += any(s.pause_after_s is not None or s.pause_before_s for s in want)
        for cuts in (range(1, len(data)),                                                       # one byte at a time
                     sorted(rng.sample(range(len(data) + 1), min(len(data) + 1, rng.randint(0, 8)))),  # a few cuts anywhere
                     []):                                                                       # in one piece
            fed, rest = _fed(text, cuts, opts)
            assert fed + rest == want, (seed, text, max_bytes, list(cuts))
            n_early += len(fed)
    assert n_tagged > 10 and n_early > 100 and (block or n_long)


def test_splitter_takes_str_pieces_and_cut_characters():
    text = "Zoë aß 漢字. Noch 🙂 eins! Und <break time=\"0.5s\"/> Schluß"
    opts = SegmentOptions(max_bytes=16)
    want = split_text(text, 16)
    data = text.encode("utf-8")
    for cuts in ([5], [9, 10, 11], list(range(1, len(data)))):
        fed, rest = _fed(text, cuts, opts)
        assert fed + rest == want
    chars = [len(text[:i].encode("utf-8")) for i in range(1, len(text))]
    fed, rest = _fed(text, chars, opts, as_bytes=False)
    assert fed + rest == want


def test_splitter_returns_a_sentence_before_the_text_ends():
    from smoltts_amd.longform import IncrementalSplitter

    first, second = "The first sentence is here.", "Another one follows it! And a third."
    sp = IncrementalSplitter(SegmentOptions(max_bytes=32))
    assert sp.feed(first) == [] and sp.feed(" ") == []    # the next sentence may still be packed with it
    got = sp.feed(second[:7])                              # "Another" cannot: sentence 1 is settled before close()
    assert [s.text for s in got] == [first] and got[0].pause_after_s is None
    got += sp.feed(second[7:]) + sp.close()
    assert got == split_text(f"{first} {second}", 32)
    # a break tag cut across two feeds is never half a tag, and the segment in front of it waits for the tags' sum
    sp = IncrementalSplitter(SegmentOptions(max_bytes=300))
    assert sp.feed('One. <break time="0.') == [] and sp.feed('5s"/> <break time=') == [] and sp.feed("'1s'/>") == []
    got = sp.feed(" T")
    assert got == [("One.", 1.5, 0.0)]
    assert got + sp.close() == split_text('One. <break time="0.5s"/> <break time=\'1s\'/> T', 300)
    with pytest.raises(ValueError, match="break time"):
        IncrementalSplitter(SegmentOptions()).feed('a <break time="4s"/>')
    sp = IncrementalSplitter(SegmentOptions())
    sp.close()
    with pytest.raises(ValueError, match="closed"):
        sp.feed("more")
    # flush speaks the remainder now: not the whole text's split
    sp = IncrementalSplitter(SegmentOptions(max_bytes=300))
    assert sp.feed("An unfinished") == [] and [s.text for s in sp.flush()] == ["An unfinished"]
    assert [s.text for s in sp.feed(" sentence.") + sp.close()] == ["sentence."]


def test_growing_plan_opens_segments_as_the_whole_text_plan_once_closed():
    from smoltts_amd.longform import GrowingPlan, IncrementalSplitter
    from smoltts_amd.seam import FINAL, FIRST, pause_samples

    text = '<break time="1s"/>The first sentence is here. A second one follows it! <break time="0.5s"/> And a third. <break time="2s"/>'
    opts = SegmentOptions(max_bytes=40, pause_s=0.2)
    whole = SegmentPlan.create(text, opts)
    sp, plan = IncrementalSplitter(opts), GrowingPlan(opts)
    tag, third = text.index('<break time="0.5'), text.index("And a third") + 5
    plan.extend(sp.feed(text[:tag]))
    assert len(plan.segs) == 1 and not plan.final(0)
    assert plan.seam_args(0) == (pause_samples(0.2), FIRST, pause_samples(1.0)) == whole.seam_args(0)
    plan.extend(sp.feed(text[tag:third]))
    assert len(plan.segs) == 2 and plan.seam_args(1) == whole.seam_args(1)
    plan.extend(sp.feed(text[third:]) + sp.close())
    assert plan.seam_args(2) == (pause_samples(2.0), 0, pause_samples(1.0))  # not closed yet: a seam with its tags' pause
    plan.close()
    assert plan.final(2) and [plan.seam_args(k) for k in range(3)] == [whole.seam_args(k) for k in range(3)]
    assert plan.seam_args(2)[1] == FINAL
    with pytest.raises(ValueError):
        plan.extend([])


def test_settings_carry_the_incremental_timeouts():
    from smoltts_amd.server.settings import ServerSettings

    st = ServerSettings(checkpoint_dir="/ckpt")
    assert st.idle_timeout_s == 10.0 and st.flush_after_s is None
    assert ServerSettings(checkpoint_dir="/ckpt", idle_timeout_s=2, flush_after_s=0.4).flush_after_s == 0.4
    with pytest.raises(ValueError):
        ServerSettings(checkpoint_dir="/ckpt", idle_timeout_s=0)


# ---------------------------------------------------------------------------------------------- the stream-input route
def _ndjson(*objs) -> bytes:
    return b"".join(json.dumps(o).encode() + b"\n" for o in objs)


@pytest.fixture()
def served():
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    from incremental_helpers import PullingTTS

    from smoltts_amd.server.app import create_app

    model = PullingTTS()
    return TestClient(create_app(model, {"segment_max_bytes": 120, "seam_pause_ms": 100})), model


def test_route_reads_its_options_from_the_first_line(served):
    client, model = served
    body = _ndjson({"seed": 7, "temperature": 0.5, "voice_settings": {"speed": 1.25}, "loudness": -20.0},
                   {"text": "Hello th"}, {"text": "ere. More"}, {"flush": True}, {"text": " text."})
    r = client.post("/v1/text-to-speech/nova/stream-input?output_format=pcm_16000", content=body)
    assert r.status_code == 200 and r.headers["x-sample-rate"] == "16000" and r.headers["x-seed"] == "7"
    got = np.frombuffer(r.content, np.float32).reshape(-1, 4)
    assert got[:, 0].tolist() == [1, 2, 3, 4] and got[:, 1].tolist() == [8, 9, 0, 6] and got[:, 2].tolist() == [0, 0, 1, 0]
    call = model.calls[0]
    assert call["voice"] == "nova" and call["output_format"] == "pcm_16000" and call["speed"] == 1.25 and call["loudness"] == -20.0
    assert call["sampling"].seed == 7 and call["sampling"].temperature == 0.5
    assert call["segment"] == {"max_bytes": 120, "pause_s": 0.1}
    r = client.post("/v1/text-to-speech/nova/stream-input", content=_ndjson({}, {"text": "Plain."}))  # no options, no last newline needed
    assert r.status_code == 200 and r.headers["x-sample-rate"] == "24000" and "x-seed" not in r.headers
    assert set(model.calls[1]) == {"voice", "segment"}
    r = client.post("/v1/text-to-speech/nova/stream-input", content=b'{}\n{"text": "no newline"}')
    assert r.status_code == 200 and np.frombuffer(r.content, np.float32)[1] == 10


def test_route_refuses_bad_lines(served):
    client, model = served
    post = lambda body, q="": client.post("/v1/text-to-speech/nova/stream-input" + q, content=body)
    assert post(b"").status_code == 422                                              # no first line
    assert post(b"not json\n").status_code == 422
    assert post(_ndjson({"voice_settings": {"speed": 9}}, {"text": "x"})).status_code == 422   # as the /stream body
    assert post(_ndjson({"seed": -1})).status_code == 422
    assert post(_ndjson([1, 2])).status_code == 422
    assert post(_ndjson({}), "?output_format=mp3_44100").status_code == 422
    assert post(_ndjson({"loudness": -90.0}, {"text": "x"})).status_code == 400       # options the engine refuses, as on /stream
    assert not model.calls
    # behind the first line: a line that is not JSON, or not a text or a flush, before any audio has gone out
    for bad in (b'{"text": 5}\n', b"{oops\n", b'{"flush": false}\n', b'{"text": "a", "flush": true}\n'):
        r = post(_ndjson({}) + bad)
        assert r.status_code == 422 and "line 2" in r.json()["detail"], bad
    r = post(_ndjson({}, {"text": 'a <break time="9s"/>'}))  # text the engine refuses: the stream never started
    assert r.status_code in (400, 422)


def _asgi_stream_input(app, parts, wait_for_audio_before):
    """POST ``parts`` (bytes) to the stream-input route over ASGI, holding back ``parts[wait_for_audio_before:]`` until a chunk
    of audio has come out.  Returns (status, what had been received when the first audio went out, all audio)."""
    sent = {"status": None, "audio": b"", "parts_at_first_audio": None}
    given = 0
    audio_out = asyncio.Event()

    async def receive():
        nonlocal given
        if given == wait_for_audio_before:
            await asyncio.wait_for(audio_out.wait(), timeout=20)
        if given < len(parts):
            given += 1
            return {"type": "http.request", "body": parts[given - 1], "more_body": given < len(parts)}
        await asyncio.sleep(3600)

    async def send(msg):
        if msg["type"] == "http.response.start":
            sent["status"] = msg["status"]
        elif msg["type"] == "http.response.body" and msg.get("body"):
            if sent["parts_at_first_audio"] is None:
                sent["parts_at_first_audio"] = given
            sent["audio"] += msg["body"]
            audio_out.set()

    scope = {"type": "http", "asgi": {"version": "3.0"}, "http_version": "1.1", "method": "POST", "scheme": "http",
             "path": "/v1/text-to-speech/nova/stream-input", "raw_path": b"/v1/text-to-speech/nova/stream-input",
             "query_string": b"", "root_path": "", "headers": [(b"host", b"test"), (b"content-type", b"application/x-ndjson")],
             "client": ("test", 1), "server": ("test", 80)}
    asyncio.run(asyncio.wait_for(app(scope, receive, send), timeout=30))
    return sent["status"], sent["parts_at_first_audio"], sent["audio"]


def test_route_speaks_while_the_body_is_still_arriving():
    from incremental_helpers import PullingTTS

    from smoltts_amd.server.app import create_app

    app = create_app(PullingTTS(), None)
    parts = [_ndjson({}), _ndjson({"text": "A first sentence. "}), _ndjson({"text": "The rest of it"}), _ndjson({"text": " comes later."})]
    status, at_first, audio = _asgi_stream_input(app, parts, wait_for_audio_before=2)
    assert status == 200 and at_first == 2  # audio went out with half of the body still to come
    got = np.frombuffer(audio, np.float32).reshape(-1, 4)
    assert got[:, 0].tolist() == [1, 2, 3] and got[:, 1].tolist() == [18, 14, 13]
    # a bad line behind the first audio cannot be answered any more: the stream ends
    status, at_first, audio = _asgi_stream_input(app, [_ndjson({}), _ndjson({"text": "Good."}), b"{bad\n", _ndjson({"text": "never"})], 2)
    assert status == 200 and at_first == 2 and np.frombuffer(audio, np.float32).reshape(-1, 4)[:, 1].tolist() == [5]


# ---------------------------------------------------------------------------------------------- the pool
def test_pool_forwards_the_text_calls_to_the_owning_worker():
    from incremental_helpers import make_echo_incremental

    from smoltts_amd.server.pool import GpuPool

    pool = GpuPool(make_echo_incremental, devices=[0, 1], respawn=False)
    try:
        a = pool.submit_incremental("nova", output_format="pcm_16000", speed=1.5, idle_timeout_s=3.0)
        b = pool.submit_incremental("sky")
        assert {a.worker, b.worker} == {0, 1}
        a.feed("Hello")
        b.feed("xy")
        a.flush()
        a.feed(" there.")
        a.close()
        got = np.stack(list(a))
        # voice length and the options that travelled (format, speed, segment, idle timeout), then one answer per call, in order
        assert got.tolist() == [[4, 4], [1, 5], [2, 0], [3, 7], [4, 0]]
        with pytest.raises(ValueError):
            a.feed("too late")
        chunks = pool.iter_chunks(b)
        assert [next(chunks).tolist(), next(chunks).tolist()] == [[3, 2], [1, 2]]
        b.cancel()  # reaches the worker's scheduler, which ends the stream
        assert list(chunks) == []
        c = pool.submit_incremental("sky")
        c.feed("__bad__")  # the worker's scheduler refuses the text: the stream ends with its ValueError
        with pytest.raises(ValueError, match="bad break tag"):
            list(c)
        with pytest.raises(ValueError):
            pool.submit_incremental("sky", speed=9.0)  # refused here, before a worker sees it
        assert pool.loads() == [0, 0]
    finally:
        pool.close()
