"""The score of the slow pick and best_of, host side: the numpy model of the device's log-probability, the takes' seeds, the
ranking, every refusal, the route bodies and the C ABI's new exports."""
import re
from pathlib import Path

import numpy as np
import pytest

from smoltts_amd import abi
from smoltts_amd.config import (MAX_BEST_OF, GenerationSettings, RequestSampling, check_best_of, mean_logprob, rank_takes, take_sampling,
                                take_seed)
from smoltts_amd.sampling import LOGPROB_MARGIN, TOP_P_EDGE_MARGIN, length_patch, pick_logprob

ROOT = Path(__file__).resolve().parents[1]


def _log_softmax64(row, picked):
    """float64 log-softmax of the fp32-subtracted row (the model mirrors that subtract; everything behind it in float64)."""
    x = np.asarray(row, np.float32)
    z = (x - x.max()).astype(np.float32).astype(np.float64)
    return float(z[picked] - np.log(np.exp(z).sum()))


@pytest.mark.parametrize("n", [5, 1028, 2052, 65836])
@pytest.mark.parametrize("scale", [0.01, 1.0, 30.0, 1e4])
def test_model_against_float64_log_softmax(n, scale):
    rng = np.random.default_rng(n + int(scale * 100))
    for _ in range(4):
        row = (rng.standard_normal(n) * scale).astype(np.float32)
        for picked in (int(np.argmax(row)), int(rng.integers(n)), int(np.argmin(row))):
            got, want = pick_logprob(row, picked), _log_softmax64(row, picked)
            # fp32 exp of the model (as on the device) and the 2^-40 quantum against float64: within the margin; the result is fp32
            assert abs(got - want) <= LOGPROB_MARGIN + abs(want) * 2.0**-23, (n, scale, picked, got, want)


def test_edge_rows():
    assert LOGPROB_MARGIN == 1e-5 == TOP_P_EDGE_MARGIN
    for n in (1, 2, 5, 1000, 65836):
        assert abs(pick_logprob(np.full(n, 3.25, np.float32), n // 2) - (-np.log(n))) <= 1e-6  # a flat row
    row = np.zeros(1000, np.float32)
    row[17] = 50.0
    assert abs(pick_logprob(row, 17)) <= 1e-6  # one column 50 above the rest: about 0 ...
    lp = pick_logprob(row, 3)
    assert np.isfinite(lp) and abs(lp + 50.0) <= 1e-5  # ... and a column beyond |z| = 28 has mass 0 and still a finite score
    assert np.floor(np.exp(np.float32(-28.0)) * 2.0**40) == 0.0
    # a -inf column from a length block contributes nothing: the score of the rest is that of the row without the column
    row = (np.random.default_rng(3).standard_normal(64) * 2).astype(np.float32)
    blocked = length_patch(row, im_end=9, frame=0, min_frames=4)
    assert blocked[9] == -np.inf
    keep = [j for j in range(64) if j != 9]
    assert pick_logprob(blocked, 20) == pick_logprob(row[keep], keep.index(20))
    # the bias is part of the row the score sees
    biased = length_patch(row, im_end=9, frame=7, min_frames=4, eos_bias=3.5)
    assert biased[9] == np.float32(row[9] + np.float32(3.5)) and pick_logprob(biased, 9) > pick_logprob(row, 9)


def test_take_seeds_wrap():
    assert [take_seed(5, k) for k in range(3)] == [5, 6, 7]
    assert [take_seed(2**64 - 2, k) for k in range(4)] == [2**64 - 2, 2**64 - 1, 0, 1]
    base = RequestSampling(temperature=0.9, seed=2**64 - 1, best_of=3).resolve(GenerationSettings.greedy())
    assert base.best_of == 3 and base.takes == 3 and base.scored and not base.logprobs
    takes = [take_sampling(base, k) for k in range(3)]
    assert [t.seed for t in takes] == [2**64 - 1, 0, 1] and all(t.best_of is None and t.logprobs and t.takes == 1 for t in takes)
    assert all(t.temperature == base.temperature and t.eos_bias == base.eos_bias for t in takes)
    # best_of = 1 is the request without it
    one = RequestSampling(temperature=0.9, seed=4, best_of=1).resolve(GenerationSettings.greedy())
    assert one.takes == 1 and not one.scored
    # the two fields sit at the end with defaults: positional construction of the fields before them still works
    assert RequestSampling(0.5, 0.5, 0.0, 1, 1.0, 0, 1.0, 16, 0, 0.0) == RequestSampling(0.5, 0.5, 0.0, 1, 1.0, 0, 1.0, 16, 0, 0.0, False, None)


def test_ranking():
    assert rank_takes([("length", -1.0), ("stop", -9.0), ("stop", -2.0)]) == [2, 1, 0]  # stop beats length, then the higher mean
    assert rank_takes([("stop", -2.0), ("stop", -2.0), ("stop", -3.0)]) == [0, 1, 2]  # ties go to the lower k
    assert rank_takes([("length", -2.0), ("length", -1.0)]) == [1, 0]
    assert rank_takes([("stop", -1.0)]) == [0]
    assert mean_logprob(np.array([-1.0, -2.0, -4.5], np.float32)) == -2.5 and mean_logprob([]) == float("-inf")


def test_every_refusal_has_its_message():
    gs = GenerationSettings.greedy()
    ok = RequestSampling(temperature=0.9, seed=1, best_of=3).resolve(gs)
    check_best_of(ok, 3)
    check_best_of(RequestSampling(temperature=0.0, best_of=1).resolve(gs), 1, stream=True, segmented=True)  # one take: nothing to refuse
    with pytest.raises(ValueError, match="needs a blocking request"):
        check_best_of(ok, 8, stream=True)
    with pytest.raises(ValueError, match="segmented or incremental"):
        check_best_of(ok, 8, segmented=True)
    with pytest.raises(ValueError, match="sampled slow token"):
        check_best_of(RequestSampling(temperature=0.0, fast_temperature=0.8, best_of=2).resolve(gs), 8)
    with pytest.raises(ValueError, match="best_of=3 exceeds the 2 slots"):
        check_best_of(ok, 2)
    for bad in (0, -1, MAX_BEST_OF + 1, 2.0, True):
        with pytest.raises(ValueError, match="best_of must be an integer"):
            RequestSampling(best_of=bad)
    with pytest.raises(ValueError, match="logprobs must be true or false"):
        RequestSampling(logprobs=1)
    assert MAX_BEST_OF == 8 and RequestSampling(best_of=MAX_BEST_OF).takes == 8


def test_route_bodies_carry_the_two_fields():
    pytest.importorskip("fastapi")
    from pydantic import ValidationError

    from smoltts_amd.server.app import CreateSpeechRequest, SpeechRequest, TTSCore, _score_headers
    from smoltts_amd.server.settings import ServerSettings

    a = SpeechRequest(input="x", temperature=0.9, best_of=3).request_sampling()
    assert a.best_of == 3 and a.logprobs is False and a.scored
    b = CreateSpeechRequest(text="x", logprobs=True).request_sampling()
    assert b.logprobs is True and b.best_of is None
    assert SpeechRequest(input="x").request_sampling() is None
    with pytest.raises(ValidationError):
        SpeechRequest(input="x", best_of=0)
    with pytest.raises(ValidationError):
        SpeechRequest(input="x", best_of=9)
    assert ServerSettings.model_fields["max_best_of"].default == 4
    assert _score_headers({}) == {} and _score_headers({"mean_logprob": -1.23456, "best_of": 3}) == {"X-Mean-Logprob": "-1.2346", "X-Best-Of": "3"}
    core = TTSCore.__new__(TTSCore)
    core.settings = {"max_best_of": 2}
    core._check_best_of(RequestSampling(best_of=2))
    with pytest.raises(ValueError, match="max_best_of=2"):
        core._check_best_of(RequestSampling(best_of=3))
    with pytest.raises(ValueError, match="blocking"):
        core._check_best_of(RequestSampling(best_of=2), stream=True)


NEW_EXPORTS = ("smoltts_session_set_slot_score", "smoltts_session_logprobs", "smoltts_session_slow_logits", "smoltts_k_sample_rows_scored")


def test_header_exports_are_bound_and_the_abi_version_stays():
    header = (ROOT / "include" / "smoltts_hip.h").read_text()
    assert abi.ABI_VERSION == 9 and re.search(r"#define\s+SMOLTTS_ABI_VERSION\s+9\b", header)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in abi.SIGNATURES, name
        decl = header[header.index("int " + name + "("):]
        n_args = decl[:decl.index(");")].count(",") + 1
        assert len(abi.SIGNATURES[name][1].split()) == n_args, name
    assert header.count("(ABI 9, additive)") >= 4 + 2  # the four here beside the length control's two
