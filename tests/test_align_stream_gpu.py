"""The causal fit kernel (csrc/align_fit.hip) against its numpy model (align.StreamFit), bit for bit: planted rows, no LM."""
import numpy as np
import pytest

import align_stream_helpers as hp

pytestmark = pytest.mark.gpu

B, MAX_FRAMES, MAX_TOKENS = 3, 40, 320
OFFERED = 48  # the counters run past max_frames: those frames are ignored
INPUTS = {"ramp": lambda H, n: hp.ramp(MAX_FRAMES, H, max(n, 2)), "outlier": lambda H, n: hp.ramp(MAX_FRAMES, H, max(n, 2), outlier=True),
          "gaps": lambda H, n: hp.gaps(MAX_FRAMES, H, max(n, 2)), "weightless": lambda H, n: hp.weightless(MAX_FRAMES, H)}


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def fitter(torch):
    from smoltts_amd.lm import AlignFitter

    f = AlignFitter(torch.device("cuda"), B, MAX_FRAMES, MAX_TOKENS)
    yield f
    f.close()


def _device_rows(torch, per_slot, H):
    rows = np.zeros((B, MAX_FRAMES, H, 2), np.float32)
    for b, ms in per_slot.items():
        rows[b, :, :, 0], rows[b, :, :, 1] = ms
    return torch.from_numpy(rows).cuda()


def _read(torch, fitter):
    torch.cuda.synchronize()
    return fitter.starts.cpu().numpy(), fitter.committed.cpu().numpy()


def _expected(m, s1, n, lag, shown, ended, cache):
    """The model's starts after the slot has been shown ``shown`` frames (``ended``: and has finished there)."""
    key = (n, lag)
    if key not in cache:
        cache[key] = hp.model_trace(m, s1, n, lag)[0]
    trace = cache[key]
    F = min(shown, MAX_FRAMES)
    if ended:
        sf = hp.align.StreamFit(n, lag)
        for f in range(F):
            sf.push(m[f], s1[f])
        return sf.finish(F)
    return trace[F - 1] if F > 0 else np.zeros(1 if n > 0 else 0)


@pytest.mark.parametrize("H", [1, 4, 16])
@pytest.mark.parametrize("name", list(INPUTS))
def test_kernel_equals_model_after_every_call(torch, fitter, name, H):
    n_frames = torch.zeros(B, dtype=torch.int32, device="cuda")
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    for n in (0, 1, 12, 300):
        m, s1 = INPUTS[name](H, n)
        m2, s2 = hp.noisy(7, MAX_FRAMES, H, max(n, 2))  # the second tenant of slot 2
        for lag in (1, 6, 64):
            caches = ({}, {}, {})
            finals = []
            for step in (1, 4, 8, OFFERED):
                rows = _device_rows(torch, {0: (m, s1), 1: (m, s1), 2: (m, s1)}, H)
                n_frames.zero_()
                fitter.reset_slots([0, 1, 2], [n, None, 12], [lag, lag, lag], [MAX_FRAMES] * 3)
                second = False  # slot 2 starts over with another text half way
                shown2 = 0
                for shown in range(step, OFFERED + 1, step):
                    if not second and shown > OFFERED // 2:
                        second = True
                        shown2 = 0
                        rows[2, :, :, 0], rows[2, :, :, 1] = torch.from_numpy(m2).cuda(), torch.from_numpy(s2).cuda()
                        fitter.reset_slots([2], [n], [lag], [MAX_FRAMES])
                    shown2 = shown2 + step if second else shown
                    n_frames.copy_(torch.tensor([shown, shown, shown2], dtype=torch.int32))
                    fitter.push(rows, n_frames, done)
                    starts, committed = _read(torch, fitter)
                    want0 = _expected(m, s1, n, lag, shown, shown >= MAX_FRAMES, caches[0])
                    want2 = (_expected(m2, s2, n, lag, shown2, shown2 >= MAX_FRAMES, caches[2]) if second
                             else _expected(m, s1, 12, lag, shown2, shown2 >= MAX_FRAMES, caches[1]))
                    where = f"{name} H={H} n={n} lag={lag} step={step} shown={shown}"
                    assert committed[0] == want0.size and committed[2] == want2.size and committed[1] == 0, where
                    assert np.array_equal(starts[0, :want0.size].view(np.int64), want0.view(np.int64)), where
                    assert np.array_equal(starts[2, :want2.size].view(np.int64), want2.view(np.int64)), where + " (slot 2)"
                assert committed[0] == n
                finals.append(starts[0, :n].copy())
            for f in finals[1:]:  # the same bits however the calls cut the frames
                assert np.array_equal(f.view(np.int64), finals[0].view(np.int64)), f"{name} H={H} n={n} lag={lag}"


def test_done_flag_ends_the_stream_at_its_frames(torch, fitter):
    """A slot that stops with 25 frames finishes at F = 25; a budget of 30 ends another at 30; both keep their bits afterwards."""
    H, n, lag = 4, 12, 6
    m, s1 = hp.gaps(MAX_FRAMES, H, n)
    rows = _device_rows(torch, {0: (m, s1), 2: (m, s1)}, H)
    fitter.reset_slots([0, 1, 2], [n, None, n], [lag] * 3, [MAX_FRAMES, MAX_FRAMES, 30])
    n_frames = torch.tensor([24, 24, 24], dtype=torch.int32, device="cuda")
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    fitter.push(rows, n_frames, done)
    starts, committed = _read(torch, fitter)
    want = _expected(m, s1, n, lag, 24, False, {})
    assert committed[0] == committed[2] == want.size < n and np.array_equal(starts[0, :want.size], want)
    n_frames.copy_(torch.tensor([25, 25, 32], dtype=torch.int32))
    done.copy_(torch.tensor([1, 1, 0], dtype=torch.int32))
    fitter.push(rows, n_frames, done)
    starts, committed = _read(torch, fitter)
    for b, F in ((0, 25), (2, 30)):
        want = _expected(m, s1, n, lag, F, True, {})
        assert committed[b] == n and np.array_equal(starts[b, :n].view(np.int64), want.view(np.int64)), b
    n_frames.copy_(torch.tensor([40, 40, 40], dtype=torch.int32))  # a finished slot is left alone
    fitter.push(rows, n_frames, done)
    again, _ = _read(torch, fitter)
    assert np.array_equal(again, starts)


def test_reset_refuses_bad_values(torch, fitter):
    from smoltts_amd.abi import SmolttsError

    for args in (([0], [MAX_TOKENS + 1], [6], [MAX_FRAMES]), ([0], [12], [0], [MAX_FRAMES]), ([0], [12], [65], [MAX_FRAMES]),
                 ([0], [12], [6], [MAX_FRAMES + 1]), ([0], [12], [6], [0]), ([B], [12], [6], [MAX_FRAMES])):
        with pytest.raises(SmolttsError):
            fitter.reset_slots(*args)
