"""The limiter stage on the device against its numpy model (``smoltts_amd/limiter.py``), bit for bit: the stream kernel sample
for sample and state for state over ragged calls of three widths with ends and a restart, the whole-utterance entry at the
lengths around its window sizes, and the stage inside ``StreamConverter`` beside unlimited slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import engine, limiter as LM, tsm  # noqa: E402

from limiter_helpers import bits, driven  # noqa: E402


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _assert_state(dev_state, model, what):
    m = model.state()
    assert dev_state["on"] == 1, what
    assert (dev_state["pos"], dev_state["ended"]) == (m["pos"], m["ended"]), (what, dev_state["pos"], dev_state["ended"], m["pos"], m["ended"])
    assert dev_state["c"] == m["c"] and dev_state["min_g"] == m["min_g"], (what, dev_state["c"], dev_state["min_g"], m["c"], m["min_g"])
    assert np.array_equal(dev_state["r"].view(np.uint64), m["r"].view(np.uint64)), what
    assert np.array_equal(bits(dev_state["x"]), bits(m["x"])), what


# ------------------------------------------------------------------------------- the kernel against the model
WIDTHS = [1920] * 6 + [7680] * 3 + [31920] + [1920] * 3 + [7680]  # (31920: 17 in-launch rounds)
CEIL_DB = [0.0, None, -1.0, -6.0, -12.0]
LAST_AT = {0: 8, 2: len(WIDTHS) - 1, 3: 9, 4: len(WIDTHS) - 1}  # the call in which each slot's stream ends
RESET_AT = 5  # slot 4 starts a new stream in front of this call, under another ceiling


def test_stream_kernel_equals_the_model_bit_for_bit(device):
    """Five slots, slot 1 off, the others under 0, -1, -6 and -12 dBFS, every signal driven +20 dB so that all of them limit.
    Ragged valid counts from {0, 1, 125, 126, 127, n_in}; slot 0 ends in a 7680 call, slot 3 in the 31920 call, slot 2 with an
    empty call, slot 4 is restarted mid-run.  Every float behind counts[b] and the off slot's row keep a NaN."""
    B = 5
    sig = [driven(20 + b, 20.0, 4.0) for b in range(B)]
    rng = np.random.default_rng(3)
    st = engine.PeakLimiter(device, B)
    try:
        st.reset_slots(list(range(B)), [0.0 if d is None else LM.ceiling_of_db(d) for d in CEIL_DB])
        models = [None if d is None else LM.StreamState(d) for d in CEIL_DB]
        cursor = [0] * B
        for call, n_in in enumerate(WIDTHS):
            if call == RESET_AT:
                st.reset_slots([4], [LM.ceiling_of_db(-3.0)])
                models[4] = LM.StreamState(-3.0)
            batch = B if call % 4 != 2 else 4  # some calls leave the last slot out: it carries its state
            valid = rng.choice([0, 1, 125, 126, 127, n_in], size=B, p=[0.1, 0.1, 0.1, 0.1, 0.1, 0.5]).astype(np.int32)
            if n_in == 31920:
                valid[:] = [n_in, n_in, 127, n_in, n_in]
            last = np.array([int(LAST_AT.get(b) == call) for b in range(B)], np.int32)
            if last[2]:
                valid[2] = 0  # `last` arrives with an empty call
            pcm = np.full((batch, n_in), 1e3, np.float32)  # garbage past the valid samples must not be read
            for b in range(batch):
                pcm[b, :valid[b]] = sig[b][cursor[b]: cursor[b] + valid[b]]
            out, counts = st.new_outputs(batch, n_in)
            assert out.shape[1] == n_in + LM.HOLD_BACK
            out.fill_(float("nan"))
            st.chunk(torch.from_numpy(pcm).to(device), n_in, out, counts, valid=torch.from_numpy(valid[:batch].copy()).to(device),
                     last=torch.from_numpy(last[:batch].copy()).to(device))
            out, counts = out.cpu().numpy(), counts.cpu().numpy()
            for b in range(batch):
                if models[b] is None:
                    assert counts[b] == 0 and np.all(np.isnan(out[b])), (call, b)
                    continue
                fed_before, ended_before = models[b].pos, models[b].ended
                want = models[b].process(pcm[b, :valid[b]], last=bool(last[b]))
                assert counts[b] == want.size, (call, b, int(counts[b]), want.size)
                if not ended_before:
                    fed = fed_before + int(valid[b])
                    assert want.size == (fed if last[b] else max(0, fed - 126)) - max(0, fed_before - 126), (call, b)
                assert np.array_equal(bits(out[b, :want.size]), bits(want)), (call, b, n_in, int(valid[b]))
                assert np.all(np.isnan(out[b, want.size:])), (call, b)
                cursor[b] += int(valid[b])
            if call in (0, 4, 6, 9, len(WIDTHS) - 1):
                for b in (0, 2, 3, 4):
                    _assert_state(st.slot_state(b), models[b], (call, b))
                assert st.slot_state(1)["on"] == 0
        assert all(models[b].ended for b in (0, 2, 3, 4))
        assert all(models[b].min_g < 1.0 for b in (0, 2, 3, 4))
    finally:
        st.close()


@pytest.mark.parametrize("n", [1, 5, 126, 127, 1325, 1326, 1327, 48000])
def test_apply_equals_the_model_bit_for_bit(device, n):
    x = driven(31, 12.0)
    lo = min(max(0, int(np.argmax(np.abs(x))) - n // 2), x.size - n)  # around the signal's largest peak: every length limits
    x = x[lo: lo + n]
    want, g = LM.limit(x, -6.0)
    got, red = engine.peak_limit(x, -6.0, device)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert red == LM.reduction_db(g) > 0.0


def test_an_utterance_under_the_ceiling_comes_back_bit_identical(device):
    x = driven(32, 0.0)
    x[100] = -0.0
    assert float(np.abs(x).max()) < LM.ceiling_of_db(-1.0)
    got, red = engine.peak_limit(x, -1.0, device)
    assert red == 0.0 and np.array_equal(bits(got), bits(x))
    assert engine.peak_limit(np.zeros(0, np.float32), -1.0, device)[0].size == 0


def test_limiter_stage_refuses_bad_arguments_under_its_own_name(device):
    import ctypes as C

    from smoltts_amd.abi import E_CAPACITY, E_INVALID

    B = 3
    lib = engine.load_library()
    need = lib.smoltts_limiter_bytes(B)
    slab = torch.zeros(need, dtype=torch.uint8, device=device)
    tab = LM.packed()
    h = C.c_void_p()

    def err():
        return lib.smoltts_last_error().decode()

    create = lib.smoltts_limiter_create
    assert create(engine.dptr(slab), need - 1, B, tab.ctypes.data, tab.size, C.byref(h)) == E_CAPACITY
    assert err() == f"limiter_create: slab has {need - 1} bytes, {need} needed" and not h.value
    assert create(engine.dptr(slab) + 1, need, B, tab.ctypes.data, tab.size, C.byref(h)) == E_INVALID and not h.value
    assert create(engine.dptr(slab), need, B, tab.ctypes.data, tab.size - 1, C.byref(h)) == E_INVALID and not h.value
    assert err() == "limiter_create: tables of 35 doubles, 36 expected"
    assert create(engine.dptr(slab), need, B, None, tab.size, C.byref(h)) == E_INVALID and not h.value
    assert create(engine.dptr(slab), need, B, tab.ctypes.data, tab.size, C.byref(h)) == 0 and h.value
    try:
        ints = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
        dbl = lambda *v: (C.c_double * len(v))(*v)  # noqa: E731
        reset = lib.smoltts_limiter_reset_slots
        assert reset(h, ints(B), dbl(0.5), 1, None) == E_INVALID and err() == f"limiter_reset_slots: slot {B} out of range"
        for bad in (1.5, -0.1, float("nan")):
            assert reset(h, ints(0), dbl(bad), 1, None) == E_INVALID
        assert reset(h, ints(0), None, 1, None) == E_INVALID and reset(h, ints(0), dbl(0.5), 0, None) == E_INVALID
        pcm = torch.zeros(B + 1, 16, dtype=torch.float32, device=device)
        out = torch.zeros(B + 1, 16 + LM.HOLD_BACK, dtype=torch.float32, device=device)
        counts = torch.zeros(B + 1, dtype=torch.int32, device=device)

        def chunk(batch=B, n_in=16, stride=16, ostride=16 + LM.HOLD_BACK, p=engine.dptr(pcm), o=engine.dptr(out), c=engine.dptr(counts), s=h):
            return lib.smoltts_limiter_chunk(s, p, stride, batch, n_in, None, None, o, ostride, c, None)

        assert chunk(batch=B + 1) == E_INVALID and err() == f"limiter_chunk: batch {B + 1} (1..{B})"
        assert chunk(batch=0) == E_INVALID and chunk(n_in=-1) == E_INVALID and chunk(stride=15) == E_INVALID
        assert chunk(n_in=61441, stride=61441, ostride=70000) == E_INVALID and err() == "limiter_chunk: n_in 61441 above 61440"
        assert chunk(ostride=16 + LM.HOLD_BACK - 1) == E_CAPACITY and err() == "limiter_chunk: out_stride 141 < 142 samples"
        assert chunk(p=None) == E_INVALID and chunk(o=None) == E_INVALID and chunk(c=None) == E_INVALID and chunk(s=None) == E_INVALID
        res = torch.zeros(1, dtype=torch.float64, device=device)
        apply = lib.smoltts_limiter_apply
        assert apply(h, engine.dptr(pcm), -1, 0.5, engine.dptr(out), engine.dptr(res), None) == E_INVALID
        assert apply(h, engine.dptr(pcm), 16, 0.0, engine.dptr(out), engine.dptr(res), None) == E_INVALID
        assert err() == "limiter_apply: ceiling 0 outside (0, 1]"
        assert apply(h, engine.dptr(pcm), 16, 2.0, engine.dptr(out), engine.dptr(res), None) == E_INVALID
        assert apply(h, None, 16, 0.5, engine.dptr(out), engine.dptr(res), None) == E_INVALID
        assert apply(h, engine.dptr(pcm), 16, 0.5, engine.dptr(out), None, None) == E_INVALID
        st_i, st_v = (C.c_int64 * 3)(), np.zeros(2 + LM.R_HIST + LM.HOLD_BACK)
        assert lib.smoltts_limiter_slot_state(h, B, st_i, st_v.ctypes.data, None) == E_INVALID
        assert lib.smoltts_limiter_slot_state(h, 0, None, st_v.ctypes.data, None) == E_INVALID
        assert lib.smoltts_limiter_slot_state(h, 0, st_i, st_v.ctypes.data, None) == 0 and list(st_i) == [0, 0, 0]  # every slot starts off
        torch.cuda.synchronize()
        assert not out.any() and not counts.any()  # nothing was launched
    finally:
        lib.smoltts_limiter_destroy(h)


def test_rows_wider_than_one_call_go_through_in_pieces(device):
    """``PeakLimiter.run`` at 70000 samples a row (more than the 61440 one call takes): slot 0 ends its stream with the row, slot 1
    has fewer valid samples and goes on in a second, narrow pass."""
    wide = 70000
    sig = [driven(50 + b, 12.0, 3.5) for b in range(2)]
    st = engine.PeakLimiter(device, 2)
    try:
        st.reset_slots([0, 1], [LM.ceiling_of_db(-6.0)] * 2)
        models = [LM.StreamState(-6.0), LM.StreamState(-6.0)]
        at = [0, 0]
        for n_in, valid, last in ((wide, [wide, 62000], [1, 0]), (1920, [1920, 1920], [0, 1])):
            pcm = np.full((2, n_in), 1e3, np.float32)
            for b in range(2):
                pcm[b, :valid[b]] = sig[b][at[b]: at[b] + valid[b]]
            out, counts = st.new_outputs(2, n_in)
            assert out.shape[1] == n_in + LM.HOLD_BACK
            st.run(torch.from_numpy(pcm).to(device), n_in, out, counts, torch.tensor(valid, dtype=torch.int32, device=device),
                   torch.tensor(last, dtype=torch.int32, device=device))
            out, counts = out.cpu().numpy(), counts.cpu().numpy()
            for b in range(2):
                want = models[b].process(pcm[b, :valid[b]], last=bool(last[b]))
                assert counts[b] == want.size and np.array_equal(bits(out[b, :want.size]), bits(want)), (n_in, b)
                at[b] += valid[b]
        assert models[0].min_g < 1.0 and models[1].min_g < 1.0 and st.slot_state(1)["min_g"] == models[1].min_g
    finally:
        st.close()


# ------------------------------------------------------------------------------- through the converter
FORMATS = ["pcm_16000", "pcm_16000", None, None]
SPEEDS = [tsm.speed_q(1.25), tsm.speed_q(1.25), None, tsm.speed_q(1.25)]
CONTAINERS = ["flac", "flac", None, None]
DB = -6.0


def _run_converter(device, x, limit):
    B, n = x.shape[0], x.shape[1] // 1920
    conv = engine.StreamConverter(device, B, 1920)
    try:
        conv.reset_slots(list(range(B)), FORMATS, SPEEDS, CONTAINERS, limit=limit)
        assert (conv.lim is not None) == (limit is not None and any(limit))
        assert conv.ends(range(B)) == (True, False)
        got = [[] for _ in range(B)]
        for f in range(n):
            pcm = torch.from_numpy(x[:, f * 1920:(f + 1) * 1920].copy()).to(device)
            valid = torch.full((B,), 1920, dtype=torch.int32, device=device)
            last = torch.full((B,), int(f == n - 1), dtype=torch.int32, device=device)
            p = conv.run(pcm, 1920, valid, last)
            assert ("limit" in p.plan.stages) == (conv.lim is not None)
            p.to_host(torch.cuda.current_stream())
            torch.cuda.synchronize()
            for b in range(B):
                if p.converts(b):
                    got[b].append(p.chunk(b, f == n - 1))
        assert conv.lim is not None or "limit" not in conv.plan(range(B)).rows
        return [np.concatenate(g) if g else None for g in got]
    finally:
        conv.close()


def test_a_limited_slot_beside_unlimited_ones_in_the_converter(device):
    """Slot 0: stretch, limiter, pcm_16000, FLAC; slot 1: its unlimited twin; slot 2: a plain slot; slot 3: stretch and limiter
    as float32.  Against the numpy model over the stretch stage's own output, and against a run that never made the stage."""
    from math import gcd

    from scipy.signal import resample_poly

    from flac_decode_helpers import decode_mono16

    one = driven(41, 12.0)[:20 * 1920]
    x = np.stack([one, one, one, one])
    c = LM.ceiling_of_db(DB)
    on = _run_converter(device, x, [c, None, None, c])
    off = _run_converter(device, x, None)
    assert on[2] is None and off[2] is None  # the plain slot goes through no stage
    assert on[1].tobytes() == off[1].tobytes()  # the unlimited twin: the bytes of a run that never made the stage
    want, g = LM.limit(off[3], DB)  # (off[3]: the stretch stage's own float32 output)
    assert g < 1.0 and on[3].shape == off[3].shape and np.array_equal(bits(on[3]), bits(want))
    # pcm_16000 in FLAC: lossless, so the resampler's int16 of the limited stream, within its house bound against scipy
    k = gcd(24000, 16000)
    s16 = np.rint(np.clip(resample_poly(want.astype(np.float64), 16000 // k, 24000 // k), -1.0, 1.0) * 32767).astype(np.int16)
    dec = np.asarray(decode_mono16(on[0].tobytes()), np.int16)
    d = np.abs(dec.astype(np.int32) - s16.astype(np.int32))
    assert dec.shape == s16.shape and d.max() <= 1 and np.mean(d == 0) >= 0.999
    assert on[0].tobytes() != on[1].tobytes()
