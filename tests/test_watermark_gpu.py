"""The watermark stage on the device against its numpy model (``smoltts_amd/watermark.py``): the stream kernel sample for sample
and state for state over ragged calls of every size class, the whole-utterance entry, the stage's bad-argument cases, and the
stage inside ``StreamConverter`` beside the other stages and beside an unmarked slot."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import engine, tsm, watermark as W  # noqa: E402
from smoltts_amd.abi import E_CAPACITY, E_INVALID  # noqa: E402

from watermark_helpers import speechlike, ulaw_decode  # noqa: E402

KEY = W.Watermark(0x0123456789ABCDEF, -26.0)
SIZES = (1, 479, 480, 481, 1920, 7680)
STREAM, WIDE = 52800, 70000


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_state(dev_state, model, what):
    m = model.state()
    assert dev_state["on"] == 1 and dev_state["pos"] == m["pos"], (what, dev_state["pos"], m["pos"])
    assert np.array_equal(dev_state["values"].view(np.uint64), m["values"].view(np.uint64)), (what, dev_state["values"], m["values"])


# ------------------------------------------------------------------------------- the kernel against the model
def test_stream_kernel_equals_the_model_bit_for_bit(device):
    """Slot 0 is on from the start, slot 1 is off, slot 2 is restarted in the middle.  Calls of 1, 479, 480, 481, 1920 and 7680
    samples with ragged valid counts (0 among them) until slot 0 has consumed 52800 samples, then one call of 70000."""
    B = 3
    sig = [speechlike(40 + b, (STREAM + WIDE + 7680) / 24000.0) for b in range(B)]
    rng = np.random.default_rng(11)
    st = engine.Watermarker(device, B, KEY)
    try:
        st.reset_slots([0, 1, 2], [KEY.gain, 0.0, W.gain_of_db(-20.0)])
        models = [W.StreamState(KEY), None, W.StreamState(KEY, W.gain_of_db(-20.0))]
        cursor, got0, fed0 = [0] * B, [], []
        sizes = list(SIZES) * 2  # every size at least twice, then by chance
        call, restarted = 0, False
        while cursor[0] < STREAM + WIDE:
            wide = cursor[0] >= STREAM
            n_in = WIDE if wide else (sizes[call] if call < len(sizes) else int(rng.choice(SIZES[2:])))
            batch = B if call % 5 else 2  # some calls leave the last slot out: it carries its state
            if call == 14:  # slot 2 starts a new stream mid-run, the others go on
                st.reset_slots([2], [W.gain_of_db(-33.0)])
                models[2], restarted = W.StreamState(KEY, W.gain_of_db(-33.0)), True
            valid = rng.integers(0, n_in + 1, size=B).astype(np.int32)
            if call % 3 == 0 or wide:
                valid[0] = n_in
            if call % 7 == 3:
                valid[call % 2 * 2] = 0
            pcm = np.full((batch, n_in), 1e3, np.float32)  # garbage past the valid samples must not be read
            for b in range(batch):
                valid[b] = min(valid[b], sig[b].size - cursor[b])
                pcm[b, :valid[b]] = sig[b][cursor[b]: cursor[b] + valid[b]]
            out, counts = st.new_outputs(batch, n_in)
            out.fill_(-7.0)
            st.chunk(torch.from_numpy(pcm).to(device), n_in, out, counts, valid=torch.from_numpy(valid[:batch].copy()).to(device))
            out, counts = out.cpu().numpy(), counts.cpu().numpy()
            for b in range(batch):
                if models[b] is None:
                    assert counts[b] == 0 and np.all(out[b] == -7.0), (call, b)  # the off slot's row is untouched
                    continue
                want = models[b].process(pcm[b, :valid[b]])
                assert counts[b] == valid[b], (call, b)
                assert np.array_equal(_bits(out[b, :valid[b]]), _bits(want)), (call, b, n_in, int(valid[b]))
                assert np.all(out[b, valid[b]:] == -7.0), (call, b)
                if b == 0:
                    got0.append(out[0, :valid[0]].copy())
                    fed0.append(pcm[0, :valid[0]].copy())
                cursor[b] += int(valid[b])
            if call in (2, 7, 20) or wide:
                for b in (0, 2):
                    _assert_state(st.slot_state(b), models[b], (call, b))
                assert st.slot_state(1)["on"] == 0
            call += 1
        assert restarted and call > 20 and cursor[2] > 0  # every size twice, the restart, more calls, and the wide one
        got0, fed0 = np.concatenate(got0), np.concatenate(fed0)
        d = W.detect(got0, KEY.key)
        print(f"slot 0: {got0.size} samples, score {d.score:.2f} at offset {d.offset}")
        assert d.detected and d.offset == 0
        assert not W.detect(fed0, KEY.key).detected
        # the blocking entry: the whole utterance in one launch gives the stream's bytes
        whole = engine.watermark_embed(fed0, KEY, device)
        assert np.array_equal(_bits(whole), _bits(got0))
        assert engine.watermark_embed(np.zeros(0, np.float32), KEY, device).size == 0
    finally:
        st.close()


# ------------------------------------------------------------------------------- bad arguments
def test_watermark_stage_refuses_bad_arguments_under_its_own_name(device):
    B = 4
    lib = engine.load_library()
    need = lib.smoltts_watermark_bytes(B)
    assert need > 0 and need % 256 == 0 and lib.smoltts_watermark_bytes(0) == 0
    slab = torch.zeros(need, dtype=torch.uint8, device=device)
    tab = KEY.packed()
    assert tab.size == lib.smoltts_watermark_table_doubles()
    h = C.c_void_p()

    def err():
        return lib.smoltts_last_error().decode()

    create = lib.smoltts_watermark_create
    assert create(engine.dptr(slab), need - 1, B, tab.ctypes.data, tab.size, C.byref(h)) == E_CAPACITY
    assert err() == f"watermark_create: slab has {need - 1} bytes, {need} needed" and not h.value
    assert create(engine.dptr(slab) + 1, need, B, tab.ctypes.data, tab.size, C.byref(h)) == E_INVALID
    assert err() == "watermark_create: slab must be 256-byte aligned" and not h.value
    assert create(engine.dptr(slab), need, B, tab.ctypes.data, tab.size - 1, C.byref(h)) == E_INVALID and not h.value
    assert create(engine.dptr(slab), need, B, None, tab.size, C.byref(h)) == E_INVALID and not h.value
    bad = tab.copy()
    bad[W.TAPS + 100] = 0.5
    assert create(engine.dptr(slab), need, B, bad.ctypes.data, bad.size, C.byref(h)) == E_INVALID and not h.value
    assert err() == "watermark_create: chip 100 is not +-1"
    assert create(engine.dptr(slab), need, B, tab.ctypes.data, tab.size, C.byref(h)) == 0 and h.value
    try:
        ints = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
        dbl = lambda *v: (C.c_double * len(v))(*v)  # noqa: E731
        assert lib.smoltts_watermark_reset_slots(h, ints(B), dbl(0.05), 1, None) == E_INVALID
        assert err() == f"watermark_reset_slots: slot {B} out of range"
        assert lib.smoltts_watermark_reset_slots(h, ints(-1), dbl(0.05), 1, None) == E_INVALID
        assert lib.smoltts_watermark_reset_slots(h, ints(0), dbl(1.5), 1, None) == E_INVALID
        assert lib.smoltts_watermark_reset_slots(h, ints(0), dbl(-0.1), 1, None) == E_INVALID
        assert lib.smoltts_watermark_reset_slots(h, ints(0), dbl(float("nan")), 1, None) == E_INVALID
        assert lib.smoltts_watermark_reset_slots(h, ints(0), None, 1, None) == E_INVALID
        assert lib.smoltts_watermark_reset_slots(h, ints(0), dbl(0.05), 0, None) == E_INVALID
        pcm = torch.zeros(B + 1, 16, dtype=torch.float32, device=device)
        out = torch.zeros(B + 1, 16, dtype=torch.float32, device=device)
        counts = torch.zeros(B + 1, dtype=torch.int32, device=device)

        def chunk(batch=B, n_in=16, stride=16, ostride=16, p=engine.dptr(pcm), o=engine.dptr(out), c=engine.dptr(counts), s=h):
            return lib.smoltts_watermark_chunk(s, p, stride, batch, n_in, None, o, ostride, c, None)

        assert chunk(batch=B + 1) == E_INVALID
        assert err() == f"watermark_chunk: batch {B + 1} (1..{B})"
        assert chunk(batch=0) == E_INVALID and chunk(n_in=-1) == E_INVALID and chunk(stride=15) == E_INVALID
        assert chunk(ostride=15) == E_CAPACITY
        assert err() == "watermark_chunk: out_stride 15 < 16 samples"
        assert chunk(p=None) == E_INVALID and chunk(o=None) == E_INVALID and chunk(c=None) == E_INVALID and chunk(s=None) == E_INVALID
        assert lib.smoltts_watermark_embed(h, engine.dptr(pcm), -1, 0.05, engine.dptr(out), None) == E_INVALID
        assert lib.smoltts_watermark_embed(h, engine.dptr(pcm), 16, 2.0, engine.dptr(out), None) == E_INVALID
        assert lib.smoltts_watermark_embed(h, None, 16, 0.05, engine.dptr(out), None) == E_INVALID
        st_i, st_v = (C.c_int64 * 2)(), np.zeros(5)
        assert lib.smoltts_watermark_slot_state(h, B, st_i, st_v.ctypes.data, None) == E_INVALID
        assert lib.smoltts_watermark_slot_state(h, 0, None, st_v.ctypes.data, None) == E_INVALID
        torch.cuda.synchronize()
        assert not out.any() and not counts.any()  # nothing was launched
    finally:
        lib.smoltts_watermark_destroy(h)


# ------------------------------------------------------------------------------- through the converter
FORMATS = ["pcm_16000", "ulaw_8000", None, None, "pcm_16000"]
SPEEDS = [None, None, None, tsm.speed_q(1.25), tsm.speed_q(1.25)]
CONTAINERS = [None, None, "flac", None, None]
MARKED = [True, True, True, True, False]


def _run_converter(device, x, marked):
    B, n = x.shape[0], x.shape[1] // 1920
    conv = engine.StreamConverter(device, B, 1920, watermark=KEY)
    try:
        conv.reset_slots(list(range(B)), FORMATS, SPEEDS, CONTAINERS, watermark=marked)
        assert (conv.wm is not None) == any(marked)
        got = [[] for _ in range(B)]
        for f in range(n):
            pcm = torch.from_numpy(x[:, f * 1920:(f + 1) * 1920].copy()).to(device)
            valid = torch.full((B,), 1920, dtype=torch.int32, device=device)
            last = torch.full((B,), int(f == n - 1), dtype=torch.int32, device=device)
            p = conv.run(pcm, 1920, valid, last)
            assert ("watermark" in p.plan.stages) == any(marked)
            p.to_host(torch.cuda.current_stream())
            torch.cuda.synchronize()
            for b in range(B):
                got[b].append(p.chunk(b, f == n - 1))
        return [np.concatenate(g) for g in got]
    finally:
        conv.close()


def _want_s16(x24, rate):
    from math import gcd

    from scipy.signal import resample_poly

    g = gcd(24000, rate)
    return np.rint(np.clip(resample_poly(np.asarray(x24, np.float64), rate // g, 24000 // g), -1.0, 1.0) * 32767).astype(np.int16)


def test_marked_slots_beside_an_unmarked_one_in_the_converter(device):
    """Marked slots as pcm_16000, ulaw_8000, FLAC at 24 kHz and float32 at speed 1.25 beside an unmarked, stretched pcm_16000
    slot, against the chained models (tsm, watermark, the resampler's reference or flac.quantize) and a run without the stage."""
    from smoltts_amd import flac
    from smoltts_amd.formats import lin2ulaw

    from flac_decode_helpers import decode_mono16

    x = np.stack([speechlike(60 + b, 2.0)[:25 * 1920] for b in range(5)])
    on = _run_converter(device, x, MARKED)
    off = _run_converter(device, x, [False] * 5)
    assert on[4].tobytes() == off[4].tobytes()  # the unmarked slot: the bytes of a run that never made the stage
    marked = [W.embed(x[b], KEY) for b in range(3)]
    # pcm_16000 and ulaw_8000: the house bound of the resampler against scipy (at most one step, 99.9 % equal)
    want = _want_s16(marked[0], 16000)
    d = np.abs(on[0].astype(np.int32) - want.astype(np.int32))
    assert on[0].shape == want.shape and d.max() <= 1 and np.mean(d == 0) >= 0.999
    assert on[1].dtype == np.uint8 and np.mean(on[1] == lin2ulaw(_want_s16(marked[1], 8000))) >= 0.999
    # FLAC of the float32 stream: lossless, so exactly the model's samples quantised
    assert np.array_equal(np.asarray(decode_mono16(on[2].tobytes()), np.int16), flac.quantize(marked[2]))
    # behind the stretch: bit for bit the model over the stretch stage's own output, and the chained models within the stretch
    # kernel's bound against its model (1e-6) carried through the mark (whose own error it scales by 10^(-26/20))
    assert np.array_equal(_bits(on[3]), _bits(W.embed(off[3], KEY)))
    chain = W.embed(tsm.stretch(x[3], 1.25), KEY)
    assert on[3].shape == chain.shape and float(np.abs(on[3] - chain).max()) <= 2e-6
    for b, (pcm, rate) in enumerate([(on[0], 16000), (ulaw_decode(on[1]), 8000), (decode_mono16(on[2].tobytes()), 24000), (on[3], 24000)]):
        det = W.detect(np.asarray(pcm), KEY.key, rate)
        print(f"slot {b}: score {det.score:.2f}")
        assert det.detected, b
    assert not W.detect(off[3], KEY.key).detected and not W.detect(on[4], KEY.key, 16000).detected
