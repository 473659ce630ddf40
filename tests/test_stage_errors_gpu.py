"""Argument refusals of the four post-codec stages (csrc/resample.hip, tsm.hip, seam.hip, flac.hip) through the ctypes layer:
the error code and the call's own name at the start of the last-error text.  Every refusal happens on the host before any launch."""
import ctypes as C

import pytest
import torch

from smoltts_amd import engine
from smoltts_amd.abi import E_CAPACITY, E_INVALID
from smoltts_amd.engine import dptr
from smoltts_amd.formats import ENC_S16

pytestmark = pytest.mark.gpu

B = 4


def _ints(*v):
    return (C.c_int32 * len(v))(*v)


def _last_error(lib):
    return lib.smoltts_last_error().decode()


def _reset_resampler(lib, h, slot):
    return lib.smoltts_resampler_reset_slots(h, _ints(slot), _ints(8000), _ints(ENC_S16), 1, None)


def _reset_tsm(lib, h, slot):
    return lib.smoltts_tsm_reset_slots(h, _ints(slot), _ints(65536), 1, None)


def _reset_seam(lib, h, slot):
    return lib.smoltts_seam_reset_slots(h, _ints(slot), _ints(0), _ints(0), _ints(0), 1, None)


def _reset_flac(lib, h, slot):
    return lib.smoltts_flac_reset_slots(h, _ints(slot), _ints(24000), _ints(engine.FLAC_F32), 1, None)


def _chunk_resampler(lib, h, batch, pcm, out, counts):
    return lib.smoltts_resample_chunk(h, dptr(pcm), pcm.stride(0), batch, 16, None, dptr(out), out.shape[1], dptr(counts), None)


def _chunk_tsm(lib, h, batch, pcm, out, counts):
    return lib.smoltts_tsm_chunk(h, dptr(pcm), pcm.stride(0), batch, 16, None, None, dptr(out), out.shape[1] // 4, dptr(counts), None)


def _chunk_seam(lib, h, batch, pcm, out, counts):
    return lib.smoltts_seam_chunk(h, dptr(pcm), pcm.stride(0), batch, 16, None, None, None, 0, dptr(out), out.shape[1] // 4,
                                  dptr(counts), None)


def _chunk_flac(lib, h, batch, pcm, out, counts):
    return lib.smoltts_flac_chunk(h, dptr(pcm), pcm.stride(0), 16, None, None, 0, None, batch, None, dptr(out), out.shape[1],
                                  dptr(counts), 1, None)


STAGES = {
    "resampler": ("resampler", "resample_chunk", _reset_resampler, _chunk_resampler),
    "tsm": ("tsm", "tsm_chunk", _reset_tsm, _chunk_tsm),
    "seam": ("seam", "seam_chunk", _reset_seam, _chunk_seam),
    "flac": ("flac", "flac_chunk", _reset_flac, _chunk_flac),
}


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_refuses_bad_arguments_under_its_own_name(stage):
    name, chunk_name, reset, chunk = STAGES[stage]
    lib = engine.load_library()
    dev = torch.device("cuda", 0)
    need = getattr(lib, f"smoltts_{name}_bytes")(B)
    assert need > 0 and need % 256 == 0
    slab = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert dptr(slab) % 256 == 0
    create, destroy = getattr(lib, f"smoltts_{name}_create"), getattr(lib, f"smoltts_{name}_destroy")
    h = C.c_void_p()

    assert create(dptr(slab), need - 1, B, C.byref(h)) == E_CAPACITY  # a slab one byte short
    assert _last_error(lib) == f"{name}_create: slab has {need - 1} bytes, {need} needed"
    assert not h.value
    assert create(dptr(slab) + 1, need, B, C.byref(h)) == E_INVALID
    assert _last_error(lib) == f"{name}_create: slab must be 256-byte aligned"
    assert not h.value

    assert create(dptr(slab), need, B, C.byref(h)) == 0 and h.value
    try:
        assert reset(lib, h, B) == E_INVALID  # slot == max_batch
        assert _last_error(lib) == f"{name}_reset_slots: slot {B} out of range"
        pcm = torch.zeros(B + 1, 16, dtype=torch.float32, device=dev)
        out = torch.zeros(B + 1, 1 << 20, dtype=torch.uint8, device=dev)
        counts = torch.zeros(B + 1, 2, dtype=torch.int32, device=dev)
        assert chunk(lib, h, B + 1, pcm, out, counts) == E_INVALID  # batch == max_batch + 1
        assert _last_error(lib) == f"{chunk_name}: batch {B + 1} (1..{B})"
        torch.cuda.synchronize()
        assert not out.any() and not counts.any()  # nothing was launched
    finally:
        destroy(h)
