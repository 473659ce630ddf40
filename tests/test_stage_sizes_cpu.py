"""Slab and row sizes of the post-codec stages (csrc/resample.hip, tsm.hip, seam.hip, flac.hip): pure host functions of the C ABI,
pinned to the numbers of the build in which each stage's slab layout was first written once (csrc/stage.h).  A stage that grows a
region changes its row here on purpose."""
import pytest

from smoltts_amd import engine

BATCHES = (-1, 0, 1, 2, 7, 32, 64)
SLAB_BYTES = {
    "resampler": (0, 0, 53248, 53760, 56320, 70400, 88832),
    "tsm": (0, 0, 20736, 39168, 131328, 592128, 1181952),
    "seam": (0, 0, 197120, 393728, 1377792, 6296576, 12593152),
    "flac": (0, 0, 768, 768, 1280, 3328, 6656),
}
N_IN = (-1, 0, 1, 1920, 7680)
ROWS = {
    "smoltts_tsm_out_samples": (0, 2928, 2932, 10608, 33648),
    "smoltts_resampler_out_bytes": (0, 44, 48, 7724, 30764),
    "smoltts_flac_out_bytes": (0, 50, 52, 3890, 15430),
    "smoltts_flac_max_blocks": (0, 1, 1, 1, 2),
}


@pytest.mark.parametrize("stage", sorted(SLAB_BYTES))
def test_slab_bytes(stage):
    f = getattr(engine.load_library(), f"smoltts_{stage}_bytes")
    assert tuple(f(b) for b in BATCHES) == SLAB_BYTES[stage]


def test_row_sizes():
    lib = engine.load_library()
    for name, want in ROWS.items():
        assert tuple(getattr(lib, name)(n) for n in N_IN) == want, name
    assert tuple(lib.smoltts_seam_out_samples(n, 6000) for n in N_IN) == (0, 30240, 30241, 32160, 37920)
    assert lib.smoltts_seam_out_samples(1920, 480001) == 0
