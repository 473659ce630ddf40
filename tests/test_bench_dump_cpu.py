"""`bench.py --dump-outputs DIR`: the arrays land as float32 .npy files within the size budget; an array over its share is a
fixed, seeded sample of its elements with the indices beside it."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_small_outputs_are_written_whole_in_float32(tmp_path):
    codes = np.arange(4 * 3 * 9, dtype=np.int32).reshape(4, 3, 9)
    pcm = np.linspace(-1, 1, 4 * 3 * 1920).reshape(4, -1)
    shapes = bench.dump_outputs(tmp_path, {"codes": codes, "pcm": pcm})
    assert shapes == {"codes": [4, 3, 9], "pcm": [4, 3 * 1920]}
    c, p = np.load(tmp_path / "codes.npy"), np.load(tmp_path / "pcm.npy")
    assert c.dtype == np.float32 and np.array_equal(c, codes) and p.dtype == np.float32 and np.array_equal(p, pcm.astype(np.float32))
    assert sorted(os.listdir(tmp_path)) == ["codes.npy", "pcm.npy"]


def test_large_outputs_are_a_seeded_sample_within_the_budget(tmp_path):
    big = np.arange(20_000_000, dtype=np.float32).reshape(2, -1)  # 80 MB
    small = np.ones((2, 2), np.float32)
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(d, {"pcm": big, "codes": small})
        assert sum(f.stat().st_size for f in d.iterdir()) <= bench.DUMP_BYTES
    a, b = np.load(tmp_path / "a" / "pcm.npy"), np.load(tmp_path / "b" / "pcm.npy")
    idx = np.load(tmp_path / "a" / "pcm_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and np.array_equal(idx, np.load(tmp_path / "b" / "pcm_index.npy"))
    assert np.array_equal(a, b) and np.array_equal(a, big.reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "codes.npy"), small)
