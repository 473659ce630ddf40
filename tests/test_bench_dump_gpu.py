"""`bench.py --dump-outputs DIR` on the GPU, at a small size: the timed path's last step is written out, and two runs with the
same arguments write the same bits (the inputs are seeded), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
ARGS = ["--model", "tiny", "--batch", "4", "--chunk", "4", "--steps", "3", "--warmup", "1", "--cpu-frames", "0", "--no-latency",
        "--no-kernel-timing"]


def _bench(out: Path) -> dict:
    env = dict(os.environ, TORCH_COMPILE_DISABLE="1")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *ARGS, "--dump-outputs", str(out)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_step_and_repeat_bit_for_bit(tmp_path):
    lines = [_bench(tmp_path / "a"), _bench(tmp_path / "b")]
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    codes, pcm = np.load(tmp_path / "a" / "codes.npy"), np.load(tmp_path / "a" / "pcm.npy")
    assert codes.dtype == np.float32 and codes.shape == (4, 4, 9) and pcm.dtype == np.float32 and pcm.shape == (4, 4 * 1920)
    assert np.all(codes >= 0) and np.all(codes == np.round(codes)) and np.all(np.isfinite(pcm)) and float(np.abs(pcm).max()) > 0
    for name in ("codes", "pcm"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name
