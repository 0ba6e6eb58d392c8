"""bench.py --dump-outputs: the file holds what the headline's timed loop computes -- the correction of one V-cycle from
zero on the seeded C2 residual -- recomputed here in-process on the same inputs; above bench.DUMP_SAMPLE cells it holds
the same seeded sample of that field at every call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_hold_the_timed_vcycle_correction(tmp_path, monkeypatch):
    n = 64
    out_dir = tmp_path / "out"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", str(n), "--no-cpu-baseline",
           "--no-c4", "--no-c5", "--no-cartesian", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert sorted(os.listdir(out_dir)) == ["c2_correction.npy"]
    got = np.load(out_dir / "c2_correction.npy")
    assert got.dtype == np.float64 and got.shape == (n ** 3,)

    import bench
    from somar_amd import api, synthetic
    gpu, _, _ = bench.build_c2(api, synthetic, n, 1, 0, None, "stretched")
    try:
        assert gpu.num_local_patches == 1
        bench.upload_c2_residual(gpu, api, bench.c2_random_field(n))
        gpu.vcycleFromZero(api.F_CORR, api.F_RES)
        gpu.sync()
        want = gpu.download(api.F_CORR, 0, (0, 0, 0)).ravel(order="F")
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())

        monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
        samples = []
        for name in ("s1", "s2"):
            bench.dump_c2_outputs(gpu, api, n, str(tmp_path / name))
            samples.append(np.load(tmp_path / name / "c2_correction.npy"))
        assert samples[0].shape == (1000,)
        np.testing.assert_array_equal(samples[0], samples[1])
        assert np.isin(samples[0], want).all()
    finally:
        gpu.undefine()
