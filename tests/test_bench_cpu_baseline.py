"""bench.py's CPU baseline on a checkout it may not write to: oracle/cpu_vcycle's host-tuned timing library is made from a
copy of the module, its C sources and Makefile outside the tree, nothing is written into oracle/, and the copy's V-cycle
agrees with the in-tree exact build (liboracle_cpu_exact.so, made by build(); -march=native may contract into FMA)."""
import os

import numpy as np


def test_cpu_vcycle_library_is_made_outside_a_read_only_checkout(tmp_path, monkeypatch):
    import bench
    from oracle import cpu_vcycle as cv
    from somar_amd import synthetic
    oracle_dir = os.path.dirname(os.path.abspath(cv.__file__))
    access = os.access
    monkeypatch.setattr(os, "access", lambda p, mode, **kw: False if (os.path.abspath(p) == oracle_dir and mode & os.W_OK)
                        else access(p, mode, **kw))
    before = sorted(os.listdir(oracle_dir))
    copy = bench.cpu_vcycle_module(cv, str(tmp_path))
    assert os.path.dirname(os.path.abspath(copy.__file__)) == str(tmp_path)

    n = 16
    dx = (1.0 / n,) * 3
    jg, jinv = synthetic.stretched_diagonal_metric((0, 0, 0), (n - 1,) * 3, dx, (1.0, 1.0, 1.0))
    res = np.asfortranarray(np.random.default_rng(5).uniform(-1.0, 1.0, (n,) * 3))
    res -= float((res / jinv).sum() / (1.0 / jinv).sum())

    def one_vcycle(module, fast):
        h = module.CpuVCycle((n,) * 3, dx, jg, jinv, nthreads=1, fast=fast)
        corr = np.zeros((n + 2,) * 3, order="F")
        h.vcycle(corr, res)
        h.close()
        return corr

    got = one_vcycle(copy, True)
    assert any(f.startswith("liboracle_cpu_") and f.endswith(".so") for f in os.listdir(tmp_path))
    assert sorted(os.listdir(oracle_dir)) == before
    want = one_vcycle(cv, False)
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())
