"""`bench.py --dump-outputs DIR`: what the last timed step returned, written as DIR/<name>.npy (fp64, a fixed seeded sample of
the per-point rows), so that two builds run with the same arguments can be compared output for output."""
import os

import numpy as np
import pytest

from test_bench_launcher import run_bench


def test_dump_sample_is_fixed_and_within_budget():
    import bench
    assert np.array_equal(bench.dump_sample(1000, 13), np.arange(1000))          # small batches are written whole
    for rows in (13, 15, 67):
        a, b = bench.dump_sample(10_000_000, rows), bench.dump_sample(10_000_000, rows)
        assert np.array_equal(a, b)                                              # same points from run to run
        assert 8 * rows * len(a) <= bench.DUMP_BYTES < 64_000_000
        assert len(np.unique(a)) == len(a) and np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < 10_000_000


@pytest.mark.gpu
def test_dump_is_the_last_step_and_repeats(tmp_path):
    import oracle_lib as ol
    from cmad_amd.synthetic import gauss_point_batch
    B = 400_000                                                                   # more than the budget holds: sampled
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = run_bench(["--gpus", "1", "--steps", "4", "--warmup", "1", "--points", str(B), "--no-cpu-baseline",
                         "--dump-outputs", str(d)])
        assert out["steps"] == 4 and out["ms_per_step"] > 0
        assert sorted(os.listdir(d)) == ["grad.npy", "sigma.npy", "xi.npy"]
        arrays = {n: np.load(d / f"{n}.npy") for n in ("xi", "sigma", "grad")}
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000_000
        n = out["dump"]["points"]["sampled"]
        assert 0 < n < B and arrays["xi"].shape == (7, n) and arrays["sigma"].shape == (6, n) and arrays["grad"].shape == (12,)
        dumps.append(arrays)
    for name in dumps[0]:
        np.testing.assert_array_equal(dumps[0][name], dumps[1][name])
    # the dumped rows are those of the sampled points: the oracle's update of the same inputs (bench.py: seed 22, xi_prev = 0)
    import bench
    idx = bench.dump_sample(B, 13)[:2000]
    g = gauss_point_batch(B, seed=22, eps_y=1e-3)[:, idx]
    xi_o, sig_o, _, _ = ol.Material(ol.j2_voce_values()).update_batch(ol.newton_settings(), g, np.zeros((7, len(idx))))
    np.testing.assert_allclose(dumps[0]["xi"][:, :2000], xi_o, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(dumps[0]["sigma"][:, :2000], sig_o, rtol=1e-10, atol=1e-8)
