"""CPU: bench.dump_outputs (what `bench.py --dump-outputs DIR` writes) - float64 .npy files, at most 64 MB in all,
and beyond that the same fixed, seeded sample of points for every array and every run."""
import os
import sys

import numpy as np

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    a = {"abs_coef": np.arange(10.0), "transmittance": np.linspace(0, 1, 10, dtype=np.float32)}
    info = bench.dump_outputs(str(tmp_path), a)
    assert sorted(os.listdir(tmp_path)) == ["abs_coef.npy", "transmittance.npy"]
    for k, v in a.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v.astype(np.float64))
        assert info["arrays"][k] == {"shape": [10], "sampled_from_points": None}


def test_large_outputs_keep_one_seeded_sample_under_the_cap(tmp_path):
    n = 400_000
    rng = np.random.default_rng(7)
    toa = rng.random(n)
    rows = [toa * (i + 1) for i in range(30)]                  # 30 x 3.2 MB + 3.2 MB: over 64 MB
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    info = bench.dump_outputs(d1, {"toa": toa, "transmittance": rows})
    bench.dump_outputs(d2, {"toa": toa, "transmittance": rows})
    assert _size(d1) <= 64_000_000 and _size(d1) > 60_000_000
    t, tr = np.load(os.path.join(d1, "toa.npy")), np.load(os.path.join(d1, "transmittance.npy"))
    assert tr.shape == (30, t.size) and t.size < n and info["arrays"]["toa"]["sampled_from_points"] == n
    assert np.array_equal(tr[0], t) and np.array_equal(tr[29], 30 * t)        # the same points in every array
    assert np.isin(t, toa).all()
    for f in ("toa.npy", "transmittance.npy"):                                  # and in every run
        assert np.array_equal(np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f)))
