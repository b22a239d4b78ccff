"""bench.py --dump-outputs: the writer itself (host only: CPU tensors stand in for a
launcher's output buffers) — names, dtypes, the fixed seeded sample of a large output."""

import os
import types

import numpy as np
import torch

import bench


def test_dump_small_outputs_whole(tmp_path):
    out = torch.arange(1000, dtype=torch.float32) * 0.5
    ldj = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    launcher = types.SimpleNamespace(out=out, ldj=ldj, logp=None, B=1000)
    names = bench.dump_outputs(str(tmp_path / "d"), launcher, {"mean_log_prob": -1.25, "nonfinite_log_prob": 0,
                                                               "absent": None})
    assert names == ["log_prob", "ldj", "mean_log_prob", "nonfinite_log_prob"]
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in names)
    lp = np.load(tmp_path / "d" / "log_prob.npy")
    assert lp.dtype == np.float32 and np.array_equal(lp, out.numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "ldj.npy"), ldj.numpy())  # shape kept
    m = np.load(tmp_path / "d" / "mean_log_prob.npy")
    assert m.dtype == np.float64 and m.tolist() == [-1.25]
    assert np.load(tmp_path / "d" / "nonfinite_log_prob.npy").tolist() == [0.0]


def test_dump_large_output_is_a_fixed_sample(tmp_path):
    n = 3 * bench.DUMP_MAX_ELEMS + 7
    grad_t = torch.arange(n, dtype=torch.float32).reshape(-1, 1)  # exact in fp32: n < 2^24
    assert n < 1 << 24
    launcher = types.SimpleNamespace(grad_t=grad_t)
    for sub in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / sub), launcher, {}) == ["grad_t"]
    a, b = np.load(tmp_path / "a" / "grad_t.npy"), np.load(tmp_path / "b" / "grad_t.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(a, b)  # the same elements every run
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, bench.DUMP_MAX_ELEMS))
    assert np.array_equal(a, idx.astype(np.float32))  # the documented sample of the flattened output
    assert a.nbytes * 7 < 64e6  # at most seven arrays per mode
