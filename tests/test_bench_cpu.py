"""bench.py's output dump (--dump-outputs), host side: array formats, the size cap and the fixed row
sample that lets two builds be compared array for array."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_formats_and_fixed_sample(tmp_path):
    g = torch.Generator().manual_seed(3)
    d = 512
    rows = bench.DUMP_BYTES // (4 * d) + 1000   # over the cap: cut to a sample of rows
    big = torch.randn(rows, d, generator=g)
    arrays = {"big": big, "ids": torch.arange(12).reshape(1, 12, 1), "lens": torch.tensor([3, 4], dtype=torch.int32),
              "small3d": torch.randn(2, 3, 5, generator=g).to(torch.bfloat16)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    assert sorted(os.listdir(a)) == ["big.npy", "big_rows.npy", "ids.npy", "lens.npy", "small3d.npy"]
    total = 0
    for f in os.listdir(a):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y)   # the sample is the same every time
        total += x.nbytes
    assert total <= 64 << 20
    x, r = np.load(os.path.join(a, "big.npy")), np.load(os.path.join(a, "big_rows.npy")).astype(np.int64)
    assert x.shape == (bench.DUMP_BYTES // (4 * d), d) and x.nbytes <= bench.DUMP_BYTES
    assert (np.diff(r) > 0).all() and r[0] >= 0 and r[-1] < rows
    assert np.array_equal(x, big.numpy()[r])
    assert np.load(os.path.join(a, "ids.npy")).dtype == np.float64
    assert np.array_equal(np.load(os.path.join(a, "lens.npy")), np.array([3.0, 4.0]))
    assert np.load(os.path.join(a, "small3d.npy")).shape == (6, 5)
