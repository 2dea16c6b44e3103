"""bench.py --dump-outputs: the dump's size budget, number formats and fixed sample (CPU)."""
import os

import numpy as np


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """Arrays that fit are written whole (integers as floats that hold them exactly); one that
    does not fit its share is a sorted sample of the same elements in every run; the files stay
    within the budget and are float32 / float64."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40_000)
    rng = np.random.default_rng(5)
    arrays = {"color": rng.random((3, 50, 70), dtype=np.float32),            # 42,000 B: sampled
              "radii": rng.integers(0, 200, 1001, dtype=np.int32),           # whole, as float32
              "num_rendered": np.asarray(3_000_000_000, dtype=np.int64)}     # > 2^24: float64
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), {k: v.copy() for k, v in reversed(list(arrays.items()))})
    assert sorted(os.listdir(a)) == ["color.npy", "num_rendered.npy", "radii.npy"]
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 40_000
    got = {f[:-4]: np.load(a / f) for f in os.listdir(a)}
    for f in os.listdir(a):
        assert np.load(b / f).tobytes() == got[f[:-4]].tobytes()
    assert got["radii"].dtype == np.float32 and np.array_equal(got["radii"], arrays["radii"])
    assert got["num_rendered"].dtype == np.float64 and got["num_rendered"][0] == 3_000_000_000
    c = got["color"]
    # what the two whole arrays and 1 KiB per .npy header leave, in float32 elements
    assert c.dtype == np.float32 and c.shape == ((40_000 - 3 * 1024 - 8 - 4 * 1001) // 4,)
    keep = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(10_500, c.size, replace=False))
    assert np.array_equal(c, arrays["color"].reshape(-1)[keep])

