"""Point clouds for the nearest-neighbour search (gsr_knn_mean_dist2): seeded, small, and each at or
near something the search can get wrong -- a box edge (boxes hold 256 sorted points), a Morton
seam, a tie, a degenerate axis, float32 cancellation.  Shared by the CPU tests of the reference
(test_knn_reference.py) and the GPU tests (test_gpu_knn.py).  No tests here."""
import functools

import numpy as np

f32 = np.float32
SMALL_N = (1, 2, 3, 4, 255, 256, 257, 513)


def _build():
    rng = np.random.default_rng(1)
    s = {}
    # more than 23 boxes: a block has to go on beyond its neighbours
    s["uniform"] = rng.random((6000, 3)).astype(f32)
    # eight Gaussian clusters of 700: boxes that overlap in space
    s["clusters"] = np.concatenate([rng.normal(c, 0.02, (700, 3))
                                    for c in rng.random((8, 3)) * 4]).astype(f32)
    # offset by 1e4: the differences cancel to a few float32 steps
    s["offset"] = (rng.random((3000, 3)) + 1e4).astype(f32)
    # a 12^3 integer lattice: ties everywhere
    s["lattice"] = np.stack(np.meshgrid(*[np.arange(12)] * 3), -1).reshape(-1, 3).astype(f32)
    # a slab 0.001 thick across x = 0.5, plus 300 uniform: the nearest neighbours lie across the
    # top Morton bit, far away in the sorted order
    s["slab"] = np.concatenate([rng.random((2000, 3)) * [0.001, 1, 1] + [0.4995, 0, 0],
                                rng.random((300, 3))]).astype(f32)
    # 300 points, each five times: every result is 0
    s["duplicates"] = np.repeat(rng.random((300, 3)).astype(f32), 5, 0)
    # 1,000 points on a line: two axes of zero extent
    s["line"] = np.stack([rng.random(1000), np.zeros(1000), np.zeros(1000)], 1).astype(f32)
    # 600 identical points: no extent at all
    s["identical"] = np.ones((600, 3), f32)
    # an isolated pair far from 1,500 uniform points: its third neighbour is in a far box
    s["isolated_pair"] = np.concatenate([rng.random((1500, 3)),
                                         np.array([[50, 50, 50], [50.1, 50, 50]])]).astype(f32)
    for n in SMALL_N:
        s["n%d" % n] = rng.random((n, 3)).astype(f32)
    # read through a pointer that is 4-byte but not 16-byte aligned (see offset_rows)
    s["unaligned"] = rng.random((777, 3)).astype(f32)
    return s


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> float32 (N, 3); the same arrays on every call: do not write into them."""
    out = _build()
    for a in out.values():
        a.setflags(write=False)
    return out


NAMES = tuple(_build().keys())
# the scenes on which a search that stops short of the far boxes is wrong on many rows; on the
# lattice, the duplicates, the line and the identical scene it is right
REACH_SCENES = ("uniform", "slab", "isolated_pair")


def offset_rows(xyz):
    """A copy of a (N, 3) float32 numpy array whose first word sits 4 bytes past a 16-byte
    boundary: the rows of `xyz`, read through a pointer that is not 16-byte aligned."""
    n = xyz.shape[0]
    raw = np.empty(3 * n + 4, f32)
    skew = (1 - raw.ctypes.data // 4) % 4  # words to one word past a 16-byte boundary
    view = raw[skew:skew + 3 * n].reshape(n, 3)
    view[:] = xyz
    assert view.ctypes.data % 16 == 4
    return view
