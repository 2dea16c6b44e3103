"""The scenes of stop_scenes.py on the CPU, in the manner of test_blend_reference.py: the float32
oracle alone passes the float64 blend check (gpu_helpers.assert_blend_exact) on every scene, and
each scene does what it was built for, so that test_gpu_blend_stop.py drives the blend's early
exit where it claims to."""
import numpy as np
import pytest

import blend_scenes as bs
import stop_scenes as ss
from gpu_helpers import UNSTABLE_CAP, assert_blend_exact

CUTS = tuple(f"stop_{s}_cut" for s in ss.STOP_S)


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            sc = ss.build(oracle_mod, name)
            bs.run(oracle_mod, sc)
            cache[name] = sc
        return cache[name]
    return get


def _checked(oracle_mod, sc, name):
    orc = sc["orc"]
    ratio = assert_blend_exact(oracle_mod, orc, orc, sc["s"]["bg"], bs.features(sc, orc),
                               parity=False, what=name)
    assert ratio <= 1.0
    ref = orc["_f64"]
    assert 1.0 - ref["stable"].mean() <= UNSTABLE_CAP
    assert len(orc["ranges"]) == 1  # one tile: a list position is an index + 1
    s, e = (int(v) for v in orc["ranges"][0])
    np.testing.assert_array_equal(orc["point_list"][s:e], np.arange(e - s))
    return orc, ref, e - s


@pytest.mark.parametrize("name", ss.NAMES[:len(ss.STOP_S)])
def test_stop_S_terminates_every_pixel_at_S(oracle_mod, scenes, name):
    S = int(name.split("_")[1])
    orc, ref, n = _checked(oracle_mod, scenes(name), name)
    assert n == S + ss.N_AFTER and n > 64 * ((S + 63) // 64)  # followers reach the next chunk
    assert ref["stable"].all()
    for nc in (orc["n_contrib"], ref["n_contrib"]):
        assert (nc == S - 1).all()
    # the weak splats: alpha 0.02 .. 0.05 at every pixel, T clear of the 1e-4 edge at S-1 and S
    T = ref["final_T"]
    assert (T <= 0.98 * 0.0101).all() and (T >= 0.035 * 0.0099).all()
    co = orc["conic_opacity"]
    assert S >= 3 and (co[:S - 2, 3] >= 0.0225).all() and (co[:S - 2, 3] <= 0.05).all()
    assert (co[S - 2:, 3] == 1.0).all()
    # the head alone gives the same pixels (the device asserts the bits)
    cut = scenes(name + "_cut")
    oc, rc, nc_ = _checked(oracle_mod, cut, name + "_cut")
    assert nc_ == S
    for k in ("color", "final_T", "n_contrib"):
        np.testing.assert_array_equal(oc[k], orc[k], err_msg=k)


def test_stop_spread_quadrant_terminates_over_many_positions(oracle_mod, scenes):
    orc, ref, n = _checked(oracle_mod, scenes("stop_spread"), "stop_spread")
    assert n == ss.SPREAD_STOP + ss.N_AFTER
    nc, st = ref["n_contrib"].astype(np.int64), ref["stable"]
    np.testing.assert_array_equal(orc["n_contrib"][st], nc[st])
    # the other three quadrants: only the final pair terminates a pixel
    other = np.ones((16, 16), bool)
    other[:8, :8] = False
    assert (nc[other] == ss.SPREAD_STOP - 1).all() and st[other].all()
    # quadrant A: pixels done among the narrow splats (n_contrib + 1 = the terminating position),
    # spread over at least 24 positions of the first chunk, the rest at the final pair
    a = nc[:8, :8]
    early = a[a < ss.SPREAD_NARROW]
    print(f"stop_spread: quadrant A n_contrib {np.unique(a).tolist()}")
    assert early.size >= 12 and len(np.unique(early)) >= 6
    assert early.max() - early.min() >= 24 and early.max() + 1 <= ss.SPREAD_NARROW < 64
    assert (a == ss.SPREAD_STOP - 1).sum() >= 16  # most of the wave's lanes stay live to the end
    # the columns of rows 3 and 4 (half a pixel off the centres' row) go in order
    for row in (3, 4):
        assert a[row, 0] < a[row, 1] < a[row, 2] < a[row, 3] < ss.SPREAD_NARROW
        assert (a[row, 4:] == ss.SPREAD_STOP - 1).all()


def test_stop_never_terminates_no_pixel(oracle_mod, scenes):
    orc, ref, n = _checked(oracle_mod, scenes("stop_never"), "stop_never")
    assert n == 127 + ss.N_AFTER
    assert (orc["final_T"] >= 1e-4).all() and (ref["final_T"] >= 1e-3).all()
    assert (ref["flags"] & 4 == 0).all()  # no termination event
    assert (orc["n_contrib"] == n).all()


@pytest.mark.parametrize("name", ("stop_66", "stop_spread"))
def test_depth_and_median_references_decide(oracle_mod, scenes, name):
    """The references test_gpu_blend_stop.py holds the depth and the median planes to exist and
    decide on these scenes (conditions on the scene, as in the suites they come from)."""
    import depth_scenes as ds
    import median_reference as mr
    sc = scenes(name)
    orc = sc["orc"]
    ref = ds.reference(oracle_mod, sc, orc)
    for k in ds.PLANES:
        assert 1.0 - ref[k]["stable"].mean() <= UNSTABLE_CAP
    mr.assert_scene_decides(mr.reference(oracle_mod, sc, orc), name)
