"""CPU: the numpy restatement of the nearest-neighbour kernel's algorithm (knn_reference.boxed:
Morton order, boxes of 256, the outward visit, the two prunes) equals the brute-force statement of
include/gsr.h bit for bit on every scene, and every way of getting it wrong that the tests are
meant to catch is caught by a named scene."""
import numpy as np
import pytest

import knn_reference as kr
import knn_scenes as ks


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ks.NAMES)
def test_boxed_equals_brute(name):
    xyz = ks.scenes()[name]
    want = kr.brute_cached(xyz)
    stats = {}
    got = kr.boxed(xyz, stats=stats)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert want.shape == (len(xyz),) and want.dtype == np.float32 and np.isfinite(want).all()
    nb = (len(xyz) + 255) // 256
    assert stats["scanned"].shape == (nb,) and (stats["scanned"] >= 1).all()
    assert (stats["scanned"] <= nb).all()


def test_small_clouds_average_the_neighbours_they_have():
    s = ks.scenes()
    assert kr.brute(s["n1"]).tolist() == [0.0]
    a, b = s["n2"].astype(np.float32)
    d = a - b
    d01 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    np.testing.assert_array_equal(_bits(kr.brute(s["n2"])), _bits(np.array([d01, d01])))
    three = kr.brute(s["n3"])
    dd = kr._dist(s["n3"], s["n3"])
    for i in range(3):
        lo, hi = sorted(float(dd[i, j]) for j in range(3) if j != i)
        assert three[i] == (np.float32(lo) + np.float32(hi)) / np.float32(2)
    assert kr.brute(np.zeros((0, 3), np.float32)).shape == (0,)
    assert kr.boxed(np.zeros((0, 3), np.float32)).shape == (0,)


def test_expected_values_of_the_degenerate_scenes():
    s = ks.scenes()
    assert not kr.brute_cached(s["duplicates"]).any()
    assert not kr.brute_cached(s["identical"]).any()
    # the lattice: an inner point has six neighbours at distance 1
    lat = kr.brute_cached(s["lattice"])
    inner = ((s["lattice"] > 0) & (s["lattice"] < 11)).all(1)
    assert (lat[inner] == 1.0).all() and lat.max() == 1.0
    # the isolated pair: each other at 0.1, then two points of the cloud some 85 units away
    pair = kr.brute_cached(s["isolated_pair"])[-2:]
    assert (pair > 4000.0).all()


def test_unaligned_view_holds_the_same_rows():
    xyz = ks.scenes()["unaligned"]
    view = ks.offset_rows(xyz)
    assert view.ctypes.data % 16 == 4 and view.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(view, xyz)


MUTANTS = {
    "reach_1": (dict(reach=1), ks.REACH_SCENES),
    "reach_2": (dict(reach=2), ks.REACH_SCENES),
    "self_not_excluded": (dict(exclude_self=False), ("uniform", "lattice", "n2")),
    "bounds_from_first_point": (dict(first_point_bounds=True), ("uniform", "clusters", "slab")),
    "always_divide_by_3": (dict(always_three=True), ("n1", "n2", "n3")),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_are_caught(mutant):
    """Each wrong search differs from brute force on every scene named for it."""
    kw, names = MUTANTS[mutant]
    for name in names:
        xyz = ks.scenes()[name]
        wrong = int((_bits(kr.boxed(xyz, **kw)) != _bits(kr.brute_cached(xyz))).sum())
        print(f"{mutant} on {name}: {wrong} of {len(xyz)} rows differ")
        assert wrong > 0, (mutant, name)


def test_short_reach_is_wrong_on_many_rows_and_right_on_the_degenerate_scenes():
    s = ks.scenes()
    for name in ks.REACH_SCENES:
        want = _bits(kr.brute_cached(s[name]))
        r1 = int((_bits(kr.boxed(s[name], reach=1)) != want).sum())
        r2 = int((_bits(kr.boxed(s[name], reach=2)) != want).sum())
        assert r1 >= r2 >= 50, (name, r1, r2)
    for name in ("lattice", "duplicates", "line", "identical"):
        want = _bits(kr.brute_cached(s[name]))
        np.testing.assert_array_equal(_bits(kr.boxed(s[name], reach=1)), want)


def test_scaling_spread_constant():
    """SCALING_F32_SPREAD is what a float32 evaluation of log(sqrt(.)) strays from the float64
    reference over the scenes, within a factor 2."""
    measured = kr.scaling_spread(ks.scenes().values())
    print(f"measured {measured:.4g}, recorded {kr.SCALING_F32_SPREAD:.4g}")
    assert 0.5 * measured <= kr.SCALING_F32_SPREAD <= 2.0 * measured
    d = np.array([0.0, 1e-9, 1.0], np.float32)
    np.testing.assert_allclose(kr.scaling_reference(d)[:2], 0.5 * np.log(1e-7), rtol=1e-12)
    assert kr.scaling_reference(d)[2] == 0.0
