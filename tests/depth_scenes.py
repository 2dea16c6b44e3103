"""Scenes, features and the float64 reference of the depth planes (gsr_forward_depth), shared by
test_depth_maps_host.py (CPU: the oracle alone meets the assertions) and test_gpu_depth_maps.py.

The planes are colour channels with the feature z or 1 / z in place of the colour (the twin
property), so the reference is oracle.render_f64 of the scene's own records and
lists with features (f, f, f) and no background, and the check is assert_blend_exact's: on the
reference's stable pixels the plane within the pixel's bound and n_contrib equal, on the others
within IMG_MAX max|f|, at most UNSTABLE_CAP of the pixels unstable.

Scenes: every scene of blend_scenes.py with precomputed colours (all but `synthetic`), and
  depth_range   64x32; 200 splats at view depths log-uniform in 0.3 .. 50 shuffled over the
                splats, sigma 1 .. 12 px, opacity 0.05 .. 0.95: z and 1 / z differ by orders of
                magnitude from splat to splat and from each other, so a swapped plane, a z taken by
                list position instead of by id, or a reciprocal approximation shows up.
"""
from __future__ import annotations

import numpy as np

import blend_scenes as bs
from gpu_helpers import IMG_MAX, UNSTABLE_CAP

F32 = np.float32
NAMES = tuple(n for n in bs.NAMES if n != "synthetic") + ("depth_range",)
PLANES = ("depth_map", "inv_depth_map")


def build(oracle, name):
    if name != "depth_range":
        sc = bs.build(oracle, name)
        assert sc["colors"] is not None
        return sc
    rng = np.random.default_rng(sum(map(ord, name)))
    W, H, n = 64, 32, 200
    depth = rng.permutation(np.exp(np.linspace(np.log(0.3), np.log(50.0), n)))
    return bs._splats(W, H, rng.uniform(-2, W + 2, n), rng.uniform(-2, H + 2, n), depth,
                      bs._iso(rng.uniform(1.0, 12.0, n)), rng.uniform(0.05, 0.95, n),
                      rng.uniform(0, 1, (n, 3)))


def zero_bg(sc):
    """The scene's inputs with a black background (the planes have no background term)."""
    return dict(sc["s"], bg=np.zeros(3, F32))


def features(depths, radii):
    """(z, 1 / z) per Gaussian as float32, from the `depths` output (the view-space z bits): the
    IEEE quotient; 0 for a Gaussian that is not rendered (radius 0: its depth is not written and
    it is in no list)."""
    z = np.where(radii > 0, depths, F32(1)).astype(F32)
    iz = (F32(1) / z).astype(F32)
    on = radii > 0
    return np.where(on, z, F32(0)).astype(F32), np.where(on, iz, F32(0)).astype(F32)


def triple(f):
    return np.repeat(np.asarray(f, F32)[:, None], 3, axis=1)


def reference(oracle, sc, orc):
    """{plane: render_f64 of the oracle's records and lists with features (f, f, f), bg 0},
    computed once per scene and kept in it.  (render_f64 directly: gpu_helpers.blend_reference
    keeps one result per oracle result, the colour's.)"""
    if "_depth_ref" not in sc:
        fz, fiz = features(orc["depths"], orc["radii"])
        W, H = sc["W"], sc["H"]
        sc["_depth_ref"] = {
            k: dict(oracle.render_f64(orc["ranges"], orc["point_list"], orc["means2D"],
                                      orc["conic_opacity"], triple(f), np.zeros(3, F32), W, H),
                    fmax=float(np.abs(f).max()) if len(f) else 0.0)
            for k, f in zip(PLANES, (fz, fiz))}
    return sc["_depth_ref"]


def assert_plane_exact(plane, n_contrib, ref, what):
    """One plane against its float64 reference; prints err / bound as assert_blend_exact does
    and returns it."""
    st = ref["stable"]
    share = 1.0 - float(st.mean()) if st.size else 0.0
    assert share <= UNSTABLE_CAP, f"{what}: {share:.4f} of pixels unstable"
    err = np.abs(plane.astype(np.float64) - ref["color"][0])
    ratio = float((err[st] / ref["bound"][st]).max()) if st.any() else 0.0
    print(f"{what}: unstable {share:.5f}, stable max err {err[st].max() if st.any() else 0.0:.3e}"
          f" = {ratio:.3f} of bound (max bound {ref['bound'][st].max() if st.any() else 0.0:.3e},"
          f" max |f| {ref['fmax']:.3g})")
    assert np.isfinite(plane).all(), f"{what}: non-finite values"
    if n_contrib is not None:
        bad_n = st & (n_contrib != ref["n_contrib"])
        assert not bad_n.any(), f"{what}: n_contrib differs at {int(bad_n.sum())} stable pixels"
    bad = st & ~(err <= ref["bound"])
    assert not bad.any(), (f"{what}: {int(bad.sum())} stable pixels beyond their bound, worst "
                           f"{ratio:.2f} x bound")
    worst = float(err[~st].max()) if (~st).any() else 0.0
    assert worst <= IMG_MAX * ref["fmax"], f"{what}: unstable pixel off by {worst}"
    return ratio
