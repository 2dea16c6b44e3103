"""CPU: pins the reference of the absolute means2D gradient (absgrad_reference) to the reference
the other gradients are held to (grad_reference / plane_grad_reference), re-measures the float32
spread the GPU tolerance is built from, and checks the condition on the cancellation scene."""
import numpy as np
import pytest

import absgrad_reference as ab
import grad_reference as gr
import grad_scenes
import oracle
import plane_grad_reference as pg
from gpu_helpers import run_oracle

_cache = {}


def _oracle(sc):
    if "orc" not in sc:
        sc["orc"] = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"],
                               cov3D_precomp=sc["cov6"])
    return sc["orc"]


def _ref64(name, loss):
    if (name, loss) not in _cache:
        sc = grad_scenes.get(name)
        orc = _oracle(sc)
        dL, dLp = ab.loss_gradients(sc, loss)
        _cache[(name, loss)] = ab.scene_abs_gradients(sc, (orc["ranges"], orc["point_list"]),
                                                      orc["radii"], dL, dLp)
    return _cache[(name, loss)]


@pytest.mark.parametrize("name,loss", ab.CASES)
def test_signed_sums_are_the_existing_reference(name, loss):
    """The per-pixel gradients summed with their signs are scene_gradients' means2D_px (and, in
    upstream's units, its means2D) to float64 rounding; no decision near its gate."""
    sc = grad_scenes.get(name)
    orc, r = _oracle(sc), _ref64(name, loss)
    assert r["near"] == (0, 0)
    lists = (orc["ranges"], orc["point_list"])
    if loss == "colour":
        ref = gr.scene_gradients(sc, lists, orc["radii"], sc["dL"])
    else:
        ref = pg.scene_gradients(sc, lists, orc["radii"], *pg.loss_gradients(sc, loss))
    assert np.abs(ref["means2D_px"]).max() > 0
    assert gr.rel_err(r["means2D_px_signed"], ref["means2D_px"]) <= 1e-12
    assert gr.rel_err(r["means2D_signed"], ref["means2D"]) <= 1e-12


@pytest.mark.parametrize("name,loss", ab.CASES)
def test_abs_dominates_signed_and_zeros(name, loss):
    sc = grad_scenes.get(name)
    orc, r = _oracle(sc), _ref64(name, loss)
    a, s = r["means2D_abs"], r["means2D_signed"]
    assert a.shape == (len(orc["radii"]), 3) and (a[:, 2] == 0).all()
    assert (a >= np.abs(s)).all() and (a >= 0).all()
    assert (a[:, :2].sum(0) > np.abs(s[:, :2]).sum(0) * 1.5).all()  # the signs do cancel here
    assert (a[orc["radii"] == 0] == 0).all()
    if name == "edges":
        assert (orc["radii"] == 0).sum() >= 5


def test_float32_spread_constants():
    """F32_SPREAD and ROW_SPREAD (the GPU tests' yardsticks) are what a float32 evaluation of the
    reference gives here, to within a factor 2 either way."""
    seen, seen_row = {}, {}
    for name, loss in ab.CASES:
        sc = grad_scenes.get(name)
        orc = _oracle(sc)
        seen[(name, loss)], seen_row[(name, loss)] = ab.spread(
            sc, (orc["ranges"], orc["point_list"]), orc["radii"], loss, _ref64(name, loss))
    print({k: f"{v:.3e}" for k, v in seen.items()})
    print({k: f"{v:.3e}" for k, v in seen_row.items()})
    f, f_row = max(seen.values()), max(seen_row.values())
    assert 0.5 * f <= ab.F32_SPREAD <= 2.0 * f, (f, ab.F32_SPREAD)
    assert 0.5 * f_row <= ab.ROW_SPREAD <= 2.0 * f_row, (f_row, ab.ROW_SPREAD)


def test_cancellation_scene_condition():
    """The scene of the GPU cancellation test: the Gaussian sits on the tile's centre, is isotropic
    on screen, and the reference's signed gradient is at most CANCEL_RATIO of its absolute one."""
    sc = ab.cancellation_scene()
    orc = _oracle(sc)
    assert (orc["radii"] > 0).all() and orc["num_rendered"] == 1
    assert (orc["means2D"] == np.float32(7.5)).all()
    co = orc["conic_opacity"][0]
    assert co[0] == co[2] and co[1] == 0
    dL = sc["dL"]
    assert (dL == dL[:, :, ::-1]).all() and (dL == dL[:, ::-1, :]).all()
    r = ab.scene_abs_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"], dL)
    assert r["near"] == (0, 0)
    a, s = r["means2D_abs"][0, :2], np.abs(r["means2D_signed"][0, :2])
    assert (a > 1.0).all() and (s <= ab.CANCEL_RATIO * a).all()
