"""CPU: pins the per-row yardstick of the backward tests (row_grad_reference): its closed-form sums
against autograd of the references, pair by pair on the toy scenes; the float32 spread the GPU
bound is built from, re-measured; and the gap it closes, shown without a GPU -- mutations of the
float64 reference that today's norm-wise check (rel_err <= bound) lets through and row_err does
not.  Everything here comes from the C oracle's lists and the float64 references alone."""
import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import grad_reference as gr
import oracle
import row_grad_reference as rr
from gpu_helpers import run_oracle

_cases = {}


def _lists(sc):
    if "orc" not in sc:
        sc["orc"] = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"],
                               cov3D_precomp=sc["cov6"])
    return (sc["orc"]["ranges"], sc["orc"]["point_list"]), sc["orc"]["radii"]


def _case(name, planes):
    """(sc, ref, sums, S) of a scene and loss, once per module."""
    if (name, planes) not in _cases:
        sc, dL, dLp = rr.case(name)
        lists, radii = _lists(sc)
        _cases[(name, planes)] = (sc,) + rr.scene_scales(sc, lists, radii, dL,
                                                         dLp if planes else None)
    return _cases[(name, planes)]


def _keys(ref, S):
    return [k for k in S if k in ref and k not in ("tile", "pos")]


@pytest.mark.parametrize("planes", (False, True), ids=("colour", "planes"))
@pytest.mark.parametrize("name", rr.SCENES)
def test_sums_equal_autograd(name, planes):
    """The closed form's signed sums are autograd's 2D gradients of the reference to within
    1e-11 x A2d per word, and zero wherever A2d is."""
    sc, ref, sums, S = _case(name, planes)
    assert set(sums["sum"]) == {"means2D_px", "conic", "opacity", "rgb"} | ({"depths"} if planes else set())
    for k, v in sums["sum"].items():
        want = ref[k].reshape(v.shape)
        e, i, zeros = rr.row_err(v, want, sums["A"][k])
        print(f"{name}/{planes}: {k} max |sum - autograd| / A = {e:.2e}")
        assert e <= 1e-11 and zeros, (k, e, i)
        assert (want[sums["A"][k] == 0] == 0).all() and (sums["A"][k] >= np.abs(v)).all(), k
    # the rows with a scale are the composited ones, and each names a tile that lists it
    comp = sums["A"]["rgb"].max(1) > 0 if not planes else sums["A"]["depths"][:, 0] > 0
    assert comp.any() and ((sums["tile"] >= 0) == comp).all()
    ranges = np.asarray(_lists(sc)[0][0]).reshape(-1, 2).astype(np.int64)
    for i in np.flatnonzero(comp)[:50]:
        r0 = ranges[sums["tile"][i], 0]
        assert _lists(sc)[0][1][r0 + sums["pos"][i]] == i


@pytest.mark.parametrize("planes", (False, True), ids=("colour", "planes"))
@pytest.mark.parametrize("name", ("chain", "precomputed"))
def test_closed_form_pair_by_pair(name, planes):
    """On the toy scenes every (pixel, position) contribution of the closed form is the gradient
    autograd leaves in that pair's own leaves: to 1e-12 of the word's largest term in the tile."""
    sc, dL, dLp = rr.case(name)
    _, ref, _, _ = _case(name, planes)
    lists, radii = _lists(sc)
    cam = gr.camera_constants(sc["s"])
    with torch.no_grad():
        lv = gr.leaves(sc, torch.float64)
        m2, conic, rgb, _, _ = gr.project(cam, radii, lv["means3D"], lv["means2D"],
                                          lv.get("scales"), lv.get("rotations"), lv.get("cov3D"),
                                          lv.get("shs"), lv.get("colors"))
        z = rr.pg.view_depth(cam, radii, lv["means3D"])
    rec, p = (m2, conic, lv["opacity"].detach(), rgb), (dLp if planes else None)
    mine = rr.blend_sums(lists, rec, ref["gates"][1], sc["W"], sc["H"], sc["s"]["bg"], dL, p, z,
                         keep=True)["terms"]
    theirs = rr.pixel_terms(lists, rec, ref["gates"][1], sc["W"], sc["H"], sc["s"]["bg"], dL, p, z)
    assert set(mine) == set(theirs) and len(mine) >= 4
    pairs = 0
    for tile, (ids, t) in mine.items():
        assert (theirs[tile][0] == ids).all()
        for k, v in t.items():
            w = theirs[tile][1][k]
            assert v.shape == w.shape
            assert np.abs(v - w).max() <= 1e-12 * np.abs(w).max(), (tile, k)
        pairs += t["opacity"].size
    assert pairs > 10000


def _spread(name, planes):
    sc, ref, _, S = _case(name, planes)
    _, dL, dLp = rr.case(name)
    lists, radii = _lists(sc)
    r32 = rr.reference(sc, lists, radii, dL, dLp if planes else None, torch.float32, ref["gates"])
    out = {}
    for k in _keys(ref, S):
        e, _, zeros = rr.row_err(r32[k], ref[k], S[k])
        assert zeros, (name, k)
        if np.asarray(S[k]).max() > 0:
            out[k] = e
    return out


def test_row_spread_constants():
    """ROW_SPREAD (the GPU tests' yardstick) is what a float32 evaluation of the references gives
    here in units of S, to within a factor 2 either way; a float32 evaluation is exactly zero
    wherever S is."""
    seen = {}
    for name in rr.SCENES:
        for planes in (False, True):
            for k, e in _spread(name, planes).items():
                seen[k] = max(seen.get(k, 0.0), e)
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(rr.ROW_SPREAD)
    for k, f in seen.items():
        assert 0.5 * f <= rr.ROW_SPREAD[k] <= 2.0 * f, (k, f, rr.ROW_SPREAD[k])


# ---- the gap, shown without a GPU -------------------------------------------------------------------
MUTATED = ("wall", "long_lists")


def _today(name, key):
    return fs.bound(name, "colour", key) if name in fs.NAMES else gr.bound(key)


def _rowmax(v):
    return np.abs(v.reshape(len(v), -1)).max(1)


def _small_rows(name, key, v, k=1.0, behind=True):
    """The composited rows whose largest entry lies below k x today's bound x max|ref|; on wall
    (behind) only the Gaussians behind the near layer."""
    m = _rowmax(v)
    sel = (m > 0) & (m < k * _today(name, key) * np.abs(v).max())
    if name == "wall" and behind:
        sel[:fs.FRONT] = False
    return np.flatnonzero(sel)


def _verdicts(name, ref, S, mutated):
    """Per mutated tensor: (passes today's check, fails the row check)."""
    out = {}
    for k, v in mutated.items():
        today = gr.rel_err(v, ref[k]) <= _today(name, k)
        e, _, zeros = rr.row_err(v, ref[k], S[k])
        out[k] = (today, e > rr.bound(k) or not zeros)
        print(f"{name}: {k:11s} today's check {'passes' if today else 'fails'}, row_err / bound = "
              f"{e / rr.bound(k):.3g}")
    return out


def _push(sc, radii, sums):
    """The 3D gradients of mutated 2D sums: project's backward with them as grad_outputs."""
    lv = gr.leaves(sc, torch.float64)
    m2, conic, rgb, _, _ = gr.project(gr.camera_constants(sc["s"]), radii, lv["means3D"],
                                      lv["means2D"], lv.get("scales"), lv.get("rotations"),
                                      lv.get("cov3D"), lv.get("shs"), lv.get("colors"))
    keys = [k for k in ("means3D", "means2D", "scales", "rotations", "shs") if k in lv]
    grads = torch.autograd.grad([m2, conic, rgb], [lv[k] for k in keys],
                                [torch.as_tensor(sums[k]) for k in ("means2D_px", "conic", "rgb")])
    out = {k: g.numpy() for k, g in zip(keys, grads)}
    out["opacity"] = sums["opacity"].reshape(-1, 1)
    return out


@pytest.mark.parametrize("name", MUTATED)
def test_a_zeroed_small_rows(name):
    """Mutation a: every row below today's allowance (wall: of the Gaussians behind the near
    layer) set to zero.  Today's check passes every tensor; the row check fails every tensor that
    has such a row."""
    sc, ref, sums, S = _case(name, False)
    mutated = {}
    for k in _keys(ref, S):
        rows = _small_rows(name, k, ref[k])
        if len(rows):
            mutated[k] = ref[k].copy()
            mutated[k][rows] = 0.0
    assert len(mutated) >= (9 if name == "wall" else 2), sorted(mutated)
    v = _verdicts(name, ref, S, mutated)
    assert all(today and row for today, row in v.values()), v


@pytest.mark.parametrize("name", MUTATED)
def test_b_one_percent_on_the_lowest_third(name):
    """Mutation b: the third of the composited rows with the smallest magnitude times 1.01.  The
    row check fails every tensor.  Today's check passes every tensor of wall but opacity (whose
    rows span the fewest decades: its lowest third reaches within two decades of the maximum); of
    long_lists it passes the tensors whose lowest third lies that far down (means3D, means2D and
    the blend's position word among them) and sees the others."""
    sc, ref, sums, S = _case(name, False)
    mutated = {}
    for k in _keys(ref, S):
        m = _rowmax(ref[k])
        rows = np.flatnonzero(m > 0)
        rows = rows[np.argsort(m[rows])][:len(rows) // 3]
        mutated[k] = ref[k].copy()
        mutated[k][rows] *= 1.01
    v = _verdicts(name, ref, S, mutated)
    assert all(row for _, row in v.values()), v
    unseen = {k for k, (today, _) in v.items() if today}
    if name == "wall":
        assert unseen == set(v) - {"opacity"}, v
    else:
        assert {"means3D", "means2D", "means2D_px"} <= unseen, v


@pytest.mark.parametrize("name", MUTATED)
def test_c_last_contributing_position_dropped(name):
    """Mutation c: every pixel's last contributing list position adds nothing (the closed form
    recomputes the 2D sums, project's backward carries them to the inputs).  The row check fails
    every tensor.  This one is visible to today's metric as well -- the last position of a pixel
    that runs to the end of its list is no small addend -- in every tensor."""
    sc, ref, _, S = _case(name, False)
    _, dL, _ = rr.case(name)
    lists, radii = _lists(sc)
    _, dropped, _ = rr.scene_scales(sc, lists, radii, dL, None, ref=ref, drop_last=True)
    mutated = dict(dropped["sum"])
    mutated["opacity"] = mutated["opacity"].reshape(-1)
    mutated.update(_push(sc, radii, dropped["sum"]))
    mutated = {k: v.reshape(ref[k].shape) for k, v in mutated.items() if k in ref}
    assert len(mutated) >= 9
    v = _verdicts(name, ref, S, mutated)
    assert all(row for _, row in v.values()), v
    assert not any(today for today, _ in v.values()), v


@pytest.mark.parametrize("name", MUTATED)
def test_d_two_small_rows_swapped(name):
    """Mutation d: the two largest of the rows below half of today's allowance change places (half:
    two rows differ by at most the sum of their sizes).  On wall today's check passes every tensor
    that has two such rows (all but opacity) and the row check fails each.  No tensor of long_lists
    has two (its rows span 4.7 decades, and one or two lie that low), so there its two smallest
    composited rows change places: the row check fails every tensor, and this one is visible to
    today's metric as well."""
    sc, ref, sums, S = _case(name, False)
    mutated = {}
    for k in _keys(ref, S):
        rows = _small_rows(name, k, ref[k], 0.5)
        if name == "long_lists":  # (no tensor of it has two such rows)
            m = _rowmax(ref[k])
            rows = np.flatnonzero(m > 0)
            rows = rows[np.argsort(m[rows])][:2]
        if len(rows) >= 2:
            a, b = rows[np.argsort(_rowmax(ref[k])[rows])][-2:]
            mutated[k] = ref[k].copy()
            mutated[k][[a, b]] = ref[k][[b, a]]
    assert len(mutated) >= 8, sorted(mutated)
    v = _verdicts(name, ref, S, mutated)
    assert all(row for _, row in v.values()), v
    unseen = {k for k, (today, _) in v.items() if today}
    assert unseen == (set(v) if name == "wall" else set()), v
