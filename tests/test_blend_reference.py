"""The float64 blend reference (oracle.render_f64) and the per-pixel check built on it
(gpu_helpers.assert_blend_exact), on the CPU: the float32 oracle passes on every scene of
blend_scenes.py exactly the assertions the device faces (test_gpu_blend_exact.py), every scene
reaches the events it was built for on stable pixels, and the check catches a mutated blend."""
import numpy as np
import pytest

import blend_scenes as bs
from gpu_helpers import (IMG_ATOL, IMG_FRAC, IMG_MAX, UNSTABLE_CAP, assert_blend_exact,
                         assert_image_close, blend_reference)

f32 = np.float32


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            sc = bs.build(oracle_mod, name)
            bs.run(oracle_mod, sc)
            cache[name] = sc
        return cache[name]
    return get


def _events(ref):
    st, fl, F = ref["stable"], ref["flags"], {}
    for key, bit in (("skip", 1), ("cap", 2), ("term", 4), ("long", 8)):
        F[key] = int((st & ((fl & bit) != 0)).sum())
    return F


@pytest.mark.parametrize("name", bs.NAMES)
def test_oracle_passes_and_scene_reaches_its_events(oracle_mod, scenes, name):
    sc = scenes(name)
    orc = sc["orc"]
    ratio = assert_blend_exact(oracle_mod, orc, orc, sc["s"]["bg"], bs.features(sc, orc),
                               parity=False, what=name)
    assert ratio <= 1.0
    ref = orc["_f64"]
    st, ev = ref["stable"], _events(ref)
    assert 1.0 - st.mean() <= UNSTABLE_CAP
    nc = ref["n_contrib"]
    counts = orc["ranges"][:, 1].astype(np.int64) - orc["ranges"][:, 0]
    if name.startswith("chunk_edges_"):
        n = int(name.rsplit("_", 1)[1])
        assert (counts == n).all() and ev["term"] == 0
        assert st.all() and (nc == n).all()  # every splat contributes at every pixel
    elif name == "chunk_survivors":
        per_quadrant, margin = bs.quadrant_survivors(orc, 0, sc["W"])
        assert margin > 0.1  # ln(255 alpha_max): clear of the cull's ~1 % margins
        assert per_quadrant[:, 0].tolist() == [64, 63, 1, 0], per_quadrant
        assert per_quadrant[3, 1] == 5 and per_quadrant[2, 1] == 3, per_quadrant
    elif name.startswith("pads_"):
        assert (counts == 64).all() and st.all() and ev["term"] == 0
        for t in range(8):
            k = 63 - 2 * (8 * int(name[-1]) + t)
            per_quadrant, margin = bs.quadrant_survivors(orc, t, sc["W"])
            assert margin > 0.1 and per_quadrant[:, 0].tolist() == [k, 0, 0, 64 - k]
        assert nc.max() == 64  # the last list entry contributes somewhere
    elif name == "indefinite":
        co = orc["conic_opacity"].astype(np.float64)
        det = co[:, 0] * co[:, 2] - co[:, 1] ** 2
        assert ((det < 0) == sc["indefinite"]).all()
        assert 0.4 < sc["indefinite"].mean() < 0.6
        assert (counts == 256).all()  # list position = index: chunks all-PD, all-indefinite, mixed
        np.testing.assert_array_equal(orc["point_list"][:256], np.arange(256))
        assert ev["skip"] >= 50 and (nc[st] > 128).any()
    elif name == "on_centre":
        np.testing.assert_array_equal(orc["means2D"], sc["targets"])
        on_pixel = np.flatnonzero((sc["targets"] == np.round(sc["targets"])).all(axis=1))
        faint = [i for i in on_pixel if sc["s"]["g"].opacity[i, 0] == bs.A_MIN]
        assert len(on_pixel) == 16 and len(faint) >= 4
        for i in faint:  # alpha = opacity = float32(1/255) at the centre: it contributes
            x, y = (int(v) for v in sc["targets"][i])
            t = (y // 16) * 4 + x // 16
            pos = int(np.flatnonzero(orc["point_list"][orc["ranges"][t, 0]:orc["ranges"][t, 1]]
                                     == i)[0]) + 1
            assert orc["n_contrib"][y, x] >= pos
    elif name == "opacity_edges":
        assert ev["cap"] >= 50 and ev["term"] >= 1
        op = orc["conic_opacity"][orc["radii"] > 0, 3]
        for v in (0.0, 1e-40, bs.A_MIN, 1.0, 1.5):
            assert (op == f32(v)).sum() >= 6, v
        assert (op.view(np.uint32) == f32(1e-40).view(np.uint32)).any()  # still a denormal
    elif name == "opaque_stack":
        capped = st & ((ref["flags"] & 2) != 0)
        assert ev["term"] >= 50 and capped.sum() >= 50
        assert (nc[capped] == 1).all()
        np.testing.assert_allclose(ref["final_T"][capped], 1.0 - float(f32(0.99)), rtol=1e-12)
    elif name == "term_window":
        assert ev["term"] >= 50 and (nc[st] == 2).all()
        T = ref["final_T"][st]
        assert (T >= 1e-4).all() and (T < 1.1e-4).all()
    elif name.startswith("ragged_"):
        assert orc["num_rendered"] > 0 and (counts > 64).all()
        if sc["W"] * sc["H"] > 1:
            assert ev["term"] >= 1
    elif name == "synthetic":
        assert 1.0 - st.mean() < 0.01 and ref["bound"][st].max() < 1e-3


def test_reference_of_hand_computed_pixels(oracle_mod):
    """render_f64 on lists written by hand: one tile, three splats centred on pixel (3, 2) with
    unit conic.  At the centre: |power| = 0 <= dp, so the pixel is unstable; at (5, 2) every
    decision is clear and colour, T and n_contrib follow upstream's formula."""
    m2 = np.array([[3, 2]] * 3, f32)
    co = np.array([[1, 0, 1, 0.5], [1, 0, 1, 1.5], [1, 0, 1, 0.001]], f32)
    ft = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], f32)
    ref = oracle_mod.render_f64(np.array([[0, 3]], np.uint32), np.arange(3, dtype=np.uint32), m2,
                                co, ft, (0.0, 0.0, 1.0), 16, 16)
    assert not ref["stable"][2, 3] and ref["stable"][2, 5]
    g = np.exp(-2.0)
    a0, a1 = 0.5 * g, 1.5 * g
    T = (1 - a0) * (1 - a1)
    np.testing.assert_allclose(ref["color"][:, 2, 5], [a0, a1 * (1 - a0), T], rtol=1e-14)
    np.testing.assert_allclose(ref["final_T"][2, 5], T, rtol=1e-14)
    assert ref["n_contrib"][2, 5] == 2 and ref["flags"][2, 5] == 0
    # dominated by KAPPA u M (a0 + a1 (1 - a0)), M = (9^2 + 7^2) / 2 = 65
    lead = 16 * 2.0 ** -24 * 65 * (a0 + a1 * (1 - a0))
    assert lead < ref["bound"][2, 5] < 3 * lead
    # at the centre the second splat's alpha is capped at float32(0.99)
    assert ref["flags"][2, 3] & 2
    np.testing.assert_allclose(ref["final_T"][2, 3], 0.5 * (1 - float(f32(0.99))), rtol=1e-14)
    # far away nothing reaches 1/255
    assert ref["n_contrib"][15, 15] == 0 and ref["color"][2, 15, 15] == 1.0


MUTATIONS = ("drop_chunk_last", "threshold_254", "no_cap", "term_1.1e-4", "position",
             "swap_pair_blue")


def numpy_blend(orc, feats, bg, W, H, mutation=None):
    """Upstream's per-pixel blend in numpy float32, rounding every operation as the oracle does
    (the restatement of test_oracle_restatement.py py_render_pixel, a tile's 256 pixels at a
    time), with switchable mutations:
      drop_chunk_last  the entry at list position 63 of every tile (the last of chunk 0) is lost
      threshold_254    alpha < 1/254 skipped instead of 1/255
      no_cap           alpha not capped at 0.99
      term_1.1e-4      terminated at test_T < 1.1e-4 instead of 1e-4
      position         n_contrib is the list position instead of position + 1
      swap_pair_blue   list positions 2 and 3 of every tile blend each other's blue"""
    gx = (W + 15) // 16
    color = np.zeros((3, H, W), f32)
    final_T = np.zeros((H, W), f32)
    n_contrib = np.zeros((H, W), np.uint32)
    a_min = f32(1) / f32(254 if mutation == "threshold_254" else 255)
    t_min = f32(0.00011) if mutation == "term_1.1e-4" else f32(0.0001)
    bg = np.asarray(bg, f32)
    for t, (s, e) in enumerate(orc["ranges"]):
        x0, y0 = 16 * (t % gx), 16 * (t // gx)
        xs, ys = np.meshgrid(np.arange(x0, min(x0 + 16, W)), np.arange(y0, min(y0 + 16, H)))
        pfx, pfy = xs.astype(f32), ys.astype(f32)
        T = np.ones(xs.shape, f32)
        C = np.zeros((3,) + xs.shape, f32)
        last = np.zeros(xs.shape, np.uint32)
        done = np.zeros(xs.shape, bool)
        for j in range(int(s), int(e)):
            pos = j - int(s)
            if mutation == "drop_chunk_last" and pos == 63:
                continue
            gid = orc["point_list"][j]
            x, y = orc["means2D"][gid]
            a, b, c, o = orc["conic_opacity"][gid]
            rgb = np.array(feats[gid], f32)
            if mutation == "swap_pair_blue" and pos in (2, 3) and int(e) - int(s) >= 4:
                rgb[2] = feats[orc["point_list"][int(s) + (5 - pos)]][2]
            dx, dy = x - pfx, y - pfy
            power = f32(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
            with np.errstate(over="ignore", under="ignore"):
                alpha = o * np.exp(power)
            if mutation != "no_cap":
                alpha = np.minimum(f32(0.99), alpha)
            vis = ~done & ~(power > 0) & ~(alpha < a_min)
            test_T = T * (f32(1) - alpha)
            done |= vis & (test_T < t_min)
            acc = vis & ~done
            for ch in range(3):
                C[ch] = np.where(acc, C[ch] + rgb[ch] * alpha * T, C[ch])
            T = np.where(acc, test_T, T)
            last = np.where(acc, np.uint32(pos if mutation == "position" else pos + 1), last)
            if done.all():
                break
        sl = (slice(y0, y0 + xs.shape[0]), slice(x0, x0 + xs.shape[1]))
        final_T[sl], n_contrib[sl] = T, last
        for ch in range(3):
            color[ch][sl] = C[ch] + T * bg[ch]
    assert color.dtype == f32 and final_T.dtype == f32
    return dict(color=color, final_T=final_T, n_contrib=n_contrib)


def _old_bar_catches(got, orc):
    """Would assert_image_close + the 1e-4 n_contrib bar of assert_parity have failed?"""
    try:
        assert_image_close(got["color"], orc["color"])
        assert_image_close(got["final_T"], orc["final_T"], "final_T")
    except AssertionError:
        return True
    return float((got["n_contrib"] != orc["n_contrib"]).mean()) > 1e-4


# mutation -> (scene on which assert_blend_exact must catch it, does the old bar catch it there)
TEETH = {
    "drop_chunk_last": ("chunk_edges_129", True),
    "threshold_254": ("synthetic", True),
    "no_cap": ("opacity_edges", True),
    "term_1.1e-4": ("term_window", True),
    "position": ("synthetic", True),
    "swap_pair_blue": ("synthetic", True),
}


@pytest.mark.parametrize("name", ["synthetic", "chunk_edges_129", "opacity_edges", "term_window",
                                  "indefinite"])
def test_unmutated_numpy_blend_passes(oracle_mod, scenes, name):
    sc = scenes(name)
    orc = sc["orc"]
    got = numpy_blend(orc, bs.features(sc, orc), sc["s"]["bg"], sc["W"], sc["H"])
    assert_blend_exact(oracle_mod, got, orc, sc["s"]["bg"], bs.features(sc, orc), parity=False)
    np.testing.assert_array_equal(got["n_contrib"], orc["n_contrib"])
    assert not _old_bar_catches(got, orc)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_check_catches_a_mutated_blend(oracle_mod, scenes, mutation):
    """Each mutation of numpy_blend fails assert_blend_exact's stable-pixel assertions (the
    unstable pixels' allowance is not what catches it: the failure is asserted to name stable
    pixels).  Whether today's bar (assert_image_close + n_contrib at <= 1e-4 of pixels) would
    have caught the same mutation on the same scene, as asserted below:
      drop_chunk_last  chunk_edges_129  caught (every pixel loses a splat of alpha ~0.03)
      threshold_254    synthetic        caught (15 pixels lose a contributor)
      no_cap           opacity_edges    caught
      term_1.1e-4      term_window      caught (built so that every pixel sits in the window)
      position         synthetic        caught (n_contrib off by one wherever it is not 0)
      swap_pair_blue   synthetic        caught
    So at these frame sizes (<= 160x120) the old bar misses none of them: its 99.99 % / 1e-4
    shares allow fewer than six values and two pixels there, which makes it nearly per-pixel
    already.  Its gap opens with the frame: at 640x480 it lets 92 values and 30 pixels through,
    at 1080p 622 and 207, each off by up to 4e-3 or by one contributor
    (test_small_shift_on_few_pixels_passes_the_old_bar_only shows it at 160x120), where the
    per-pixel bound is <= ~2e-4 and typically 1e-6."""
    name, old = TEETH[mutation]
    sc = scenes(name)
    orc = sc["orc"]
    got = numpy_blend(orc, bs.features(sc, orc), sc["s"]["bg"], sc["W"], sc["H"], mutation)
    with pytest.raises(AssertionError, match="stable pixels"):
        assert_blend_exact(oracle_mod, got, orc, sc["s"]["bg"], bs.features(sc, orc),
                           parity=False)
    assert _old_bar_catches(got, orc) == old


def test_small_shift_on_few_pixels_passes_the_old_bar_only(oracle_mod, scenes):
    """What the statistical bar lets through on a frame of ordinary size: 5 pixels of the
    160x120 scene off by 3e-3 in one channel, and one n_contrib off by one, pass it; the
    per-pixel check fails on every one of them."""
    sc = scenes("synthetic")
    orc = sc["orc"]
    ref = blend_reference(oracle_mod, orc, sc["s"]["bg"], bs.features(sc, orc))
    ys, xs = np.nonzero(ref["stable"] & (ref["n_contrib"] > 0))
    got = {k: orc[k].copy() for k in ("color", "final_T", "n_contrib")}
    for y, x in zip(ys[:5], xs[:5]):
        got["color"][1, y, x] += f32(3e-3)
    assert 3e-3 < IMG_MAX and 5 <= (1 - IMG_FRAC) * got["color"].size and IMG_ATOL < 3e-3
    assert not _old_bar_catches(got, orc)
    with pytest.raises(AssertionError, match="5 stable pixels beyond"):
        assert_blend_exact(oracle_mod, got, orc, sc["s"]["bg"], parity=False)
    got = {k: orc[k].copy() for k in ("color", "final_T", "n_contrib")}
    got["n_contrib"][ys[7], xs[7]] -= 1
    assert not _old_bar_catches(got, orc)
    with pytest.raises(AssertionError, match="n_contrib differs at 1 stable pixels"):
        assert_blend_exact(oracle_mod, got, orc, sc["s"]["bg"], parity=False)
