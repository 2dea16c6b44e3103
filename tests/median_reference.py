"""References of the median planes (gsr_forward_surface), shared by
test_median_reference.py (CPU: the float32 restatement alone meets the assertions) and
test_gpu_median.py.

walk(orc, W, H, dtype): upstream's per-pixel composite on the oracle's float32 records and lists,
a tile at a time over the tile's 256 pixels.  dtype float64 is the reference (the arithmetic of
gsr_oracle.c oracle_render_f64: every operation in double, the constants 0.99f, 1/255f, 0.0001f as
their float32 values); dtype float32 is the restatement in upstream's operation order (numpy's
float32 exp in place of expf).  Per tile it keeps, for every list entry, whether each pixel
composites it and the transmittance in front of and behind it; from them the median position and id.

The check is an accept set.  delta, a per-pixel bound on |T_float32 - T_float64| for every prefix
of the pixel's composite, is the `bound` plane of oracle.render_f64 with features (1, 1, 1) and no
background (why that bounds every prefix T: DESIGN.md 3g; it must come out <= DELTA_MAX).  At a
pixel that render_f64 calls stable -- the float32 composite takes the float64 one's decisions --
the median id must be a composited splat k with T_k > 0.5 - delta and T_{k+1} <= 0.5 + delta, or
-1 if final_T > 0.5 - delta.  So that this cannot hold vacuously, at most UNSTABLE_CAP of a scene's
pixels may have more than one acceptable answer (a condition on the scene; chunk_edges_128, whose
pixels all share one T sequence that passes 0.5 between two faint splats, is exempt).
"""
from __future__ import annotations

import numpy as np

from gpu_helpers import UNSTABLE_CAP

F32 = np.float32
DELTA_MAX = 3e-4  # the project's largest derived blend bound: delta must not exceed it
UNCAPPED = ("chunk_edges_128",)


def walk(orc, W, H, dtype=np.float64):
    """{"tiles": [per tile None (empty list) or dict(ids [L], comp [L,256] bool, T_front [L,256],
    T_behind [L,256])], "final_T", "n_contrib", "median_pos" (list position, -1 none), "median_id"
    (-1 none): [H,W]}.  A tile's pixel l is (16 ty + l // 16, 16 tx + l % 16)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    m2 = orc["means2D"].astype(dtype)
    co = orc["conic_opacity"].astype(dtype)
    cap, amin, tmin = (dtype(F32(0.99)), dtype(F32(1.0) / F32(255.0)), dtype(F32(0.0001)))
    half, one, mhalf = dtype(0.5), dtype(1.0), dtype(-0.5)
    final_T = np.ones((H, W), dtype)
    n_contrib = np.zeros((H, W), np.uint32)
    median_pos = np.full((H, W), -1, np.int64)
    median_id = np.full((H, W), -1, np.int64)
    tiles = []
    ly, lx = np.divmod(np.arange(256), 16)
    for tile in range(gx * gy):
        ty, tx = divmod(tile, gx)
        r0, r1 = (int(v) for v in orc["ranges"][tile])
        ids = orc["point_list"][r0:r1].astype(np.int64)
        L = len(ids)
        px, py = tx * 16 + lx, ty * 16 + ly
        inside = (px < W) & (py < H)
        X, Y = px.astype(dtype), py.astype(dtype)
        T = np.ones(256, dtype)
        done = ~inside
        last = np.zeros(256, np.uint32)
        comp = np.zeros((L, 256), bool)
        T_front = np.ones((L, 256), dtype)
        T_behind = np.ones((L, 256), dtype)
        with np.errstate(all="ignore"):
            for j, i in enumerate(ids):
                dx, dy = m2[i, 0] - X, m2[i, 1] - Y
                a, b, c, o = co[i]
                power = mhalf * (a * dx * dx + c * dy * dy) - b * dx * dy
                alpha = np.fmin(cap, o * np.exp(power))  # (fminf: a NaN gives 0.99)
                vis = ~(power > 0) & ~(alpha < amin) & ~done
                test_T = T * (one - alpha)
                term = vis & (test_T < tmin)
                acc = vis & ~term
                comp[j], T_front[j] = acc, T
                T = np.where(acc, test_T, T)
                T_behind[j] = T
                last[acc] = j + 1
                done |= term
                if done.all():
                    T_front[j + 1:], T_behind[j + 1:] = T, T
                    break
        cross = comp & (T_front > half) & (T_behind <= half)
        assert (cross.sum(axis=0) <= 1).all()
        pos = np.where(cross.any(axis=0), cross.argmax(axis=0), -1) if L else np.full(256, -1)
        y, x = py[inside], px[inside]
        final_T[y, x] = T[inside]
        n_contrib[y, x] = last[inside]
        median_pos[y, x] = pos[inside]
        if L:
            median_id[y, x] = np.where(pos >= 0, ids[np.maximum(pos, 0)], -1)[inside]
        tiles.append(dict(ids=ids, comp=comp, T_front=T_front, T_behind=T_behind) if L else None)
    return dict(tiles=tiles, final_T=final_T, n_contrib=n_contrib, median_pos=median_pos,
                median_id=median_id)


def _tile_pixels(tile, W, H):
    gx = (W + 15) // 16
    ty, tx = divmod(tile, gx)
    ly, lx = np.divmod(np.arange(256), 16)
    px, py = tx * 16 + lx, ty * 16 + ly
    inside = (px < W) & (py < H)
    return py, px, inside


def reference(oracle, sc, orc):
    """The float64 walk of a scene with its accept sets, computed once per scene and kept in it:
    walk()'s dict plus stable, delta [H,W], accept (per tile [L,256] bool or None), allow_none
    [H,W] (-1 acceptable) and answers [H,W] (the size of the pixel's accept set)."""
    if "_median_ref" in sc:
        return sc["_median_ref"]
    W, H = sc["W"], sc["H"]
    P = len(orc["means2D"])
    f64 = oracle.render_f64(orc["ranges"], orc["point_list"], orc["means2D"],
                            orc["conic_opacity"], np.ones((P, 3), F32), np.zeros(3, F32), W, H)
    ref = walk(orc, W, H, np.float64)
    st = f64["stable"]
    # the walk restates oracle_render_f64: on stable pixels nothing but the last bits can differ
    assert (ref["n_contrib"] == f64["n_contrib"])[st].all()
    assert np.abs(ref["final_T"] - f64["final_T"])[st].max(initial=0.0) <= 1e-12
    delta = f64["bound"]
    assert delta.max() <= DELTA_MAX, f"delta {delta.max():.3e}: the derivation is wrong"
    allow_none = ref["final_T"] > 0.5 - delta
    answers = allow_none.astype(np.int64)
    accept = []
    for tile, t in enumerate(ref["tiles"]):
        if t is None:
            accept.append(None)
            continue
        py, px, inside = _tile_pixels(tile, W, H)
        d = np.zeros(256)
        d[inside] = delta[py[inside], px[inside]]
        acc = t["comp"] & (t["T_front"] > 0.5 - d) & (t["T_behind"] <= 0.5 + d)
        accept.append(acc)
        answers[py[inside], px[inside]] += acc.sum(axis=0)[inside]
    ref.update(stable=st, delta=delta, accept=accept, allow_none=allow_none, answers=answers)
    sc["_median_ref"] = ref
    return ref


def assert_scene_decides(ref, name):
    """The conditions on the scene: few unstable pixels, few pixels with more than one acceptable
    answer, none without any.  Returns the two shares."""
    assert (ref["answers"] >= 1).all(), f"{name}: a pixel without an acceptable answer"
    unstable = 1.0 - float(ref["stable"].mean())
    multi = float((ref["answers"] > 1).mean())
    print(f"{name}: delta max {ref['delta'].max():.3e}, unstable {unstable:.5f}, "
          f"multi-answer {multi:.5f}, distinct medians "
          f"{len(np.unique(ref['median_id'][ref['median_id'] >= 0]))}, "
          f"no surface {float((ref['median_id'] < 0).mean()):.4f}")
    assert unstable <= UNSTABLE_CAP, f"{name}: {unstable:.4f} of pixels unstable"
    if name not in UNCAPPED:
        assert multi <= UNSTABLE_CAP, f"{name}: {multi:.4f} of pixels have several answers"
    return unstable, multi


def assert_median_accepted(ref, sc, median_id, median_depth, depths, what):
    """median_id [H,W] against the accept sets on every stable pixel; median_depth [H,W] (or None)
    bit for bit depths[median_id], 0.0 for -1, on every pixel.  Returns how many stable pixels
    differ from the float64 median (all of them inside their accept sets)."""
    W, H = sc["W"], sc["H"]
    median_id = np.asarray(median_id)
    assert median_id.shape == (H, W) and median_id.dtype == np.int32, (what, median_id.dtype)
    P = len(depths)
    assert ((median_id >= -1) & (median_id < P)).all(), f"{what}: an id outside [-1, P)"
    ok = (median_id == -1) & ref["allow_none"]
    for tile, t in enumerate(ref["tiles"]):
        if t is None:
            continue
        py, px, inside = _tile_pixels(tile, W, H)
        got = np.full(256, -2, np.int64)
        got[inside] = median_id[py[inside], px[inside]]
        hit = ((t["ids"][:, None] == got[None, :]) & ref["accept"][tile]).any(axis=0)
        ok[py[inside], px[inside]] |= hit[inside]
    bad = ref["stable"] & ~ok
    assert not bad.any(), (f"{what}: median_id outside the accept set at {int(bad.sum())} stable "
                           f"pixels, first (y, x) {tuple(np.argwhere(bad)[0])}: got "
                           f"{median_id[tuple(np.argwhere(bad)[0])]}, float64 median "
                           f"{ref['median_id'][tuple(np.argwhere(bad)[0])]}")
    if median_depth is not None:
        median_depth = np.asarray(median_depth)
        assert median_depth.shape == (H, W) and median_depth.dtype == np.float32
        want = np.where(median_id >= 0, np.asarray(depths, F32)[np.maximum(median_id, 0)], F32(0))
        np.testing.assert_array_equal(median_depth.view(np.uint32),
                                      want.astype(F32).view(np.uint32),
                                      err_msg=f"{what}: median_depth is not depths[median_id]")
    differ = int((ref["stable"] & (median_id != ref["median_id"])).sum())
    print(f"{what}: {differ} stable pixels take another acceptable answer than the float64 median")
    return differ


def expected_depth(ref, sc, depths):
    """The expected depth of the covered part, sum z w / (1 - final_T), from the float64 walk
    ([H,W]; NaN where nothing is composited)."""
    W, H = sc["W"], sc["H"]
    out = np.full((H, W), np.nan)
    for tile, t in enumerate(ref["tiles"]):
        if t is None:
            continue
        py, px, inside = _tile_pixels(tile, W, H)
        w = np.where(t["comp"], t["T_front"] - t["T_behind"], 0.0)
        num = (w * np.asarray(depths, np.float64)[t["ids"]][:, None]).sum(axis=0)
        den = w.sum(axis=0)
        with np.errstate(all="ignore"):
            out[py[inside], px[inside]] = (num / den)[inside]
    return out
