"""Float64 restatement of the GL shadings (include/gsr.h gsr_forward_shaded; the fragment rule of
shaders/gau_frag.glsl:15-38 on the rasterizer's lists), vectorised numpy per tile over an oracle
result's ranges, point_list, means2D and conic_opacity plus the colours.

For a pixel (x, y), walking its tile's list in order, with the float32 record (mx, my), (a, b, c),
o, rgb taken to float64:
    dx = mx - x, dy = my - y, power = -(a dx^2 + c dy^2) / 2 - b dx dy
    shading 1 (billboard):  hit <=> |dx| <= ex and |dy| <= ey,  ex = 3 sqrt(c / det),
                            ey = 3 sqrt(a / det), det = a c - b^2 (a NaN extent never hits)
    shading 2, 3 (ball):    hit <=> power <= 0 and power > thr,  thr = ln(0.22f / o)
                            (alpha = min(0.99, o exp(power)) > 0.22, and 0.99 > 0.22; an opacity
                            <= 0.22f or NaN never hits; 0.22f is the float32 constant)
The first hit at list position k gives n_contrib = k + 1, final_T = 0 and the colour rgb (1, 2:
the float32 values themselves) or rgb exp(power) (3); no hit gives bg, final_T = 1, n_contrib = 0.

Stability.  u = 2^-24.  A float32 evaluation differs from the above by at most:
  power: dp = KAPPA u M, M = (|a| Dx^2 + |c| Dy^2) / 2 + |b| Dx Dy, Dx = |dx| + 7, Dy = |dy| + 7,
    KAPPA = 16 -- the bound oracle.render_f64 (gsr_oracle.c) uses for a float32 quadratic form:
    upstream's order spends 5 roundings on it (1 on each of dx, dy, which enter every term twice,
    2 per product chain, 1 per sum), a form expanded about any point of the pixel's 8x8 quadrant
    about 13, and the +7 covers the terms of such an expansion, so the bound does not depend on
    how a kernel stages the splat;
  thr: dt = 4 u (1 + |thr|): the quotient 0.22f / o rounds once (u on the argument, so u on its
    logarithm), a logarithm good to 1 ulp adds 2 u |thr|; the factor 2 left over is slack for a
    log2-based evaluation (one more rounding of the product with ln 2);
  ex (ey): de = 8 u (ex + |dx|): the determinant from exact products rounds once or twice (2 u),
    the quotient once, the square root halves what it is given (1.5 u) and rounds once, the
    product with 3 once -- 3.5 u ex -- and dx rounds once (u |dx|); the rest is slack.
An entry's outcome is uncertain when one of its decisions (power against 0, power against thr;
|dx| against ex, |dy| against ey) lies within these margins and no other decision of the entry
fails clear of them (a quad edge beside a pixel whose row is clearly outside the quad decides
nothing).  Ball entries with o <= 0.22f are decided by that float32 comparison alone.  A pixel
is unstable when an entry at or before its hit -- any entry, without a hit -- is uncertain, or
(shading 3) when dp >= 1/4 at its hit (first order no longer holds).

Bound (shading 3, stable pixels): |rgb| exp(power) (expm1(dp) + 4 u) + 2^-149 per channel, taken
with max |rgb|: the power's error, an exp good to 1 ulp (2 u), the product (u), 1 u of slack, and
the denormal floor.  Shadings 1 and 2 copy bits: bound 0.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
KAPPA, C_THR, K_EXT = 16.0, 4.0, 8.0
O_MIN = np.float32(0.22)
BILLBOARD, FLAT_BALL, GAUSS_BALL = 1, 2, 3


def entry_tests(shading, dx, dy, a, b, c, o):
    """(hit, uncertain, power, dp) of list entries against pixels, broadcast over any shapes."""
    with np.errstate(all="ignore"):
        if shading == BILLBOARD:
            det = a * c - b * b
            ex, ey = 3.0 * np.sqrt(c / det), 3.0 * np.sqrt(a / det)
            ax, ay = np.abs(dx), np.abs(dy)
            hit = (ax <= ex) & (ay <= ey)
            mx = np.where(np.isfinite(ex), K_EXT * U * (ex + ax), 0.0)
            my = np.where(np.isfinite(ey), K_EXT * U * (ey + ay), 0.0)
            near = (np.abs(ax - ex) <= mx) | (np.abs(ay - ey) <= my)
            clear_fail = ~(ax <= ex + mx) | ~(ay <= ey + my)  # (a NaN extent fails clearly)
            return hit, near & ~clear_fail, None, None
        power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
        live = o > np.float64(O_MIN)  # (False for NaN)
        thr = np.log(np.float64(O_MIN) / o)
        Dx, Dy = np.abs(dx) + 7.0, np.abs(dy) + 7.0
        dp = KAPPA * U * (0.5 * (np.abs(a) * Dx * Dx + np.abs(c) * Dy * Dy) + np.abs(b) * Dx * Dy)
        dt = dp + C_THR * U * (1.0 + np.abs(thr))
        hit = live & (power <= 0.0) & (power > thr)
        near = (np.abs(power) <= dp) | (np.abs(power - thr) <= dt)
        clear_fail = (power > dp) | (power < thr - dt)
        return hit, live & near & ~clear_fail, power, dp


def render(ranges, point_list, means2D, conic_opacity, features, bg, W, H, shading) -> dict:
    """color [3,H,W] (float32 bit copies for shadings 1, 2; float64 for 3), final_T, n_contrib,
    stable, bound and list_len (the pixel's tile's list length), all [H,W]."""
    assert shading in (BILLBOARD, FLAT_BALL, GAUSS_BALL)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    ranges = np.asarray(ranges).reshape(gx * gy, 2).astype(np.int64)
    feats32 = np.ascontiguousarray(features, np.float32).reshape(-1, 3)
    bg32 = np.asarray(bg, np.float32).reshape(3)
    exact = shading != GAUSS_BALL
    color = np.empty((3, H, W), np.float32 if exact else np.float64)
    color[:] = bg32[:, None, None]
    final_T = np.ones((H, W), np.float64)
    n_contrib = np.zeros((H, W), np.uint32)
    stable = np.ones((H, W), bool)
    bound = np.zeros((H, W), np.float64)
    list_len = np.zeros((H, W), np.int64)
    for t in range(gx * gy):
        x0, y0 = 16 * (t % gx), 16 * (t // gx)
        xs, ys = np.arange(x0, min(x0 + 16, W)), np.arange(y0, min(y0 + 16, H))
        X, Y = (v.reshape(-1) for v in np.meshgrid(xs, ys))
        ids = np.asarray(point_list[ranges[t, 0]:ranges[t, 1]], np.int64)
        list_len[Y, X] = len(ids)
        if len(ids) == 0:
            continue
        m2 = np.asarray(means2D, np.float32).reshape(-1, 2)[ids].astype(np.float64)
        co = np.asarray(conic_opacity, np.float32).reshape(-1, 4)[ids].astype(np.float64)
        dx, dy = m2[:, 0:1] - X[None, :], m2[:, 1:2] - Y[None, :]
        hit, unc, power, dp = entry_tests(shading, dx, dy, co[:, 0:1], co[:, 1:2], co[:, 2:3],
                                          co[:, 3:4])
        any_hit = hit.any(axis=0)
        k = np.where(any_hit, hit.argmax(axis=0), len(ids) - 1)  # scan all without a hit
        upto = np.arange(len(ids))[:, None] <= k[None, :]
        unstable = (unc & upto).any(axis=0)
        hx, hy, hk = X[any_hit], Y[any_hit], k[any_hit]
        n_contrib[hy, hx] = hk + 1
        final_T[hy, hx] = 0.0
        rgb = feats32[ids[hk]]  # [n_hit, 3] float32
        if exact:
            color[:, hy, hx] = rgb.T
        else:
            p, d = power[hk, np.flatnonzero(any_hit)], dp[hk, np.flatnonzero(any_hit)]
            e = np.exp(p)
            color[:, hy, hx] = rgb.T.astype(np.float64) * e
            bound[hy, hx] = np.abs(rgb).max(axis=1) * e * (np.expm1(d) + 4.0 * U) + 2.0 ** -149
            unstable[np.flatnonzero(any_hit)] |= ~(d < 0.25)
        stable[Y, X] = ~unstable
    return dict(color=color, final_T=final_T, n_contrib=n_contrib, stable=stable, bound=bound,
                list_len=list_len)


def render_loop(ranges, point_list, means2D, conic_opacity, features, bg, W, H, shading) -> dict:
    """The same by a per-pixel, per-entry Python loop (the check of the vectorised form)."""
    gx = (W + 15) // 16
    ranges = np.asarray(ranges).reshape(-1, 2)
    m2 = np.asarray(means2D, np.float32).reshape(-1, 2)
    co = np.asarray(conic_opacity, np.float32).reshape(-1, 4)
    feats32 = np.ascontiguousarray(features, np.float32).reshape(-1, 3)
    color = np.empty((3, H, W), np.float64)
    color[:] = np.asarray(bg, np.float32).reshape(3).astype(np.float64)[:, None, None]
    final_T = np.ones((H, W))
    n_contrib = np.zeros((H, W), np.uint32)
    stable = np.ones((H, W), bool)
    bound = np.zeros((H, W))
    f = np.float64
    for y in range(H):
        for x in range(W):
            r0, r1 = (int(v) for v in ranges[(y // 16) * gx + x // 16])
            for j in range(r0, r1):
                i = int(point_list[j])
                hit, unc, power, dp = entry_tests(
                    shading, f(m2[i, 0]) - x, f(m2[i, 1]) - y, f(co[i, 0]), f(co[i, 1]),
                    f(co[i, 2]), f(co[i, 3]))
                if unc:
                    stable[y, x] = False
                if hit:
                    rgb = feats32[i].astype(np.float64)
                    if shading == GAUSS_BALL:
                        e = np.exp(power)
                        rgb = rgb * e
                        bound[y, x] = (np.abs(feats32[i]).max() * e * (np.expm1(dp) + 4.0 * U)
                                       + 2.0 ** -149)
                        if not dp < 0.25:
                            stable[y, x] = False
                    color[:, y, x] = rgb
                    final_T[y, x] = 0.0
                    n_contrib[y, x] = j - r0 + 1
                    break
    return dict(color=color, final_T=final_T, n_contrib=n_contrib, stable=stable, bound=bound)


def reported_entry(ranges, point_list, means2D, conic_opacity, W, H, n_contrib) -> dict:
    """Per pixel, the list entry a result's n_contrib names (its tile's entry at position
    n_contrib - 1): id [H,W] (-1 where n_contrib is 0) and, in float64, its power and dp there.
    exp(p + d) differs from exp(p) by at most exp(p) expm1(|d|) for any d, so
    |rgb| exp(power) (expm1(dp) + 4 u) bounds the gaussian ball's colour at any pixel whose hit
    is this entry, stable or not."""
    gx = (W + 15) // 16
    ranges = np.asarray(ranges).reshape(-1, 2).astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    nc = np.asarray(n_contrib).astype(np.int64)
    has = nc > 0
    pos = ranges[(yy // 16) * gx + xx // 16, 0] + nc - 1
    ids = np.where(has, np.asarray(point_list, np.int64)[np.where(has, pos, 0)], -1)
    i = np.where(has, ids, 0)
    m2 = np.asarray(means2D, np.float32).reshape(-1, 2)[i].astype(np.float64)
    co = np.asarray(conic_opacity, np.float32).reshape(-1, 4)[i].astype(np.float64)
    _, _, power, dp = entry_tests(FLAT_BALL, m2[..., 0] - xx, m2[..., 1] - yy, co[..., 0],
                                  co[..., 1], co[..., 2], co[..., 3])
    return dict(id=ids, power=power, dp=dp)


def reference(sc, orc, shading) -> dict:
    """render() of a scene's oracle result, computed once per (scene, shading) and kept in it."""
    key = f"_shade{shading}"
    if key not in orc:
        feats = orc["rgb"] if sc["colors"] is None else sc["colors"]
        orc[key] = render(orc["ranges"], orc["point_list"], orc["means2D"], orc["conic_opacity"],
                          feats, sc["s"]["bg"], sc["W"], sc["H"], shading)
        orc[key]["features"] = np.ascontiguousarray(feats, np.float32).reshape(-1, 3)
    return orc[key]
