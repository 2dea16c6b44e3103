"""A numpy float64 evaluation of upstream's preprocessCUDA from the float32 inputs, with a bound
on what a correct float32 evaluation may differ from it -- the per-Gaussian counterpart of
oracle.render_f64 (the blend).  CPU only; used by test_preprocess_reference.py.

Every quantity is carried as a pair (value, err): the float64 value and an absolute bound on
the error of the float32 operation chain that upstream writes (forward.cu preprocessCUDA,
computeCov3D, computeCov2D, computeColorFromSH; auxiliary.h), propagated operation by operation
in upstream's order (running error analysis, first order plus the product of two errors):

    a + b : err_a + err_b + u |v|          a * b : |a| err_b + |b| err_a + err_a err_b + u |v|
    a / b : (err_a + |v| err_b) / (|b| - err_b) + u |v|       sqrt a : sqrt a - sqrt(a - err_a) + u |v|
    max, min : the larger err of the two (both are 1-Lipschitz); a float32 constant: err 0

u = 2^-24 (1 + 2^-10) is one correctly rounded float32 operation (the slack covers |v| being the
float64 value, not the rounded one); every operation also adds 2^-149 for a result that
underflows.  ndc2Pix runs in double upstream and rounds once.  Nothing is fitted to a run.

The conic c / det inherits its conditioning from the chain: det = a c - b b carries
u (|a c| + |b b|) plus what a, b, c carry, so the conic's relative bound grows as
(a c + b^2) / |det|.

Decisions (visible: z > 0.2, det != 0, a non-empty rect; the radius ceil and its saturation;
the four truncations of getRect) are taken on the float64 value; a Gaussian is `stable` only if
no decision changes anywhere within the bound of its argument.  `finite` is false where an
input is not finite or an intermediate leaves float32's range (the float32 chain then holds inf
or NaN where float64 holds a number).  Only stable, finite Gaussians are judged: decisions
equal, floats within their bound.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24 * (1.0 + 2.0 ** -10)
TINY = 2.0 ** -149
F32_MAX = 3.0e38
INT_MAX = 2 ** 31 - 1
F32 = np.float32

# upstream's constants, as the float32 values the kernels hold
SH_C0 = float(F32(0.28209479177387814))
SH_C1 = float(F32(0.4886025119029199))
SH_C2 = [float(F32(v)) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005,
                                 -1.0925484305920792, 0.5462742152960396)]
SH_C3 = [float(F32(v)) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658,
                                 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
                                 -0.5900435899266435)]
LOW_PASS = float(F32(0.3))
CLAMP = float(F32(1.3))
NEAR = float(F32(0.2))
LAMBDA_FLOOR = float(F32(0.1))


class E:
    """(value, err) arrays with float32 rounding added per operation; `over` collects, per
    Gaussian, whether any result left float32's range or was not finite."""
    over = None

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(np.float64(x))

    @staticmethod
    def _out(v, e):
        e = e + U * np.abs(v) + TINY
        bad = ~(np.abs(v) < F32_MAX)
        if E.over is not None and bad.shape == E.over.shape:
            E.over |= bad
        elif E.over is not None and bad.any():
            E.over |= bool(bad.all()) if bad.ndim == 0 else bad
        return E(v, e)

    def __add__(self, o):
        o = E.lift(o)
        return E._out(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.lift(o)
        return E._out(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.lift(o) - self

    def __neg__(self):
        return E(-self.v, self.e)

    def __mul__(self, o):
        o = E.lift(o)
        return E._out(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        v = self.v / o.v
        den = np.abs(o.v) - o.e
        e = np.where(den > 0, (self.e + np.abs(v) * o.e) / np.where(den > 0, den, 1.0), np.inf)
        return E._out(v, e)

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def sqrt(self):
        v = np.sqrt(self.v)
        return E._out(v, v - np.sqrt(np.maximum(self.v - self.e, 0.0)))

    def fmax(self, o):
        o = E.lift(o)
        return E(np.fmax(self.v, o.v), np.maximum(self.e, o.e))

    def fmin(self, o):
        o = E.lift(o)
        return E(np.fmin(self.v, o.v), np.maximum(self.e, o.e))


def _mat_mul(A, B):
    """glm operator*(mat3, mat3) on m[col][row] lists, upstream's sum order."""
    return [[(A[0][i] * B[j][0] + A[1][i] * B[j][1]) + A[2][i] * B[j][2] for i in range(3)]
            for j in range(3)]


def _transpose(A):
    return [[A[i][j] for i in range(3)] for j in range(3)]


def _cols(*a):
    return [[E.lift(a[3 * c + r]) for r in range(3)] for c in range(3)]


def _tp(p, M, k):
    return ((M[k] * p[0] + M[4 + k] * p[1]) + M[8 + k] * p[2]) + M[12 + k]


def _trunc_clamp(x, g):
    """min(g, max(0, f2i_sat(x))) for float64 x (finite)."""
    return np.minimum(g, np.maximum(0, np.trunc(np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1)))).astype(np.int64)


def evaluate(sc) -> dict:
    """The reference of a scene dict (preprocess_scenes / blend_scenes layout): per Gaussian
    visible, radius, rect (x0, y0, x1, y1), tiles; depth, means2D, conic, rgb as float64 with
    their bounds (`*_bound`); stable, finite and rgb_finite."""
    s = sc["s"]
    g = s["g"]
    P = len(g.xyz)
    W, H = int(s["W"]), int(s["H"])
    gx, gy = (W + 15) // 16, (H + 15) // 16
    with np.errstate(all="ignore"):
        E.over = ~np.isfinite(g.xyz.astype(np.float64)).all(axis=1)
        vm = [float(v) for v in np.asarray(s["view"], F32).reshape(-1)]
        pm = [float(v) for v in np.asarray(s["proj"], F32).reshape(-1)]
        p = [E(g.xyz[:, k]) for k in range(3)]
        pv = [_tp(p, vm, k) for k in range(3)]
        unstable = np.abs(pv[2].v - NEAR) <= pv[2].e
        in_frustum = pv[2].v > NEAR
        ph = [_tp(p, pm, k) for k in range(4)]
        p_w = 1.0 / (ph[3] + float(F32(0.0000001)))
        pp = [ph[0] * p_w, ph[1] * p_w]
        if sc.get("cov6") is not None:
            c6 = np.asarray(sc["cov6"], F32)
            E.over |= ~np.isfinite(c6.astype(np.float64)).all(axis=1)
            c = [E(c6[:, k]) for k in range(6)]
        else:
            E.over |= ~(np.isfinite(g.scale.astype(np.float64)).all(axis=1) &
                        np.isfinite(g.rot.astype(np.float64)).all(axis=1))
            mod = float(F32(s["scale_modifier"]))
            S = _cols(1, 0, 0, 0, 1, 0, 0, 0, 1)
            for k in range(3):
                S[k][k] = mod * E(g.scale[:, k])
            r, x, y, z = (E(g.rot[:, k]) for k in range(4))
            R = _cols(1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
                      2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
                      2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y))
            Mm = _mat_mul(S, R)
            Sig = _mat_mul(_transpose(Mm), Mm)
            c = [Sig[0][0], Sig[0][1], Sig[0][2], Sig[1][1], Sig[1][2], Sig[2][2]]
        tanx, tany = E(float(F32(s["tx"]))), E(float(F32(s["ty"])))
        fy = float(H) / (2.0 * tany)
        fx = float(W) / (2.0 * tanx)
        limx, limy = CLAMP * tanx, CLAMP * tany
        t = list(pv)
        t[0] = (t[0] / t[2]).fmax(-limx).fmin(limx) * t[2]
        t[1] = (t[1] / t[2]).fmax(-limy).fmin(limy) * t[2]
        tz2 = t[2] * t[2]
        J = _cols(fx / t[2], 0, -(fx * t[0]) / tz2, 0, fy / t[2], -(fy * t[1]) / tz2, 0, 0, 0)
        Wm = _cols(vm[0], vm[4], vm[8], vm[1], vm[5], vm[9], vm[2], vm[6], vm[10])
        T = _mat_mul(Wm, J)
        Vrk = _cols(c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5])
        cov = _mat_mul(_mat_mul(_transpose(T), _transpose(Vrk)), T)
        a, b, cc = cov[0][0] + LOW_PASS, cov[0][1], cov[1][1] + LOW_PASS
        det = a * cc - b * b
        unstable |= in_frustum & (np.abs(det.v) <= det.e)
        det_ok = det.v != 0
        di = 1.0 / det
        conic = [cc * di, -b * di, a * di]
        mid = 0.5 * (a + cc)
        root = (mid * mid - det).fmax(LAMBDA_FLOOR).sqrt()
        l1, l2 = mid + root, mid - root
        arg = 3.0 * l1.fmax(l2).sqrt()
        lo, hi = np.ceil(arg.v - arg.e), np.ceil(arg.v + arg.e)
        sat = lambda v: np.clip(v, -2.0 ** 31, float(INT_MAX))  # noqa: E731
        unstable |= in_frustum & det_ok & ~(sat(lo) == sat(hi))
        radius = sat(np.ceil(arg.v)).astype(np.int64)
        px = E(((pp[0].v + 1.0) * W - 1.0) * 0.5, pp[0].e * W * 0.5)
        py = E(((pp[1].v + 1.0) * H - 1.0) * 0.5, pp[1].e * H * 0.5)
        px, py = E._out(px.v, px.e), E._out(py.v, py.e)  # the one rounding to float
        rf = E(F32(radius).astype(np.float64))  # (float)max_radius
        q = [(px - rf) / 16.0, (py - rf) / 16.0, ((px + rf) + 16.0 - 1.0) / 16.0,
             ((py + rf) + 16.0 - 1.0) / 16.0]
        rect = []
        for k, qq in enumerate(q):
            gk = gx if k % 2 == 0 else gy
            r0 = _trunc_clamp(qq.v, gk)
            unstable |= in_frustum & det_ok & ((_trunc_clamp(qq.v - qq.e, gk) != r0) |
                                               (_trunc_clamp(qq.v + qq.e, gk) != r0) |
                                               ~np.isfinite(qq.v))
            rect.append(r0)
        tiles = (rect[2] - rect[0]) * (rect[3] - rect[1])
        visible = in_frustum & det_ok & (radius > 0) & (tiles > 0)
        geom_over = E.over.copy()
        cond = (np.abs(a.v * cc.v) + b.v * b.v) / np.abs(det.v)
        # colour
        rgb = None
        if sc.get("colors") is None:
            D = int(s["sh_degree"])
            M = g.sh.shape[1] // 3
            sh = np.asarray(g.sh, F32).reshape(P, M, 3)
            E.over = ~np.isfinite(sh.astype(np.float64)).all(axis=(1, 2))
            cp = [float(v) for v in np.asarray(s["campos"], F32).reshape(-1)]
            res = [SH_C0 * E(sh[:, 0, k]) for k in range(3)]
            if D > 0:
                d = [p[k] - cp[k] for k in range(3)]
                ln = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).sqrt()
                x, y, z = (v / ln for v in d)
                co = lambda m, k: E(sh[:, m, k])  # noqa: E731
                a1, a2, a3 = SH_C1 * y, SH_C1 * z, SH_C1 * x
                res = [res[k] - a1 * co(1, k) + a2 * co(2, k) - a3 * co(3, k) for k in range(3)]
                if D > 1:
                    xx, yy, zz = x * x, y * y, z * z
                    xy, yz, xz = x * y, y * z, x * z
                    bb = [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy),
                          SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
                    for k in range(3):
                        for m in range(5):
                            res[k] = res[k] + bb[m] * co(4 + m, k)
                    if D > 2:
                        ee = [SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z,
                              SH_C3[2] * y * (4.0 * zz - xx - yy),
                              SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy),
                              SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
                              SH_C3[6] * x * (xx - 3.0 * yy)]
                        for k in range(3):
                            for m in range(7):
                                res[k] = res[k] + ee[m] * co(9 + m, k)
            rgb = [(res[k] + 0.5).fmax(0.0) for k in range(3)]
            rgb_over = E.over.copy()
        E.over = None
    out = dict(visible=visible, radius=np.where(visible, radius, 0), tiles=np.where(visible, tiles, 0),
               rect=np.stack(rect, axis=1), stable=~unstable, finite=~geom_over,
               depth=pv[2].v, depth_bound=pv[2].e,
               means2D=np.stack([px.v, py.v], 1), means2D_bound=np.stack([px.e, py.e], 1),
               conic=np.stack([v.v for v in conic], 1), conic_bound=np.stack([v.e for v in conic], 1),
               conditioning=cond)
    if rgb is not None:
        out["rgb"] = np.stack([v.v for v in rgb], 1)
        out["rgb_bound"] = np.stack([v.e for v in rgb], 1)
        out["rgb_finite"] = ~rgb_over & np.isfinite(out["rgb_bound"]).all(axis=1)
    return out


FLOATS = (("depth", "depths"), ("means2D", "means2D"), ("conic", "conic_opacity"), ("rgb", "rgb"))


def check(ref, got, what="") -> dict:
    """A float32 preprocess result (the oracle's dict, or the HIP path's) against the reference:
    on stable, finite Gaussians the decisions are equal and every float of a visible one is
    within its bound.  Returns the unstable share and max err / bound per quantity."""
    judged = ref["stable"] & ref["finite"]
    share = 1.0 - float(ref["stable"][ref["finite"]].mean()) if ref["finite"].any() else 0.0
    vis = np.asarray(got["radii"]) > 0
    bad = judged & (vis != ref["visible"])
    assert not bad.any(), f"{what}: visibility differs at {np.flatnonzero(bad)[:8]}"
    bad = judged & (np.asarray(got["radii"]) != ref["radius"])
    assert not bad.any(), (f"{what}: radius differs at {np.flatnonzero(bad)[:8]}: "
                           f"{np.asarray(got['radii'])[bad][:8]} vs {ref['radius'][bad][:8]}")
    bad = judged & (np.asarray(got["tiles_touched"]).astype(np.int64) != ref["tiles"])
    assert not bad.any(), f"{what}: tiles_touched differs at {np.flatnonzero(bad)[:8]}"
    ratios = {"unstable": share}
    sel = judged & ref["visible"]
    for key, name in FLOATS:
        if key not in ref:
            continue
        m = sel & ref["rgb_finite"] if key == "rgb" else sel
        r = ref[key].reshape(len(sel), -1)
        v = np.asarray(got[name], np.float64).reshape(len(sel), -1)[:, :r.shape[1]]
        bnd = ref[key + "_bound"].reshape(len(sel), -1)
        err = np.abs(v - r)[m]
        ratio = float((err / bnd[m]).max()) if m.any() else 0.0
        ratios[key] = ratio
        over = ~(err <= bnd[m])
        assert not over.any(), (f"{what}: {key} beyond its bound at Gaussian "
                                f"{np.flatnonzero(m)[np.argwhere(over)[0][0]]}: {ratio:.3g} x bound")
    return ratios
