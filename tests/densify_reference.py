"""numpy restatement of gsr_densify_plan / gsr_densify_apply (include/gsr.h, csrc/densify.hip),
operation by operation in float32: the classification, the output order, the rows, Philox4x32-10
and the split samples -- and a float64 evaluation of the child positions from the same Philox
words (the same float32 u_k, everything after them in double).

The GPU is held bit for bit to densify() in everything but the child positions: those go through
logf, cosf, sinf (and expf in log space), whose last bits differ between libraries.  They are held
to the float64 positions within 8 x SPREAD x scale, where per child
    scale = max|xyz(source)| + sum_k sigma_k rad_k,   rad_0 = rad_1 = sqrt(-2 ln u0), rad_2 likewise
bounds the magnitude of every term of the position, and SPREAD is the largest float32 error of
this file's own float32 evaluation against the float64 one in units of scale, measured over 10^4
split sources by tests/test_densify_reference.py (which holds the constant to a factor 2).  A
wrong Philox word moves a child by the order of sigma, some 10^6 x the bound.
"""
from __future__ import annotations

import numpy as np

F = np.float32
ROLES = ("xyz", "scaling", "rotation", "opacity")
ROLE_M = dict(xyz=3, scaling=3, rotation=4, opacity=1)
LOG16 = F(np.log(1.6))
TWO_PI = F(6.2831855)
SPREAD = 4.0e-7  # measured 3.4e-7 (linear space) and 3.7e-7 (log space); see the module docstring
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two -> four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def uniforms(seed, rows, child):
    """The four float32 u_k of (seed, source row, child): ((x_k >> 8) + 0.5f) * 2^-24."""
    seed = int(seed) & (2 ** 64 - 1)
    x = philox4x32_10((np.asarray(rows, np.uint64), child, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return [((v >> np.uint32(8)).astype(F) + F(0.5)) * F(2.0 ** -24) for v in x]


def normals(u, dtype=F):
    """Box-Muller as the header states it -> z [n, 3] and the radii (rad0, rad2), in `dtype`."""
    t = dtype
    u = [v.astype(t) for v in u]
    two_pi = TWO_PI.astype(t)
    with np.errstate(divide="ignore"):
        rad0 = np.sqrt(t(-2.0) * np.log(u[0]))
        rad2 = np.sqrt(t(-2.0) * np.log(u[2]))
    ang0, ang2 = two_pi * u[1], two_pi * u[3]
    z = np.stack([rad0 * np.cos(ang0), rad0 * np.sin(ang0), rad2 * np.cos(ang2)], 1)
    return z.astype(t), rad0, rad2


def rotation_matrix(q, dtype=F):
    """Upstream's build_rotation of (r, x, y, z) rows, in the header's operation order."""
    t = dtype
    q = q.astype(t)
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    r, x, y, z = (q[:, k] / n for k in range(4))
    one, two = t(1.0), t(2.0)
    R = np.empty((len(q), 3, 3), t)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - r * z)
    R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y)
    R[:, 2, 1] = two * (y * z + r * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def child_positions(seed, rows, child, xyz, scaling, rotation, log_space, dtype=F):
    """The positions of child `child` of the source `rows` (their xyz / scaling / rotation rows
    given) in `dtype` -> (positions [n, 3], scale [n] of the module docstring, float64)."""
    t = dtype
    u = uniforms(seed, rows, child)
    z, rad0, rad2 = normals(u, t)
    s = scaling.astype(t)
    sigma = np.exp(s) if log_space else s
    v = sigma * z
    R = rotation_matrix(rotation, t)
    x = xyz.astype(t)
    pos = np.stack([((R[:, k, 0] * v[:, 0] + R[:, k, 1] * v[:, 1]) + R[:, k, 2] * v[:, 2]) + x[:, k]
                    for k in range(3)], 1)
    sig = np.abs(sigma.astype(np.float64))
    scale = (np.abs(x.astype(np.float64)).max(1) + sig[:, 0] * rad0 + sig[:, 1] * rad0 +
             sig[:, 2] * rad2)
    return pos.astype(t), scale


def child_scaling(s, log_space):
    return (s - LOG16 if log_space else s / F(1.6)).astype(F)


def classify(grad_accum, denom, scaling, opacity, max_radii, thresholds, radius_threshold,
             log_space):
    """-> (keep, clone, split) bool [P]: the row survives unsplit, its clone survives, its two
    children survive.  thresholds = (grad, scale split, opacity prune, scale prune), float32."""
    grad_thr, split_thr, opacity_thr, scale_thr = (F(v) for v in thresholds)
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = (grad_accum.reshape(-1).astype(F) / denom.reshape(-1).astype(F)).astype(F)
    avg[np.isnan(avg)] = F(0.0)
    hot = avg >= grad_thr
    s = scaling.reshape(-1, 3).astype(F)
    smax = np.fmax(np.fmax(s[:, 0], s[:, 1]), s[:, 2])
    split = hot & (smax > split_thr)
    clone = hot & (smax <= split_thr)
    tested = np.where(split, child_scaling(smax, log_space), smax)
    with np.errstate(invalid="ignore"):
        pruned = (opacity.reshape(-1) < opacity_thr) | (tested > scale_thr)
    if max_radii is not None and radius_threshold > 0:
        pruned |= max_radii.reshape(-1) > radius_threshold
    return ~split & ~pruned, clone & ~pruned, split & ~pruned


def densify(groups, grad_accum, denom, max_radii, thresholds, radius_threshold, log_space, seed):
    """groups: list of dict(p [P, M], m, v (both None for a tensor without moments), role (a name
    of ROLES or None)) -> dict(counts, source_index, groups (p, m, v per group), xyz64 (the child
    positions in float64, [2 n_split, 3]), scale (their bound's unit), children (a slice of the
    output rows))."""
    by_role = {g["role"]: g for g in groups if g["role"]}
    P = len(by_role["xyz"]["p"])
    keep, clone, split = classify(grad_accum, denom, by_role["scaling"]["p"],
                                  by_role["opacity"]["p"], max_radii, thresholds,
                                  radius_threshold, log_space)
    rows = np.arange(P, dtype=np.int32)
    kept, cloned, parents = rows[keep], rows[clone], rows[split]
    source_index = np.concatenate([kept, cloned, parents, parents]).astype(np.int32)
    counts = (len(kept), len(cloned), len(parents), P - len(kept) - len(parents))
    n_kept = len(kept)
    out = []
    for g in groups:
        p = np.ascontiguousarray(g["p"][source_index])
        m = v = None
        if g["m"] is not None:
            m, v = np.zeros_like(p), np.zeros_like(p)
            m[:n_kept], v[:n_kept] = g["m"][kept], g["v"][kept]
        out.append(dict(p=p, m=m, v=v))
    first = n_kept + len(cloned)
    children = slice(first, first + 2 * len(parents))
    xyz_g, scaling_g = (out[groups.index(by_role[r])] for r in ("xyz", "scaling"))
    src = {r: by_role[r]["p"].reshape(P, -1)[parents] for r in ("xyz", "scaling", "rotation")}
    scaling_g["p"][children] = np.tile(child_scaling(src["scaling"], log_space), (2, 1))
    pos32, pos64, scale = [], [], []
    for child in (0, 1):
        a = child_positions(seed, parents, child, src["xyz"], src["scaling"], src["rotation"],
                            log_space, F)
        b = child_positions(seed, parents, child, src["xyz"], src["scaling"], src["rotation"],
                            log_space, np.float64)
        pos32.append(a[0])
        pos64.append(b[0])
        scale.append(b[1])
    xyz_g["p"][children] = np.concatenate(pos32).reshape(xyz_g["p"][children].shape)
    return dict(counts=counts, source_index=source_index, groups=out, children=children,
                xyz64=np.concatenate(pos64), scale=np.concatenate(scale))


# ---- test scenes: every class of row, and every threshold met exactly -----------------------------
# name, M, role, in the optimizer (has moments): the 3DGS six and one tensor without moments
GROUPS = (("xyz", 3, "xyz", True), ("f_dc", 3, None, True), ("f_rest", 45, None, True),
          ("opacity", 1, "opacity", True), ("scaling", 3, "scaling", True),
          ("rotation", 4, "rotation", True), ("extra", 17, None, False))
ROLES_ONLY = tuple(g for g in GROUPS if g[2])
# thresholds in linear units: grad, sigma split, opacity prune, sigma prune; and the radius
LINEAR = (0.5, 0.25, 0.1, 2.0)
RADIUS = 20
# the classes of a row (what it is built to be)
KEEP, CLONE, SPLIT, LOW_OPACITY, BIG, BIG_RADIUS, SPLIT_LOW_OPACITY, COLD_NO_DENOM, HOT_NO_DENOM, \
    SPLIT_HUGE, SPLIT_CHILD_BIG, EDGES = range(12)
PATTERNS = {"keep": [KEEP, COLD_NO_DENOM], "clone": [CLONE, HOT_NO_DENOM],
            "split": [SPLIT, SPLIT_HUGE],
            "prune": [LOW_OPACITY, BIG, BIG_RADIUS, SPLIT_LOW_OPACITY, SPLIT_CHILD_BIG],
            "mix": list(range(11)), "runs": list(range(11)), "edges": [EDGES]}


def thresholds(log_space):
    """The float32 thresholds in the stored space (the doubles rounded once)."""
    g, s, o, w = LINEAR
    if log_space:
        s, o, w = np.log(s), np.log(o / (1.0 - o)), np.log(w)
    return tuple(F(v) for v in (g, s, o, w))


def make_scene(P, rng, log_space, pattern="mix", groups=GROUPS, radius_on=True, poison=True):
    """-> dict(groups (for densify()), grad_accum, denom, max_radii, thresholds, radius_threshold,
    log_space, cls).  With `poison`, NaN in every word the apply step must not read: the moments
    of every row that is not kept, and the other tensors of a row of which nothing survives."""
    thr = thresholds(log_space)
    kinds = np.asarray(PATTERNS[pattern])
    cls = rng.choice(kinds, P)
    if pattern == "runs":  # long runs of one class: whole scan blocks of one kind
        cls = np.repeat(rng.choice(kinds, P // 97 + 1), 97)[:P]
    uni = lambda lo, hi, shape=P: rng.uniform(lo, hi, shape).astype(F)  # noqa: E731
    denom = rng.integers(1, 9, P).astype(F)
    hot = np.isin(cls, (CLONE, SPLIT, SPLIT_LOW_OPACITY, HOT_NO_DENOM, SPLIT_HUGE, SPLIT_CHILD_BIG))
    accum = (np.where(hot, uni(0.6, 3.0), uni(0.0, 0.4)) * denom).astype(F)
    nod = np.isin(cls, (COLD_NO_DENOM, HOT_NO_DENOM))
    denom[nod] = 0.0
    accum[cls == COLD_NO_DENOM] = 0.0  # 0 / 0 = NaN -> 0: cold;  x / 0 = inf: hot
    sigma = uni(0.01, 0.2, (P, 3))
    for c, lo, hi in ((SPLIT, 0.3, 1.5), (SPLIT_LOW_OPACITY, 0.3, 1.5), (BIG, 2.5, 4.0),
                      (SPLIT_HUGE, 2.2, 3.0), (SPLIT_CHILD_BIG, 3.5, 4.0)):
        n = int((cls == c).sum())
        col = rng.integers(0, 3, n)  # one large axis is enough: the test is on the max
        big = sigma[cls == c]
        big[np.arange(n), col] = uni(lo, hi, n)
        sigma[cls == c] = big
    opacity = uni(0.2, 0.9, (P, 1))
    low = np.isin(cls, (LOW_OPACITY, SPLIT_LOW_OPACITY))
    opacity[low] = uni(0.01, 0.08, (int(low.sum()), 1))
    radii = rng.integers(0, RADIUS + 1, P).astype(np.int32)
    radii[cls == BIG_RADIUS] = rng.integers(RADIUS + 1, 60, int((cls == BIG_RADIUS).sum()))
    scaling = np.log(sigma).astype(F) if log_space else sigma
    if log_space:
        opacity = np.log(opacity / (F(1.0) - opacity)).astype(F)
    e = np.flatnonzero(cls == EDGES)
    if len(e):
        # eight kinds of row, each AT a threshold or one float beside it
        k = np.arange(len(e)) % 8
        denom[e] = 1.0
        accum[e] = np.where(k < 2, thr[0], np.where(k == 4, np.nextafter(thr[0], F(0)), F(0.1)))
        scaling[e] = thr[1] - F(1.0)                     # below the split threshold
        scaling[e[k == 1], 1] = thr[1]                   # k 1: hot, smax == threshold: a clone
        accum[e[k == 5]] = thr[0]
        scaling[e[k == 5], 2] = np.nextafter(thr[1], F(np.inf))   # k 5: one above: split
        opacity[e] = thr[2] + F(1.0) if log_space else F(0.5)
        opacity[e[k == 2]] = thr[2]                      # k 2: o == threshold stays
        opacity[e[k == 6]] = np.nextafter(thr[2], F(-np.inf))     # k 6: one below goes
        radii[e] = 3
        radii[e[k == 3]] = RADIUS                        # k 3: r == threshold stays
        radii[e[k == 7]] = RADIUS + 1                    # k 7: goes (with the radius test on)
    host = dict(xyz=uni(-2.0, 2.0, (P, 3)), scaling=scaling, opacity=opacity,
                rotation=(rng.standard_normal((P, 4)) * uni(0.5, 2.0, (P, 1))).astype(F))
    out = []
    for name, M, role, has in groups:
        p = host[name] if name in host else rng.standard_normal((P, M)).astype(F)
        m = (0.01 * rng.standard_normal((P, M))).astype(F) if has else None
        v = rng.uniform(0, 1e-3, (P, M)).astype(F) if has else None
        out.append(dict(name=name, role=role, p=np.ascontiguousarray(p), m=m, v=v))
    sc = dict(groups=out, grad_accum=accum, denom=denom, max_radii=radii if radius_on else None,
              thresholds=thr, radius_threshold=RADIUS if radius_on else 0, log_space=log_space,
              cls=cls)
    if poison:
        keep, _, split = classify(accum, denom, scaling, opacity, sc["max_radii"], thr,
                                  sc["radius_threshold"], log_space)
        for g in out:
            if g["m"] is not None:
                g["m"][~keep] = np.nan
                g["v"][~keep] = np.nan
            if g["role"] not in ("scaling", "opacity"):
                g["p"][~keep & ~split] = np.nan
    return sc


def run(sc, seed):
    return densify(sc["groups"], sc["grad_accum"], sc["denom"], sc["max_radii"], sc["thresholds"],
                   sc["radius_threshold"], sc["log_space"], seed)
