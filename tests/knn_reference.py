"""The nearest-neighbour search of gsr_knn_mean_dist2 (include/gsr.h) in numpy float32: the
brute-force statement that is the specification, and a restatement of the kernel's algorithm
(csrc/knn.hip) that must equal it bit for bit.  Shared code, no tests.

numpy evaluates float32 expressions operation by operation with IEEE rounding and without
contraction, which is the arithmetic include/gsr.h fixes, so `brute` gives the bits the GPU has to
give; there is no tolerance anywhere in the search."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)


def _mean(best, n):
    """best (m, 3) ascending -> the mean of the first k = min(3, n - 1) in the header's order."""
    k = min(3, n - 1)
    if k == 0:
        return np.zeros(len(best), f32)
    acc = best[:, 0].copy()
    for j in range(1, k):
        acc = acc + best[:, j]
    return acc / f32(k)


def _dist(q, r):
    dx = q[:, None, 0] - r[None, :, 0]
    dy = q[:, None, 1] - r[None, :, 1]
    dz = q[:, None, 2] - r[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def brute(xyz, chunk=512):
    """dist2 of include/gsr.h over all pairs: float32, self excluded by index, k = min(3, N - 1)."""
    p = np.ascontiguousarray(xyz, f32)
    n = len(p)
    out = np.zeros(n, f32)
    k = min(3, n - 1)
    if k <= 0:
        return out
    for s in range(0, n, chunk):
        q = p[s:s + chunk]
        d = _dist(q, p)
        d[np.arange(len(q)), np.arange(s, s + len(q))] = INF
        b = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
        b = np.concatenate([b, np.full((len(q), 3 - k), INF, f32)], 1)
        out[s:s + len(q)] = _mean(b, n)
    return out


def morton(xyz):
    """The kernel's 30-bit code: cell = clamp(int(((p - lo) / ext) * 1023)) per axis, an axis of
    zero extent in cell 0, x in bits 0, 3, ..., y in 1, 4, ..., z in 2, 5, ..."""
    p = np.ascontiguousarray(xyz, f32)
    lo, hi = p.min(0), p.max(0)
    ext = hi - lo
    c = np.zeros((len(p), 3), np.uint32)
    for a in range(3):
        if ext[a] > 0:
            t = ((p[:, a] - lo[a]) / ext[a]) * f32(1023)
            c[:, a] = np.clip(np.clip(t, f32(0), f32(1023)).astype(np.int64), 0, 1023)

    def spread(v):
        v = v.astype(np.uint32) & np.uint32(0x3FF)
        v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
        v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
        v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
        v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
        return v
    return spread(c[:, 0]) | (spread(c[:, 1]) << np.uint32(1)) | (spread(c[:, 2]) << np.uint32(2))


def _gap(lo, hi, p):
    return np.maximum(np.maximum(lo - p, p - hi), f32(0))


def boxed(xyz, B=256, *, reach=None, exclude_self=True, first_point_bounds=False,
          always_three=False, stats=None):
    """csrc/knn.hip in numpy: Morton order (stable), boxes of B sorted points with their bounds,
    per box a scan of itself and then the other boxes outward (b + 1, b - 1, b + 2, ...) in rounds
    of B candidates: a candidate is dropped when its distance to the box's own bounds exceeds the
    box's largest third best, and a survivor is skipped when every point's distance to it exceeds
    the point's third best.  `stats`, a dict, receives "scanned" (boxes scanned per box).
    The keyword arguments switch on the mutants test_knn_reference.py runs: `reach` = visit only
    boxes within that many of the own one; `exclude_self=False`; `first_point_bounds` = a box's
    bounds are its first point; `always_three` = divide by 3 whatever N is."""
    p = np.ascontiguousarray(xyz, f32)
    n = len(p)
    out = np.zeros(n, f32)
    if n == 0:
        return out
    perm = np.argsort(morton(p), kind="stable")
    s = p[perm]
    nb = (n + B - 1) // B
    if first_point_bounds:
        lo = np.array([s[b * B] for b in range(nb)])
        hi = lo.copy()
    else:
        lo = np.array([s[b * B:(b + 1) * B].min(0) for b in range(nb)])
        hi = np.array([s[b * B:(b + 1) * B].max(0) for b in range(nb)])
    scanned = np.zeros(nb, np.int64)
    for b in range(nb):
        q = s[b * B:(b + 1) * B]
        m = len(q)
        best = np.full((m, 3), INF, f32)

        def scan(c, mine, best):
            d = _dist(q, s[c * B:(c + 1) * B])
            if c == b and exclude_self:
                d[np.arange(m), np.arange(m)] = INF
            new = np.sort(np.concatenate([best, d], 1), 1)[:, :3]
            scanned[b] += 1
            return np.where(mine[:, None], new, best)

        best = scan(b, np.ones(m, bool), best)
        total = 2 * max(b, nb - 1 - b)
        for base in range(0, total, B):
            mb = best[:, 2].max()
            survivors = []
            for pos in range(base, min(base + B, total)):
                step = (pos >> 1) + 1
                c = b - step if pos & 1 else b + step
                if not 0 <= c < nb or (reach is not None and step > reach):
                    continue
                g = [np.maximum(np.maximum(lo[c, a] - hi[b, a], lo[b, a] - hi[c, a]), f32(0))
                     for a in range(3)]
                if not (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] > mb:
                    survivors.append(c)
            for c in survivors:
                g = [_gap(lo[c, a], hi[c, a], q[:, a]) for a in range(3)]
                mine = ~((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] > best[:, 2])
                if mine.any():
                    best = scan(c, mine, best)
        out[perm[b * B:(b + 1) * B]] = _mean(best, 4 if always_three else n)
    if stats is not None:
        stats["scanned"] = scanned
    return out


MIN_DIST2 = 1e-7


def scaling_reference(dist2, min_dist2=MIN_DIST2):
    """The initial log scale of create_from_pcd in float64: 0.5 log(max(dist2, min_dist2))."""
    return 0.5 * np.log(np.maximum(np.asarray(dist2, np.float64), min_dist2))


def scaling_f32(dist2, min_dist2=MIN_DIST2):
    """The same as upstream writes it, log(sqrt(clamp_min(dist2, min_dist2))), in numpy float32."""
    return np.log(np.sqrt(np.maximum(np.asarray(dist2, f32), f32(min_dist2))))


def scaling_spread(scene_arrays):
    """The largest |scaling_f32 - scaling_reference| over the scenes' brute-force dist2."""
    worst = 0.0
    for xyz in scene_arrays:
        d = brute_cached(xyz)
        if len(d):
            worst = max(worst, float(np.abs(scaling_f32(d).astype(np.float64) -
                                            scaling_reference(d)).max()))
    return worst


# scaling_spread over knn_scenes.scenes(), measured once and recorded (test_knn_reference.py
# measures it again and asks for agreement within a factor 2).  Eight times this is the bound the
# GPU's scaling is held to against scaling_reference of the GPU's own dist2.
SCALING_F32_SPREAD = 4.9e-7  # (measured: 4.885e-07, about one float32 step at |log| = 8)

_brute_cache = {}


def brute_cached(xyz):
    """brute(xyz), computed once per array (the scenes are shared and read-only)."""
    key = (xyz.ctypes.data, xyz.shape)
    if key not in _brute_cache:
        _brute_cache[key] = (xyz, brute(xyz))  # (the array is kept alive with its result)
    return _brute_cache[key][1]
