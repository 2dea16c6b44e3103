"""gsr_adam_step and gsr_densify_stats (include/gsr.h) restated in numpy float32, operation by
operation in the header's order; masking by np.where, so a row that is not updated keeps its bits
whatever its gradient holds.  numpy's float32 multiply, add, subtract, divide and sqrt are IEEE
correctly rounded and nothing here contracts into an FMA, which is what the kernels promise: the
GPU tests compare bit for bit."""
import numpy as np

F = np.float32


def row_mask(P, visible=None, radii=None):
    """The rows a call updates: bool [P]."""
    assert visible is None or radii is None
    if visible is not None:
        return np.asarray(visible).reshape(P) != 0
    if radii is not None:
        return np.asarray(radii).reshape(P) > 0
    return np.ones(P, bool)


def adam_step(p, g, m, v, lr, eps, beta1, beta2, bc1=1.0, bc2_sqrt=1.0, rows=None):
    """One step of one [P, M] group -> (p, m, v), new float32 arrays.  `rows`: bool [P] or None."""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    lr, eps, beta1, beta2, bc1, bc2_sqrt = (F(x) for x in (lr, eps, beta1, beta2, bc1, bc2_sqrt))
    omb1, omb2 = F(1.0) - beta1, F(1.0) - beta2
    step = lr / bc1
    with np.errstate(all="ignore"):
        m1 = beta1 * m + omb1 * g
        v1 = beta2 * v + (omb2 * g) * g
        p1 = p - step * (m1 / (np.sqrt(v1) / bc2_sqrt + eps))
    assert p1.dtype == m1.dtype == v1.dtype == F
    if rows is None:
        return p1, m1, v1
    sel = np.asarray(rows, bool).reshape((-1,) + (1,) * (p.ndim - 1))
    return np.where(sel, p1, p), np.where(sel, m1, m), np.where(sel, v1, v)


def bias_corrections(beta1, beta2, t):
    """(1 - beta1^t, sqrt(1 - beta2^t)) in double, as torch.optim.Adam computes them."""
    return 1.0 - float(beta1) ** t, float(np.sqrt(1.0 - float(beta2) ** t))


def densify_stats(radii, grad2d, accum, denom, max_radii=None):
    """-> (accum, denom, max_radii or None), new arrays; grad2d is [P, 3] (x, y read)."""
    radii = np.asarray(radii, np.int32)
    grad2d, accum, denom = (np.asarray(a, F) for a in (grad2d, accum, denom))
    on = radii > 0
    x, y = grad2d[:, 0], grad2d[:, 1]
    with np.errstate(all="ignore"):
        norm = np.sqrt(x * x + y * y)
        a1 = np.where(on.reshape(accum.shape), accum + norm.reshape(accum.shape), accum)
        d1 = np.where(on.reshape(denom.shape), denom + F(1.0), denom)
    assert a1.dtype == d1.dtype == F
    r1 = None
    if max_radii is not None:
        max_radii = np.asarray(max_radii, np.int32)
        r1 = np.where(on, np.maximum(max_radii, radii), max_radii).astype(np.int32)
    return a1, d1, r1


def gradients(rng, shape, zeros=True):
    """float32 gradients over six decades (1e-6 .. 1, the decade drawn per row), both signs, with
    exact zeros sprinkled in."""
    P = shape[0]
    scale = 10.0 ** rng.uniform(-6.0, 0.0, (P,) + (1,) * (len(shape) - 1))
    g = (rng.uniform(0.1, 1.0, shape) * rng.choice([-1.0, 1.0], shape) * scale).astype(F)
    if zeros:
        g[rng.uniform(size=shape) < 0.1] = 0.0
    return g
