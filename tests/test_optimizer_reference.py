"""CPU: the numpy float32 restatement of gsr_adam_step and gsr_densify_stats
(tests/optimizer_reference.py) is right -- against torch.optim.Adam in float64, against upstream's
uncorrected form, and in what a mask leaves alone."""
import numpy as np
import torch

import optimizer_reference as R
from grad_reference import BOUND_FACTOR, rel_err

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _torch_adam(p0, grads, dtype, lr, eps, betas):
    """torch.optim.Adam over the float32 gradients, in `dtype` -> (p, exp_avg, exp_avg_sq)."""
    p = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
    opt = torch.optim.Adam([p], lr=lr, eps=eps, betas=betas)
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        opt.step()
    st = opt.state[p]
    return tuple(t.detach().double().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))


def test_bias_corrected_steps_are_torch_adam():
    """Seven steps on [257, 45] with a full mask and bias correction: within 8 x the float32
    spread (torch's own float32 Adam against its float64 run on the same float32 gradients) of
    the float64 run, for the parameter and both moments."""
    rng = np.random.default_rng(11)
    shape, lr, eps, betas, steps = (257, 45), 1.6e-4, 1e-15, (0.9, 0.999), 7
    p0 = rng.standard_normal(shape).astype(F)
    grads = [R.gradients(rng, shape) for _ in range(steps)]
    rows = np.abs(grads[0]).max(axis=1)  # a decade per row, 1e-6 .. 1
    assert rows.min() < 1e-5 and 0.1 < rows.max() <= 1.0 and (grads[0] == 0).any()
    p, m, v = p0, np.zeros(shape, F), np.zeros(shape, F)
    full = np.ones(shape[0], bool)
    for t, g in enumerate(grads, 1):
        bc1, bc2s = R.bias_corrections(*betas, t)
        p, m, v = R.adam_step(p, g, m, v, lr, eps, *betas, bc1, bc2s, rows=full)
    ref = _torch_adam(p0, grads, torch.float64, lr, eps, betas)
    f32 = _torch_adam(p0, grads, torch.float32, lr, eps, betas)
    # The moments' weights are the ABI's float32 1.0f - beta (upstream's adamUpdate), torch's the
    # double 1 - beta rounded to the tensor's type: the two differ by `weight` relative (2.4e-7
    # for beta1 = 0.9, 1.3e-5 for beta2 = 0.999) in every term of a moment, by definition and not
    # by rounding, so a moment's bound has that on top.  The parameter sees half of beta2's
    # through the square root, times the size of the update (~7 lr against |p| ~ 1): nothing.
    weight = [0.0] + [abs(float(F(1.0) - F(b)) / (1.0 - b) - 1.0) for b in betas]
    for name, got, want, own, w in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), ref, f32,
                                       weight):
        spread, e = rel_err(own, want), rel_err(got, want)
        print(f"{name}: restatement {e:.3g}, torch float32 {spread:.3g} of the float64 run, "
              f"weight {w:.3g}")
        assert spread > 0.0 and e <= BOUND_FACTOR * spread + w, (name, e, spread, w)
    print(f"param against torch's float32 run: {rel_err(p, f32[0]):.3g}")


def test_masked_rows_keep_their_bits():
    rng = np.random.default_rng(12)
    shape = (65, 45)
    p, m, v = (rng.standard_normal(shape).astype(F), rng.standard_normal(shape).astype(F),
               rng.uniform(0, 1, shape).astype(F))
    g = R.gradients(rng, shape)
    radii = rng.integers(-2, 5, shape[0]).astype(np.int32)
    radii[:3] = (0, -1, 7)
    rows = R.row_mask(shape[0], radii=radii)
    assert (rows == (radii > 0)).all() and 0 < rows.sum() < shape[0]
    g[~rows] = np.nan
    g[1, 0] = np.inf
    p1, m1, v1 = R.adam_step(p, g, m, v, 1e-3, 1e-8, 0.9, 0.999, rows=rows)
    for new, old in ((p1, p), (m1, m), (v1, v)):
        np.testing.assert_array_equal(_bits(new[~rows]), _bits(old[~rows]))
        assert np.isfinite(new).all()
        assert (_bits(new[rows]) != _bits(old[rows])).any()
    vis = np.where(rows, rng.choice([1, 255], shape[0]), 0).astype(np.uint8)
    again = R.adam_step(p, g, m, v, 1e-3, 1e-8, 0.9, 0.999, rows=R.row_mask(shape[0], visible=vis))
    for a, b in zip(again, (p1, m1, v1)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    # no mask: every row, and NaN propagates
    dense = R.adam_step(p, g, m, v, 1e-3, 1e-8, 0.9, 0.999)
    assert np.isnan(dense[0][~rows]).all()
    np.testing.assert_array_equal(_bits(dense[0][rows]), _bits(p1[rows]))


def test_unit_corrections_are_upstreams_form():
    """With both corrections 1 the divisions are exact: p - lr * (m / (sqrt(v) + eps))."""
    rng = np.random.default_rng(13)
    shape = (64, 3)
    p, m, v = (rng.standard_normal(shape).astype(F), (0.01 * rng.standard_normal(shape)).astype(F),
               rng.uniform(0, 1e-3, shape).astype(F))
    g = R.gradients(rng, shape)
    for lr, eps in ((1.6e-4, 1e-15), (2.5e-3, 1e-8)):
        p1, m1, v1 = R.adam_step(p, g, m, v, lr, eps, 0.9, 0.999)
        b1, b2 = F(0.9), F(0.999)
        m2 = b1 * m + (F(1.0) - b1) * g
        v2 = b2 * v + ((F(1.0) - b2) * g) * g
        p2 = p - F(lr) * (m2 / (np.sqrt(v2) + F(eps)))
        for a, b in ((p1, p2), (m1, m2), (v1, v2)):
            np.testing.assert_array_equal(_bits(a), _bits(b))
    # g = 0, v = 0, eps > 0: p stays
    z = np.zeros(shape, F)
    p1, m1, v1 = R.adam_step(p, z, z, z, 1e-3, 1e-15, 0.9, 0.999)
    np.testing.assert_array_equal(_bits(p1), _bits(p))
    assert not m1.any() and not v1.any()


def test_statistics_are_the_direct_evaluation():
    rng = np.random.default_rng(14)
    P = 257
    radii = rng.integers(-1, 40, P).astype(np.int32)
    radii[::5] = 0
    g = R.gradients(rng, (P, 3), zeros=False)
    accum, denom = rng.uniform(0, 1, P).astype(F), rng.integers(0, 9, P).astype(F)
    maxr = rng.integers(0, 30, P).astype(np.int32)
    a1, d1, r1 = R.densify_stats(radii, g, accum, denom, maxr)
    on = radii > 0
    want = accum.copy()
    want[on] += np.sqrt(g[on, 0] * g[on, 0] + g[on, 1] * g[on, 1])
    np.testing.assert_array_equal(_bits(a1), _bits(want))
    np.testing.assert_array_equal(d1, denom + on)
    np.testing.assert_array_equal(r1, np.where(on, np.maximum(maxr, radii), maxr))
    # upstream's norm, and [P, 1] accumulators
    up = torch.norm(torch.tensor(g[on, :2]), dim=-1).numpy()
    assert rel_err(a1[on] - accum[on], up) <= 4 * np.finfo(F).eps
    a2, d2, none = R.densify_stats(radii, g, accum.reshape(P, 1), denom.reshape(P, 1))
    assert none is None and a2.shape == d2.shape == (P, 1)
    np.testing.assert_array_equal(_bits(a2.reshape(P)), _bits(a1))
