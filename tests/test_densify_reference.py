"""CPU: the numpy restatement of densify-and-prune (tests/densify_reference.py) against known
answers, against a direct torch transcription of upstream's densify_and_clone / densify_and_split /
prune_points, and against the statistics its samples must have.

   1 Philox4x32-10 known answers (the first two are Random123's kat vectors)
   2 restatement == transcription in everything but the sampled positions: counts, order (through
     source_index and every copied word), zero moments, child scaling; both scale spaces,
     max_screen_size=None (upstream's screen-size test never fires: gsr.h's deviation), every
     class of row present.  In linear space the child scaling is one division on both sides: bit
     for bit.  In log space upstream writes log(exp(s) / 1.6) where the kernel writes s - log 1.6
     (one operation, gsr.h): equal within 4 float32 roundings of a value of size max(1, |s|) --
     exp, the division and log each within 1 ulp of their argument (a relative error e in log's
     argument is an absolute error e in its value), plus the restatement's own rounding
   3 over 10^4 split sources of one shape, the 2 x 10^4 children have mean 0 and covariance
     R diag(sigma^2) R^T within the sampling error (derivation at the test)
   4 the float32 spread of the child positions against float64, which tests/test_gpu_densify.py
     multiplies by 8 for its bound: SPREAD holds, to a factor 2
"""
import numpy as np
import pytest
import torch

import densify_reference as D

F = np.float32


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{int(v[0]):08x}" for v in D.philox4x32_10(counter, key)) == want


def test_philox_is_elementwise_and_the_uniforms_stay_in_range():
    rows = np.array([0, 1, 77, 2 ** 30 - 1])
    both = D.philox4x32_10((rows, 1, 0, 0), (5, 9))
    for j, r in enumerate(rows):
        one = D.philox4x32_10((int(r), 1, 0, 0), (5, 9))
        assert [int(v[j]) for v in both] == [int(v[0]) for v in one]
    u = np.concatenate(D.uniforms(123456789123, np.arange(100000), 0))
    assert u.dtype == F and u.min() > 0.0 and u.max() <= 1.0
    # the smallest and the largest word: 2^-25, and 1 (the one rounded add of gsr.h)
    lo, hi = (((np.uint32(x) >> np.uint32(8)).astype(F) + F(0.5)) * F(2.0 ** -24)
              for x in (0, 0xFFFFFFFF))
    assert lo == F(2.0 ** -25) and hi == F(1.0)


# ---- 2 ------------------------------------------------------------------------------------------
def upstream(sc, max_grad, min_opacity, extent, percent_dense, N=2):
    """densify_and_prune of upstream's GaussianModel with max_screen_size=None, on float32 CPU
    tensors; the optimizer's tensors are sc's groups, the activations exp / sigmoid in log space
    and the identity in linear space.  -> (params, exp_avg, exp_avg_sq by name, new xyz rows)."""
    log_space = sc["log_space"]
    p = {g["name"]: torch.tensor(g["p"]) for g in sc["groups"]}
    m = {g["name"]: torch.tensor(g["m"]) for g in sc["groups"] if g["m"] is not None}
    v = {g["name"]: torch.tensor(g["v"]) for g in sc["groups"] if g["v"] is not None}
    scaling_act = torch.exp if log_space else (lambda t: t)
    scaling_inv = torch.log if log_space else (lambda t: t)
    opacity_act = torch.sigmoid if log_space else (lambda t: t)

    def postfix(new):  # densification_postfix / cat_tensors_to_optimizer
        for k in p:
            if k in m:
                m[k] = torch.cat((m[k], torch.zeros_like(new[k])), dim=0)
                v[k] = torch.cat((v[k], torch.zeros_like(new[k])), dim=0)
            p[k] = torch.cat((p[k], new[k]), dim=0)

    def prune_points(mask):  # _prune_optimizer
        valid = ~mask
        for k in p:
            if k in m:
                m[k], v[k] = m[k][valid], v[k][valid]
            p[k] = p[k][valid]

    grads = torch.tensor(sc["grad_accum"]).reshape(-1, 1) / torch.tensor(sc["denom"]).reshape(-1, 1)
    grads[grads.isnan()] = 0.0
    # densify_and_clone
    sel = torch.where(torch.norm(grads, dim=-1) >= max_grad, True, False)
    sel = torch.logical_and(sel, torch.max(scaling_act(p["scaling"]), dim=1).values
                            <= percent_dense * extent)
    postfix({k: t[sel] for k, t in p.items()})
    # densify_and_split
    n_init = p["xyz"].shape[0]
    padded = torch.zeros(n_init)
    padded[:grads.shape[0]] = grads.squeeze()
    sel = torch.where(padded >= max_grad, True, False)
    sel = torch.logical_and(sel, torch.max(scaling_act(p["scaling"]), dim=1).values
                            > percent_dense * extent)
    new = {k: t[sel].repeat(N, *([1] * (t.dim() - 1))) for k, t in p.items()}
    new["scaling"] = scaling_inv(scaling_act(p["scaling"])[sel].repeat(N, 1) / (0.8 * N))
    n_new = new["xyz"].shape[0]
    postfix(new)
    prune_points(torch.cat((sel, torch.zeros(N * int(sel.sum()), dtype=torch.bool))))
    # the prune of densify_and_prune, max_screen_size None
    prune_points((opacity_act(p["opacity"]) < min_opacity).squeeze(-1))
    return p, m, v, n_new


@pytest.mark.parametrize("log_space", [False, True])
def test_restatement_equals_upstreams_transcription(log_space):
    P = 3000
    sc = D.make_scene(P, np.random.default_rng(11 + log_space), log_space, "mix",
                      radius_on=False, poison=False)
    g, s, o, _ = D.LINEAR
    sc["thresholds"] = D.thresholds(log_space)[:3] + (F(np.inf),)  # max_screen_size=None
    # no row so near a threshold that exp / sigmoid could decide it the other way
    by = {x["name"]: x["p"] for x in sc["groups"]}
    sig = np.exp(by["scaling"].astype(np.float64)) if log_space else by["scaling"]
    opa = 1 / (1 + np.exp(-by["opacity"].astype(np.float64))) if log_space else by["opacity"]
    assert (np.abs(sig.max(1) / s - 1) > 1e-4).all() and (np.abs(opa / o - 1) > 1e-4).all()
    want = D.run(sc, seed=3)
    p, m, v, n_new = upstream(sc, max_grad=g, min_opacity=o, extent=s / 0.01, percent_dense=0.01)
    nk, nc, ns, nr = want["counts"]
    assert min(nk, nc, ns, nr) > 0 and len(p["xyz"]) == nk + nc + 2 * ns
    assert len(np.unique(sc["cls"])) == 11
    children = want["children"]
    for x, w in zip(sc["groups"], want["groups"]):
        name = x["name"]
        got = p[name].numpy()
        same = np.ones(len(got), bool)
        if name in ("xyz", "scaling"):
            same[children] = False
        np.testing.assert_array_equal(got[same].view(np.uint32), w["p"][same].view(np.uint32),
                                      err_msg=name)
        if x["m"] is not None:
            np.testing.assert_array_equal(m[name].numpy().view(np.uint32), w["m"].view(np.uint32))
            np.testing.assert_array_equal(v[name].numpy().view(np.uint32), w["v"].view(np.uint32))
            assert not w["m"][nk:].any() and not w["v"][nk:].any()
        else:
            assert name not in m and w["m"] is None
    got, ref = p["scaling"].numpy()[children], want["groups"][4]["p"][children]
    if log_space:
        bound = 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    else:
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    # the order of the children is upstream's too: child j of the k-th split source
    src = want["source_index"][children]
    assert (src[:ns] == src[ns:]).all() and (np.diff(src[:ns]) > 0).all()


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_space", [False, True])
def test_children_have_the_sources_distribution(log_space):
    """n = 2 x 10^4 independent samples d = child - source of N(0, S), S = R diag(sigma^2) R^T.
    The sample mean of d_i has standard deviation sqrt(S_ii / n); the sample second moment of
    d_i d_j (the mean is known to be 0) has standard deviation sqrt((S_ii S_jj + S_ij^2) / n)
    (Isserlis).  Each of the 3 + 6 statistics is held within 5 of its standard deviations, which
    a correct sampler misses with probability < 1e-5 in all -- and the seed is fixed."""
    n_src = 10000
    q = np.tile(np.array([[0.9, -0.3, 0.5, 0.2]], F) * F(1.7), (n_src, 1))
    sigma = np.tile(np.array([[0.5, 0.1, 1.2]], F), (n_src, 1))
    scaling = np.log(sigma).astype(F) if log_space else sigma
    xyz = np.zeros((n_src, 3), F)
    rows = np.arange(n_src)
    d = np.concatenate([D.child_positions(99, rows, c, xyz, scaling, q, log_space, F)[0]
                        for c in (0, 1)]).astype(np.float64)
    n = len(d)
    R = D.rotation_matrix(q[:1], np.float64)[0]
    S = R @ np.diag(sigma[0].astype(np.float64) ** 2) @ R.T
    assert (np.abs(d.mean(0)) < 5 * np.sqrt(np.diag(S) / n)).all()
    second = d.T @ d / n
    sd = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / n)
    assert (np.abs(second - S) < 5 * sd).all()
    # and the two children of a source are different samples
    assert (d[:n_src] != d[n_src:]).any(1).all()


# ---- 4 ------------------------------------------------------------------------------------------
def measured_spread(log_space):
    sc = D.make_scene(10000, np.random.default_rng(4), log_space, "split", poison=False)
    r = D.run(sc, seed=2024)
    assert r["counts"][2] == 10000
    err = np.abs(r["groups"][0]["p"][r["children"]].astype(np.float64) - r["xyz64"]).max(1)
    return float((err / r["scale"]).max())


def test_float32_spread_of_the_child_positions():
    spreads = [measured_spread(False), measured_spread(True)]
    print("float32 spread of the child positions, linear and log space:", spreads)
    assert D.SPREAD / 2 <= max(spreads) <= D.SPREAD
