"""GPU: a multi-view fit held to its float64 restatement (tests/multiview_fit_reference.py), view
by view.  The fits of tests/test_gpu_fit_chain.py are one camera, one frame shape, one SH degree and
one densify; this one is the same scene, start and parametrisations under what a training loop
does: four cameras of different eyes and frame shapes (40 x 24, 24 x 40, 33 x 17 and 48 x 40 px) in
a seeded order, new settings every iteration, the SH degree raised every eight iterations, and
densify_and_prune after iterations 20 and 36 of 48.  So from one iteration to the next the
context's tile grid, lists and deterministic slots grow and shrink, the sparse Adam's row mask
changes, the statistics accumulate over frames of different sizes, f_rest coefficients are stored
but inactive, and the second densify rebinds what the first one made.

Each fit ("activated" on the deterministic backward, "stored" on the atomic one) runs once per
module, keeps every tensor after every iteration on the host, and snapshots what the iterations
mv.CHECKPOINTS = 1, 8, 9, 16, 17, 20, 21, 22, 24, 25, 36, 37, 38, 48 read and wrote.  Per (fit,
checkpoint), from the GPU's own state, the checks of fit_step_reference.check_all on this fit's
measured tables: forward (image and radii against lists of a no-grad replay), loss value and loss
gradient, chain and joint gradients (left out where the float64 evaluation is near a gate, within
mv.cap_holds), Adam and the statistics bit for bit; after 20 and 36 the densify's counts and
source_index are densify_reference's classification of the GPU's own statistics, and at 21 and 37
the rebind holds (kept rows carry their source row's bits, new rows start from zero moments).

Added for this fit:
  inactive SH   while degree(it) < 3 the gradient of every coefficient above the degree is zero in
                every word; those coefficients and their moments keep their bits from the start
                until the first step at their degree, and the moments are then non-zero;
  unseen rows   at every iteration, a row the frame's radii do not see keeps every bit of every
                parameter and both moments; a row no frame of a stretch between densifies sees
                has them unchanged over the stretch; denom is the number of frames since the last
                densify that saw the row; the row behind every camera never changes;
  replay        after the fit, every checkpoint's snapshot through a context that never saw the
                fit (slot 1): color and radii equal the fit's bits, and in the deterministic fit
                the backward of the snapshot's dL equals the fit's gradients bit for bit;
  reproducible  the deterministic fit run again ends with the same bits in every parameter,
                moment and statistic and in both source_index, and so do the fits under
                GSR_OPT_FRAME_GRAPHS 1 and 2 (every recorded graph is stale at the next frame);
  loss          the free-running losses of the 20 iterations before the first densify against
                the float64 fit's, within 8 x the float32 fit's spread.

Measured on an MI355X (DESIGN.md 3s has the table per tensor).  The counts of both densifies are
the float64 fit's in both fits (activated 95 / 92 / 1 / 2 and 6 / 2 / 168 / 15 kept / cloned /
split / removed, P 98 -> 189 -> 344; stored 96 / 93 / 1 / 1 and 6 / 2 / 182 / 3, P 98 -> 191 ->
372).  The chain check left out 2 of 14 checkpoints in the activated fit (22 and 37) and none in
the stored one.  The largest gradient error was 0.056 of its bound (activated, means3D, iteration
9) and 0.100 (stored, opacity, 16); in the joint check 0.186 (activated, opacities, 25) and 0.165
(stored, scaling, 24); the loss value used 0.009 of its bound, the loss gradient 0.085; the images
differ from float64 by at most 5.1e-7; no word of a parameter, a moment, a statistic, a count or a
source_index differed anywhere, nor in the replays, the second run or the runs under frame graphs.
The loss sequence differed from float64's by 1.2e-5 (activated, 0.18 of its bound 6.7e-5) and
1.5e-5 to 1.7e-5 in two runs (stored, 0.15 of 1.1e-4).  The module takes 5 s.
"""
import types

import numpy as np
import pytest
import torch

import fit_step_reference as fr
import multiview_fit_reference as mv
from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer,
                                         SparseGaussianAdam, _lib, densification_stats,
                                         densify_and_prune, photometric_loss)
from gaussiansplattingviewer_amd.rasterizer import rasterize_gaussians_backward_native
from gpu_helpers import ALL_EXTRAS, run_hip, set_option, to_dev

pytestmark = pytest.mark.gpu

_fits, _refs = {}, {}


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _settings(gpu, it, activated, D=None):
    s = mv.view_scene(mv.view_of(it), mv.degree(it) if D is None else D)["s"]
    kwargs = dict(deterministic=True) if activated else {}
    rs = GaussianRasterizationSettings(
        s["H"], s["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, **kwargs)
    assert rs.deterministic is (True if activated else None)
    return rs


def _run(gpu, parametrisation, trace):
    """The 48 iterations -> dict(states (checkpoint -> state, fit_step_reference's layout),
    losses, radii (per iteration), after (with `trace`: iteration -> every tensor after it, on the
    host; 0 is the start), final (name -> bits), counts and source_index (densify iteration ->))."""
    names, lrs = fr.GROUPS[parametrisation], mv.GROUP_LRS[parametrisation]
    activated = parametrisation == "activated"
    unperturbed = {k: to_dev(v, gpu) for k, v in fr.parameters(fr.scene(), False).items()}
    targets = {}
    with torch.no_grad():
        for view in range(len(mv.VIEWS)):
            it = mv.visits(view)[0]
            targets[view], _ = GaussianRasterizer(_settings(gpu, it, activated, 3))(
                means2D=None, colors_precomp=None, cov3D_precomp=None, **unperturbed)
    start = fr.parameters(fr.scene(), True, parametrisation)
    params = {k: torch.nn.Parameter(to_dev(start[k], gpu)) for k in names}
    P = len(start[names[0]])
    opt = SparseGaussianAdam([{"params": [params[k]], "lr": lrs[k], "name": k} for k in names],
                             lr=0.0, eps=fr.EPS, betas=fr.BETAS)
    accum = torch.zeros((P, 1), device=gpu)
    denom = torch.zeros((P, 1), device=gpu)
    max_radii = torch.zeros(P, dtype=torch.int32, device=gpu)

    def moments(key):
        return {k: _host(opt.state[params[k]][key]) if key in opt.state.get(params[k], {})
                else np.zeros(params[k].shape, np.float32) for k in names}

    def everything():
        return dict(params={k: _host(params[k]) for k in names}, m=moments("exp_avg"),
                    v=moments("exp_avg_sq"), stats=(_host(accum), _host(denom), _host(max_radii)))

    out = dict(states={}, losses=[], radii=[], after={}, counts={}, source_index={},
               targets={v: _host(t) for v, t in targets.items()}, sh_grad_words={})
    if trace:
        out["after"][0] = everything()
    for it in range(1, mv.ITERATIONS + 1):
        keep = trace and it in mv.CHECKPOINTS
        view = mv.view_of(it)
        target = targets[view]
        if keep:
            before = out["after"][it - 1]
            st = dict(it=it, target=out["targets"][view], params=before["params"], m=before["m"],
                      v=before["v"], stats=before["stats"])
        raster = GaussianRasterizer(_settings(gpu, it, activated))  # rebuilt, as a loop does
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((P, 3), device=gpu, requires_grad=True)
        act = fr.activate(params)
        color, radii = raster(means2D=means2D, colors_precomp=None, cov3D_precomp=None, **act)
        assert tuple(color.shape) == tuple(target.shape)
        loss = photometric_loss(color, target, fr.LAMBDA)
        if keep:
            color.retain_grad()
        loss.backward()
        if keep:
            st.update(dL=_host(color.grad), color=_host(color),
                      activated={k: _host(v) for k, v in act.items()},
                      radii=_host(radii), loss=_host(loss),
                      grads={k: _host(params[k].grad) for k in names})
            st["grads"]["means2D"] = _host(means2D.grad)
        if trace:
            # the words of the SH gradient above the frame's degree that are not zero
            g = params["shs" if activated else "f_rest"].grad
            n = (mv.degree(it) + 1) ** 2 - (0 if activated else 1)
            out["sh_grad_words"][it] = int((g[:, n:].contiguous().view(torch.int32) != 0).sum())
        densification_stats(radii, means2D.grad, accum, denom, max_radii)
        opt.step(radii, P)
        out["losses"].append(float(loss.detach()))
        out["radii"].append(_host(radii))
        if trace:
            out["after"][it] = everything()
        if keep:
            after = out["after"][it]
            st.update(params1=after["params"], m1=after["m"], v1=after["v"], stats1=after["stats"])
            out["states"][it] = st
        if it in mv.DENSIFY_AFTER:
            r = densify_and_prune(opt, accum, denom, max_radii, seed=mv.DENSIFY_SEEDS[it],
                                  roles=fr.ROLES[parametrisation], activated=activated,
                                  **mv.CONTROL[parametrisation][it])
            params = dict(r.params)
            accum, denom, max_radii = r.grad_accum, r.denom, r.max_radii2D
            P = r.counts.total
            out["counts"][it] = tuple(int(c) for c in r.counts)
            out["source_index"][it] = _host(r.source_index)
            assert [g["params"][0] for g in opt.param_groups] == [params[k] for k in names]
            if trace:  # what iteration it + 1 starts from
                out["after"][it] = dict(everything(), before_densify=out["after"][it])
    final = {}
    for k in names:
        st_ = opt.state[params[k]]
        final[f"param {k}"], final[f"exp_avg {k}"], final[f"exp_avg_sq {k}"] = \
            _host(params[k]), _host(st_["exp_avg"]), _host(st_["exp_avg_sq"])
    final.update(grad_accum=_host(accum), denom=_host(denom), max_radii=_host(max_radii))
    for it, src in out["source_index"].items():
        final[f"source_index {it}"] = src
    out["final"] = {k: v.view(np.uint32) if v.dtype == np.float32 else v for k, v in final.items()}
    return out


def _fit(gpu, parametrisation):
    if parametrisation not in _fits:
        _fits[parametrisation] = _run(gpu, parametrisation, trace=True)
    return _fits[parametrisation]


def _scene_of_state(state):
    a = state["activated"]
    P = len(a["means3D"])
    g = types.SimpleNamespace(xyz=a["means3D"], sh=a["shs"].reshape(P, -1), opacity=a["opacities"],
                              scale=a["scales"], rot=a["rotations"])
    return dict(mv.scene_of(state["it"])["s"], g=g)


def _reference(gpu, parametrisation, it):
    """The float64 restatement of the GPU's iteration `it`, on the lists and radii of a no-grad
    replay of the snapshot through the GPU forward (computed once, read-only)."""
    key = (parametrisation, it)
    if key not in _refs:
        state = _fit(gpu, parametrisation)["states"][it]
        fwd = run_hip(_scene_of_state(state), gpu, extras=ALL_EXTRAS, binning=True)
        lists = (fwd["ranges"], fwd["point_list"])
        _refs[key] = (fr.reference_of(mv.scene_of(it), state, lists, fwd["radii"]), lists)
    return _refs[key]


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b, err_msg=what)


@pytest.mark.parametrize("it", mv.CHECKPOINTS)
@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_checkpoint(parametrisation, it, gpu):
    fit = _fit(gpu, parametrisation)
    state = fit["states"][it]
    P = len(state["radii"])
    done = [d for d in mv.DENSIFY_AFTER if d < it]
    assert P == (98 if not done else fit["counts"][done[-1]][0] + fit["counts"][done[-1]][1]
                 + 2 * fit["counts"][done[-1]][2])
    W, H, _ = mv.VIEWS[mv.view_of(it)]
    assert state["color"].shape == (3, H, W)
    ref, lists = _reference(gpu, parametrisation, it)
    checks, _ = mv.check_all(state, parametrisation, lists, ref["radii"], ref)
    if it in mv.DENSIFY_AFTER:
        checks["densify"] = mv.check_densify(
            state, dict(counts=fit["counts"][it], source_index=fit["source_index"][it]),
            parametrisation)
    bad = []
    for name, rows in checks.items():
        if rows is None:
            print(f"{parametrisation} {it}: near {ref['near']}: the {name} check is left out here")
            continue
        fr.show(rows, f"{parametrisation} {it} {name}: ")
        for what, e, b in rows:
            if b > 0:
                print(f"FRACTION {parametrisation} {it} {name} | {what} | {e / b:.4f}")
        bad += fr.failures(rows)
    assert not bad, bad
    assert (state["grads"]["means2D"][:, 2] == 0).all()
    if it - 1 in mv.DENSIFY_AFTER:
        # the rebind: kept rows carry their source row's parameters and moments of the iteration
        # before, clones its parameters; clones and children start from zero moments, all from
        # zero statistics
        last, src = fit["states"][it - 1], fit["source_index"][it - 1]
        n_kept, n_clone = fit["counts"][it - 1][:2]
        kept, fresh = slice(0, n_kept), slice(n_kept, P)
        assert len(src) == P and len(np.unique(src[kept])) == n_kept
        for k in fr.GROUPS[parametrisation]:
            for now, then in (("params", "params1"), ("m", "m1"), ("v", "v1")):
                _same_bits(state[now][k][kept], last[then][k][src[kept]], k)
            clones = slice(n_kept, n_kept + n_clone)
            _same_bits(state["params"][k][clones], last["params1"][k][src[clones]], k)
            assert not state["m"][k][fresh].any() and not state["v"][k][fresh].any(), k
            assert state["m"][k][kept].any() and state["v"][k][kept].any(), k
        assert not state["stats"][0].any() and not state["stats"][1].any()
        assert not state["stats"][2].any()
        if it - 1 == mv.DENSIFY_AFTER[1]:
            # some kept rows are rows the first densify created, with the moments iteration 36
            # wrote into them
            first = fit["counts"][mv.DENSIFY_AFTER[0]]
            made = src[kept] >= first[0]
            print(f"{parametrisation}: {int(made.sum())} of the {n_kept} rows kept by the second "
                  "densify were created by the first")
            assert made.any()
            k = fr.GROUPS[parametrisation][0]
            assert state["m"][k][kept][made].any() and state["v"][k][kept][made].any()


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_chain_skips_within_cap(parametrisation, gpu):
    """What the chain check left out is within the cap: at most 3 of the 14, never both
    neighbours of a densify, never both sides of a degree change."""
    near = {it: _reference(gpu, parametrisation, it)[0]["near"] for it in mv.CHECKPOINTS}
    skipped = fr.left_out(near)
    print(f"{parametrisation}: the chain check skipped {len(skipped)} of {len(mv.CHECKPOINTS)} "
          f"checkpoints: {skipped}")
    assert mv.cap_holds(skipped), skipped


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_loss_sequence(parametrisation, gpu):
    """The free-running losses of the twenty iterations before the first densify against the
    float64 fit's, within 8 x s; and density control did what the thresholds were chosen for."""
    fit = _fit(gpu, parametrisation)
    losses = np.array(fit["losses"])
    assert len(losses) == mv.ITERATIONS and np.isfinite(losses).all()
    e = mv.loss_sequence_error(losses, parametrisation)
    s = mv.LOSS_SPREAD[parametrisation]
    print(f"{parametrisation}: losses " + " ".join(f"{v:.5f}" for v in losses))
    print(f"{parametrisation}: counts {fit['counts']}, the reference's "
          f"{mv.COUNTS[parametrisation]}")
    print(f"{parametrisation}: max |loss_gpu / loss_ref - 1| = {e:.3e}, s = {s:.1e}, "
          f"bound {fr.LOSS_FACTOR * s:.1e} ({e / (fr.LOSS_FACTOR * s):.3f} of it)")
    assert e <= fr.LOSS_FACTOR * s
    for it in mv.DENSIFY_AFTER:
        n_kept, n_clone, n_split, n_removed = fit["counts"][it]
        assert n_clone >= 1 and n_split >= 1 and n_removed >= 1
    assert len(fit["radii"][-1]) <= mv.MAX_FINAL_P


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_inactive_sh_coefficients(parametrisation, gpu):
    fit = _fit(gpu, parametrisation)
    key, dc = ("shs", 0) if parametrisation == "activated" else ("f_rest", 1)
    start = fit["after"][0]
    for it in range(1, mv.ITERATIONS + 1):
        if mv.degree(it) < 3:
            assert fit["sh_grad_words"][it] == 0, (it, fit["sh_grad_words"][it])
    for D in (1, 2, 3):
        first = 8 * D + 1  # the first iteration at degree D
        assert mv.degree(first) == D and mv.degree(first - 1) == D - 1
        assert first <= mv.DENSIFY_AFTER[0] or D == 3
        lo, hi = D * D - dc, (D + 1) ** 2 - dc
        # rows keep their places up to the first densify; degree 3 starts behind it
        if first <= mv.DENSIFY_AFTER[0]:
            before, after = fit["after"][first - 1], fit["after"][first]
            _same_bits(before["params"][key][:, lo:], start["params"][key][:, lo:], f"{key} {D}")
            seen = fit["radii"][first - 1] > 0
        else:
            before, after = fit["after"][first - 1], fit["after"][first]
            src = fit["source_index"][mv.DENSIFY_AFTER[0]]
            # every row there is a copy of a row of the start, whose coefficients never moved
            _same_bits(before["params"][key][:, lo:], start["params"][key][src][:, lo:],
                       f"{key} {D}")
            seen = fit["radii"][first - 1] > 0
        # a row the frame sees may still reach no pixel: the rows that moved are those with a
        # gradient (`first` is a checkpoint), all of them seen
        moved = (fit["states"][first]["grads"][key][:, lo:hi] != 0).any(axis=(1, 2))
        assert moved.any() and not (moved & ~seen).any() and 2 * moved.sum() >= seen.sum()
        for mom in ("m", "v"):
            assert not before[mom][key][:, lo:].view(np.uint32).any(), (mom, D)
            assert not after[mom][key][~moved][:, lo:].view(np.uint32).any(), (mom, D)
            assert not after[mom][key][:, hi:].view(np.uint32).any(), (mom, D)
        assert after["m"][key][moved][:, lo:hi].any(axis=(1, 2)).all(), D
        assert after["v"][key][moved][:, lo:hi].any()
        print(f"{parametrisation}: degree {D} from iteration {first}: coefficients {lo}..{hi - 1} "
              f"of {key} untouched before it, moments non-zero in the {int(moved.sum())} rows with "
              f"a gradient, of {int(seen.sum())} seen")


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_unseen_rows_keep_every_bit(parametrisation, gpu):
    fit = _fit(gpu, parametrisation)
    names = fr.GROUPS[parametrisation]
    longest = (0, None, None)
    stretch_start = 0
    for end in mv.DENSIFY_AFTER + (mv.ITERATIONS,):
        its = range(stretch_start + 1, end + 1)
        radii = np.stack([fit["radii"][it - 1] for it in its])
        assert stretch_start == 0 or not fit["after"][stretch_start]["stats"][1].any()
        for i, it in enumerate(its):
            off = radii[i] <= 0
            assert off.any(), it
            before, after = fit["after"][it - 1], fit["after"][it].get("before_densify",
                                                                       fit["after"][it])
            for k in names:
                for part in ("params", "m", "v"):
                    _same_bits(after[part][k][off], before[part][k][off], f"{part} {k} at {it}")
        # a row that a run of consecutive frames does not see: the same over the whole run
        for row in np.flatnonzero((radii > 0).any(0)):
            run = 0
            for i in range(len(its)):
                run = run + 1 if radii[i, row] <= 0 else 0
                if run > longest[0]:
                    longest = (run, row, its[i])
        last = fit["after"][end].get("before_densify", fit["after"][end])
        _same_bits(last["stats"][1].reshape(-1), (radii > 0).sum(0).astype(np.float32), "denom")
        _same_bits(last["stats"][2], np.where(radii > 0, radii, 0).max(0).astype(np.int32),
                   "max_radii")
        stretch_start = end
    n, row, end = longest
    print(f"{parametrisation}: the longest run that leaves out a row it otherwise sees: row {row}, "
          f"iterations {end - n + 1}..{end}")
    assert n >= 2
    # ... and the row behind every camera: nothing of it changes until a densify drops or moves it
    assert all(r[fr.BEHIND] <= 0 for r in fit["radii"][:mv.DENSIFY_AFTER[0]])
    a, b = fit["after"][0], fit["after"][mv.DENSIFY_AFTER[0]]["before_densify"]
    for k in names:
        for part in ("params", "m", "v"):
            _same_bits(b[part][k][fr.BEHIND], a[part][k][fr.BEHIND], f"{part} {k}")
    assert b["stats"][1][fr.BEHIND] == 0


_GRADS = dict(means3D="dL_dmeans3D", shs="dL_dsh", opacities="dL_dopacity", scales="dL_dscales",
              rotations="dL_drotations", means2D="dL_dmeans2D")


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_replay_on_a_context_that_never_saw_the_fit(parametrisation, gpu):
    """Every checkpoint's snapshot through slot 1, after the fit: what the fit's context carried
    from the previous shape or P did not reach its outputs."""
    fit = _fit(gpu, parametrisation)
    for it in mv.CHECKPOINTS:
        state = fit["states"][it]
        s = _scene_of_state(state)
        fwd = run_hip(s, gpu, extras=(), binning=False, slot=1)
        _same_bits(fwd["color"], state["color"], f"color at {it}")
        _same_bits(fwd["radii"], state["radii"], f"radii at {it}")
        if parametrisation != "activated":
            continue
        a = {k: to_dev(v, gpu) for k, v in state["activated"].items()}
        g = rasterize_gaussians_backward_native(
            to_dev(s["bg"], gpu), a["means3D"], None, a["opacities"], a["scales"], a["rotations"],
            s["scale_modifier"], None, to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"],
            s["ty"], to_dev(state["dL"], gpu), a["shs"], s["sh_degree"], to_dev(s["campos"], gpu),
            deterministic=True, slot=1)
        for k, name in _GRADS.items():
            _same_bits(_host(g[name]).reshape(state["grads"][k].shape), state["grads"][k],
                       f"{name} at {it}")


def test_deterministic_fit_is_reproducible_with_and_without_frame_graphs(gpu):
    """The "activated" fit again, and under GSR_OPT_FRAME_GRAPHS 1 and 2 on its context: the same
    bits in every parameter, moment and statistic and in source_index of both densifies."""
    first = _fit(gpu, "activated")["final"]
    runs = {"again": _run(gpu, "activated", trace=False)["final"]}
    try:
        for mode in (1, 2):
            set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, mode)
            runs[f"graphs {mode}"] = _run(gpu, "activated", trace=False)["final"]
    finally:
        set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, 0)
    for what, got in runs.items():
        assert set(got) == set(first)
        for k in first:
            np.testing.assert_array_equal(got[k], first[k], err_msg=f"{what}: {k}")
