"""A multi-view fit and its float64 restatement on the CPU, over tests/fit_step_reference.py.

The fits of fit_step_reference are one camera, one frame shape, one SH degree and one densify.
This one is the scene, start and parametrisations of that module ("activated" on the deterministic
backward, "stored" on the atomic one) fitted as a training loop fits:

  views     VIEWS: four static_camera(W, H, eye=...) of different eyes and frame shapes, one taller
            than wide, one with odd W and H (a 1-pixel partial tile column and row), one larger
            than 40 x 24; their tile grids are 3 x 2, 2 x 3, 3 x 2 and 3 x 3.  At the start they see
            96, 85, 95 and 82 of the 98 rows; every view leaves out a row another sees, and the row
            behind the first camera is behind all four (test_multiview_fit_reference.py holds the
            conditions);
  order     ORDER: a seeded permutation of the four per epoch (ORDER_SEED); across the epoch
            boundary 8 | 9 the same view comes twice in a row, under a new SH degree;
  degree    degree(it) = min(3, (it - 1) // 8); the settings are rebuilt every iteration;
  targets   per view, the render of the unperturbed scene at degree 3;
  control   ITERATIONS = 48 with densify_and_prune after 20 and after 36 (neither on a degree
            change), the statistics zeroed after each; CONTROL, per parametrisation and densify,
            was chosen on the float64 fit, before any GPU run (the margins are in DESIGN.md 3s);
  rates     GROUP_LRS: fit_step_reference's but for the scales.

trajectory() is the float64 fit, recording the state in front of every iteration of CHECKPOINTS;
`step32` is the float32 restatement of one iteration from such a record and, with `mutant`, one
of eight wrong iterations.  The checks of an iteration are fit_step_reference's on this fit's
measured tables (CHAIN_SPREAD, JOINT_SPREAD), and `check_densify` for the two density controls.
The GPU's part is tests/test_gpu_fit_multiview.py.
"""
from __future__ import annotations

import numpy as np
import torch

import densify_reference as D
import fit_step_reference as fr
import grad_reference as gr
import loss_reference as L
import optimizer_reference as O
from gaussiansplattingviewer_amd.camera import static_camera
from gpu_helpers import scene_inputs

F32 = np.float32
# (W, H, eye)
VIEWS = ((40, 24, (0.0, 0.0, 4.0)), (24, 40, (1.8, 0.3, 3.5)), (33, 17, (-0.5, 2.5, 2.4)),
         (48, 40, (-0.6, -0.9, 2.7)))
ITERATIONS = 48
DENSIFY_AFTER = (20, 36)
DENSIFY_SEEDS = {20: 20, 36: 36}
STEPS = 20  # the loss sequence: the iterations before the first densify
ORDER_SEED = 105
# np.concatenate([default_rng(ORDER_SEED).permutation(4) for _ in range(12)]): the view of
# iteration it is ORDER[it - 1]
ORDER = (0, 1, 3, 2, 0, 1, 3, 2, 2, 1, 0, 3, 2, 1, 0, 3, 0, 3, 1, 2, 1, 3, 2, 0,
         1, 0, 2, 3, 1, 0, 2, 3, 2, 3, 0, 1, 3, 0, 2, 1, 2, 3, 0, 1, 0, 1, 3, 2)
PAIR = (8, 9)  # the same view twice in a row
CHECKPOINTS = (1, 8, 9, 16, 17, 20, 21, 22, 24, 25, 36, 37, 38, 48)
DEGREE_CHANGES = ((8, 9), (16, 17), (24, 25))
MAX_FINAL_P = 400
# fit_step_reference's learning rates but for the scales (there 1e-3 and, in log space, 5e-3): at
# those the largest rows grow by up to a quarter in twenty iterations and no split threshold
# between the two largest keeps its 10 % on both sides
GROUP_LRS = dict(activated=dict(fr.GROUP_LRS["activated"], scales=3e-4),
                 stored=dict(fr.GROUP_LRS["stored"], scaling=1e-3))
# densify iteration -> thresholds, per parametrisation.  Every statistic of every row has to lie
# 10 % from its threshold (fit_step_reference.densify_margins), and the 98 largest scales lie too
# close together for a split threshold anywhere but in the tails: after 20 it sits between the large
# near Gaussian and the next largest row (one split, the other hot rows cloned), after 36 between
# the smallest row (with its clone) and the next (two clones, the other hot rows split).  One set
# of thresholds for both densifies does not exist.  max_screen_size is a non-integer: no radius
# can sit on it.
CONTROL = dict(
    activated={20: dict(max_grad=3.37e-4, min_opacity=0.11, extent=8.3, max_screen_size=200.5,
                        percent_dense=0.04842),
               36: dict(max_grad=1.57e-5, min_opacity=0.01, extent=8.3, max_screen_size=45.5,
                        percent_dense=0.00752)},
    stored={20: dict(max_grad=3.95e-4, min_opacity=0.064, extent=8.3, max_screen_size=200.5,
                     percent_dense=0.04909),
            36: dict(max_grad=4e-5, min_opacity=0.022, extent=8.3, max_screen_size=57.5,
                     percent_dense=0.00756)})
# (kept, cloned, split, removed) of the float64 fit, which the float32 fit reaches too
COUNTS = dict(activated={20: (95, 92, 1, 2), 36: (6, 2, 168, 15)},
              stored={20: (96, 93, 1, 1), 36: (6, 2, 182, 3)})

def degree(it):
    return min(3, (it - 1) // 8)


def view_of(it):
    return ORDER[it - 1]


_SCENES, _TARGETS, _TRAJECTORY = {}, {}, {}


def view_scene(view, D_, overrides=None):
    """The scene of fit_step_reference under VIEWS[view] at SH degree D_ (a grad_scenes-layout
    dict: read-only, shared).  overrides: entries of s to replace (a copy then)."""
    key = (view, D_)
    if key not in _SCENES:
        base = fr.scene()
        W, H, eye = VIEWS[view]
        s = scene_inputs(base["s"]["g"], static_camera(W, H, eye=eye), D_, bg=base["s"]["bg"],
                         scale_modifier=base["s"]["scale_modifier"])
        _SCENES[key] = dict(name=f"chain_fit_view{view}_d{D_}", s=s, W=W, H=H, colors=None,
                            cov6=None)
    sc = _SCENES[key]
    if overrides:
        sc = dict(sc, s=dict(sc["s"], **overrides))
    return sc


def scene_of(it):
    return view_scene(view_of(it), degree(it))


def target64(view):
    """The float64 render of the unperturbed scene from VIEWS[view] at degree 3 (computed once)."""
    if view not in _TARGETS:
        sc = view_scene(view, 3)
        _TARGETS[view] = fr.render64(sc, fr.parameters(sc, False))[0].detach()
    return _TARGETS[view]


# ---- the reference fit -------------------------------------------------------------------------------
def fit(parametrisation, dtype=torch.float64, iterations=ITERATIONS, checkpoints=(),
        densify_after=DENSIFY_AFTER, control=None):
    """The multi-view fit in `dtype` -> dict(losses, radii (per iteration), records (iteration of
    `checkpoints` -> the state in front of it, rounded to float32), counts and before_densify
    (densify iteration -> ...))."""
    names, lrs = fr.GROUPS[parametrisation], GROUP_LRS[parametrisation]
    control = control or CONTROL[parametrisation]
    p = {k: torch.tensor(v.astype(np.float64), dtype=dtype, requires_grad=True)
         for k, v in fr.parameters(fr.scene(), True, parametrisation).items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    P = len(p[names[0]])
    stats = [np.zeros((P, 1)), np.zeros((P, 1)), np.zeros(P, np.int32)]
    out = dict(losses=[], radii=[], records={}, counts={}, before_densify={})
    f32 = lambda d: {k: np.ascontiguousarray(t.detach().to(torch.float32).numpy())  # noqa: E731
                     for k, t in d.items()}
    for it in range(1, iterations + 1):
        sc = scene_of(it)
        lists, radii = fr.oracle_lists(sc, p)
        ch = fr.chain(sc, p, lists, radii, dtype)
        loss = L.loss_values(ch["color"], target64(view_of(it)).to(dtype), fr.LAMBDA)[0]
        out["losses"].append(float(loss.detach()))
        out["radii"].append(radii)
        if it in checkpoints:
            out["records"][it] = dict(
                it=it, params=f32(p), m=f32(m), v=f32(v2), radii=radii, lists=lists,
                stats=(stats[0].astype(F32), stats[1].astype(F32), stats[2].copy()),
                near=ch["near"])
        for t in p.values():
            t.grad = None
        loss.backward()
        on = radii > 0
        g2 = ch["leaves"]["means2D"].grad.double().numpy()
        stats[0][on, 0] += np.sqrt(g2[on, 0] ** 2 + g2[on, 1] ** 2)
        stats[1][on, 0] += 1.0
        stats[2][on] = np.maximum(stats[2][on], radii[on])
        fr._adam(p, m, v2, names, lrs, torch.as_tensor(on))
        if it in densify_after:
            p, m, v2, out["counts"][it], out["before_densify"][it] = fr._densify(
                parametrisation, p, m, v2, stats, control[it], DENSIFY_SEEDS[it])
            P = len(p[names[0]])
            stats = [np.zeros((P, 1)), np.zeros((P, 1)), np.zeros(P, np.int32)]
    return out


def trajectory(parametrisation):
    """The float64 fit with its records at CHECKPOINTS (computed once per parametrisation,
    read-only)."""
    if parametrisation not in _TRAJECTORY:
        _TRAJECTORY[parametrisation] = fit(parametrisation, checkpoints=CHECKPOINTS)
    return _TRAJECTORY[parametrisation]


def densify_margins(parametrisation, it, before=None):
    """fit_step_reference.densify_margins of the state in front of the densify after `it`."""
    b = before or trajectory(parametrisation)["before_densify"][it]
    return fr.densify_margins(parametrisation, b, CONTROL[parametrisation][it])


def visits(view, iterations=ITERATIONS):
    return [it for it in range(1, iterations + 1) if view_of(it) == view]


# ---- the constants the GPU tests are held to: measured here, not chosen ------------------------------
# The loss of fit(dtype=float64) in front of each of the STEPS iterations before the first densify.
LOSSES = dict(
    activated=(0.05382117082855212, 0.03539983278736941, 0.03403994045569472,
               0.04524765028697342, 0.030573320893698804, 0.033824425596929594,
               0.02931795778682102, 0.035950778246240496, 0.04867095732601709,
               0.03508210232798739, 0.03972674790816064, 0.029675539317924465,
               0.029810285398095694, 0.023953007796341047, 0.030325253732275202,
               0.02275458017760658, 0.04893031725219012, 0.03279562676922602,
               0.037956781001596426, 0.05734501117957025),
    stored=(0.05382117036905003, 0.035792889929367876, 0.034082014330765874,
            0.0450731361285385, 0.030261172732407998, 0.03133172438474478,
            0.029772808716184544, 0.03713100612577655, 0.05035133408579603,
            0.03426820134999581, 0.039082821794577664, 0.02912977865191003,
            0.029240862063926083, 0.02479140423047391, 0.028299704570699396,
            0.02436876650572143, 0.05021289416328564, 0.030968297734181888,
            0.03699662863845647, 0.05514856327669265))
# s = max_i |loss32[i] / loss64[i] - 1| over those, loss32 of fit(dtype=float32): measured 8.4e-6
# and 1.4e-5 (fit_step_reference's single view has 1.8e-2 and 8.5e-3)
LOSS_SPREAD = dict(activated=8.4e-6, stored=1.4e-5)
# fit_step_reference.CHAIN_SPREAD and JOINT_SPREAD, measured the same way (`measure_chain_spread`:
# `step32` against `reference_of`) over this fit's CHECKPOINTS whose `near` is (0, 0)
CHAIN_SPREAD = dict(
    activated=dict(means3D=1.2e-5, shs=2.4e-5, opacities=1.5e-5, scales=2.0e-5, rotations=1.9e-5,
                   means2D=1.2e-5),     # the largest at iterations 16, 37, 16, 36, 9, 8
    stored=dict(xyz=2.2e-5, f_dc=4.8e-5, f_rest=4.2e-5, opacity=1.3e-5, scaling=2.7e-5,
                rotation=2.6e-5, means2D=3.3e-5))   # at 37, 37, 37, 16, 1, 37, 37
JOINT_SPREAD = dict(
    activated=dict(means3D=2.8e-6, shs=5.6e-7, opacities=5.6e-7, scales=1.0e-6, rotations=2.5e-6,
                   means2D=3.5e-6),     # the largest at iterations 21, 48, 38, 16, 48, 38
    stored=dict(xyz=2.5e-6, f_dc=6.9e-7, f_rest=6.7e-7, opacity=7.3e-7, scaling=9.4e-7,
                rotation=2.7e-6, means2D=2.6e-6))   # at 36, 20, 37, 21, 25, 16, 36

def chain_f(parametrisation, key, table=None):
    return fr.chain_f(parametrisation, key, CHAIN_SPREAD if table is None else table)


def measure_chain_spread(parametrisation, per_iteration=None):
    """(CHAIN_SPREAD[parametrisation], JOINT_SPREAD[parametrisation], where each maximum fell) as
    measured now."""
    keys = fr.chain_keys(parametrisation)
    f, fj = {k: 0.0 for k in keys}, {k: 0.0 for k in keys}
    at, atj = {}, {}
    for it, rec in trajectory(parametrisation)["records"].items():
        state = step32(rec, parametrisation)
        ref = fr.reference_of(scene_of(it), state, rec["lists"], rec["radii"])
        if ref["near"] != (0, 0):
            continue
        for k in keys:
            own = gr.rel_err(state["grads"][k], ref["grads"][k])
            joint = gr.rel_err(state["grads"][k], ref["joint"][k])
            if per_iteration is not None:
                per_iteration.setdefault(it, {})[k] = (own, joint)
            if own >= f[k]:
                f[k], at[k] = own, it
            if joint >= fj[k]:
                fj[k], atj[k] = joint, it
    return f, fj, (at, atj)


def measure_loss_spread(parametrisation):
    l32 = np.array(fit(parametrisation, torch.float32, STEPS, densify_after=())["losses"])
    return float(np.abs(l32 / np.array(LOSSES[parametrisation]) - 1.0).max())


def loss_sequence_error(losses, parametrisation):
    """max_i |losses[i] / LOSSES[i] - 1| over the STEPS iterations before the first densify."""
    got = np.asarray(losses, np.float64)[:STEPS]
    assert len(got) == STEPS
    return float(np.abs(got / np.array(LOSSES[parametrisation]) - 1.0).max())


# ---- which checkpoints the chain-gradient check may leave out ----------------------------------------
def cap_holds(skipped):
    """At most 3 of the checkpoints, never both neighbours of a densify (20 and 21, 36 and 37),
    never both sides of a degree change."""
    s = set(skipped)
    return (s <= set(CHECKPOINTS) and len(s) <= fr.MAX_LEFT_OUT
            and not any({a, a + 1} <= s for a in DENSIFY_AFTER)
            and not any(set(pair) <= s for pair in DEGREE_CHANGES))


# ---- the checks ----------------------------------------------------------------------------------------
def check_all(state, parametrisation, lists, radii, ref=None):
    """fit_step_reference.check_all of a state of iteration state["it"], on this fit's tables."""
    return fr.check_all(scene_of(state["it"]), state, parametrisation, lists, radii, ref,
                        (CHAIN_SPREAD, JOINT_SPREAD), GROUP_LRS[parametrisation])


def classify32(state, parametrisation, stats=None):
    """densify_reference's classification of a state's parameters and statistics after its step
    (or of given statistics) -> dict(counts, source_index)."""
    roles = fr.ROLES[parametrisation]
    accum, denom, max_radii = stats or state["stats1"]
    thresholds, radius, log_space = fr.densify_thresholds(parametrisation,
                                                          CONTROL[parametrisation][state["it"]])
    keep, clone, split = D.classify(accum, denom, state["params1"][roles["scaling"]],
                                    state["params1"][roles["opacity"]], max_radii, thresholds,
                                    radius, log_space)
    P = len(keep)
    rows = np.arange(P, dtype=np.int32)
    return dict(counts=(int(keep.sum()), int(clone.sum()), int(split.sum()),
                        int(P - keep.sum() - split.sum())),
                source_index=np.concatenate([rows[keep], rows[clone], rows[split], rows[split]]))


def check_densify(state, result, parametrisation):
    """The densify after the state's iteration: the counts and source_index of `result` are
    densify_reference's classification of the state's own parameters and statistics."""
    want = classify32(state, parametrisation)
    got = np.asarray(result["source_index"])
    same_shape = got.shape == want["source_index"].shape
    return [("densify counts", float(sum(a != b for a, b in zip(result["counts"], want["counts"]))),
             0.0),
            ("densify source_index",
             float((got != want["source_index"]).sum()) if same_shape else float("inf"), 0.0)]


# ---- a float32 restatement of one iteration, and its mutants -----------------------------------------
# mutant -> the check that must reject it
MUTANTS = {"previous view matrix": "forward", "previous tile grid": "forward",
           "previous target": "loss", "moments of unseen rows decay": "adam",
           "denom for every row": "stats", "max_radii overwritten": "stats",
           "next degree one iteration early": "forward",
           "second densify on the first's statistics": "densify"}


def _stale(a, shape):
    """A buffer of another shape read at `shape`: its words in order, zeros beyond its end."""
    flat = np.asarray(a).reshape(-1)
    out = np.zeros(int(np.prod(shape)), flat.dtype)
    n = min(len(out), len(flat))
    out[:n] = flat[:n]
    return out.reshape(shape)


def step32(rec, parametrisation, mutant=None, stale=None):
    """One iteration from a trajectory() record in float32, as a state of fit_step_reference's
    layout (plus "it"); with `mutant`, a wrong one.  stale: for the densify mutant, the statistics
    from before the first densify."""
    assert mutant is None or mutant in MUTANTS
    it = rec["it"]
    names = fr.GROUPS[parametrisation]
    sc = scene_of(it)
    target = target64(view_of(it)).numpy().astype(F32)
    lists, radii = rec["lists"], np.asarray(rec["radii"], np.int32)
    r64 = fr.chain(sc, rec["params"], lists, radii)
    gates = r64["gates"]
    if mutant == "previous view matrix":
        sc = view_scene(view_of(it), degree(it), dict(view=scene_of(it - 1)["s"]["view"]))
    if mutant == "next degree one iteration early":
        sc = view_scene(view_of(it), degree(it) + 1)
    if mutant in ("previous view matrix", "next degree one iteration early"):
        lists, radii = fr.oracle_lists(sc, rec["params"])
        gates = None
    if mutant == "previous tile grid":
        # the lists are this frame's; the blend finds tile (x, y) at y * (the previous grid's
        # width) + x
        gx, gy = (sc["W"] + 15) // 16, (sc["H"] + 15) // 16
        gx0 = (scene_of(it - 1)["W"] + 15) // 16
        assert gx0 != gx
        ranges = np.asarray(lists[0]).reshape(-1, 2)
        moved = np.zeros_like(ranges)
        for y in range(gy):
            for x in range(gx):
                if y * gx0 + x < len(ranges):
                    moved[y * gx + x] = ranges[y * gx0 + x]
        lists, gates = (moved, lists[1]), None
    ch = fr.chain(sc, rec["params"], lists, radii, torch.float32, gates)
    color = np.ascontiguousarray(ch["color"].detach().numpy(), F32)
    if mutant == "previous target":
        loss, dL = fr.loss_gradient(color, _stale(target64(view_of(it - 1)).numpy().astype(F32),
                                                  target.shape), torch.float32)
    else:
        loss, dL = fr.loss_gradient(color, target, torch.float32)
    dL = np.ascontiguousarray(dL, F32)
    grads = {k: v.astype(F32) for k, v in fr.chain_gradients(ch, dL).items()}
    mask = radii > 0
    state = dict(it=it, params=rec["params"], activated=fr.activated32(rec["params"]), color=color,
                 radii=radii, loss=F32(loss), target=target, grads=grads, dL=dL, m=rec["m"],
                 v=rec["v"], stats=rec["stats"], params1={}, m1={}, v1={})
    for k in names:
        p1, m1, v1 = O.adam_step(rec["params"][k], grads[k], rec["m"][k], rec["v"][k],
                                 GROUP_LRS[parametrisation][k], fr.EPS, fr.BETAS[0],
                                 fr.BETAS[1], rows=mask)
        if mutant == "moments of unseen rows decay":
            sel = mask.reshape((-1,) + (1,) * (m1.ndim - 1))
            m1 = np.where(sel, m1, F32(fr.BETAS[0]) * rec["m"][k]).astype(F32)
            v1 = np.where(sel, v1, F32(fr.BETAS[1]) * rec["v"][k]).astype(F32)
        state["params1"][k], state["m1"][k], state["v1"][k] = p1, m1, v1
    a1, d1, r1 = O.densify_stats(radii, grads["means2D"], *rec["stats"])
    if mutant == "denom for every row":
        d1 = (rec["stats"][1] + F32(1.0)).astype(F32)
    if mutant == "max_radii overwritten":
        r1 = np.where(mask, radii, rec["stats"][2]).astype(np.int32)
    state["stats1"] = (a1, d1, r1)
    if it in DENSIFY_AFTER:
        stats = None
        if mutant == "second densify on the first's statistics":
            stats = tuple(_stale(a, b.shape) for a, b in zip(stale, state["stats1"]))
        state["densify"] = classify32(state, parametrisation, stats)
    return state
