"""The small fit of tests/test_gpu_fit_step.py, and its float64 restatement on the CPU.

The scene is grad_scenes "chain" (P = 96, 40 x 24 px) plus two Gaussians: one behind the camera,
which no frame ever sees, and one made large and near enough for a screen radius above 20 px.
The target is the scene's own render; the start is a seeded perturbation of the means, the
opacities and the SH coefficients.  An iteration is render -> L1 + D-SSIM loss -> backward ->
densification statistics -> sparse Adam step over the parameter tensors, the rows chosen by the
frame's radii.

Two parametrisations of the same fit:
  "activated"  the five tensors the rasterizer takes (NAMES), as tests/test_gpu_fit_step.py and
               tests/test_gpu_fit_densify.py run it, on the deterministic backward;
  "stored"     upstream's six groups (GROUPS["stored"]): xyz, f_dc and f_rest (slices of shs),
               logit opacities, log scales and unnormalised quaternions (each row times a seeded
               factor in [0.5, 2]), activated in torch (`activate`) in front of the rasterizer,
               on the default (atomic) backward, with densify_and_prune(activated=False).

reference_fit() runs either in float64 with the torch restatements of tests/grad_reference.py (the
lists and radii of every iteration from the CPU oracle on the current parameters) and
tests/loss_reference.py, and a float64 sparse Adam in upstream's uncorrected form.  The
perturbation, the learning rates, the step count and the densify thresholds below were chosen with
it, before any GPU run, so that the reference's loss at least halves in STEPS steps and every
densify statistic lies at least 10 % from its threshold (test_fit_step_reference.py holds both).
trajectory() is the same loop for ITERATIONS iterations with the densify of
tests/densify_reference.py after iteration DENSIFY_AFTER, recording the state at CANDIDATES.

What the GPU tests assert with it (tests/test_gpu_fit_chain.py):
  * per checkpoint, one iteration started from the GPU's own state ("teacher forced") against the
    float64 restatement of that iteration: the checks of `check_forward`, `check_loss`,
    `check_loss_gradient`, `check_chain`, `check_joint`, `check_adam` and `check_stats` below;
  * the free-running loss sequence of the first STEPS iterations against LOSSES within
    8 x LOSS_SPREAD.
test_fit_step_reference.py feeds the same checks a float32 restatement of the iteration (`step32`)
in the GPU's place, which they accept, and eight mutants of it, which they reject.

Checkpoints.  CANDIDATES = 1, 2, 3, 10, 19, 20, 21, 22, 30, 40 (21 is the first frame at the new
P).  A checkpoint whose float64 evaluation has a float decision within rounding of its gate
(grad_reference's `near` != (0, 0)) is left out of the chain-gradient check only; `cap_holds`
states what may be left out.  On the float64 reference's own trajectory none of the ten is left
out, in either parametrisation (test_fit_step_reference.py holds <= 1).
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import densify_reference as D
import grad_reference as gr
import grad_scenes
import loss_reference as L
import optimizer_reference as O

F32 = np.float32
STEPS = 20
SEED = 2024
LAMBDA = 0.2
EPS = 1e-15
BETAS = (0.9, 0.999)
# the rasterizer's argument names, in the optimizer's group order
NAMES = ("means3D", "shs", "opacities", "scales", "rotations")
LRS = dict(means3D=4e-3, shs=1e-2, opacities=1e-2, scales=1e-3, rotations=1e-3)
PERTURB = dict(means3D=0.04, shs=0.15, opacities=0.08)
BEHIND, LARGE = 96, 97  # the two added rows
MIN_LARGE_RADIUS = 20

# ---- the two parametrisations ----------------------------------------------------------------------
PARAMETRISATIONS = ("activated", "stored")
GROUPS = dict(activated=NAMES,
              stored=("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))
GROUP_LRS = dict(activated=LRS,
                 stored=dict(xyz=4e-3, f_dc=1e-2, f_rest=1e-2, opacity=5e-2, scaling=5e-3,
                             rotation=1e-3))
# densify_and_prune's roles -> the group that holds them
ROLES = dict(activated=dict(xyz="means3D", scaling="scales", rotation="rotations",
                            opacity="opacities"),
             stored=dict(xyz="xyz", scaling="scaling", rotation="rotation", opacity="opacity"))
ROTATION_FACTOR = (0.5, 2.0)

# ---- the forty iterations with density control (tests/test_gpu_fit_densify.py) ---------------------
ITERATIONS, DENSIFY_AFTER, DENSIFY_SEED = 40, 20, 20
CANDIDATES = (1, 2, 3, 10, 19, 20, 21, 22, 30, 40)
# "activated": the thresholds of tests/test_gpu_fit_densify.py (its docstring has their margins).
# "stored": chosen the same way from trajectory("stored"); `densify_margins` measures them.
CONTROL = dict(
    activated=dict(max_grad=2.4e-4, min_opacity=0.005, extent=8.3, max_screen_size=24,
                   percent_dense=0.01),
    stored=dict(max_grad=2.4e-4, min_opacity=0.005, extent=8.3, max_screen_size=24,
                percent_dense=0.011))
MIN_MARGIN = 0.10


def scene():
    """"chain" with the two added Gaussians: a grad_scenes-layout dict (the target's scene)."""
    sc = copy.deepcopy(grad_scenes.get("chain"))
    sc.pop("orc", None)
    sc.pop("ref64", None)
    g = sc["s"]["g"]
    add = lambda a, rows: np.ascontiguousarray(np.concatenate([a, np.asarray(rows, F32)]), F32)  # noqa: E731
    sh = np.zeros((2, g.sh.shape[1]), F32)
    sh[:, :3] = ((0.5, -0.2, 0.1), (-0.3, 0.4, 0.6))
    # the eye is at z = 4 and looks down -z: z = 6 is behind it; z = 2 is near
    g.xyz = add(g.xyz, [(0.3, -0.2, 6.0), (0.4, 0.1, 2.0)])
    g.rot = add(g.rot, [(1.0, 0.0, 0.0, 0.0), (0.8, 0.0, 0.6, 0.0)])
    g.scale = add(g.scale, [(0.2, 0.2, 0.2), (0.45, 0.3, 0.2)])
    g.opacity = add(g.opacity, [(0.7,), (0.35,)])
    g.sh = add(g.sh, sh)
    sc["name"] = "chain_fit"
    return sc


def parameters(sc, perturbed, parametrisation="activated"):
    """name -> float32 array by the group names of `parametrisation`; with `perturbed` the fit's
    start (the two added rows keep their places).  "stored" is the same start, stored as upstream
    stores it: computed in double from the float32 activated values and rounded once."""
    g = sc["s"]["g"]
    P = len(g.xyz)
    out = dict(means3D=g.xyz.copy(), shs=g.sh.reshape(P, -1, 3).copy(), opacities=g.opacity.copy(),
               scales=g.scale.copy(), rotations=g.rot.copy())
    if perturbed:
        rng = np.random.default_rng(SEED)
        for k, amp in PERTURB.items():
            d = (amp * rng.standard_normal(out[k].shape)).astype(F32)
            d[BEHIND:] = 0.0
            out[k] = out[k] + d
        out["opacities"] = np.clip(out["opacities"], 0.05, 0.95).astype(F32)
    if parametrisation == "stored":
        o = out["opacities"].astype(np.float64)
        factor = np.random.default_rng(SEED + 1).uniform(*ROTATION_FACTOR, (P, 1))
        out = dict(xyz=out["means3D"], f_dc=out["shs"][:, :1], f_rest=out["shs"][:, 1:],
                   opacity=np.log(o / (1.0 - o)), scaling=np.log(out["scales"].astype(np.float64)),
                   rotation=out["rotations"].astype(np.float64) * factor)
    elif parametrisation != "activated":
        raise ValueError(f"parametrisation must be one of {PARAMETRISATIONS}")
    return {k: np.ascontiguousarray(v, F32) for k, v in out.items()}


def activate(p):
    """The tensors of either parametrisation -> the rasterizer's arguments by NAMES.  Torch
    operations only: the same function is the float64 chain's activation, the float32
    restatement's, and the GPU fit's (tests/test_gpu_fit_chain.py)."""
    if "means3D" in p:
        return {k: p[k] for k in NAMES}
    return dict(means3D=p["xyz"], shs=torch.cat([p["f_dc"], p["f_rest"]], dim=1),
                opacities=torch.sigmoid(p["opacity"]), scales=torch.exp(p["scaling"]),
                rotations=torch.nn.functional.normalize(p["rotation"]))


def activated32(params):
    """The float32 arrays the rasterizer gets for float32 parameters (arrays or tensors)."""
    t = {k: (v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(torch.float32)
         for k, v in params.items()}
    return {k: np.ascontiguousarray(v.numpy(), F32) for k, v in activate(t).items()}


def _oracle_lists(sc, params):
    import oracle
    s = sc["s"]
    f = {k: np.ascontiguousarray(v, F32) for k, v in params.items()}
    P = len(f["means3D"])
    return oracle.forward(f["means3D"], f["opacities"], s["view"], s["proj"], s["campos"], s["tx"],
                          s["ty"], s["W"], s["H"], shs=f["shs"].reshape(P, -1), sh_degree=s["sh_degree"],
                          scales=f["scales"], rotations=f["rotations"],
                          scale_modifier=s["scale_modifier"], bg=s["bg"])


def oracle_lists(sc, params):
    """The CPU oracle's integer decisions for float32 parameters of either parametrisation ->
    ((ranges, point_list), radii)."""
    orc = _oracle_lists(sc, activated32(params))
    return (orc["ranges"], orc["point_list"]), np.asarray(orc["radii"])


def render64(sc, params, orc=None):
    """The float64 restatement's image of `params` (tensors or arrays) -> (color, radii)."""
    s = sc["s"]
    cam = gr.camera_constants(s)
    t = {k: v if torch.is_tensor(v) else torch.tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    if orc is None:
        orc = _oracle_lists(sc, {k: v.detach().numpy() for k, v in t.items()})
    zero = torch.zeros((len(t["means3D"]), 3), dtype=torch.float64)
    m2, conic, rgb, _, _ = gr.project(cam, orc["radii"], t["means3D"], zero, t["scales"],
                                      t["rotations"], None, t["shs"], None)
    color, _, _ = gr.composite((orc["ranges"], orc["point_list"]), m2, conic, t["opacities"], rgb,
                               s["bg"], cam["W"], cam["H"])
    return color, np.asarray(orc["radii"])


# ---- the chain: parameters -> activation -> project -> composite, differentiable -------------------
def chain(sc, params, lists, radii, dtype=torch.float64, gates=None):
    """The image of the parameters of either parametrisation (arrays become leaves of `dtype`,
    tensors are taken as they are) over given lists and radii, with a zero means2D leaf.
    gates: (project gates, composite gates) of a float64 run.
    -> dict(color (with its graph), leaves (the groups and "means2D"), near, gates)."""
    s = sc["s"]
    cam = gr.camera_constants(s)
    leaves = {k: v if torch.is_tensor(v) else
              torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True)
              for k, v in params.items()}
    P = len(next(iter(leaves.values())))
    leaves["means2D"] = torch.zeros((P, 3), dtype=dtype, requires_grad=True)
    a = activate(leaves)
    gp, gc = gates if gates is not None else (None, None)
    m2, conic, rgb, gates_p, near_p = gr.project(cam, radii, a["means3D"], leaves["means2D"],
                                                 a["scales"], a["rotations"], None, a["shs"], None,
                                                 gp)
    color, gates_c, near_c = gr.composite(lists, m2, conic, a["opacities"], rgb, s["bg"], cam["W"],
                                          cam["H"], gc)
    return dict(color=color, leaves=leaves, near=(near_p, near_c), gates=(gates_p, gates_c))


def chain_gradients(ch, dL, retain_graph=False):
    """J^T dL of a chain() result -> name -> float64 array, "means2D" (in upstream's units: the
    offset is added in NDC) among them."""
    color, names = ch["color"], list(ch["leaves"])
    out = (color * torch.as_tensor(np.asarray(dL, np.float64)).to(color.dtype)).sum()
    grads = torch.autograd.grad(out, [ch["leaves"][k] for k in names], retain_graph=retain_graph,
                                allow_unused=True)
    return {k: (torch.zeros_like(ch["leaves"][k]) if g is None else g).detach().double().numpy()
            for k, g in zip(names, grads)}


def loss_gradient(image, target, dtype=torch.float64):
    """(loss, dL_dimage) of loss_reference in `dtype` at float32 images."""
    ev = L.evaluate(np.asarray(image, F32), np.asarray(target, F32), LAMBDA, dtype)
    return ev["loss"], ev["dL_dimage"]


_TARGET = {}


def target64():
    """The float64 render of the unperturbed scene (computed once, read-only)."""
    if "t" not in _TARGET:
        sc = scene()
        _TARGET["t"] = render64(sc, parameters(sc, False))[0].detach()
    return _TARGET["t"]


# ---- the reference fit -------------------------------------------------------------------------------
def _adam(p, m, v2, names, lrs, rows):
    with torch.no_grad():
        for k in names:
            g = p[k].grad
            sel = rows.reshape((-1,) + (1,) * (g.dim() - 1))
            m1 = BETAS[0] * m[k] + (1.0 - BETAS[0]) * g
            v1 = BETAS[1] * v2[k] + (1.0 - BETAS[1]) * g * g
            p1 = p[k] - lrs[k] * (m1 / (v1.sqrt() + EPS))
            m[k], v2[k] = torch.where(sel, m1, m[k]), torch.where(sel, v1, v2[k])
            p[k].copy_(torch.where(sel, p1, p[k]))


def densify_thresholds(parametrisation, control=None):
    """((grad, scale split, opacity prune, scale prune), radius) in the stored space, and whether
    that space is log space.  control: another fit's thresholds (default CONTROL's)."""
    from gaussiansplattingviewer_amd import densify
    activated = parametrisation == "activated"
    thresholds, radius = densify.stored_thresholds(activated=activated,
                                                   **(control or CONTROL[parametrisation]))
    return thresholds, radius, not activated


def _densify(parametrisation, p, m, v2, stats, control=None, seed=None):
    """tests/densify_reference.py on the float32 roundings of the fit's state -> the new state in
    the fit's dtype, and the counts.  control, seed: another fit's (default CONTROL's and
    DENSIFY_SEED)."""
    names = GROUPS[parametrisation]
    role_of = {v: k for k, v in ROLES[parametrisation].items()}
    f32 = lambda t: np.ascontiguousarray(t.detach().to(torch.float32).numpy())  # noqa: E731
    groups = [dict(name=k, role=role_of.get(k), p=f32(p[k]), m=f32(m[k]), v=f32(v2[k]))
              for k in names]
    thresholds, radius, log_space = densify_thresholds(parametrisation, control)
    before = dict(accum=stats[0].astype(F32), denom=stats[1].astype(F32), max_radii=stats[2].copy(),
                  scaling=groups[names.index(ROLES[parametrisation]["scaling"])]["p"].copy(),
                  opacity=groups[names.index(ROLES[parametrisation]["opacity"])]["p"].copy())
    r = D.densify(groups, before["accum"], before["denom"], before["max_radii"], thresholds, radius,
                  log_space, DENSIFY_SEED if seed is None else seed)
    dt = p[names[0]].dtype
    new = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dt)  # noqa: E731
    p1 = {k: new(g["p"]).requires_grad_(True) for k, g in zip(names, r["groups"])}
    m1 = {k: new(g["m"]) for k, g in zip(names, r["groups"])}
    v1 = {k: new(g["v"]) for k, g in zip(names, r["groups"])}
    return p1, m1, v1, r["counts"], before


def _fit(parametrisation, dtype, iterations, densify_after=None, checkpoints=(), final=False):
    sc = scene()
    names, lrs = GROUPS[parametrisation], GROUP_LRS[parametrisation]
    target = target64().to(dtype)
    p = {k: torch.tensor(v.astype(np.float64), dtype=dtype, requires_grad=True)
         for k, v in parameters(sc, True, parametrisation).items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    P = len(p[names[0]])
    stats = [np.zeros((P, 1)), np.zeros((P, 1)), np.zeros(P, np.int32)]
    out = dict(losses=[], radii=[], records={}, counts=None, before_densify=None)
    f32 = lambda d: {k: np.ascontiguousarray(t.detach().to(torch.float32).numpy())  # noqa: E731
                     for k, t in d.items()}
    for it in range(1, iterations + 1 + int(final)):
        lists, radii = oracle_lists(sc, p)
        ch = chain(sc, p, lists, radii, dtype)
        loss = L.loss_values(ch["color"], target, LAMBDA)[0]
        out["losses"].append(float(loss.detach()))
        out["radii"].append(radii)
        if it > iterations:
            break
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
        _adam(p, m, v2, names, lrs, torch.as_tensor(on))
        if it == densify_after:
            p, m, v2, out["counts"], out["before_densify"] = _densify(parametrisation, p, m, v2, stats)
            P = len(p[names[0]])
            stats = [np.zeros((P, 1)), np.zeros((P, 1)), np.zeros(P, np.int32)]
    return out


def reference_fit(steps=STEPS, parametrisation="activated", dtype=torch.float64):
    """The fit without density control -> dict(losses [steps + 1] (the last after the final step),
    radii per iteration).  dtype float32: the same loop in float32 (the restatements at float32,
    Adam in float32, the lists from the oracle at the float32 parameters)."""
    r = _fit(parametrisation, dtype, steps, final=True)
    return dict(losses=r["losses"], radii=r["radii"])


_TRAJECTORY = {}


def trajectory(parametrisation):
    """The float64 fit of ITERATIONS iterations with the densify after DENSIFY_AFTER -> dict(losses
    [ITERATIONS], records (iteration of CANDIDATES -> the state before it, rounded to float32),
    counts, before_densify).  Computed once per parametrisation, read-only."""
    if parametrisation not in _TRAJECTORY:
        _TRAJECTORY[parametrisation] = _fit(parametrisation, torch.float64, ITERATIONS,
                                            DENSIFY_AFTER, CANDIDATES)
    return _TRAJECTORY[parametrisation]


def densify_margins(parametrisation, before=None, control=None):
    """The smallest relative distance of a statistic from its threshold, per test, in linear
    units, on the reference's state before the densify (or a given one of that layout, under
    given thresholds)."""
    b = before or trajectory(parametrisation)["before_densify"]
    ctl = control or CONTROL[parametrisation]
    scaling, opacity = b["scaling"].astype(np.float64), b["opacity"].astype(np.float64).reshape(-1)
    if parametrisation == "stored":
        scaling, opacity = np.exp(scaling), 1.0 / (1.0 + np.exp(-opacity))
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.nan_to_num(b["accum"].reshape(-1).astype(np.float64) / b["denom"].reshape(-1))
    dist = lambda v, thr: float(np.abs(np.asarray(v, np.float64) / thr - 1.0).min())  # noqa: E731
    smax = scaling.max(1)
    return dict(grad=dist(avg, ctl["max_grad"]),
                split=dist(smax, ctl["percent_dense"] * ctl["extent"]),
                opacity=dist(opacity, ctl["min_opacity"]),
                radius=dist(b["max_radii"], ctl["max_screen_size"]),
                world=min(dist(smax, 0.1 * ctl["extent"]), dist(smax / 1.6, 0.1 * ctl["extent"])))


# ---- the constants the GPU tests are held to: measured here, not chosen ------------------------------
# The loss of reference_fit(), float64, before each of the STEPS steps and after the last.
LOSSES = dict(
    activated=(0.07460647847488798, 0.04380503501133834, 0.03290212816858354,
               0.03430742895978656, 0.031694486384562494, 0.024888734761029145,
               0.024976195317797958, 0.02159444300970933, 0.02115713041623319,
               0.020605410518181877, 0.01875467385734408, 0.017051192080101737,
               0.016725432802565974, 0.015668150366175467, 0.014257739572017043,
               0.014576375463932163, 0.012852143702124329, 0.01332229493443966,
               0.011748846281040051, 0.012131922840296855, 0.011023092957485187),
    stored=(0.07460647797826664, 0.04377898036674446, 0.0323924406536123,
            0.034677945043275184, 0.031208021556847355, 0.025409639218047148,
            0.024529188876282755, 0.02192626320485034, 0.0228033820903709,
            0.019622247869886297, 0.01851392257294643, 0.016308155109279132,
            0.015161856015740285, 0.0153645944162848, 0.01348941797059897,
            0.012280555500017751, 0.01254202910376155, 0.011128698097877554,
            0.011353887623536656, 0.010568035849298444, 0.010122815789147244))
# s = max_i |loss32[i] / loss64[i] - 1| over the first STEPS values, loss32 the same fit run in
# float32 (reference_fit(dtype=torch.float32)).  The GPU's free-running sequence is held to
# LOSS_FACTOR x s; test_fit_step_reference.py re-measures s and holds it within a factor 2.
LOSS_SPREAD = dict(activated=1.8e-2, stored=8.5e-3)
LOSS_FACTOR = 8.0

# f of the chain-gradient check: rel_err of the whole backward chain in float32 (`step32`: the
# loss gradient by loss_reference in float32 at the float32 image, pulled back through the
# float32 chain; lists and gates from the float64 run, so only rounding differs) against the float64
# chain with the float64 loss gradient at that same image (`reference_of`) -- what the GPU is
# compared with, a float32 restatement in its place.  The largest over the CANDIDATES of
# trajectory() whose `near` is (0, 0).  The GPU tests allow grad_reference.BOUND_FACTOR x
# max(this, grad_reference.F32_SPREAD of the same tensor): that table was measured with a given
# dL; here the float32 loss gradient's own rounding comes in (loss_reference.F32_SPREAD
# "dL_dimage"), and late in a fit the sums over the pixels cancel harder.
CHAIN_SPREAD = dict(
    activated=dict(means3D=1.8e-5, shs=1.8e-5, opacities=1.6e-5, scales=2.7e-5, rotations=1.4e-5,
                   means2D=1.6e-5),     # the largest at iterations 40, 30, 30, 10, 19, 10
    stored=dict(xyz=2.2e-5, f_dc=1.4e-5, f_rest=1.5e-5, opacity=2.7e-5, scaling=2.1e-5,
                rotation=2.7e-5, means2D=1.5e-5))   # at 40, 22, 22, 10, 19, 40, 19
# f of the joint check, which takes the loss gradient as given: rel_err of the float32 chain's
# pull-back of the float32 loss gradient against the float64 chain's pull-back of THE SAME
# gradient, over the same checkpoints (grad_reference.F32_SPREAD's measurement, with the loss's
# dL).  The loss gradient itself is then held to loss_reference's table.
JOINT_SPREAD = dict(
    activated=dict(means3D=3.1e-6, shs=4.8e-7, opacities=1.0e-6, scales=1.5e-6, rotations=8.4e-7,
                   means2D=4.1e-6),     # the largest at iterations 40, 2, 30, 30, 2, 40
    stored=dict(xyz=7.1e-6, f_dc=1.4e-6, f_rest=1.0e-6, opacity=9.0e-7, scaling=2.2e-6,
                rotation=1.8e-6, means2D=7.5e-6))   # at 22, 22, 22, 21, 40, 30, 22
# the group of a parametrisation -> the key of grad_reference.F32_SPREAD that is the same tensor
SAME_TENSOR = dict(means3D="means3D", means2D="means2D", shs="shs", opacities="opacity",
                   scales="scales", rotations="rotations", xyz="means3D")


def chain_keys(parametrisation):
    return GROUPS[parametrisation] + ("means2D",)


def chain_f(parametrisation, key, table=None):
    """table: JOINT_SPREAD, or another fit's table of either kind (default CHAIN_SPREAD)."""
    f = (CHAIN_SPREAD if table is None else table)[parametrisation][key]
    return max(f, gr.F32_SPREAD[SAME_TENSOR[key]]) if key in SAME_TENSOR else f


def measure_chain_spread(parametrisation, per_iteration=None):
    """(CHAIN_SPREAD[parametrisation], JOINT_SPREAD[parametrisation]) as measured now."""
    sc = scene()
    keys = chain_keys(parametrisation)
    f, fj = {k: 0.0 for k in keys}, {k: 0.0 for k in keys}
    for it, rec in trajectory(parametrisation)["records"].items():
        state = step32(sc, rec, parametrisation)
        ref = reference_of(sc, state, rec["lists"], rec["radii"])
        if ref["near"] != (0, 0):
            continue
        own = {k: gr.rel_err(state["grads"][k], ref["grads"][k]) for k in keys}
        joint = {k: gr.rel_err(state["grads"][k], ref["joint"][k]) for k in keys}
        if per_iteration is not None:
            per_iteration[it] = (own, joint)
        f = {k: max(f[k], own[k]) for k in keys}
        fj = {k: max(fj[k], joint[k]) for k in keys}
    return f, fj


def measure_loss_spread(parametrisation):
    """LOSS_SPREAD[parametrisation] as measured now."""
    l32 = np.array(reference_fit(STEPS, parametrisation, torch.float32)["losses"][:STEPS])
    return float(np.abs(l32 / np.array(LOSSES[parametrisation][:STEPS]) - 1.0).max())


def loss_sequence_error(losses, parametrisation):
    """max_i |losses[i] / LOSSES[i] - 1| over the STEPS iterations before the densify."""
    got = np.asarray(losses, np.float64)[:STEPS]
    assert len(got) == STEPS
    return float(np.abs(got / np.array(LOSSES[parametrisation][:STEPS]) - 1.0).max())


# ---- which checkpoints the chain-gradient check may leave out ----------------------------------------
MAX_LEFT_OUT = 3


def left_out(near_by_iteration):
    """The iterations whose float64 evaluation has a decision within rounding of a gate."""
    return tuple(sorted(it for it, near in near_by_iteration.items() if tuple(near) != (0, 0)))


def cap_holds(skipped):
    """At most 3 of the 10 candidates, never both of 20 and 21, never all of 1, 2 and 3."""
    s = set(skipped)
    return (s <= set(CANDIDATES) and len(s) <= MAX_LEFT_OUT and not {20, 21} <= s
            and not {1, 2, 3} <= s)


# ---- the checks of one teacher-forced iteration ------------------------------------------------------
# A state is what one iteration read and wrote, on the host, float32 unless said:
#   params, params1   group -> array, before and after the step
#   activated         NAMES -> array: what the rasterizer was given
#   color [3, H, W], radii int32 [P], loss (a float32 scalar), target [3, H, W]
#   grads             group -> array, and "means2D" [P, 3]
#   dL [3, H, W]      the loss gradient as it reached the rasterizer's backward (color.grad)
#   m, v, m1, v1      group -> the moments before and after
#   stats, stats1     (grad_accum [P, 1], denom [P, 1], max_radii int32 [P]) before and after
# Every check returns rows (what, error, bound): the check holds where error <= bound.

def failures(rows):
    return [f"{what}: {e:.3e} > {b:.3e}" for what, e, b in rows if not e <= b]


def show(rows, head=""):
    for what, e, b in rows:
        print(f"{head}{what}: error {e:.3e}, bound {b:.3e}" + ("" if e <= b else "  FAILS"))


def reference_of(sc, state, lists, radii):
    """The float64 restatement of the state's iteration: the chain at the state's parameters over
    (lists, radii), and its gradients for the float64 loss gradient AT THE STATE'S OWN IMAGE (so
    sign(image - target) has one argument on both sides).
    -> dict(color, radii, near, grads, loss and dL (float64, of the state's image), joint (the
    same chain's pull-back of the state's own dL))."""
    ch = chain(sc, state["params"], lists, radii)
    loss, dL = loss_gradient(state["color"], state["target"])
    return dict(color=ch["color"].detach().numpy(), radii=np.asarray(radii), near=ch["near"],
                grads=chain_gradients(ch, dL, retain_graph=True), loss=loss, dL=dL,
                joint=chain_gradients(ch, np.asarray(state["dL"], np.float64)))


def check_forward(state, ref):
    """(a): the image by gpu_helpers.assert_image_close (its three figures shown beside their
    bars), the radii equal."""
    import gpu_helpers as gh
    got = np.asarray(state["color"])
    d = np.abs(got.astype(np.float64) - ref["color"])
    rows = [("radii that differ", float((np.asarray(state["radii"]) != ref["radii"]).sum()), 0.0),
            ("color max abs", float(d.max()), gh.IMG_MAX),
            (f"color share beyond {gh.IMG_ATOL:g}", float((d > gh.IMG_ATOL).mean()),
             1.0 - gh.IMG_FRAC),
            ("color -PSNR dB", -gh.psnr_db(got, ref["color"]), -gh.IMG_PSNR_DB)]
    try:
        gh.assert_image_close(got, ref["color"])
        rows.append(("assert_image_close", 0.0, 0.0))
    except AssertionError as e:
        print(e)
        rows.append(("assert_image_close", 1.0, 0.0))
    return rows


def check_loss(state, ref):
    """(b): the loss value against loss_reference in float64 of the state's own image and target,
    within the image-loss tests' bound for the value (tests/test_gpu_image_loss.py)."""
    return [("loss", gr.rel_err(float(np.asarray(state["loss"]).reshape(-1)[0]), ref["loss"]),
             L.BOUND_FACTOR * L.F32_SPREAD["loss"][LAMBDA])]


def check_chain(state, ref, parametrisation, table=None):
    """(c): every gradient against J64^T dL64(color of the state), rel_err per tensor within
    BOUND_FACTOR x f (of `table`, default CHAIN_SPREAD)."""
    return [(f"grad {k}", gr.rel_err(np.asarray(state["grads"][k]).reshape(ref["grads"][k].shape),
                                     ref["grads"][k]),
             gr.BOUND_FACTOR * chain_f(parametrisation, k, table))
            for k in chain_keys(parametrisation)]


def check_loss_gradient(state, ref):
    """The image gradient that reached the rasterizer against loss_reference's in float64 at the
    state's own image, within the image-loss tests' bound for it."""
    return [("dL_dimage", gr.rel_err(state["dL"], ref["dL"]),
             L.BOUND_FACTOR * L.F32_SPREAD["dL_dimage"][LAMBDA])]


def check_joint(state, ref, parametrisation, table=None):
    """Every gradient against J64^T (the state's own dL): the rasterizer's backward and the
    activations as they received the loss gradient, within BOUND_FACTOR x the spread measured
    with one dL on both sides -- several times tighter than check_chain, whose bound has to
    admit the float32 loss gradient's rounding."""
    return [(f"joint {k}", gr.rel_err(np.asarray(state["grads"][k]).reshape(ref["joint"][k].shape),
                                      ref["joint"][k]),
             gr.BOUND_FACTOR * chain_f(parametrisation, k, table or JOINT_SPREAD))
            for k in chain_keys(parametrisation)]


def _words(a, b):
    """How many 32-bit words differ."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return float("inf")
    return float((a.view(np.uint32) != b.view(np.uint32)).sum())


def check_adam(state, parametrisation, lrs=None):
    """(d): parameters and both moments after the step are optimizer_reference.adam_step of the
    state's own parameters, moments and gradients, rows by radii > 0, bit for bit.  lrs: another
    fit's learning rates by group (default GROUP_LRS's)."""
    lrs = lrs or GROUP_LRS[parametrisation]
    rows_on = O.row_mask(len(state["radii"]), radii=state["radii"])
    rows = []
    for k in GROUPS[parametrisation]:
        g = np.asarray(state["grads"][k], F32).reshape(state["params"][k].shape)
        p1, m1, v1 = O.adam_step(state["params"][k], g, state["m"][k], state["v"][k],
                                 lrs[k], EPS, BETAS[0], BETAS[1], rows=rows_on)
        rows += [(f"adam param {k}", _words(state["params1"][k], p1), 0.0),
                 (f"adam exp_avg {k}", _words(state["m1"][k], m1), 0.0),
                 (f"adam exp_avg_sq {k}", _words(state["v1"][k], v1), 0.0)]
        off = ~rows_on
        same = sum(_words(state[a][k][off], state[b][k][off])
                   for a, b in (("params1", "params"), ("m1", "m"), ("v1", "v")))
        rows.append((f"adam unseen rows {k}", same, 0.0))
    return rows


def check_stats(state):
    """(e): the three statistics after the step are optimizer_reference.densify_stats of the
    state's own values and means2D gradient, bit for bit."""
    a1, d1, r1 = O.densify_stats(state["radii"], np.asarray(state["grads"]["means2D"], F32),
                                 *state["stats"])
    return [("grad_accum", _words(state["stats1"][0], a1), 0.0),
            ("denom", _words(state["stats1"][1], d1), 0.0),
            ("max_radii", _words(state["stats1"][2], r1), 0.0)]


def check_all(sc, state, parametrisation, lists, radii, ref=None, tables=(None, None), lrs=None):
    """-> (check name -> rows, ref); "chain" and "joint" are None where the reference is near a
    gate.  tables, lrs: another fit's (chain spread, joint spread) and learning rates."""
    ref = ref or reference_of(sc, state, lists, radii)
    clear = ref["near"] == (0, 0)
    return dict(forward=check_forward(state, ref), loss=check_loss(state, ref),
                loss_gradient=check_loss_gradient(state, ref),
                chain=check_chain(state, ref, parametrisation, tables[0]) if clear else None,
                joint=check_joint(state, ref, parametrisation, tables[1]) if clear else None,
                adam=check_adam(state, parametrisation, lrs), stats=check_stats(state)), ref


# ---- a float32 restatement of one iteration, and its mutants -----------------------------------------
# mutant -> the check that must reject it
MUTANTS = {"loss gradient without D-SSIM": "chain", "loss gradient times 2": "chain",
           "means2D.grad in pixels": "chain", "learning rates swapped": "adam",
           "mask radii >= 0": "stats", "moments swapped": "adam",
           "shs gradient transposed": "chain", "denom for every row": "stats"}


def step32(sc, rec, parametrisation, mutant=None):
    """One iteration from a trajectory() record in float32 (grad_reference and loss_reference at
    float32, numpy float32 Adam and statistics), as a state; with `mutant`, a wrong one."""
    assert mutant is None or mutant in MUTANTS
    names = GROUPS[parametrisation]
    target = target64().numpy().astype(F32)
    lists, radii = rec["lists"], np.asarray(rec["radii"], np.int32)
    r64 = chain(sc, rec["params"], lists, radii)
    ch = chain(sc, rec["params"], lists, radii, torch.float32, r64["gates"])
    color = np.ascontiguousarray(ch["color"].detach().numpy(), F32)
    loss, dL = loss_gradient(color, target, torch.float32)
    if mutant == "loss gradient without D-SSIM":
        dL = ((1.0 - LAMBDA) / color.size * np.sign(color - target)).astype(F32)
    if mutant == "loss gradient times 2":
        dL = 2.0 * dL
    dL = np.ascontiguousarray(dL, F32)
    grads = {k: v.astype(F32) for k, v in chain_gradients(ch, dL).items()}
    if mutant == "means2D.grad in pixels":
        W, H = color.shape[2], color.shape[1]
        grads["means2D"] = (grads["means2D"] / np.array([0.5 * W, 0.5 * H, 1.0])).astype(F32)
    if mutant == "shs gradient transposed":
        k = "shs" if parametrisation == "activated" else "f_rest"
        g = grads[k]
        grads[k] = np.ascontiguousarray(g.transpose(0, 2, 1)).reshape(g.shape)
    lrs = dict(GROUP_LRS[parametrisation])
    if mutant == "learning rates swapped":
        lrs[names[0]], lrs[names[1]] = lrs[names[1]], lrs[names[0]]
    mask = radii >= 0 if mutant == "mask radii >= 0" else radii > 0
    state = dict(params=rec["params"], activated=activated32(rec["params"]), color=color,
                 radii=radii, loss=F32(loss), target=target, grads=grads, dL=dL, m=rec["m"],
                 v=rec["v"], stats=rec["stats"], params1={}, m1={}, v1={})
    for k in names:
        m0, v0 = rec["m"][k], rec["v"][k]
        if mutant == "moments swapped":
            m0, v0 = v0, m0
        p1, m1, v1 = O.adam_step(rec["params"][k], grads[k], m0, v0, lrs[k], EPS, BETAS[0],
                                 BETAS[1], rows=mask)
        if mutant == "moments swapped":
            m1, v1 = v1, m1
        state["params1"][k], state["m1"][k], state["v1"][k] = p1, m1, v1
    seen = np.where(mask, np.maximum(radii, 1), 0)  # densify_stats tests radii > 0
    a1, d1, _ = O.densify_stats(seen, grads["means2D"], rec["stats"][0], rec["stats"][1])
    _, _, r1 = O.densify_stats(radii, grads["means2D"], *rec["stats"])
    if mutant == "denom for every row":
        d1 = (rec["stats"][1] + F32(1.0)).astype(F32)
    state["stats1"] = (a1, d1, r1)
    return state
