"""CPU: the multi-view fit's float64 restatement (tests/multiview_fit_reference.py) is what
tests/test_gpu_fit_multiview.py relies on: the views, the order and the checkpoints meet their
conditions; at both densifies every statistic keeps its margin, each count is at least 1 and the
float32 fit reaches the float64 fit's counts; every view's loss falls from its first visit to its
second; at most one checkpoint of the reference's own trajectory is near a gate; the constants the
GPU is held to are what the reference gives here; and the checks accept the float32 restatement
of every checkpoint and reject eight mutants of it."""
import numpy as np
import pytest
import torch

import fit_step_reference as fr
import multiview_fit_reference as mv

PARS = fr.PARAMETRISATIONS


def test_order_and_checkpoints():
    rng = np.random.default_rng(mv.ORDER_SEED)
    order = np.concatenate([rng.permutation(len(mv.VIEWS)) for _ in range(mv.ITERATIONS // 4)])
    assert mv.ORDER == tuple(int(v) for v in order) and len(mv.ORDER) == mv.ITERATIONS
    a, b = mv.PAIR
    assert b == a + 1 and a % 4 == 0 and mv.view_of(a) == mv.view_of(b)
    assert [it for it in range(1, mv.ITERATIONS) if mv.view_of(it) == mv.view_of(it + 1)] == [a]
    assert [mv.degree(it) for it in (1, 8, 9, 16, 17, 24, 25, 48)] == [0, 0, 1, 1, 2, 2, 3, 3]
    # neither densify falls on a degree change
    assert all(mv.degree(it) == mv.degree(it + 1) for it in mv.DENSIFY_AFTER)
    cps = mv.CHECKPOINTS
    assert 10 <= len(cps) <= 14 and tuple(sorted(set(cps))) == cps
    need = {1, a, b, mv.ITERATIONS}
    for x, y in mv.DEGREE_CHANGES:
        assert mv.degree(y) == mv.degree(x) + 1 and y == x + 1
        need |= {x, y}
    for d in mv.DENSIFY_AFTER:
        need |= {d, d + 1, d + 2}
    assert need <= set(cps)
    seen = np.bincount([mv.view_of(it) for it in cps], minlength=len(mv.VIEWS))
    assert (seen >= 2).all(), seen


def test_views_meet_their_conditions():
    shapes = [(W, H) for W, H, _ in mv.VIEWS]
    eyes = [eye for _, _, eye in mv.VIEWS]
    assert len(set(shapes)) == len(set(eyes)) == 4
    assert any(H > W for W, H in shapes)
    assert any(W % 16 == 1 and H % 16 == 1 for W, H in shapes)
    assert any(W >= 40 and H >= 24 and W * H > 40 * 24 for W, H in shapes)
    start = fr.parameters(fr.scene(), True)
    seen = []
    for view in range(4):
        for D in (0, 3):
            sc = mv.view_scene(view, D)
            lists, radii = fr.oracle_lists(sc, start)
            assert fr.chain(sc, start, lists, radii)["near"] == (0, 0), (view, D)
        seen.append(radii > 0)
    seen = np.stack(seen)
    print("rows seen at the start:", seen.sum(1), "largest radius:", radii.max())
    for view in range(4):
        others = np.delete(seen, view, 0).any(0)
        assert (~seen[view] & others).any(), view
    assert (~seen).sum(1).max() >= 15
    assert not seen[:, fr.BEHIND].any()


@pytest.mark.parametrize("parametrisation", PARS)
def test_densify_thresholds_keep_their_margins(parametrisation):
    tr = mv.trajectory(parametrisation)
    assert tuple(tr["counts"]) == mv.DENSIFY_AFTER
    P = 98
    for it in mv.DENSIFY_AFTER:
        margins = mv.densify_margins(parametrisation, it)
        n_kept, n_clone, n_split, n_removed = tr["counts"][it]
        print(f"{parametrisation} after {it}: counts {tr['counts'][it]}, margins "
              + ", ".join(f"{k} {v:.3f}" for k, v in margins.items()))
        assert all(v >= fr.MIN_MARGIN for v in margins.values()), margins
        assert n_clone >= 1 and n_split >= 1 and n_removed >= 1
        assert n_kept + n_split + n_removed == P
        assert tr["counts"][it] == mv.COUNTS[parametrisation][it]
        size = mv.CONTROL[parametrisation][it]["max_screen_size"]
        assert size != int(size)
        P = n_kept + n_clone + 2 * n_split
        assert len(tr["records"][it + 1]["radii"]) == P
    assert P <= mv.MAX_FINAL_P
    # the float32 restatement of the fit reaches the same counts
    assert mv.fit(parametrisation, torch.float32)["counts"] == tr["counts"]


@pytest.mark.parametrize("parametrisation", PARS)
def test_every_view_progresses(parametrisation):
    losses = mv.trajectory(parametrisation)["losses"]
    for view in range(len(mv.VIEWS)):
        first, second = mv.visits(view)[:2]
        print(f"{parametrisation} view {view}: loss {losses[first - 1]:.4f} at {first}, "
              f"{losses[second - 1]:.4f} at {second}")
        assert second <= mv.STEPS and losses[second - 1] < losses[first - 1]


@pytest.mark.parametrize("parametrisation", PARS)
def test_at_most_one_checkpoint_of_the_reference_is_near_a_gate(parametrisation):
    near = {it: rec["near"] for it, rec in mv.trajectory(parametrisation)["records"].items()}
    print(f"{parametrisation}: near {near}")
    assert tuple(near) == mv.CHECKPOINTS and near[1] == (0, 0)
    skipped = fr.left_out(near)
    assert len(skipped) <= 1 and mv.cap_holds(skipped)


def test_cap():
    assert mv.cap_holds(()) and mv.cap_holds((1, 20, 37)) and mv.cap_holds((8, 17, 25))
    assert not mv.cap_holds((20, 21)) and not mv.cap_holds((36, 37))
    assert not any(mv.cap_holds(pair) for pair in mv.DEGREE_CHANGES)
    assert not mv.cap_holds((1, 8, 16, 22)) and not mv.cap_holds((2,))


@pytest.mark.parametrize("parametrisation", PARS)
def test_loss_constants(parametrisation):
    tr = mv.trajectory(parametrisation)
    np.testing.assert_allclose(tr["losses"][:mv.STEPS], mv.LOSSES[parametrisation], rtol=1e-10)
    s = mv.measure_loss_spread(parametrisation)
    print(f"{parametrisation}: s = {s:.3e} (constant {mv.LOSS_SPREAD[parametrisation]:.1e})")
    assert 0.5 * s <= mv.LOSS_SPREAD[parametrisation] <= 2.0 * s
    assert mv.loss_sequence_error(mv.LOSSES[parametrisation], parametrisation) == 0.0
    shifted = mv.loss_sequence_error(tr["losses"][1:], parametrisation)
    assert shifted > fr.LOSS_FACTOR * mv.LOSS_SPREAD[parametrisation]


@pytest.mark.parametrize("parametrisation", PARS)
def test_chain_spread_constants(parametrisation):
    f, fj, at = mv.measure_chain_spread(parametrisation)
    for seen, table, where in zip((f, fj), (mv.CHAIN_SPREAD, mv.JOINT_SPREAD), at):
        print(parametrisation, {k: f"{v:.3e} at {where[k]}" for k, v in seen.items()})
        assert set(seen) == set(table[parametrisation]) == set(fr.chain_keys(parametrisation))
        for k, v in seen.items():
            assert 0.5 * v <= table[parametrisation][k] <= 2.0 * v, (k, v)
            assert mv.chain_f(parametrisation, k, table) >= table[parametrisation][k]
            assert mv.JOINT_SPREAD[parametrisation][k] < mv.CHAIN_SPREAD[parametrisation][k]


# ---- the checks have teeth -------------------------------------------------------------------------
_cache = {}


def _checked(parametrisation, it, mutant=None):
    """The checks of step32 at the reference's record of `it` -> check name -> rows."""
    key = (parametrisation, it, mutant)
    if key in _cache:
        return _cache[key]
    records = mv.trajectory(parametrisation)["records"]
    rec = records[it]
    stale = None
    if mutant == "second densify on the first's statistics":
        stale = _state(parametrisation, mv.DENSIFY_AFTER[0])["stats1"]
    state = mv.step32(rec, parametrisation, mutant, stale)
    checks, _ = mv.check_all(state, parametrisation, rec["lists"], rec["radii"])
    if it in mv.DENSIFY_AFTER:
        checks["densify"] = mv.check_densify(state, state["densify"], parametrisation)
    _cache[key] = (state, checks)
    return _cache[key]


def _state(parametrisation, it):
    return _checked(parametrisation, it)[0]


@pytest.mark.parametrize("it", mv.CHECKPOINTS)
@pytest.mark.parametrize("parametrisation", PARS)
def test_checks_accept_the_float32_restatement(parametrisation, it):
    _, checks = _checked(parametrisation, it)
    want = {"forward", "loss", "loss_gradient", "chain", "joint", "adam", "stats"}
    assert set(checks) == want | ({"densify"} if it in mv.DENSIFY_AFTER else set())
    for name, rows in checks.items():
        if rows is None:  # near a gate: capped by the test above
            continue
        fr.show(rows, f"{parametrisation} {it} {name}: ")
        assert not fr.failures(rows), (name, fr.failures(rows))


# mutant -> the checkpoint it is shown at: 21 follows another view of another tile-grid width and
# has unseen rows with moments; at 16 the statistics hold larger radii of other views; 8 is one
# iteration before degree 1; 36 is the second densify
MUTANT_AT = {"previous view matrix": 21, "previous tile grid": 21, "previous target": 21,
             "moments of unseen rows decay": 21, "denom for every row": 16,
             "max_radii overwritten": 16, "next degree one iteration early": 8,
             "second densify on the first's statistics": 36}


@pytest.mark.parametrize("mutant", sorted(mv.MUTANTS))
@pytest.mark.parametrize("parametrisation", PARS)
def test_checks_reject_the_mutant(parametrisation, mutant):
    assert set(MUTANT_AT) == set(mv.MUTANTS)
    it = MUTANT_AT[mutant]
    assert mv.view_of(it) != mv.view_of(it - 1)
    _, checks = _checked(parametrisation, it, mutant)
    named = mv.MUTANTS[mutant]
    fr.show(checks[named], f"{parametrisation} {it} [{mutant}] {named}: ")
    bad = fr.failures(checks[named])
    assert bad, f"{mutant}: the {named} check passes"
    expect = {"moments of unseen rows decay": "adam unseen rows", "denom for every row": "denom",
              "max_radii overwritten": "max_radii",
              "second densify on the first's statistics": "densify source_index"}.get(mutant)
    if expect:
        assert any(b.startswith(expect) for b in bad), bad
    quiet = {"forward": (), "loss": ("forward", "joint", "adam", "stats"),
             "adam": ("forward", "loss", "loss_gradient", "chain", "joint", "stats"),
             "stats": ("forward", "loss", "loss_gradient", "chain", "joint", "adam"),
             "densify": ("forward", "loss", "loss_gradient", "chain", "joint", "adam", "stats")}
    for name in quiet[named]:  # the other stages did their work
        assert checks[name] is None or not fr.failures(checks[name]), (name, checks[name])
    if mutant == "previous target":
        assert fr.failures(checks["loss_gradient"])
