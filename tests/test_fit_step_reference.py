"""CPU: the float64 restatement of the small fit (tests/fit_step_reference.py) does what
tests/test_gpu_fit_step.py, tests/test_gpu_fit_densify.py and tests/test_gpu_fit_chain.py rely on:
its loss at least halves in the chosen number of steps in either parametrisation, one Gaussian is
never seen and one is large on the screen; the constants the GPU tests are held to (the loss
sequences, their float32 spread s, the chain-gradient spread tables) are what it gives here; the
densify thresholds of the stored parametrisation keep their margins; no checkpoint of its own
trajectory lies near a gate; and the checks of a teacher-forced iteration accept a float32
restatement of the iteration and reject every mutant of it."""
import numpy as np
import pytest

import fit_step_reference as fr


def test_reference_fit_halves_its_loss():
    _halves("activated")


def test_stored_reference_fit_halves_its_loss():
    _halves("stored")


def _halves(parametrisation):
    ref = fr.reference_fit(parametrisation=parametrisation)
    losses, radii = ref["losses"], np.stack(ref["radii"])
    ratio = losses[-1] / losses[0]
    print(f"float64 fit, {parametrisation}: loss {losses[0]:.5f} -> {losses[-1]:.5f} in "
          f"{fr.STEPS} steps, ratio {ratio:.3f}")
    assert len(losses) == fr.STEPS + 1 and ratio <= 0.5
    assert (radii[:, fr.BEHIND] == 0).all()
    assert (radii[:, fr.LARGE] > fr.MIN_LARGE_RADIUS).all()
    assert (radii[:, :fr.BEHIND] > 0).sum() >= 0.9 * radii[:, :fr.BEHIND].size
    # the constants the GPU's free-running sequence is held to
    np.testing.assert_allclose(losses, fr.LOSSES[parametrisation], rtol=1e-12, atol=0.0)
    # ... and the trajectory with density control starts with the same twenty
    np.testing.assert_allclose(fr.trajectory(parametrisation)["losses"][:fr.STEPS],
                               fr.LOSSES[parametrisation][:fr.STEPS], rtol=1e-12, atol=0.0)


def test_start_is_a_perturbation_of_the_target():
    sc = fr.scene()
    a, b = fr.parameters(sc, False), fr.parameters(sc, True)
    assert set(a) == set(fr.NAMES) and len(a["means3D"]) == 98
    for k in fr.NAMES:
        assert a[k].dtype == b[k].dtype == np.float32 and a[k].shape == b[k].shape
        assert (a[k][fr.BEHIND:] == b[k][fr.BEHIND:]).all()
        assert (k in fr.PERTURB) == bool((a[k] != b[k]).any())
    again = fr.parameters(fr.scene(), True)
    assert all((again[k] == b[k]).all() for k in fr.NAMES)


def test_stored_start_is_the_same_start():
    """The six stored groups activate to the activated start (to float32 rounding), with
    quaternions that are not normalised."""
    sc = fr.scene()
    a, st = fr.parameters(sc, True), fr.parameters(sc, True, "stored")
    assert tuple(st) == fr.GROUPS["stored"]
    assert st["f_dc"].shape == (98, 1, 3) and st["f_rest"].shape == (98, 15, 3)
    assert all(v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] for v in st.values())
    norm = np.linalg.norm(st["rotation"], axis=1)
    assert norm.min() >= 0.49 and norm.max() <= 2.01 and (np.abs(norm - 1.0) > 0.05).mean() > 0.8
    back = fr.activated32(st)
    unit = a["rotations"] / np.linalg.norm(a["rotations"], axis=1, keepdims=True)
    for k, want in dict(a, rotations=unit).items():
        assert np.abs(back[k] - want).max() <= 4e-7 * max(1.0, np.abs(want).max()), k
    np.testing.assert_array_equal(back["shs"], a["shs"])


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_densify_thresholds_keep_their_margins(parametrisation):
    """Every statistic of the reference lies at least 10 % from its threshold before the densify,
    and each of the counts is at least 1."""
    tr = fr.trajectory(parametrisation)
    margins = fr.densify_margins(parametrisation)
    n_kept, n_clone, n_split, n_removed = tr["counts"]
    print(f"{parametrisation}: counts {tr['counts']}, margins "
          + ", ".join(f"{k} {v:.3f}" for k, v in margins.items()))
    assert all(v >= fr.MIN_MARGIN for v in margins.values()), margins
    assert n_clone >= 1 and n_split >= 1 and n_removed >= 1
    assert len(tr["losses"]) == fr.ITERATIONS
    assert len(tr["records"][fr.DENSIFY_AFTER + 1]["radii"]) == n_kept + n_clone + 2 * n_split
    assert len(tr["records"][fr.DENSIFY_AFTER]["radii"]) == 98


def test_activated_control_is_the_densify_tests():
    import test_gpu_fit_densify as t
    assert fr.CONTROL["activated"] == t.CONTROL and fr.ROLES["activated"] == t.ROLES
    assert (fr.ITERATIONS, fr.DENSIFY_AFTER, fr.DENSIFY_SEED) == (t.ITERATIONS, t.DENSIFY_AFTER,
                                                                 t.SEED)
    assert fr.trajectory("activated")["counts"] == (9, 4, 79, 10)


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_no_checkpoint_of_the_reference_is_near_a_gate(parametrisation):
    """The start is known here: iteration 1 has no decision within rounding of a gate.  And the
    reference's own trajectory, as a stand-in for the GPU's, leaves at most 1 of the 10 out."""
    sc = fr.scene()
    near = {}
    for it, rec in fr.trajectory(parametrisation)["records"].items():
        near[it] = fr.chain(sc, rec["params"], rec["lists"], rec["radii"])["near"]
    print(f"{parametrisation}: near {near}")
    assert tuple(near) == fr.CANDIDATES
    assert near[1] == (0, 0)
    skipped = fr.left_out(near)
    assert len(skipped) <= 1 and fr.cap_holds(skipped)


def test_cap():
    assert fr.cap_holds(()) and fr.cap_holds((1, 2, 20)) and fr.cap_holds((3, 21, 40))
    assert not fr.cap_holds((1, 2, 3)) and not fr.cap_holds((20, 21))
    assert not fr.cap_holds((1, 10, 19, 30)) and not fr.cap_holds((4,))
    assert fr.left_out({1: (0, 0), 2: (0, 1), 3: (2, 0)}) == (2, 3)


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_chain_spread_constants(parametrisation):
    """CHAIN_SPREAD and JOINT_SPREAD are what a float32 evaluation of the chain gives here, with
    the loss's own gradient, to within a factor 2 either way."""
    for seen, tables in zip(fr.measure_chain_spread(parametrisation),
                            (fr.CHAIN_SPREAD, fr.JOINT_SPREAD)):
        print(parametrisation, {k: f"{v:.3e}" for k, v in seen.items()})
        table = tables[parametrisation]
        assert set(seen) == set(table) == set(fr.chain_keys(parametrisation))
        for k, f in seen.items():
            assert 0.5 * f <= table[k] <= 2.0 * f, (k, f, table[k])
            assert fr.chain_f(parametrisation, k, tables) >= table[k]
            # the joint check, which takes the loss gradient as given, is the tighter one
            assert fr.JOINT_SPREAD[parametrisation][k] < fr.CHAIN_SPREAD[parametrisation][k]


@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_loss_spread_constant(parametrisation):
    """s, the float32 fit's largest relative loss difference from the float64 fit's over the
    twenty iterations, to within a factor 2 either way."""
    s = fr.measure_loss_spread(parametrisation)
    print(f"{parametrisation}: s = {s:.3e} (constant {fr.LOSS_SPREAD[parametrisation]:.1e})")
    assert 0.5 * s <= fr.LOSS_SPREAD[parametrisation] <= 2.0 * s
    # the sequence error of the reference itself is 0, and one iteration off is far beyond 8 s
    assert fr.loss_sequence_error(fr.LOSSES[parametrisation], parametrisation) == 0.0
    shifted = fr.loss_sequence_error(fr.LOSSES[parametrisation][1:], parametrisation)
    assert shifted > fr.LOSS_FACTOR * fr.LOSS_SPREAD[parametrisation]


# ---- the checks have teeth -------------------------------------------------------------------------
_standin = {}


def _state(parametrisation, it, mutant=None):
    """step32 of the reference's record, and the float64 reference of that state (shared by the
    mutants with the same image and loss gradient)."""
    sc = fr.scene()
    rec = fr.trajectory(parametrisation)["records"][it]
    state = fr.step32(sc, rec, parametrisation, mutant)
    key = (parametrisation, it, mutant if mutant and mutant.startswith("loss gradient") else None)
    if key not in _standin:
        _standin[key] = fr.reference_of(sc, state, rec["lists"], rec["radii"])
    return sc, rec, state, _standin[key]


@pytest.mark.parametrize("it", (1, 10))
@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_checks_accept_the_float32_restatement(parametrisation, it):
    sc, rec, state, ref = _state(parametrisation, it)
    checks, _ = fr.check_all(sc, state, parametrisation, rec["lists"], rec["radii"], ref)
    assert set(checks) == {"forward", "loss", "loss_gradient", "chain", "joint", "adam", "stats"}
    for name, rows in checks.items():
        assert rows is not None, f"{name} left out at iteration {it}"
        fr.show(rows, f"{parametrisation} {it} {name}: ")
        assert not fr.failures(rows), (name, fr.failures(rows))


@pytest.mark.parametrize("mutant", sorted(fr.MUTANTS))
@pytest.mark.parametrize("it", (1, 10))
@pytest.mark.parametrize("parametrisation", fr.PARAMETRISATIONS)
def test_checks_reject_the_mutant(parametrisation, it, mutant):
    sc, rec, state, ref = _state(parametrisation, it, mutant)
    checks, _ = fr.check_all(sc, state, parametrisation, rec["lists"], rec["radii"], ref)
    named = fr.MUTANTS[mutant]
    fr.show(checks[named], f"{parametrisation} {it} [{mutant}] {named}: ")
    bad = fr.failures(checks[named])
    assert bad, f"{mutant}: the {named} check passes"
    # the wrong tensor is the one that fails
    expect = {"means2D.grad in pixels": "grad means2D", "denom for every row": "denom",
              "mask radii >= 0": "denom", "moments swapped": "adam exp_avg",
              "learning rates swapped": "adam param",
              "shs gradient transposed": "grad shs" if parametrisation == "activated"
              else "grad f_rest"}.get(mutant)
    if expect:
        assert any(b.startswith(expect) for b in bad), bad
    if named != "chain":  # these gradients are the right ones
        assert not fr.failures(checks["chain"]) and not fr.failures(checks["joint"])
        assert not fr.failures(checks["loss_gradient"])
    elif mutant.startswith("loss gradient"):  # a wrong loss gradient, pulled back correctly
        assert fr.failures(checks["loss_gradient"]) and not fr.failures(checks["joint"])
    else:  # the right loss gradient, pulled back wrongly
        assert not fr.failures(checks["loss_gradient"])
        assert any(b.startswith(expect.replace("grad", "joint")) for b in fr.failures(checks["joint"]))
    if named != "adam" and mutant != "mask radii >= 0":
        assert not fr.failures(checks["adam"])
    if named != "stats":
        assert not fr.failures(checks["stats"])
