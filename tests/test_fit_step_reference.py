"""CPU: the float64 restatement of the small fit (tests/fit_step_reference.py) does what
tests/test_gpu_fit_step.py relies on: its loss at least halves in the chosen number of steps, one
Gaussian is never seen and one is large on the screen."""
import numpy as np

import fit_step_reference as fr


def test_reference_fit_halves_its_loss():
    ref = fr.reference_fit()
    losses, radii = ref["losses"], np.stack(ref["radii"])
    ratio = losses[-1] / losses[0]
    print(f"float64 fit: loss {losses[0]:.5f} -> {losses[-1]:.5f} in {fr.STEPS} steps, "
          f"ratio {ratio:.3f}")
    assert len(losses) == fr.STEPS + 1 and ratio <= 0.5
    assert (radii[:, fr.BEHIND] == 0).all()
    assert (radii[:, fr.LARGE] > fr.MIN_LARGE_RADIUS).all()
    assert (radii[:, :fr.BEHIND] > 0).sum() >= 0.9 * radii[:, :fr.BEHIND].size


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
