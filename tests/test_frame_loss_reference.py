"""CPU: the windowed construction of tests/frame_loss_reference.py, in float64, against the
frame's own values (loss_reference, not edited):

   1 over a partition of the frame's rows the ranks' shares add up to `loss_values` of the frame
     within 1e-12, and every rank's gradient rows equal `manual_gradient`'s rows within 1e-12 --
     each rank reading only its band (own rows +- 10);
   2 the saved partials on the apron are the frame's;
   3 mutants: the same construction with a 9-row halo, or with a 5-row halo, misses the gradient on
     the rows next to a seam by far more than that (the shares, which read +- 5 only, survive);
   4 the GPU tests' windows partition their frames and their bands cover what the ABI asks for.
"""
import numpy as np
import pytest

import frame_loss_reference as R
import loss_reference as L

TOL = 1e-12
# What a mutant must miss by.  One missing row enters the gradient through the outer tap of the
# partials' window and the outer tap of the gradient's: g[0]^2 ~ 1e-6 of a typical gradient
# (~ 1e-4 at these sizes), some 1e-10 -- far above float64's rounding of it, 100 x TOL at least.
MISSED = 100 * TOL
# (shape, cuts): strips of 16, 16, 8 rows; arbitrary cuts; a 1-row window; one strip; a frame
# smaller than the window cut in two
CASES = [((3, 40, 70), (16, 32)), ((2, 48, 130), (7, 23)), ((3, 33, 129), (1,)),
         ((1, 11, 5), ()), ((1, 11, 5), (4,))]
IDS = ["x".join(map(str, s)) + "-" + "_".join(map(str, c)) for s, c in CASES]


def _frame(shape, lam, gl):
    x, y = R.as_f64(L.random_pair(shape, 7300))
    return x, y, R.frame_outputs(x, y, lam, gl)


def _errors(shape, cuts, lam, gl, halo):
    """(share errors of loss, l1, ssim; the largest gradient error; the largest saved error)."""
    x, y, frame = _frame(shape, lam, gl)
    H = shape[1]
    ranks = [(own, R.rank_outputs(x, y, own, lam, gl, halo)) for own in R.partition(H, cuts)]
    shares = [abs(sum(out[k] for _, out in ranks) - frame[k]) for k in ("loss", "l1", "ssim")]
    grad = max(float(np.abs(out["dL_dimage"] - frame["dL_dimage"][:, own[0]:own[1]]).max())
               for own, out in ranks)
    saved = 0.0
    for own, out in ranks:
        a0, a1 = R.apron_of(own, H)
        scale = np.abs(frame["saved"]).max()
        saved = max(saved, float(np.abs(out["saved"] - frame["saved"][:, :, a0:a1]).max() / scale))
    return shares, grad, saved


@pytest.mark.parametrize("shape,cuts", CASES, ids=IDS)
def test_shares_and_gradients_of_a_partition(shape, cuts):
    for lam in L.LAMBDAS:
        for gl in (1.0, 0.75):
            shares, grad, saved = _errors(shape, cuts, lam, gl, R.HALO_ROWS)
            print(f"{shape} {cuts} lambda {lam} gl {gl}: shares {shares}, grad {grad:.3g}, "
                  f"saved {saved:.3g}")
            assert max(shares) <= TOL and grad <= TOL and saved <= TOL


@pytest.mark.parametrize("halo", [9, 5])
def test_short_halo_mutants_fail(halo):
    """A rank with `halo` rows of its neighbours pads a seam within the gradient's reach."""
    shape, cuts = CASES[0]
    shares, grad, _ = _errors(shape, cuts, 0.2, 1.0, halo)
    full = _errors(shape, cuts, 0.2, 1.0, R.HALO_ROWS)[1]
    typical = float(np.abs(_frame(shape, 0.2, 1.0)[2]["dL_dimage"]).mean())
    print(f"halo {halo}: gradient error {grad:.3g} (typical |gradient| {typical:.3g}), "
          f"full halo {full:.3g}")
    assert full <= TOL
    assert grad > MISSED, "the mutant went unnoticed"
    assert max(shares) <= TOL  # the map reads +- 5 rows only: the shares cannot tell


def test_mutant_errors_sit_on_the_seam_rows():
    shape = CASES[0][0]
    x, y, frame = _frame(shape, 0.2, 1.0)
    own = (12, 26)  # a seam on both sides, each more than 9 rows from the frame's edge
    got = R.rank_outputs(x, y, own, 0.2, 1.0, halo=9)["dL_dimage"]
    err = np.abs(got - frame["dL_dimage"][:, own[0]:own[1]]).max(axis=(0, 2))
    assert err[0] > MISSED and err[-1] > MISSED
    assert err[1:-1].max() <= TOL  # one missing row reaches one own row on each side


def test_gpu_windows_are_partitions_with_sufficient_bands():
    for (C, H, W), windows in R.WINDOW_CASES.items():
        owns = sorted(own for _, _, own in windows)
        assert owns[0][0] == 0 and owns[-1][1] == H
        assert all(a[1] == b[0] for a, b in zip(owns, owns[1:]))
        for row0, rows, own in windows:
            lo, hi = R.band_of(own, H)
            assert 0 <= row0 <= lo and hi <= row0 + rows <= H
    strips = R.WINDOW_CASES[(3, 40, 70)]
    assert [own for _, _, own in strips] == [(0, 16), (16, 32), (32, 40)]
    assert R.share_sum_bound(2.0, 1e-7, 3) == pytest.approx(2.0 * (8e-7 + 3 * 2.0 ** -24))
