"""Scenes for the early exit of the blend's composite loop (csrc/blend.hip kStopPairs): a quadrant
wave leaves its pair loop, and with it its chunk loop, at the first test after its last pixel is
done.  Shared by test_stop_scenes.py (CPU: each scene does what it was built for, and the oracle
alone passes the float64 check) and test_gpu_blend_stop.py.  Built with blend_scenes._splats as
the edge scenes are; one 16x16 tile each, view depths rising with the index, so a splat's list
position (counted from 1) is its index + 1.

  stop_S       positions 1 .. S-2: weak splats far wider than the frame (sigma 250 .. 300 px,
               centres 40 .. 80 px off it), alpha 0.02 .. 0.05 at every pixel, nothing culled;
               positions S-1 and S: opaque wide splats whose alpha clamps to 0.99.  T <= 0.98
               before them and T >= 0.035, so T' >= 3.5e-4 at S-1 (composited) and <= 9.8e-5 at S:
               every pixel terminates at position S, n_contrib = S-1.  70 bright opacity-1 splats
               follow, into the next chunk.  S in STOP_S: the stop before the first test, at, one
               before and one after a test of the 1-, 2-, 4- and 8-pair intervals, at a chunk's last
               pair, in the pad slot's region of an odd count, in the second and third chunks.
  stop_S_cut   stop_S without the splats behind position S (the truncation identity).
  stop_spread  positions 1 .. 40: splats narrow in x (sigma_x 1.8 px, sigma_y 1.8 px, opacity 0.8)
               centred on the first column of quadrant A, between its rows 3 and 4: A's pixels
               terminate one after another (n_contrib 6 in column 0, 8, 15 and 37 in columns 1 .. 3
               of rows 3 and 4) while the wave goes on; positions 41 .. 50 weak wide splats; 51 and 52 the opaque pair
               that finishes every other pixel mid-chunk; then the 70 followers.  The other three
               quadrants terminate at position 52 only.
  stop_never   stop_129's list without the opaque pair, the followers at the weak splats' opacity
               (at opacity 1 they would terminate every pixel themselves): no pixel terminates.
"""
from __future__ import annotations

import numpy as np

import blend_scenes as bs

STOP_S = (3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 32, 33, 34, 63, 64, 65, 66, 67, 80, 129)
N_AFTER = 70
W = H = 16
SPREAD_NARROW, SPREAD_WEAK = 40, 10
SPREAD_STOP = SPREAD_NARROW + SPREAD_WEAK + 2  # the opaque pair's second splat
NAMES = (tuple(f"stop_{s}" for s in STOP_S) + ("stop_spread", "stop_never"))


def _depth(n):
    """View depths by index, the same for a list and for its head."""
    return 3.5 + np.arange(n) / 256.0


def _wide(rng, n, op_lo, op_hi, colour_lo=0.0):
    """n splats far wider than the frame, centred 40 .. 80 px off its left or right edge (power
    stays clear of 0 in the frame): px, py, cov, opacity, colours."""
    side = rng.random(n) < 0.5
    px = np.where(side, -rng.uniform(40, 80, n), W + rng.uniform(40, 80, n))
    return (px, rng.uniform(-20, H + 20, n), bs._iso(rng.uniform(250, 300, n)),
            rng.uniform(op_lo, op_hi, n), rng.uniform(colour_lo, 1, (n, 3)))


def _opaque_pair(rng):
    """Two splats of opacity 1 and sigma 1500 px, 40 px off the frame: exp(power) > 0.999 at
    every pixel, so alpha is the cap 0.99, and |power| >= 3e-4."""
    return (np.array([-40.0, W + 40.0]), np.array([8.0, 7.0]), bs._iso(np.full(2, 1500.0)),
            np.ones(2), rng.uniform(0.1, 1, (2, 3)))


def _followers(rng, opacity=1.0):
    px, py, cov, _, col = _wide(rng, N_AFTER, 1.0, 1.0, colour_lo=0.5)
    return px, py, cov, np.full(N_AFTER, opacity), col


def _cat(parts):
    return [np.concatenate([p[i] for p in parts]) for i in range(5)]


def _scene(parts, n=None):
    px, py, cov, op, col = _cat(parts)
    n = len(px) if n is None else n
    return bs._splats(W, H, px[:n], py[:n], _depth(len(px))[:n], cov[:n], op[:n], col[:n])


def _weak_hi(n_weak):
    # T before the pair >= 0.035: 0.95^62 = 0.042, (1 - 0.026)^127 = 0.035
    return 0.05 if n_weak <= 62 else 0.026


def build(oracle, name):
    rng = np.random.default_rng(sum(map(ord, name.replace("_cut", ""))))
    if name in ("stop_spread", "stop_never"):
        if name == "stop_never":
            weak = _wide(rng, 127, 0.0225, _weak_hi(127))
            return _scene([weak, _followers(rng, 0.0225)])
        n = SPREAD_NARROW
        narrow = (np.zeros(n), np.full(n, 3.5), np.tile([1.8 ** 2, 0.0, 1.8 ** 2], (n, 1)),
                  np.full(n, 0.8), rng.uniform(0, 1, (n, 3)))
        weak = _wide(rng, SPREAD_WEAK, 0.0225, 0.05)
        return _scene([narrow, weak, _opaque_pair(rng), _followers(rng)])
    S = int(name.split("_")[1])
    weak = _wide(rng, S - 2, 0.0225, _weak_hi(S - 2))
    parts = [weak, _opaque_pair(rng), _followers(rng)]
    return _scene(parts, S if name.endswith("_cut") else None)
