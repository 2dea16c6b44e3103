"""CPU: the conditions on the frame-scale scenes of the backward-pass tests (frame_grad_scenes) --
each scene holds what it is named for, the near-gate mask stays within its caps, the mask band is
what a float32 evaluation of alpha gives -- and the float32 spread the GPU tolerance of
test_gpu_backward_frames.py is built from, re-measured.  Everything here comes from the C oracle's
lists and the float64 reference alone."""
import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import grad_reference as gr


def test_frame_holds_what_it_says():
    sc = fs.get("frame")
    orc = fs.oracle_of(sc)
    r = orc["ranges"].astype(np.int64)
    counts = r[:, 1] - r[:, 0]
    assert (sc["W"], sc["H"], len(counts)) == (200, 136, 117)
    assert counts.max() > 256 and (counts > 0).all()
    assert int((orc["radii"] > 0).sum()) > 2048
    big = set(sc["special"]["big"])
    assert len(big) == 4
    assert all(big <= set(orc["point_list"][a:b]) for a, b in r)
    # the wholly-outside quadrants: the right half of the last column, the lower half of the
    # last row
    out = fs.outside_quadrants(sc)
    assert len(out) == 2 * 9 + 2 * 13 - 1
    assert {t for t, _ in out} == {t for t in range(117) if t % 13 == 12 or t // 13 == 8}
    # ... and the tile of the bottom-right corner has a single quadrant inside
    assert sorted(q for t, q in out if t == 116) == [1, 2, 3]


def test_wide_holds_what_it_says():
    sc = fs.get("wide")
    orc = fs.oracle_of(sc)
    r = orc["ranges"].astype(np.int64)
    assert (sc["W"], sc["H"]) == (4112, 24) and (sc["W"] + 15) // 16 == 257 and len(r) == 514
    assert (r[:, 1] > r[:, 0]).all()
    assert len(fs.outside_quadrants(sc)) == 2 * 257


def test_tall_holds_what_it_says():
    """The transpose of wide: 257 tile rows (the per-pair form for its rows), every tile with a
    list, the right column's outer quadrants outside the image, a placement in the first, a
    middle and the last tile row."""
    sc = fs.get("tall")
    orc = fs.oracle_of(sc)
    r = orc["ranges"].astype(np.int64)
    assert (sc["W"], sc["H"]) == (24, 4112) and (sc["H"] + 15) // 16 == 257 and len(r) == 514
    assert (r[:, 1] > r[:, 0]).all()
    out = fs.outside_quadrants(sc)
    assert len(out) == 2 * 257 and {t % 2 for t, _ in out} == {1} and {q for _, q in out} == {1, 3}
    rows = sorted(p[2] for p in fs.PLACEMENTS if p[0] == "tall")
    assert rows[0] == 0 and 0 < rows[1] < 256 and rows[2] == 256
    assert all((16 * tx + 8 * (q & 1) < sc["W"]) for n, tx, _, q in fs.PLACEMENTS if n == "tall")


def test_wall_holds_what_it_says():
    """Where its waves stop, from the float64 contribution masks (fs.stops)."""
    sc = fs.get("wall")
    orc = fs.oracle_of(sc)
    r = orc["ranges"].astype(np.int64)
    assert (sc["W"], sc["H"], len(r)) == (32, 32, 4) and (orc["radii"] > 0).all()
    # the near layer leads every list
    front = set(sc["special"]["front"])
    for a, b in r:
        n = len(front & set(orc["point_list"][a:b]))
        assert n >= 64 and set(orc["point_list"][a:a + n]) <= front
    st = fs.stops(sc)
    assert len(st) == 16
    # a quadrant whose last contributing position lies >= 2 chunks before the end of its list,
    # and whose wave has stopped by then: every pixel terminated
    assert any(q["last"] >= 0 and q["last"] <= q["chunks"] - 3 and q["walked"] <= q["chunks"] - 2
               for q in st.values())
    # ... one whose last contributing position lies in chunk 1 or later, before the last chunk;
    # its wave walks more than one chunk and fewer than all
    assert any(1 <= q["last"] < q["chunks"] - 1 and 1 < q["walked"] < q["chunks"]
               for q in st.values())
    # ... waves stop at differing chunks
    assert len({q["walked"] for q in st.values() if q["walked"] < q["chunks"]}) >= 2
    # ... and one in which terminated pixels and pixels that run to the end coexist
    assert any(q["terminated"] >= 8 and q["running"] >= 8 for q in st.values())
    # many Gaussians are composited by no pixel (hidden by the layer, or too faint); most of the
    # layer is
    comp = fs.composited(sc)
    assert (~comp).sum() >= 100 and comp[sc["special"]["front"]].sum() >= 100


@pytest.mark.parametrize("name", fs.NAMES)
def test_mask_within_its_caps(name):
    """project's near count is 0 (asserted by fs.records); the mask covers at most 10 % of the
    scene's pixels and every quadrant keeps at least half of its pixels inside the image."""
    sc = fs.get(name)
    m = fs.mask(sc)
    ids, n = fs.quadrants(sc)
    inside = np.bincount(ids.ravel(), minlength=n)
    hit = np.bincount(ids.ravel(), m.ravel().astype(np.float64), n)
    print(f"{name}: masked {m.mean():.4f} of the pixels, at most {(hit / inside).max():.4f} of a "
          f"quadrant; near-gate pixels per set of records "
          f"{ {k: int(v[1].sum()) for k, v in fs.decisions(sc).items()} }")
    assert (inside > 0).all()
    assert m.mean() <= fs.MASK_CAP
    assert ((inside - hit) >= fs.QUADRANT_KEEP * inside).all()
    dL, dLp = fs.masked(sc)
    assert (dL[:, m] == 0).all() and (dLp[:, m] == 0).all() and (dL[:, ~m] == sc["dL"][:, ~m]).all()


def test_mask_band_is_the_measured_alpha_spread():
    """ALPHA_F32_SPREAD is what the float32 evaluation gives here, within a factor 2; the band is
    8 x it; grad_reference's own bands are unchanged by the band argument."""
    seen = {name: fs.alpha_spread(fs.get(name)) for name in fs.NAMES}
    print({k: f"{v:.3e}" for k, v in seen.items()})
    f = max(seen.values())
    assert 0.5 * f <= fs.ALPHA_F32_SPREAD <= 2.0 * f
    assert fs.BAND == 8.0 * fs.ALPHA_F32_SPREAD
    sc = fs.get("wall")
    rec = fs.records(sc)["f64"]
    with torch.no_grad():
        a = gr.composite(fs.lists_of(sc), *rec, sc["s"]["bg"], 32, 32)
        b = gr.composite(fs.lists_of(sc), *rec, sc["s"]["bg"], 32, 32, band=fs.BAND)
        c = gr.composite(fs.lists_of(sc), *rec, sc["s"]["bg"], 32, 32, band=1e-5)
    assert len(a) == 3 and len(b) == 4 and a[2] == b[2] == c[2]
    assert torch.equal(a[0], b[0])
    # at today's band the mask is the pixels of today's count: none without a counted pair
    assert (c[3].sum() > 0) == (a[2] > 0) and c[3].sum() <= a[2] and (c[3] <= b[3]).all()
    with pytest.raises(ValueError):
        gr.composite(fs.lists_of(sc), *rec, sc["s"]["bg"], 32, 32, gates=a[1], band=1e-5)


@pytest.mark.parametrize("name,kind", sorted(fs.F32_SPREAD))
def test_float32_spread_constants(name, kind):
    """F32_SPREAD (the GPU tests' yardstick) is what a float32 evaluation of the reference gives
    here -- float32 restatement, float64 gates, masked image gradients -- per scene and loss, each
    constant within a factor 2 either way."""
    sc, table = fs.get(name), fs.F32_SPREAD[(name, kind)]
    seen = {}
    if kind == "local":
        runs = [lambda dt=torch.float64, g=None, p=p: fs.localized_reference(sc, *p[1:], dt, g)
                for p in fs.PLACEMENTS if p[0] == name]
    else:
        runs = [lambda dt=torch.float64, g=None: fs.reference(sc, kind, dt, g)]
    for run in runs:
        r64 = run()
        assert r64["near"][0] == 0
        r32 = run(torch.float32, r64["gates"])
        for k in table:
            if k in r64 and np.abs(r64[k]).max() > 0:
                seen[k] = max(seen.get(k, 0.0), fs.err(r32[k], r64, k))
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(table) - {"colors"}
    for k, f in seen.items():
        assert 0.5 * f <= table[k] <= 2.0 * f, (k, f, table[k])
