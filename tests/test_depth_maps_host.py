"""CPU side of the depth planes (gsr_forward_depth): the ABI addition, the metric
disparity arithmetic, and the float32 oracle meeting on its own the per-pixel assertions the
device's planes face in test_gpu_depth_maps.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.colmap import BASELINE
from gaussiansplattingviewer_amd.stereo import disparity_u16, metric_disparity

import blend_scenes as bs
import depth_scenes as ds
from gpu_helpers import run_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr.h")
f32 = np.float32


def test_abi_declares_the_depth_forward(tmp_path):
    lib = _lib.load_library()
    assert "gsr_forward_depth" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "gsr_forward_depth")
    assert _lib.forward_depth_fn(lib).argtypes[4]._type_ is _lib.GsrDepthOutputs
    src = open(HEADER).read()
    assert re.search(r"#define\s+GSR_ABI_VERSION\s+4\b", src)  # additive: the version stays
    assert lib.gsr_abi_version() == 4 == _lib.ABI_VERSION
    fields = [f for f, _ in _lib.GsrDepthOutputs._fields_]
    assert fields == ["depth_map", "inv_depth_map"]
    probe = tmp_path / "probe.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsr_depth_outputs));']
    lines += [f'printf("{f} %zu\\n", offsetof(gsr_depth_outputs, {f}));' for f in fields]
    lines.append("return 0;}")
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(probe), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {l.split()[0]: int(l.split()[1]) for l in out.split("\n") if l}
    assert got["size"] == ctypes.sizeof(_lib.GsrDepthOutputs)
    for f in fields:
        assert got[f] == getattr(_lib.GsrDepthOutputs, f).offset, f


def test_a_library_without_the_symbol_is_named():
    class Old:  # (a build of ABI 4 from before the addition)
        pass
    with pytest.raises(RuntimeError, match="no gsr_forward_depth"):
        _lib.forward_depth_fn(Old())


def test_metric_disparity_closed_form():
    tanfovx, W = 0.75, 300
    fx = W / (2 * tanfovx)  # 200 px
    z = torch.tensor([[1.0, 2.0, 4.0], [8.0, 0.5, 50.0]])
    # covered share 1 - final_T: dyadic, so that 1 - (1 - w) is w exactly in float32
    w = torch.tensor([[1.0, 0.5, 0.25], [0.75, 0.0, 2.0 ** -10]])
    inv = w / z  # premultiplied: sum of w / z over one surface
    T = 1.0 - w
    d = metric_disparity(inv, T, tanfovx, W)
    assert d.dtype == torch.float32 and d.shape == (2, 3)
    want = fx * abs(BASELINE) / z
    want[1, 1] = 0.0  # final_T == 1: no surface
    torch.testing.assert_close(d, want, rtol=1e-6, atol=0)
    assert d[1, 1] == 0.0
    # the premultiplied map, and another baseline (its sign does not matter)
    torch.testing.assert_close(metric_disparity(inv, T, tanfovx, W, normalise=False),
                               fx * abs(BASELINE) * inv, rtol=1e-6, atol=0)
    torch.testing.assert_close(metric_disparity(inv, T, tanfovx, W, baseline=0.25),
                               metric_disparity(inv, T, tanfovx, W, baseline=-0.25))
    torch.testing.assert_close(metric_disparity(inv, T, tanfovx, W, baseline=0.25)[0, 0],
                               torch.tensor(fx * 0.25))
    # final_T slightly above 1 (rounding) is no surface either; nothing is NaN or inf
    d = metric_disparity(torch.zeros(2), torch.tensor([1.0, 1.0000001]), tanfovx, W)
    assert torch.equal(d, torch.zeros(2))
    # the KITTI encoding of the saved PNG
    enc = disparity_u16(torch.tensor([0.0, 1.0, 100.5 / 256, 255.99, 256.0, 1e9]))
    assert enc.tolist() == [0, 256, 100, 65533, 65535, 65535]


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            sc = ds.build(oracle_mod, name)
            bs.run(oracle_mod, sc)
            cache[name] = sc
        return cache[name]
    return get


def test_depth_range_scene_is_what_it_says(oracle_mod, scenes):
    sc = scenes("depth_range")
    orc = sc["orc"]
    z = orc["depths"][orc["radii"] > 0]
    assert len(z) >= 190 and z.min() < 0.35 and z.max() > 45
    assert orc["ranges"].shape[0] == 8 and (orc["ranges"][:, 1] > orc["ranges"][:, 0] + 64).all()
    # shuffled: list order (depth) is not index order
    assert not (np.diff(orc["depths"]) > 0).all()


@pytest.mark.parametrize("name", ds.NAMES)
def test_oracle_meets_the_plane_assertions(oracle_mod, scenes, name):
    """The oracle's float32 forward with colors_precomp = (f, f, f) and bg = 0, f = z and
    f = float32(1) / z, against render_f64 of the same features."""
    sc = scenes(name)
    orc = sc["orc"]
    ref = ds.reference(oracle_mod, sc, orc)
    for key, f in zip(ds.PLANES, ds.features(orc["depths"], orc["radii"])):
        got = run_oracle(oracle_mod, ds.zero_bg(sc), colors_precomp=ds.triple(f),
                         cov3D_precomp=sc["cov6"])
        np.testing.assert_array_equal(got["point_list"], orc["point_list"])
        ratio = ds.assert_plane_exact(got["color"][0], got["n_contrib"], ref[key],
                                      f"{name} {key}")
        assert ratio <= 1.0
        if orc["num_rendered"] and name != "opacity_edges":
            assert got["color"][0].max() > 0
