"""CPU side of the median planes (gsr_forward_surface): the float32 restatement of
upstream's composite meets, alone, the accept-set assertions the device's planes face in
test_gpu_median.py; the `layers` scene is what it says; the disparity arithmetic; the ABI
addition; and the capture's refusal without surface_maps."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.colmap import BASELINE
from gaussiansplattingviewer_amd.stereo import StereoCapture, median_disparity

import median_reference as mr
import median_scenes as ms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr.h")


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    return ms.scene_cache(oracle_mod)


@pytest.mark.parametrize("name", ms.NAMES)
def test_float32_restatement_meets_the_accept_sets(oracle_mod, scenes, name):
    sc = scenes(name)
    orc = sc["orc"]
    ref = mr.reference(oracle_mod, sc, orc)
    mr.assert_scene_decides(ref, name)
    f32 = mr.walk(orc, sc["W"], sc["H"], np.float32)
    # the restatement is the oracle's composite (numpy's float32 exp in place of expf)
    st = ref["stable"]
    assert (f32["n_contrib"] == orc["n_contrib"])[st].all()
    assert np.abs(f32["final_T"].astype(np.float64) - orc["final_T"])[st].max(initial=0) <= 1e-5
    ids = f32["median_id"].astype(np.int32)
    depth = np.where(ids >= 0, orc["depths"][np.maximum(ids, 0)], np.float32(0)).astype(np.float32)
    mr.assert_median_accepted(ref, sc, ids, depth, orc["depths"], f"{name} float32")
    # a median is a composited splat in front of the last contributor; none where T stays high
    pos = f32["median_pos"]
    assert (pos < f32["n_contrib"].astype(np.int64)).all()
    assert ((pos >= 0) == (f32["final_T"] <= np.float32(0.5))).all()


def test_accept_sets_reject_a_wrong_answer(oracle_mod, scenes):
    """The check has teeth: the splat after the median, the first splat of the list and -1 are
    refused on `layers`."""
    sc = scenes("layers")
    orc = sc["orc"]
    ref = mr.reference(oracle_mod, sc, orc)
    good = ref["median_id"].astype(np.int32)
    mr.assert_median_accepted(ref, sc, good, None, orc["depths"], "layers float64")
    for wrong in (np.full_like(good, -1), np.roll(good, 7, axis=1)):
        with pytest.raises(AssertionError, match="outside the accept set"):
            mr.assert_median_accepted(ref, sc, wrong, None, orc["depths"], "layers wrong")
    bad_depth = np.where(good >= 0, orc["depths"][np.maximum(good, 0)], 0).astype(np.float32)
    bad_depth[3, 5] = np.nextafter(bad_depth[3, 5], np.float32(100))
    with pytest.raises(AssertionError, match="not depths"):
        mr.assert_median_accepted(ref, sc, good, bad_depth, orc["depths"], "layers wrong depth")


def test_layers_scene_is_what_it_says(oracle_mod, scenes):
    sc = scenes("layers")
    orc = sc["orc"]
    ref = mr.reference(oracle_mod, sc, orc)
    assert (ref["final_T"] <= 1e-3).all() and (ref["median_id"] >= 0).all()  # the wall closes it
    z = orc["depths"][ref["median_id"]].astype(np.float64)
    assert not ms.in_gaps(z).any()
    share = [float(((z > lo) & (z <= hi)).mean())
             for lo, hi in zip((0.0,) + ms.LAYER_EDGES, ms.LAYER_EDGES + (np.inf,))]
    distinct = len(np.unique(ref["median_id"]))
    ez = mr.expected_depth(ref, sc, orc["depths"])
    mixed = float(ms.in_gaps(ez).mean())
    print(f"layers: medians in foreground / veil / wall {share}, {distinct} distinct ids; "
          f"expected depth between the layers at {mixed:.3f} of the pixels")
    assert min(share) > 0.1 and distinct >= 30
    assert mixed > 0.5


def test_median_disparity_closed_form():
    tanfovx, W = 0.75, 300
    fx = W / (2 * tanfovx)  # 200 px
    z = torch.tensor([[1.0, 2.0, 4.0], [0.0, 0.3, 50.0]])
    d = median_disparity(z, tanfovx, W)
    assert d.dtype == torch.float32 and d.shape == (2, 3)
    scale = np.float32(fx * abs(BASELINE))
    want = np.float32(scale) / np.where(z.numpy() > 0, z.numpy(), np.float32(1))
    want[1, 0] = 0.0  # no surface
    assert np.array_equal(d.numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert torch.equal(median_disparity(z, tanfovx, W, baseline=0.25),
                       median_disparity(z, tanfovx, W, baseline=-0.25))
    assert median_disparity(z, tanfovx, W, baseline=0.25)[0, 0] == fx * 0.25
    # nothing negative, NaN or inf from the no-surface value or a stray negative
    d = median_disparity(torch.tensor([0.0, -1.0, float("nan")]), tanfovx, W)
    assert torch.equal(d, torch.zeros(3))


def test_abi_declares_the_surface_forward(tmp_path):
    lib = _lib.load_library()
    assert "gsr_forward_surface" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "gsr_forward_surface")
    fn = _lib.forward_surface_fn(lib)
    assert fn.argtypes[4]._type_ is _lib.GsrDepthOutputs
    assert fn.argtypes[5]._type_ is _lib.GsrSurfaceOutputs and len(fn.argtypes) == 7
    src = open(HEADER).read()
    assert re.search(r"#define\s+GSR_ABI_VERSION\s+4\b", src)  # additive: the version stays
    assert lib.gsr_abi_version() == 4 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+gsr_forward_surface\s*\(\s*gsr_context\s*\*\s*\w+,\s*const\s+"
                     r"gsr_gaussians\s*\*\s*\w+,\s*const\s+gsr_raster_settings\s*\*\s*\w+,\s*"
                     r"gsr_outputs\s*\*\s*\w+,\s*const\s+gsr_depth_outputs\s*\*\s*\w+,\s*const\s+"
                     r"gsr_surface_outputs\s*\*\s*\w+,\s*void\s*\*\s*\w+\s*\)", code)
    fields = [f for f, _ in _lib.GsrSurfaceOutputs._fields_]
    assert fields == ["median_depth", "median_id"]
    probe = tmp_path / "probe.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsr_surface_outputs));',
             'printf("depth_size %zu\\n", sizeof(gsr_depth_outputs));',
             'printf("outputs_size %zu\\n", sizeof(gsr_outputs));']
    lines += [f'printf("{f} %zu\\n", offsetof(gsr_surface_outputs, {f}));' for f in fields]
    lines.append("return 0;}")
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(probe), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {l.split()[0]: int(l.split()[1]) for l in out.split("\n") if l}
    assert got["size"] == ctypes.sizeof(_lib.GsrSurfaceOutputs)
    # the existing structs keep their layout
    assert got["depth_size"] == ctypes.sizeof(_lib.GsrDepthOutputs)
    assert got["outputs_size"] == ctypes.sizeof(_lib.GsrOutputs)
    for f in fields:
        assert got[f] == getattr(_lib.GsrSurfaceOutputs, f).offset, f


def test_a_library_without_the_symbol_is_named():
    class Old:  # (a build of ABI 4 from before the addition)
        pass
    with pytest.raises(RuntimeError, match="no gsr_forward_surface"):
        _lib.forward_surface_fn(Old())


def test_median_capture_needs_surface_maps():
    class Plain:  # a renderer constructed without the keyword (depth_maps alone is not enough)
        depth_maps = True
        surface_maps = False
    with pytest.raises(RuntimeError, match="surface_maps=True"):
        StereoCapture(Plain(), None, disparity="median")
    assert "median" in StereoCapture.DISPARITIES
    with pytest.raises(ValueError, match="disparity must be one of"):
        StereoCapture(Plain(), None, disparity="mode")
    Plain.surface_maps = True
    assert StereoCapture(Plain(), None, disparity="median").disparity == "median"
