"""GPU: save_ply from device tensors (k_ply_pack, the two staging slots) and load_scene_ply onto
the device (k_ply_unpack and the host conversion's upload), csrc/ply_writer.hip.

Every comparison is bit for bit.  The device path's file is held to the host path's file of the
same scene, which tests/test_ply_scene_host.py holds to the specification (and it is compared with
the specification's bytes here as well).  Row counts on both sides of kPackRows = 64 and of the
256-thread blocks, chunks of 256 and 100 rows (P = 1000: several chunks, a partial last one, both
slots reused).  k_ply_pack takes no row offset: the host adds a chunk's first row to the pointers,
so no index in it exceeds a chunk; there is no large-index case."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fit_step_reference as fr
import ply_oracle
import ply_scene_reference as ref
from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer,
                                         SparseGaussianAdam, _lib, densification_stats,
                                         load_scene_ply, photometric_loss, ply, save_ply,
                                         scene_from_point_cloud)
from gpu_helpers import to_dev

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 255, 256, 257, 1000]
COEFFS = [1, 4, 16]
GUARD = 0x5EEDBEEF  # a NaN-free word no scene holds
DIRT = 0x7FBADBAD


def _words(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a, gpu):
    return torch.from_numpy(a.copy()).to(gpu)  # (the cached scenes are read-only arrays)


def _guarded(shape, gpu, fill):
    """(buffer, view): a contiguous float32 view of `shape` that starts 4-byte aligned but not
    16-byte aligned, 5 guard words in front of it and 7 behind; the view holds `fill` words."""
    n = int(np.prod(shape))
    buf = torch.full((n + 12,), GUARD, dtype=torch.int32, device=gpu).view(torch.float32)
    view = buf[5:5 + n].view(shape)
    if n:
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        view.view(torch.int32).fill_(fill)
    return buf, view


def _guards_hold(buf, n):
    w = _words(buf)
    return bool((w[:5] == GUARD).all() and (w[5 + n:] == GUARD).all())


def _device_scene(sc, gpu):
    """The numpy scene in guarded, unaligned device views: ({name: view}, {name: buffer})."""
    views, bufs = {}, {}
    for k, a in sc.items():
        bufs[k], views[k] = _guarded(a.shape, gpu, 0)
        if a.size:
            views[k].copy_(torch.from_numpy(a.copy()))
    return views, bufs


# ---- 1. the device path's file against the host path's ---------------------------------------------
@pytest.mark.parametrize("chunk_rows", [None, 256, 100])
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("M", COEFFS)
def test_device_file_is_the_host_file(M, P, chunk_rows, gpu, tmp_path):
    sc = ref.scene(P, M)
    save_ply(tmp_path / "host.ply", ref.copies(sc), chunk_rows=chunk_rows)
    dev = {k: _dev(v, gpu) for k, v in sc.items()}
    assert save_ply(tmp_path / "device.ply", dev, chunk_rows=chunk_rows) == P
    got = (tmp_path / "device.ply").read_bytes()
    assert got == (tmp_path / "host.ply").read_bytes()
    assert got == ref.file_bytes(sc)
    for k in sc:
        assert np.array_equal(_words(dev[k]), ref.bits(sc[k])), k  # the scene is only read
    assert sorted(os.listdir(tmp_path)) == ["device.ply", "host.ply"]


@pytest.mark.parametrize("M,degree", [(1, 3), (4, 3), (9, 4), (16, 4)])
def test_device_file_padded_to_a_higher_degree(M, degree, gpu, tmp_path):
    sc = ref.scene(257, M)
    dev = {k: _dev(v, gpu) for k, v in sc.items()}
    save_ply(tmp_path / "device.ply", dev, sh_degree=degree, chunk_rows=100)
    assert (tmp_path / "device.ply").read_bytes() == ref.file_bytes(sc, (degree + 1) ** 2)


def test_degree_4_and_parameters_without_f_rest(gpu, tmp_path):
    sc = ref.scene(321, 25)
    save_ply(tmp_path / "a.ply", {k: _dev(v, gpu) for k, v in sc.items()})
    assert (tmp_path / "a.ply").read_bytes() == ref.file_bytes(sc)
    sc = ref.scene(70, 1)
    params = {k: torch.nn.Parameter(_dev(v, gpu)) for k, v in sc.items() if k != "f_rest"}
    save_ply(tmp_path / "b.ply", params)
    assert (tmp_path / "b.ply").read_bytes() == ref.file_bytes(sc)


# ---- 2. awkward inputs ----------------------------------------------------------------------------
@pytest.mark.parametrize("M", COEFFS)
def test_unaligned_views_between_guards_on_another_stream(M, gpu, tmp_path):
    P = 1000
    sc = ref.scene(P, M)
    views, bufs = _device_scene(sc, gpu)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(stream):
        save_ply(tmp_path / "device.ply", views, chunk_rows=100)
    assert (tmp_path / "device.ply").read_bytes() == ref.file_bytes(sc)
    for k, a in sc.items():
        assert _guards_hold(bufs[k], a.size), k
        assert np.array_equal(_words(views[k]), ref.bits(a)), k


def test_mixed_devices_are_refused(gpu, tmp_path):
    sc = {k: _dev(v, gpu) for k, v in ref.scene(6, 4).items()}
    sc["opacity"] = sc["opacity"].cpu()
    with pytest.raises(ValueError, match="different devices"):
        save_ply(tmp_path / "x.ply", sc)
    assert os.listdir(tmp_path) == []


# ---- 3. load_scene_ply onto the device ---------------------------------------------------------------
def _load_between_guards(path, P, M, gpu, chunk_rows=0):
    """gsr_ply_load_scene into dirty, guarded, unaligned device views: ({name: words}, guards ok)."""
    out, bufs = {}, {}
    for k, shape in ref.shapes(P, M).items():
        bufs[k], out[k] = _guarded(shape, gpu, DIRT)
    lib = _lib.load_library()
    load = _lib.ply_scene_fns(lib)[2]
    sc = ply._c_scene(out, P, M, 0, chunk_rows)
    with torch.cuda.device(gpu):
        stream = torch.cuda.current_stream(gpu).cuda_stream
        _lib.check(load(os.fsencode(path), ctypes.byref(sc), 1, ctypes.c_void_p(stream)),
                   "gsr_ply_load_scene")
    ok = all(_guards_hold(bufs[k], out[k].numel()) for k in out)
    return {k: _words(v) for k, v in out.items()}, ok


def _file(kind, P, M, tmp_path):
    if kind == "saved":  # what save_ply writes: the fast path
        path = tmp_path / "saved.ply"
        save_ply(path, ref.copies(ref.scene(P, M)))
        return path
    return ref.fixture(kind, M, tmp_path, P)[0]


@pytest.mark.parametrize("kind", ["saved", "big_endian", "mixed"])
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("M", COEFFS)
def test_device_load_is_the_host_load(M, P, kind, gpu, tmp_path):
    path = _file(kind, P, M, tmp_path)
    host = load_scene_ply(path)
    assert host["xyz"].shape == (P, 3) and host["f_rest"].shape == (P, M - 1, 3)
    dev = load_scene_ply(path, device=gpu)
    for k in ref.NAMES:
        assert dev[k].device == gpu and dev[k].dtype == torch.float32 and dev[k].is_contiguous()
        assert tuple(dev[k].shape) == host[k].shape, k
        assert np.array_equal(_words(dev[k]), ref.bits(host[k])), k
    # dirty outputs between guard words, in chunks of 100 rows: every word written, none beyond
    got, guards = _load_between_guards(path, P, M, gpu, chunk_rows=100)
    assert guards
    for k in ref.NAMES:
        assert np.array_equal(got[k].reshape(-1), ref.bits(host[k]).reshape(-1)), k


@pytest.mark.parametrize("kind", ["shuffled", "no_normals", "extra_uchar", "doubles", "ascii"])
def test_device_load_of_other_layouts(kind, gpu, tmp_path):
    """Little-endian float files in another property order or without normals take the fast path
    too; a uchar among the properties, double positions and ascii take the host conversion."""
    P, M = 300, 9
    path = _file(kind, P, M, tmp_path)
    host = load_scene_ply(path)
    got, guards = _load_between_guards(path, P, M, gpu, chunk_rows=128)
    assert guards
    for k in ref.NAMES:
        assert np.array_equal(got[k].reshape(-1), ref.bits(host[k]).reshape(-1)), k


# ---- 4. a file the renderer opens ---------------------------------------------------------------------
NAMES = fr.GROUPS["stored"]
ITERATIONS = 10


def _fit(gpu):
    """Ten iterations of fit_step_reference's fit (its scene, camera, target, learning rates and
    activation) started from scene_from_point_cloud on the scene's own points."""
    sc = fr.scene()
    s = sc["s"]
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, deterministic=True)
    raster = GaussianRasterizer(rs)
    with torch.no_grad():
        target, _ = raster(means2D=None, colors_precomp=None, cov3D_precomp=None,
                           **{k: to_dev(v, gpu) for k, v in fr.parameters(sc, False).items()})
    assert s["sh_degree"] == 3  # the degree load_ply opens
    xyz = fr.parameters(sc, True)["means3D"]
    P = len(xyz)
    rgb = np.random.default_rng(fr.SEED).uniform(0.2, 0.8, (P, 3)).astype(np.float32)
    start = scene_from_point_cloud(xyz, rgb, sh_degree=s["sh_degree"], device=gpu)
    params = {k: torch.nn.Parameter(start[k].clone()) for k in NAMES}
    opt = SparseGaussianAdam([{"params": [params[k]], "lr": fr.GROUP_LRS["stored"][k], "name": k}
                              for k in NAMES], lr=0.0, eps=fr.EPS, betas=fr.BETAS)
    accum = torch.zeros((P, 1), device=gpu)
    denom = torch.zeros((P, 1), device=gpu)
    max_radii = torch.zeros(P, dtype=torch.int32, device=gpu)
    for _ in range(ITERATIONS):
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color, radii = raster(means2D=means2D, colors_precomp=None, cov3D_precomp=None,
                              **fr.activate(params))
        loss = photometric_loss(color, target, fr.LAMBDA)
        loss.backward()
        densification_stats(radii, means2D.grad, accum, denom, max_radii)
        opt.step(radii, P)
    return raster, params, opt, start


def test_a_fitted_scene_is_saved_resumed_and_opened_by_the_renderer(gpu, tmp_path):
    raster, params, opt, start = _fit(gpu)
    assert any(not torch.equal(params[k].detach(), start[k]) for k in NAMES)  # the fit moved
    before = {k: _words(params[k]).copy() for k in NAMES}
    path = tmp_path / "fit.ply"
    P = before["xyz"].shape[0]
    assert save_ply(path, opt) == P
    for k in NAMES:
        assert np.array_equal(_words(params[k]), before[k]), k
    # resumed: every parameter, bit for bit, as leaves a new optimizer takes
    loaded = load_scene_ply(path, device=gpu)
    assert set(loaded) == set(NAMES)
    for k in NAMES:
        assert tuple(loaded[k].shape) == tuple(params[k].shape), k
        assert np.array_equal(_words(loaded[k]), before[k]), k
    resumed = {k: torch.nn.Parameter(loaded[k]) for k in NAMES}
    SparseGaussianAdam([{"params": [resumed[k]], "lr": 1e-3, "name": k} for k in NAMES], lr=0.0,
                       eps=fr.EPS)
    with torch.no_grad():
        live = raster(means2D=None, colors_precomp=None, cov3D_precomp=None, **fr.activate(params))
        again = raster(means2D=None, colors_precomp=None, cov3D_precomp=None,
                       **fr.activate(resumed))
    assert np.array_equal(_words(again[0]), _words(live[0]))  # color
    assert torch.equal(again[1], live[1]) and int((live[1] > 0).sum()) > P // 2  # radii
    # the activated reader opens it, and reads what it reads from the independent writer's file
    mine, bbox, center = ply.load_ply(str(path), device=gpu)
    host_scene = {k: before[k].view(np.float32) for k in NAMES}
    other = tmp_path / "oracle.ply"
    ply_oracle.write_ply(other, ref.properties(host_scene))
    theirs, bbox2, center2 = ply.load_ply(str(other), device=gpu)
    for name in ("xyz", "rot", "scale", "opacity", "sh"):
        a, b = getattr(mine, name), getattr(theirs, name)
        assert a.shape == b.shape and a.shape[0] == P
        assert np.array_equal(_words(a), _words(b)), name
    assert np.array_equal(bbox, bbox2) and np.array_equal(center, center2)
    assert bool(torch.isfinite(mine.scale).all())
