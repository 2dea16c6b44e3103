"""GPU: gsr_knn_mean_dist2 gives, bit for bit, the brute-force search of include/gsr.h
(knn_reference.brute, numpy float32) on every scene of knn_scenes.py, through every route; and
scene_from_point_cloud builds upstream's create_from_pcd on it.  The comparison of the search has
no tolerance: one neighbour missed in one row fails it.

Measured on an MI355X: scaling against scaling_reference of the GPU's own dist2, largest error
8.37e-07 = 0.214 of the bound 8 x SCALING_F32_SPREAD = 3.92e-06; the boxes a block scans equal the
numpy restatement's count on every scene tried (uniform: 14.88 of 24 on average).
"""
import numpy as np
import pytest
import torch

import knn_reference as kr
import knn_scenes as ks
from gaussiansplattingviewer_amd import (knn_mean_dist2, pointcloud, scene_from_point_cloud,
                                         static_camera, synthetic_gaussians)
from gpu_helpers import run_hip, scene_inputs, to_dev, to_dev_unaligned

pytestmark = pytest.mark.gpu

ROUTES = ("ctypes", "_C", "python")
GUARD = 64
PATTERN = 0xDEADBEEF - (1 << 32)  # as int32


def _bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _points(name, gpu):
    xyz = ks.scenes()[name].copy()  # (the shared arrays are read-only)
    if name == "unaligned":
        return to_dev_unaligned(xyz, gpu)
    return to_dev(xyz, gpu).reshape(-1, 3)


def _ctypes(xyz, stream_sync=True):
    """gsr_knn_mean_dist2 by ctypes into guarded buffers -> (dist2, guards intact, workspace)."""
    N, dev = xyz.shape[0], xyz.device
    out = torch.full((N + 2 * GUARD,), PATTERN, dtype=torch.int32, device=dev)
    nbytes = pointcloud.workspace_bytes(N)
    ws = torch.full((nbytes + 4 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    dist2 = out[GUARD:GUARD + N].view(torch.float32)
    pointcloud.knn_stages(xyz, dist2, ws[:nbytes])
    intact = bool((out[:GUARD] == PATTERN).all() and (out[GUARD + N:] == PATTERN).all() and
                  (ws[nbytes:] == 0x5A).all())
    return dist2, intact, ws


def _run(route, xyz):
    if route == "ctypes":
        dist2, intact, _ = _ctypes(xyz)
        assert intact, "a word outside dist2[0, N) or past the workspace was written"
        return dist2
    if route == "_C":
        from gaussiansplattingviewer_amd import _C
        return _C.distCUDA2(xyz)
    return knn_mean_dist2(xyz)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ks.NAMES)
def test_dist2_is_brute_force_bit_for_bit(name, route, gpu):
    xyz = _points(name, gpu)
    got = _run(route, xyz)
    assert got.shape == (xyz.shape[0],) and got.dtype == torch.float32 and got.device == xyz.device
    want = kr.brute_cached(ks.scenes()[name])
    wrong = int((_bits(got) != _bits(want)).sum())
    assert wrong == 0, f"{name} via {route}: {wrong} of {len(want)} rows differ from brute force"


def test_input_rows_are_read_at_a_4_byte_aligned_pointer(gpu):
    xyz = _points("unaligned", gpu)
    assert xyz.data_ptr() % 16 == 4
    dist2, intact, _ = _ctypes(xyz)
    assert intact
    np.testing.assert_array_equal(_bits(dist2), _bits(kr.brute_cached(ks.scenes()["unaligned"])))
    # and the output, and the workspace, at such pointers too
    N = xyz.shape[0]
    out = torch.zeros(N + 1, device=gpu)[1:]
    ws = torch.zeros(pointcloud.workspace_bytes(N) + 4, dtype=torch.uint8, device=gpu)[4:]
    assert out.data_ptr() % 16 == 4 and ws.data_ptr() % 16 == 4
    pointcloud.knn_stages(xyz, out, ws)
    np.testing.assert_array_equal(_bits(out), _bits(dist2))


@pytest.mark.parametrize("name", ["uniform", "slab", "n257"])
def test_same_bits_on_a_second_stream_a_second_call_and_after_a_frame(name, gpu):
    xyz = _points(name, gpu)
    want = _bits(kr.brute_cached(ks.scenes()[name]))
    first, intact, ws = _ctypes(xyz)
    assert intact
    np.testing.assert_array_equal(_bits(first), want)
    # a second call into the same (now dirty) workspace
    again = torch.empty_like(first)
    pointcloud.knn_stages(xyz, again, ws)
    np.testing.assert_array_equal(_bits(again), want)
    # a second stream
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        on_side = knn_mean_dist2(xyz)
        on_side_ctypes, intact, _ = _ctypes(xyz)
    side.synchronize()
    assert intact
    np.testing.assert_array_equal(_bits(on_side), want)
    np.testing.assert_array_equal(_bits(on_side_ctypes), want)
    # after an unrelated frame has run on a context
    run_hip(scene_inputs(synthetic_gaussians(400, 3, seed=3), static_camera(64, 48), 3), gpu)
    np.testing.assert_array_equal(_bits(knn_mean_dist2(xyz)), want)


@pytest.mark.parametrize("name", ["uniform", "clusters", "n513"])
def test_scanned_counts_and_the_stage_prefixes(name, gpu):
    """The workspace's readable part: per block of the search, the boxes it scanned, between 1
    and the number of boxes.  gsr_knn_stages cut short writes no dist2."""
    xyz = _points(name, gpu)
    N = xyz.shape[0]
    nb = (N + 255) // 256
    dist2, intact, ws = _ctypes(xyz)
    assert intact and ws.data_ptr() % 256 == 0
    scanned = ws[:4 * nb].view(torch.int32).cpu().numpy()
    stats = {}
    kr.boxed(ks.scenes()[name], stats=stats)
    print(f"{name}: boxes scanned per block, mean {scanned.mean():.2f} of {nb} "
          f"(the numpy restatement: {stats['scanned'].mean():.2f})")
    assert (scanned >= 1).all() and (scanned <= nb).all()
    for n_stages in (1, 2, 3):
        out = torch.full((N,), PATTERN, dtype=torch.int32, device=gpu)
        pointcloud.knn_stages(xyz, out.view(torch.float32), ws, n_stages)
        assert bool((out == PATTERN).all()), n_stages
    final = torch.empty(N, device=gpu)
    pointcloud.knn_stages(xyz, final, ws, 4)
    np.testing.assert_array_equal(_bits(final), _bits(dist2))


def test_empty_cloud(gpu):
    empty = torch.zeros((0, 3), device=gpu)
    for route in ROUTES:
        out = _run(route, empty)
        assert out.shape == (0,) and out.dtype == torch.float32
    scene = scene_from_point_cloud(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8),
                                   sh_degree=1, device=gpu)
    assert scene["f_rest"].shape == (0, 3, 3) and scene["scaling"].shape == (0, 3)


def test_knn_mean_dist2_refusals(gpu):
    good = to_dev(ks.scenes()["n257"].copy(), gpu)
    with pytest.raises(ValueError, match="HIP device"):
        knn_mean_dist2(good.cpu())
    with pytest.raises(ValueError, match="float32"):
        knn_mean_dist2(good.double())
    with pytest.raises(ValueError, match="float32"):
        knn_mean_dist2(good.half())
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        knn_mean_dist2(good[:, :2].contiguous())
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        knn_mean_dist2(good.reshape(-1))
    with pytest.raises(ValueError, match="contiguous"):
        knn_mean_dist2(torch.zeros((3, 300), device=gpu).t())
    with pytest.raises(ValueError, match="contiguous"):
        knn_mean_dist2(torch.zeros((300, 6), device=gpu)[:, ::2])
    with pytest.raises(ValueError, match="tensor"):
        knn_mean_dist2(ks.scenes()["n257"])
    with pytest.raises(ValueError, match="route"):
        knn_mean_dist2(good, route="eager")
    for bad in (float("nan"), float("inf"), -float("inf")):
        x = good.clone()
        x[200, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            knn_mean_dist2(x)
        with pytest.raises(ValueError, match="not finite"):
            scene_from_point_cloud(x, torch.zeros_like(x))
    from gaussiansplattingviewer_amd import _C
    with pytest.raises(RuntimeError, match="device"):
        _C.distCUDA2(good.cpu())
    with pytest.raises(RuntimeError, match=r"\(num_points, 3\)"):
        _C.distCUDA2(good.double())


# ---- scene_from_point_cloud ---------------------------------------------------------------------
SH_C0 = 0.28209479177387814


def _ulps(got, want):
    g = np.ascontiguousarray(got, np.float32).view(np.int32).astype(np.int64)
    w = np.ascontiguousarray(want, np.float32).view(np.int32).astype(np.int64)
    g = np.where(g < 0, -(g & 0x7FFFFFFF), g)
    w = np.where(w < 0, -(w & 0x7FFFFFFF), w)
    return int(np.abs(g - w).max()) if g.size else 0


@pytest.mark.parametrize("sh_degree", [0, 3])
def test_scene_from_point_cloud(sh_degree, gpu):
    xyz = ks.scenes()["clusters"]
    N = len(xyz)
    rgb = np.random.default_rng(5).integers(0, 256, (N, 3)).astype(np.uint8)
    scene = scene_from_point_cloud(xyz, rgb, sh_degree=sh_degree, opacity=0.1, device=gpu)
    shapes = dict(xyz=(N, 3), f_dc=(N, 1, 3), f_rest=(N, (sh_degree + 1) ** 2 - 1, 3),
                  scaling=(N, 3), rotation=(N, 4), opacity=(N, 1))
    assert list(scene) == list(shapes)
    for k, shape in shapes.items():
        t = scene[k]
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.device == gpu, k
        assert t.is_contiguous() and not t.requires_grad, k
    host = {k: v.cpu().numpy() for k, v in scene.items()}
    # one operation or none: bit for bit
    np.testing.assert_array_equal(_bits(host["xyz"]), _bits(xyz))
    assert not host["f_rest"].any()
    np.testing.assert_array_equal(host["rotation"], np.tile(np.float32([1, 0, 0, 0]), (N, 1)))
    # two or three operations: within 1 ulp of numpy float32
    colour = rgb.astype(np.float32) / np.float32(255)
    f_dc = ((colour - np.float32(0.5)) / np.float32(SH_C0))[:, None, :]
    assert _ulps(host["f_dc"], f_dc) <= 1
    logit = np.float32(np.log(0.1 / (1.0 - 0.1)))
    assert _ulps(host["opacity"], np.full((N, 1), logit, np.float32)) <= 1
    # the scales: the three axes alike, and the project's rule against the float64 reference of
    # the GPU's own dist2
    dist2 = knn_mean_dist2(scene["xyz"])
    np.testing.assert_array_equal(_bits(dist2), _bits(kr.brute_cached(xyz)))
    for a in (1, 2):
        np.testing.assert_array_equal(_bits(host["scaling"][:, a]), _bits(host["scaling"][:, 0]))
    want = kr.scaling_reference(dist2.cpu().numpy())
    err = float(np.abs(host["scaling"][:, 0].astype(np.float64) - want).max())
    bound = 8 * kr.SCALING_F32_SPREAD
    print(f"scaling: largest error {err:.3g} = {err / bound:.3f} of the bound {bound:.3g}")
    assert err <= bound


def test_scene_scaling_floor_and_colour_and_input_forms(gpu):
    # duplicates: dist2 = 0 everywhere, so every scale is the floor's
    xyz = ks.scenes()["duplicates"]
    N = len(xyz)
    rgb8 = np.random.default_rng(6).integers(0, 256, (N, 3)).astype(np.uint8)
    a = scene_from_point_cloud(xyz, rgb8, sh_degree=1, min_dist2=1e-7, device=gpu)
    want = kr.scaling_reference(np.zeros(N))
    err = float(np.abs(a["scaling"].cpu().numpy().astype(np.float64) - want[:, None]).max())
    assert err <= 8 * kr.SCALING_F32_SPREAD
    b = scene_from_point_cloud(xyz, rgb8, sh_degree=1, min_dist2=1e-4, device=gpu)
    want = kr.scaling_reference(np.zeros(N), 1e-4)
    err = float(np.abs(b["scaling"].cpu().numpy().astype(np.float64) - want[:, None]).max())
    assert err <= 8 * kr.SCALING_F32_SPREAD
    # uint8 colours and the same colours as floats in [0, 1]
    rgbf = rgb8.astype(np.float32) / np.float32(255)
    c = scene_from_point_cloud(xyz, rgbf, sh_degree=1, device=gpu)
    assert _ulps(c["f_dc"].cpu().numpy(), a["f_dc"].cpu().numpy()) <= 1
    c64 = scene_from_point_cloud(xyz, rgbf.astype(np.float64), sh_degree=1, device=gpu)
    assert _ulps(c64["f_dc"].cpu().numpy(), a["f_dc"].cpu().numpy()) <= 1
    # numpy input and tensor input (host and device) give the same bits
    forms = [(torch.from_numpy(xyz.copy()), torch.from_numpy(rgb8)),
             (to_dev(xyz.copy(), gpu), to_dev(rgb8, gpu)),
             (xyz.astype(np.float64), rgb8)]
    for px, pc in forms:
        d = scene_from_point_cloud(px, pc, sh_degree=1, device=gpu)
        for k in a:
            np.testing.assert_array_equal(_bits(d[k]), _bits(a[k]), err_msg=k)
    # a device tensor decides the device, and the scene does not alias it
    dev_xyz = to_dev(xyz.copy(), gpu)
    e = scene_from_point_cloud(dev_xyz, rgb8)
    assert e["xyz"].device == gpu and e["xyz"].data_ptr() != dev_xyz.data_ptr()


def test_scene_from_point_cloud_refusals(gpu):
    xyz = ks.scenes()["n257"]
    rgb = np.zeros((257, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        scene_from_point_cloud(xyz[:, :2], rgb, device=gpu)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        scene_from_point_cloud(xyz, rgb[:, :1], device=gpu)
    with pytest.raises(ValueError, match="rows"):
        scene_from_point_cloud(xyz, rgb[:100], device=gpu)
    with pytest.raises(ValueError, match="sh_degree"):
        scene_from_point_cloud(xyz, rgb, sh_degree=-1, device=gpu)
    with pytest.raises(ValueError, match="opacity"):
        scene_from_point_cloud(xyz, rgb, opacity=1.0, device=gpu)
    with pytest.raises(ValueError, match="HIP device"):
        scene_from_point_cloud(xyz, rgb, device="cpu")
