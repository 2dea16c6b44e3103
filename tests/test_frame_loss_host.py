"""CPU: the host side of the frame's loss on a strip (gsr_image_loss_window and its backward,
include/gsr.h; losses.frame_loss_on_strip; strips.exchange_halo).  No device is needed: every
refusal comes before the first HIP call (without a device such a call would fail with another
code), and the halo exchange's plan is index arithmetic.

   1 the three entries are exported and declared; gsr_loss_window's layout is the header's
   2 the workspace query
   3 every refusal of the three C entries returns GSR_E_INVALID and leaves poisoned outputs alone
   4 the Python ValueErrors of frame_loss_on_strip (and of exchange_halo's arguments)
   5 halo_plan: a short last strip, empty trailing strips, world 1, balanced layouts, bad layouts
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import gaussiansplattingviewer_amd as gsv
from gaussiansplattingviewer_amd import _lib, losses, strips

FAKE = 0x1000  # a non-NULL pointer nothing dereferences: every call below is refused first
POISON = np.float32(-1234.5)
FRAME = dict(C=3, W=70, frame_H=40)


def _fns():
    return _lib.image_loss_window_fns(_lib.load_library())


def _inputs(H=36, lam=0.2, image=FAKE, target=FAKE, C=FRAME["C"], W=FRAME["W"]):
    return _lib.GsrImageLossInputs(C, H, W, lam, image, target)


def _window(row0=0, own=(10, 26), frame_H=FRAME["frame_H"]):
    return _lib.GsrLossWindow(frame_H, row0, own[0], own[1])


# ---- 1 ------------------------------------------------------------------------------------------
def test_exported_and_declared():
    names = ("gsr_image_loss_window_workspace", "gsr_image_loss_window",
             "gsr_image_loss_window_backward")
    lib = _lib.load_library()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert _fns() == tuple(getattr(lib, n) for n in names)
    assert losses.HALO_ROWS == 10 and gsv.HALO_ROWS == 10
    assert gsv.frame_loss_on_strip is losses.frame_loss_on_strip
    assert gsv.exchange_halo is strips.exchange_halo
    from gaussiansplattingviewer_amd import _C
    assert callable(_C.fused_image_loss_window) and callable(_C.fused_image_loss_window_backward)


def test_struct_layout_matches_header(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f for f, _ in _lib.GsrLossWindow._fields_]
    assert names == ["frame_H", "row0", "own_begin", "own_end"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             'printf("%zu\\n", sizeof(gsr_loss_window));']
    lines += [f'printf("%zu\\n", offsetof(gsr_loss_window, {f}));' for f in names]
    (tmp_path / "probe.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(repo, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True)
    got = [int(v) for v in out.stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.GsrLossWindow) == 16
    assert got[1:] == [getattr(_lib.GsrLossWindow, f).offset for f in names] == [0, 4, 8, 12]


# ---- 2 ------------------------------------------------------------------------------------------
def test_workspace_query():
    workspace = _fns()[0]

    def size(inp, win):
        return workspace(ctypes.byref(inp), ctypes.byref(win))
    # one float pair per 16 x 64 tile of the apron and channel: rows [5, 31) -> 2 tile rows
    assert size(_inputs(), _window()) == 3 * 2 * 2 * 8
    # the whole frame as a window: gsr_image_loss_workspace's size
    whole = _lib.load_library().gsr_image_loss_workspace(3, 40, 70)
    assert size(_inputs(H=40), _window(own=(0, 40))) == whole == 3 * 2 * 3 * 8
    # neither the band's pointers nor its coverage matter to the size
    assert size(_inputs(H=1, image=None, target=None), _window(row0=12)) == 3 * 2 * 2 * 8
    for inp, win in ((_inputs(C=0), _window()), (_inputs(), _window(own=(10, 10))),
                     (_inputs(), _window(own=(10, 41))), (_inputs(lam=float("nan")), _window()),
                     (_inputs(C=1 << 15, W=1 << 15), _window(frame_H=2, own=(0, 1)))):
        assert size(inp, win) == -1
        assert b"gsr_image_loss_window_workspace" in _lib.load_library().gsr_last_error()
    assert workspace(None, ctypes.byref(_window())) == -1
    assert workspace(ctypes.byref(_inputs()), None) == -1


# ---- 3 ------------------------------------------------------------------------------------------
# own = [10, 26) of a 40-row frame: with `saved` the band must cover [0, 36), without it [5, 31),
# and the backward reads of it [10, 26).
REFUSALS = {
    "in": {}, "window": {}, "values": {}, "workspace": {},
    "image": dict(inp=dict(image=None)), "target": dict(inp=dict(target=None)),
    "C": dict(inp=dict(C=0)), "W": dict(inp=dict(W=0)), "H": dict(inp=dict(H=0)),
    "frame_H": dict(win=dict(frame_H=0)),
    "too_large": dict(inp=dict(C=1 << 15, W=1 << 15, H=2), win=dict(frame_H=2, own=(0, 1))),
    "own_empty": dict(win=dict(own=(10, 10))), "own_reversed": dict(win=dict(own=(26, 10))),
    "own_negative": dict(win=dict(own=(-1, 26))), "own_past_frame": dict(win=dict(own=(10, 41))),
    "band_before_frame": dict(win=dict(row0=-1)),
    "band_past_frame": dict(inp=dict(H=36), win=dict(row0=5)),
    "band_starts_late": dict(inp=dict(H=35), win=dict(row0=1)),
    "band_ends_early": dict(inp=dict(H=35)),
    "lambda_low": dict(inp=dict(lam=-1e-6)), "lambda_high": dict(inp=dict(lam=1.0 + 1e-6)),
    "lambda_nan": dict(inp=dict(lam=float("nan"))),
}


def _buffers():
    return {k: np.full(n, POISON, np.float32)
            for k, n in (("values", 3), ("saved", 3 * 3 * 26 * 70), ("workspace", 64),
                         ("dL_dimage", 3 * 16 * 70))}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


@pytest.mark.parametrize("case", sorted(REFUSALS))
@pytest.mark.parametrize("with_saved", [True, False])
def test_forward_refusals_write_nothing(case, with_saved):
    forward = _fns()[1]
    kw = REFUSALS[case]
    if not with_saved and case in ("band_starts_late", "band_ends_early"):
        # without `saved` the band need only cover [5, 31): these two are then valid bands, and
        # the ones one row short of THAT are refused
        kw = dict(inp=dict(H=25), win=dict(row0=6)) if case == "band_starts_late" else \
            dict(inp=dict(H=25), win=dict(row0=5))
    bufs = _buffers()
    ptr = {k: b.ctypes.data for k, b in bufs.items()}
    inp = None if case == "in" else ctypes.byref(_inputs(**kw.get("inp", {})))
    win = None if case == "window" else ctypes.byref(_window(**kw.get("win", {})))
    rc = forward(inp, win, None if case == "values" else ptr["values"],
                 ptr["saved"] if with_saved else None,
                 None if case == "workspace" else ptr["workspace"], None)
    assert rc == -1 and b"gsr_image_loss_window: bad" in _lib.load_library().gsr_last_error()
    assert _untouched(bufs)


@pytest.mark.parametrize("case", sorted(set(REFUSALS) - {"values", "workspace", "band_ends_early",
                                                         "band_starts_late"}
                                        | {"saved", "dL_dimage", "band_misses_own_rows"}))
def test_backward_refusals_write_nothing(case):
    backward = _fns()[2]
    kw = REFUSALS.get(case, {})
    if case == "band_misses_own_rows":
        kw = dict(inp=dict(H=15), win=dict(row0=10))
    bufs = _buffers()
    ptr = {k: b.ctypes.data for k, b in bufs.items()}
    inp = None if case == "in" else ctypes.byref(_inputs(**kw.get("inp", {})))
    win = None if case == "window" else ctypes.byref(_window(**kw.get("win", {})))
    rc = backward(inp, win, None if case == "saved" else ptr["saved"], None,
                  None if case == "dL_dimage" else ptr["dL_dimage"], None)
    assert rc == -1
    assert b"gsr_image_loss_window_backward: bad" in _lib.load_library().gsr_last_error()
    assert _untouched(bufs)


# ---- 4 ------------------------------------------------------------------------------------------
def test_python_refusals_need_no_device():
    f = gsv.frame_loss_on_strip
    tgt = torch.rand(3, 40, 70)
    img, up, down = torch.rand(3, 16, 70), torch.rand(3, 10, 70), torch.rand(3, 8, 70)
    ok = dict(above=up, below=down)
    with pytest.raises(ValueError, match="must be tensors"):
        f(img.numpy(), tgt, (16, 32), **ok)
    with pytest.raises(ValueError, match=r"\(C, rows, W\)"):
        f(img[0], tgt, (16, 32), **ok)
    with pytest.raises(ValueError, match="must share"):
        f(img, torch.rand(3, 40, 71), (16, 32), **ok)
    with pytest.raises(ValueError, match="must share"):
        f(img, torch.rand(2, 40, 70), (16, 32), **ok)
    with pytest.raises(ValueError, match=r"rows must be \(y0, y1\)"):
        f(img, tgt, 16, **ok)
    with pytest.raises(ValueError, match="not inside the frame"):
        f(img, tgt, (30, 46), **ok)
    with pytest.raises(ValueError, match="not inside the frame"):
        f(img, tgt, (32, 16), **ok)
    with pytest.raises(ValueError, match="image has 16 rows"):
        f(img, tgt, (16, 31), **ok)
    with pytest.raises(ValueError, match="target is a constant"):
        f(img, tgt.clone().requires_grad_(True), (16, 32), **ok)
    with pytest.raises(ValueError, match="lambda_dssim"):
        f(img, tgt, (16, 32), lambda_dssim=1.5, **ok)
    with pytest.raises(ValueError, match="`above` must hold the 10"):
        f(img, tgt, (16, 32), below=down)
    with pytest.raises(ValueError, match="`below` must hold the 8"):
        f(img, tgt, (16, 32), above=up)
    with pytest.raises(ValueError, match=r"`below` must be \(3, 8, 70\)"):
        f(img, tgt, (16, 32), above=up, below=up)
    with pytest.raises(ValueError, match=r"`above` must be \(3, 0, 70\)"):
        f(img, tgt, (0, 16), above=up, below=up)
    with pytest.raises(ValueError, match="`above` is a constant"):
        f(img, tgt, (16, 32), above=up.clone().requires_grad_(True), below=down)
    with pytest.raises(ValueError, match="HIP device"):
        f(img, tgt, (16, 32), **ok)  # everything fits: only the device is missing
    with pytest.raises(ValueError, match="HIP device"):
        f(torch.rand(3, 0, 70), tgt, (40, 40))  # an empty strip needs no halo, but a device
    assert losses.halo_counts((0, 16), 40) == (0, 10)
    assert losses.halo_counts((32, 40), 40) == (10, 0)
    assert losses.halo_counts((4, 36), 40) == (4, 4)
    assert losses.apron_rows(40, (16, 32)) == (11, 37) and losses.apron_rows(40, (0, 40)) == (0, 40)
    with pytest.raises(ValueError, match="detached"):
        strips.exchange_halo(img.clone().requires_grad_(True), [(0, 1), (1, 3)], 40, 0)
    with pytest.raises(ValueError, match="strip shape"):
        strips.exchange_halo(img, [(0, 2), (2, 3)], 40, 0)


# ---- 5 ------------------------------------------------------------------------------------------
def _check_plans(layout, H, rows=10):
    """Every rank's plan against the frame: what is received is what the neighbour sends."""
    plans = [strips.halo_plan(layout, H, r, rows) for r in range(len(layout))]
    for r, p in enumerate(plans):
        y0, y1 = p["rows"]
        assert (y0, y1 - y0) == strips.strip_pixel_rows(layout[r], H)
        if y0 == y1:
            assert p["above"] is None and p["below"] is None and p["sends"] == []
            continue
        want = {"above": min(rows, y0), "below": min(rows, H - y1)}
        for side, n in want.items():
            if n == 0:
                assert p[side] is None
                continue
            peer, got = p[side]
            assert got == n and peer == (r - 1 if side == "above" else r + 1)
            # the peer sends exactly those frame rows
            sent = [(s0, s1) for to, s0, s1 in plans[peer]["sends"] if to == r]
            assert len(sent) == 1
            py0 = plans[peer]["rows"][0]
            frame_rows = (py0 + sent[0][0], py0 + sent[0][1])
            assert frame_rows == ((y0 - n, y0) if side == "above" else (y1, y1 + n))
        # nothing is sent that nobody receives
        for to, s0, s1 in p["sends"]:
            assert abs(to - r) == 1 and 0 <= s0 < s1 <= y1 - y0
            assert plans[to]["above" if to > r else "below"] == (r, s1 - s0)
    return plans


def test_halo_plan_short_last_strip():
    plans = _check_plans([(0, 1), (1, 2), (2, 3)], 40)  # 16, 16 and 8 rows
    assert plans[1]["below"] == (2, 8) and plans[2]["sends"] == [(1, 0, 8)]  # handed over whole
    assert plans[0] == {"rows": (0, 16), "above": None, "below": (1, 10), "sends": [(1, 6, 16)]}
    plans = _check_plans([(0, 2), (2, 3)], 33)  # a last strip of one row
    assert plans[0]["below"] == (1, 1) and plans[1]["above"] == (0, 10)


def test_halo_plan_empty_trailing_strips():
    layout = strips.strip_layout(3, 5)  # 3 tile rows for 5 ranks
    assert layout[3] == layout[4] == (3, 3)
    plans = _check_plans(layout, 40)
    assert plans[2]["below"] is None and [to for to, _, _ in plans[2]["sends"]] == [1]
    assert plans[3] == plans[4] == {"rows": (40, 40), "above": None, "below": None, "sends": []}


def test_halo_plan_world_one_and_balanced_layouts():
    assert _check_plans([(0, 3)], 40)[0]["sends"] == []
    rng = np.random.default_rng(3)
    for world in (2, 3, 8):
        for gy, H in ((9, 135), (68, 1080), (8, 128)):
            _check_plans(strips.balanced_layout(rng.integers(0, 1000, gy), world), H)
            _check_plans(strips.strip_layout(gy, world), H)


def test_halo_plan_refuses_what_neighbours_cannot_supply():
    with pytest.raises(ValueError, match="not a partition"):
        strips.halo_plan([(0, 1), (2, 3)], 40, 0)
    with pytest.raises(ValueError, match="not a partition"):
        strips.halo_plan([(0, 1), (1, 1), (1, 3)], 40, 0)
    with pytest.raises(ValueError, match="covers 32"):
        strips.halo_plan([(0, 1), (1, 2)], 40, 0)
    with pytest.raises(ValueError, match="shorter than the 17"):
        strips.halo_plan([(0, 1), (1, 2), (2, 3)], 40, 1, rows=17)
    with pytest.raises(ValueError, match="bad rank"):
        strips.halo_plan([(0, 3)], 40, 1)
