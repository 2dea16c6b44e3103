"""CPU: the host side of gsr_densify_workspace / gsr_densify_plan / gsr_densify_apply
(include/gsr.h).  The loaded library refuses bad arguments before any HIP call, so no device is
needed; the ctypes structs match the header; densify_and_prune refuses what it cannot run."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import SparseGaussianAdam, _lib, densify, densify_and_prune

FAKE, OTHER = 0x1000, 0x2000  # non-NULL pointers nothing dereferences: every call is refused first
SCALING, OPACITY = 0x3000, 0x4000
INVALID = -1                  # GSR_E_INVALID
NAN = float("nan")
X, S, R, O, N = (_lib.GSR_ROLE_XYZ, _lib.GSR_ROLE_SCALING, _lib.GSR_ROLE_ROTATION,
                 _lib.GSR_ROLE_OPACITY, _lib.GSR_ROLE_NONE)


def _fns():
    return _lib.densify_fns(_lib.load_library())


def _in(P=10, P_out=12, n_groups=4, scale_space=_lib.GSR_SCALE_LOG, grad=2e-4, split=-2.0,
        opacity=-5.0, scale=math.inf, radius=20, grad_accum=FAKE, denom=FAKE, max_radii=FAKE,
        scaling=SCALING, opacity_ptr=OPACITY):
    return _lib.GsrDensifyPlanInputs(P, P_out, 7, n_groups, scale_space, grad, split, opacity,
                                     scale, radius, grad_accum, denom, max_radii, scaling,
                                     opacity_ptr)


def _g(M, role, param=FAKE, m=FAKE, v=FAKE):
    param = {S: SCALING, O: OPACITY}.get(role, param) if param == FAKE else param
    return _lib.GsrDensifyGroup(M, role, param, m, v)


def four():
    return [_g(3, X), _g(3, S), _g(4, R), _g(1, O)]


def _plan(inp, workspace=FAKE, counts=FAKE):
    return _fns()[1](None if inp is None else ctypes.byref(inp), workspace, counts, None)


def _apply(inp, src, dst, workspace=FAKE, source_index=FAKE):
    arr = lambda gs: None if gs is None else (_lib.GsrDensifyGroup * len(gs))(*gs)  # noqa: E731
    return _fns()[2](None if inp is None else ctypes.byref(inp), arr(src), arr(dst), workspace,
                     source_index, None)


def dst_of(src):
    return [_lib.GsrDensifyGroup(g.M, g.role, OTHER if g.param else None,
                                 OTHER if g.exp_avg else None, OTHER if g.exp_avg_sq else None)
            for g in src]


BAD_INPUTS = {
    "P_neg": dict(P=-1), "P_2_30": dict(P=2 ** 30), "scale_space": dict(scale_space=2),
    "grad_nan": dict(grad=NAN), "split_nan": dict(split=NAN), "opacity_nan": dict(opacity=NAN),
    "scale_nan": dict(scale=NAN), "grad_accum": dict(grad_accum=None), "denom": dict(denom=None),
    "scaling": dict(scaling=None), "opacity_ptr": dict(opacity_ptr=None),
}


@pytest.mark.parametrize("case", sorted(BAD_INPUTS) + ["in", "workspace", "counts"])
def test_plan_refusals(case):
    if case == "in":
        rc = _plan(None)
    elif case in BAD_INPUTS:
        rc = _plan(_in(**BAD_INPUTS[case]))
    else:
        rc = _plan(_in(), **{case: None})
    assert rc == INVALID
    assert b"gsr_densify_plan" in _lib.load_library().gsr_last_error()


def _with(groups, i, **kw):
    out = list(groups)
    g = out[i]
    f = dict(M=g.M, role=g.role, param=g.param, exp_avg=g.exp_avg, exp_avg_sq=g.exp_avg_sq)
    f.update(kw)
    out[i] = _lib.GsrDensifyGroup(f["M"], f["role"], f["param"], f["exp_avg"], f["exp_avg_sq"])
    return out


def _apply_cases():
    c = {k: (lambda kw=kw: (_in(**kw), four(), dst_of(four()))) for k, kw in BAD_INPUTS.items()}
    c.update({
        "in": lambda: (None, four(), dst_of(four())),
        "src_groups": lambda: (_in(), None, dst_of(four())),
        "dst_groups": lambda: (_in(), four(), None),
        "n_groups_0": lambda: (_in(n_groups=0), four(), dst_of(four())),
        "n_groups_9": lambda: (_in(n_groups=9), four() + [_g(2, N)] * 5,
                               dst_of(four() + [_g(2, N)] * 5)),
        "M_0": lambda: (_in(n_groups=5), four() + [_g(0, N)], dst_of(four() + [_g(0, N)])),
        "xyz_M": lambda: (_in(), _with(four(), 0, M=4), dst_of(_with(four(), 0, M=4))),
        "scaling_M": lambda: (_in(), _with(four(), 1, M=1), dst_of(_with(four(), 1, M=1))),
        "rotation_M": lambda: (_in(), _with(four(), 2, M=3), dst_of(_with(four(), 2, M=3))),
        "opacity_M": lambda: (_in(), _with(four(), 3, M=3), dst_of(_with(four(), 3, M=3))),
        "role_unknown": lambda: (_in(n_groups=5), four() + [_g(2, 5)], dst_of(four() + [_g(2, 5)])),
        "role_missing": lambda: (_in(n_groups=3), four()[:3], dst_of(four()[:3])),
        "role_replaced": lambda: (_in(), _with(four(), 2, role=N), dst_of(_with(four(), 2, role=N))),
        "role_twice": lambda: (_in(n_groups=5), four() + [_g(3, X)], dst_of(four() + [_g(3, X)])),
        "one_moment": lambda: (_in(), _with(four(), 0, exp_avg=None),
                               dst_of(_with(four(), 0, exp_avg=None))),
        "one_moment_dst": lambda: (_in(), four(), _with(dst_of(four()), 2, exp_avg_sq=None)),
        "moments_src_only": lambda: (_in(), four(),
                                     _with(dst_of(four()), 0, exp_avg=None, exp_avg_sq=None)),
        "src_param": lambda: (_in(), _with(four(), 0, param=None), dst_of(four())),
        "dst_param": lambda: (_in(), four(), _with(dst_of(four()), 3, param=None)),
        "dst_M": lambda: (_in(), four(), _with(dst_of(four()), 0, M=2)),
        "not_the_plans_scaling": lambda: (_in(), _with(four(), 1, param=OTHER), dst_of(four())),
        "P_out_neg": lambda: (_in(P_out=-1), four(), dst_of(four())),
        "P_out_over_2P": lambda: (_in(P_out=21), four(), dst_of(four())),
        "P_out_without_P": lambda: (_in(P=0, P_out=1), four(), dst_of(four())),
    })
    return c


APPLY_REFUSALS = _apply_cases()


@pytest.mark.parametrize("case", sorted(APPLY_REFUSALS) + ["workspace", "source_index"])
def test_apply_refusals(case):
    if case in APPLY_REFUSALS:
        rc = _apply(*APPLY_REFUSALS[case]())
    else:
        rc = _apply(_in(), four(), dst_of(four()), **{case: None})
    assert rc == INVALID
    assert b"gsr_densify_apply" in _lib.load_library().gsr_last_error()


def test_the_empty_apply_is_ok_but_only_for_valid_arguments():
    """P_out == 0 (so also P == 0) is GSR_OK with no launch; NULL buffers allowed where there are
    no rows; a group without moments is fine."""
    null = lambda gs: [_lib.GsrDensifyGroup(g.M, g.role, None, None, None) for g in gs]  # noqa: E731
    assert _apply(_in(P=10, P_out=0), four(), null(four()), source_index=None) == 0
    empty = _in(P=0, P_out=0, grad_accum=None, denom=None, max_radii=None, scaling=None,
                opacity_ptr=None)
    assert _apply(empty, null(four()), null(four()), source_index=None) == 0
    five = four() + [_g(17, N, m=None, v=None)]
    assert _apply(_in(P=10, P_out=0, n_groups=5), five, dst_of(five)) == 0
    assert _apply(_in(P=10, P_out=0, grad=NAN), four(), null(four())) == INVALID
    assert _apply(_in(P=10, P_out=0), four()[:3] + [_g(1, N)], null(four())) == INVALID


def test_workspace_size():
    ws = _fns()[0]
    assert ws(-1) == INVALID and ws(2 ** 30) == INVALID
    sizes = [ws(P) for P in (0, 1, 256, 257, 1000, 2 ** 30 - 1)]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] < 5 * 2 ** 30  # about a word per row
    assert {"gsr_densify_workspace", "gsr_densify_plan", "gsr_densify_apply"} <= \
        set(_lib.EXPORTED_SYMBOLS)

    class Older:
        gsr_adam_step = object()

    with pytest.raises(RuntimeError, match="no gsr_densify_workspace"):
        _lib.densify_fns(Older())


@pytest.mark.parametrize("ctype, c_name", [(_lib.GsrDensifyGroup, "gsr_densify_group"),
                                           (_lib.GsrDensifyPlanInputs, "gsr_densify_plan_inputs")])
def test_struct_layouts_match_header(ctype, c_name, tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f for f, _ in ctype._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             f'printf("%zu\\n", sizeof({c_name}));',
             'printf("%d %d %d %d %d %d %d %d\\n", GSR_SPLIT_CHILDREN, GSR_ROLE_NONE, GSR_ROLE_XYZ,'
             " GSR_ROLE_SCALING, GSR_ROLE_ROTATION, GSR_ROLE_OPACITY, GSR_SCALE_LINEAR,"
             " GSR_SCALE_LOG);"]
    lines += [f'printf("%zu\\n", offsetof({c_name}, {f}));' for f in names]
    (tmp_path / "probe.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(repo, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True)
    got = [int(v) for v in out.stdout.split()]
    assert got[0] == ctypes.sizeof(ctype)
    assert got[1:9] == [_lib.SPLIT_CHILDREN, N, X, S, R, O, _lib.GSR_SCALE_LINEAR,
                        _lib.GSR_SCALE_LOG]
    assert got[9:] == [getattr(ctype, f).offset for f in names]


def test_stored_thresholds():
    """Upstream's arguments in the stored space: doubles, rounded once."""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    t, r = densify.stored_thresholds(2e-4, 0.005, 5.0, 20, 0.01)
    assert t == (f32(2e-4), f32(math.log(0.05)), f32(math.log(0.005 / 0.995)), f32(math.log(0.5)))
    assert r == 20
    t, r = densify.stored_thresholds(2e-4, 0.005, 5.0, None, 0.01)
    assert t[3] == math.inf and r == 0
    t, r = densify.stored_thresholds(2e-4, 0.005, 5.0, 20.7, 0.02, activated=True)
    assert t == (f32(2e-4), f32(0.1), f32(0.005), f32(0.5)) and r == 20
    assert densify.stored_thresholds(1.0, 0.0, 1.0)[0][2] == -math.inf


def test_python_refusals_need_no_device():
    P = 4
    shapes = dict(xyz=(P, 3), scaling=(P, 3), rotation=(P, 4), opacity=(P, 1))
    kw = dict(max_grad=2e-4, min_opacity=0.005, extent=1.0, seed=0)
    z = torch.zeros(P)

    def opt(names=shapes, **over):
        return SparseGaussianAdam([{"params": [torch.nn.Parameter(over.get(n, torch.zeros(s)))],
                                    "lr": 1e-3, "name": n} for n, s in names.items()],
                                  lr=0.0, eps=1e-15)

    with pytest.raises(ValueError, match="HIP device"):
        densify_and_prune(opt(), z, z.clone(), **kw)
    with pytest.raises(ValueError, match="no param group named 'rotation'"):
        densify_and_prune(opt({k: v for k, v in shapes.items() if k != "rotation"}), z, z, **kw)
    with pytest.raises(ValueError, match="no param group named 'scales'"):
        densify_and_prune(opt(), z, z, roles={"scaling": "scales"}, **kw)
    with pytest.raises(ValueError, match="roles maps"):
        densify_and_prune(opt(), z, z, roles={"colour": "xyz"}, **kw)
    with pytest.raises(ValueError, match="one group holds two roles"):
        densify_and_prune(opt(), z, z, roles={"scaling": "xyz"}, **kw)
    with pytest.raises(ValueError, match='by the param group\'s "name"'):
        densify_and_prune(SparseGaussianAdam([{"params": [torch.nn.Parameter(torch.zeros(P, 3))]}],
                                             lr=1e-3, eps=1e-15), z, z, **kw)
    two = opt()
    two.param_groups[1]["name"] = "xyz"
    with pytest.raises(ValueError, match="two param groups are named 'xyz'"):
        densify_and_prune(two, z, z, **kw)
    with pytest.raises(ValueError, match="route must be"):
        densify._use_native("torch")
