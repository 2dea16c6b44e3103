"""CPU: the host side of gsr_adam_step and gsr_densify_stats (include/gsr.h).  The loaded library
refuses bad arguments before any HIP call, so no device is needed; the ctypes structs match the
header; SparseGaussianAdam refuses what it cannot run."""
import ctypes
import os
import subprocess

import pytest
import torch

from gaussiansplattingviewer_amd import SparseGaussianAdam, _lib, densification_stats

FAKE = 0x1000  # a non-NULL pointer nothing dereferences: every call below is refused first
INVALID = -1   # GSR_E_INVALID
NAN = float("nan")


def _group(M=3, lr=1e-3, eps=1e-15, param=FAKE, grad=FAKE, exp_avg=FAKE, exp_avg_sq=FAKE):
    return _lib.GsrParamGroup(M, lr, eps, param, grad, exp_avg, exp_avg_sq)


def _settings(P=10, n_groups=1, beta1=0.9, beta2=0.999, bc1=1.0, bc2s=1.0, visible=None,
              radii=None):
    return _lib.GsrAdamSettings(P, n_groups, beta1, beta2, bc1, bc2s, visible, radii)


def _adam(settings, groups):
    adam_step, _ = _lib.optimizer_fns(_lib.load_library())
    arr = None
    if groups is not None:
        arr = (_lib.GsrParamGroup * len(groups))(*groups)
    return adam_step(None if settings is None else ctypes.byref(settings), arr, None)


ADAM_REFUSALS = {
    "s": lambda: (None, [_group()]),
    "groups": lambda: (_settings(), None),
    "P": lambda: (_settings(P=-1), [_group()]),
    "n_groups_0": lambda: (_settings(n_groups=0), [_group()]),
    "n_groups_9": lambda: (_settings(n_groups=9), [_group()] * 9),
    "M_0": lambda: (_settings(), [_group(M=0)]),
    "M_second": lambda: (_settings(n_groups=2), [_group(), _group(M=-4)]),
    "param": lambda: (_settings(), [_group(param=None)]),
    "grad": lambda: (_settings(), [_group(grad=None)]),
    "exp_avg": lambda: (_settings(), [_group(exp_avg=None)]),
    "exp_avg_sq": lambda: (_settings(n_groups=2), [_group(), _group(exp_avg_sq=None)]),
    "beta1_1": lambda: (_settings(beta1=1.0), [_group()]),
    "beta1_neg": lambda: (_settings(beta1=-0.1), [_group()]),
    "beta1_nan": lambda: (_settings(beta1=NAN), [_group()]),
    "beta2_1": lambda: (_settings(beta2=1.0), [_group()]),
    "beta2_neg": lambda: (_settings(beta2=-1e-3), [_group()]),
    "beta2_nan": lambda: (_settings(beta2=NAN), [_group()]),
    "bc1_0": lambda: (_settings(bc1=0.0), [_group()]),
    "bc1_neg": lambda: (_settings(bc1=-1.0), [_group()]),
    "bc1_nan": lambda: (_settings(bc1=NAN), [_group()]),
    "bc2_0": lambda: (_settings(bc2s=0.0), [_group()]),
    "bc2_nan": lambda: (_settings(bc2s=NAN), [_group()]),
    "lr_nan": lambda: (_settings(), [_group(lr=NAN)]),
    "eps_nan": lambda: (_settings(n_groups=2), [_group(), _group(eps=NAN)]),
    "both_masks": lambda: (_settings(visible=FAKE, radii=FAKE), [_group()]),
}


@pytest.mark.parametrize("case", sorted(ADAM_REFUSALS))
def test_adam_step_refusals(case):
    assert _adam(*ADAM_REFUSALS[case]()) == INVALID
    assert b"gsr_adam_step" in _lib.load_library().gsr_last_error()


def test_refusals_come_before_the_empty_call():
    """P == 0 is GSR_OK with no launch (NULL buffers allowed), but only for valid settings."""
    nothing = _group(param=None, grad=None, exp_avg=None, exp_avg_sq=None)
    assert _adam(_settings(P=0), [nothing]) == 0
    assert _adam(_settings(P=0, n_groups=8, radii=FAKE), [_group(M=m) for m in range(1, 9)]) == 0
    assert _adam(_settings(P=0, beta1=1.0), [nothing]) == INVALID
    assert _adam(_settings(P=0), [_group(M=0)]) == INVALID
    assert _adam(_settings(P=0, visible=FAKE, radii=FAKE), [nothing]) == INVALID


def _densify(P=10, radii=FAKE, grad=FAKE, accum=FAKE, denom=FAKE, max_radii=FAKE):
    return _lib.GsrDensifyInputs(P, radii, grad, accum, denom, max_radii)


@pytest.mark.parametrize("case", ["in", "P", "radii", "dL_dmeans2D", "grad_accum", "denom"])
def test_densify_stats_refusals(case):
    _, stats = _lib.optimizer_fns(_lib.load_library())
    kw = {"P": dict(P=-1), "radii": dict(radii=None), "dL_dmeans2D": dict(grad=None),
          "grad_accum": dict(accum=None), "denom": dict(denom=None)}.get(case, {})
    inp = None if case == "in" else ctypes.byref(_densify(**kw))
    assert stats(inp, None) == INVALID
    assert b"gsr_densify_stats" in _lib.load_library().gsr_last_error()


def test_densify_stats_empty_call():
    _, stats = _lib.optimizer_fns(_lib.load_library())
    assert stats(ctypes.byref(_densify(P=0, radii=None, grad=None, accum=None, denom=None,
                                       max_radii=None)), None) == 0


def test_optimizer_fns_needs_the_symbols():
    class Older:
        gsr_image_loss = object()

    with pytest.raises(RuntimeError, match="no gsr_adam_step"):
        _lib.optimizer_fns(Older())
    assert {"gsr_adam_step", "gsr_densify_stats"} <= set(_lib.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("ctype, c_name", [(_lib.GsrParamGroup, "gsr_param_group"),
                                           (_lib.GsrAdamSettings, "gsr_adam_settings"),
                                           (_lib.GsrDensifyInputs, "gsr_densify_inputs")])
def test_struct_layouts_match_header(ctype, c_name, tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f for f, _ in ctype._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             f'printf("%zu\\n", sizeof({c_name}));', 'printf("%d\\n", GSR_MAX_PARAM_GROUPS);']
    lines += [f'printf("%zu\\n", offsetof({c_name}, {f}));' for f in names]
    (tmp_path / "probe.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(repo, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True)
    got = [int(v) for v in out.stdout.split()]
    assert got[0] == ctypes.sizeof(ctype) and got[1] == _lib.MAX_PARAM_GROUPS
    assert got[2:] == [getattr(ctype, f).offset for f in names]


def test_python_refusals_need_no_device():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    for bad in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="does not support " + next(iter(bad))):
            SparseGaussianAdam([{"params": [p], "lr": 1e-3}], lr=0.0, eps=1e-15, **bad)
    with pytest.raises(ValueError, match="does not support weight_decay"):
        SparseGaussianAdam([{"params": [p], "lr": 1e-3, "weight_decay": 0.5}], lr=0.0, eps=1e-15)

    def stepped(param, **kw):
        opt = SparseGaussianAdam([{"params": [param], "lr": 1e-3}], lr=0.0, eps=1e-15)
        param.grad = torch.ones_like(param)
        opt.step(**kw)
        return opt

    with pytest.raises(ValueError, match="HIP device"):
        stepped(p)
    with pytest.raises(ValueError, match="HIP device"):
        stepped(p, visibility=torch.ones(4, dtype=torch.bool), N=4)
    with pytest.raises(ValueError, match="contiguous float32"):
        stepped(torch.nn.Parameter(torch.zeros(4, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="contiguous float32"):
        stepped(torch.nn.Parameter(torch.zeros(3, 4).t()))
    q = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="one tensor per param group"):
        SparseGaussianAdam([{"params": [p, q]}], lr=1e-3, eps=1e-15).step()
    # the defaults are upstream's, the state keys torch's (nothing is created before a step)
    opt = SparseGaussianAdam([{"params": [p], "lr": 1e-3}], lr=0.0, eps=1e-15)
    assert opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.bias_correction is False
    assert isinstance(opt, torch.optim.Adam) and len(opt.state) == 0

    z = torch.zeros(4)
    with pytest.raises(ValueError, match="HIP device"):
        densification_stats(torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3), z, z.clone())
