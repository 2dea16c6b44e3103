"""CPU: what gsr_backward_abs refuses before it touches the context, in the manner of
test_backward_refusals.py: each case one fault under an otherwise valid request, the context a
buffer that is never dereferenced.  With the absolute gradient in use every message speaks as
gsr_backward_abs; without it (a NULL struct or a NULL member) the entry is gsr_backward_features,
message for message.  Also the struct's layout and the exported symbol."""
import ctypes

import pytest

from gaussiansplattingviewer_amd import _lib

PTR = 0x1000  # a device pointer's stand-in: the host never reads through it
GSR_E_INVALID = -1
BAD_STRIPS = ((-1, 2), (0, 4), (2, 2), (2, 1), (3, 0))  # of a frame with 3 tile rows


def _call(entry="gsr_backward_abs", null=(), rows=(0, 0), feat=False, det=None, abs_ptr=PTR,
          abs_struct=True, dL_dcolor=PTR, P=4):
    """(return code, message) of one request: 4 Gaussians with SHs, scales and rotations on a
    40 x 40 frame, as test_backward_refusals.py's."""
    lib = _lib.load_library()
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    g = _lib.GsrGaussians(P=P, D=0, M=1, scale_modifier=1.0, means3D=PTR, scales=PTR,
                          rotations=PTR, opacities=PTR, shs=PTR)
    st = _lib.GsrRasterSettings(image_width=40, image_height=40, tanfovx=0.5, tanfovy=0.5,
                                viewmatrix=PTR, projmatrix=PTR, campos=PTR, bg=PTR,
                                tile_row_begin=rows[0], tile_row_end=rows[1])
    inp = _lib.GsrBackwardInputs(dL_dcolor=dL_dcolor)
    out = _lib.GsrGradients(dL_dmeans3D=PTR)
    order = None if det is None else _lib.GsrBackwardOrder(deterministic=det)
    ft = _lib.GsrFeatureGradients(C=3, features=PTR, dL_dfeature_map=PTR) if feat else None
    ab = _lib.GsrAbsGradients(dL_dmeans2D_abs=abs_ptr) if abs_struct else None
    ref = lambda name, s: None if name in null or s is None else ctypes.byref(s)  # noqa: E731
    args = [None if "ctx" in null else ctx, ref("g", g), ref("st", st), ref("in", inp), None, None,
            None, ref("order", order), ref("feat", ft)]
    if entry == "gsr_backward_abs":
        args.append(ref("abs", ab))
    rc = getattr(lib, entry)(*args, ref("gr", out), None)
    return rc, lib.gsr_last_error().decode("latin-1")


def test_symbol_and_struct_layout():
    lib = _lib.load_library()
    assert "gsr_backward_abs" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "gsr_backward_abs")
    assert _lib.backward_abs_fn(lib) is not None
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4
    assert [n for n, _ in _lib.GsrAbsGradients._fields_] == ["dL_dmeans2D_abs"]
    assert ctypes.sizeof(_lib.GsrAbsGradients) == ctypes.sizeof(ctypes.c_void_p)
    assert _lib.GsrAbsGradients.dL_dmeans2D_abs.offset == 0
    assert lib.gsr_backward_abs.argtypes[-3]._type_ is _lib.GsrAbsGradients


@pytest.mark.parametrize("name", ("ctx", "g", "st", "in", "gr"))
def test_null_arguments(name):
    assert _call(null={name}) == (GSR_E_INVALID, "gsr_backward_abs: NULL argument")


def test_features_with_the_absolute_gradient():
    rc, msg = _call(feat=True)
    assert rc == GSR_E_INVALID and msg.startswith("gsr_backward_abs: ")
    assert "feature gradient" in msg and "cannot be split over passes" in msg
    # ... on a strip and in the deterministic order too (whose own refusal of features comes first,
    # under the features' name, as without the absolute gradient)
    rc, msg = _call(feat=True, rows=(1, 3))
    assert rc == GSR_E_INVALID and msg.startswith("gsr_backward_abs: ") and "passes" in msg
    assert _call(feat=True, det=1) == _call("gsr_backward_features", feat=True, det=1)


@pytest.mark.parametrize("rows", BAD_STRIPS)
def test_bad_strip(rows):
    assert _call(rows=rows) == (GSR_E_INVALID, "gsr_backward_abs: bad tile row strip")


def test_other_faults_speak_as_the_entry():
    assert _call(det=2) == (GSR_E_INVALID,
                            "gsr_backward_abs: deterministic must be 0 or 1, got 2")
    assert _call(dL_dcolor=None) == (GSR_E_INVALID, "gsr_backward_abs: dL_dcolor is required")
    assert _call(P=-1) == (GSR_E_INVALID, "gsr_backward_abs: bad P")


@pytest.mark.parametrize("kw", (dict(abs_struct=False), dict(abs_ptr=None)),
                         ids=("null_struct", "null_member"))
def test_without_the_option_it_is_gsr_backward_features(kw):
    """Every refusal above, with the option off: gsr_backward_features' code and message."""
    faults = [dict(null={n}) for n in ("ctx", "g", "st", "in", "gr")]
    faults += [dict(rows=r) for r in BAD_STRIPS]
    faults += [dict(det=2), dict(dL_dcolor=None), dict(P=-1), dict(feat=True, det=1),
               dict(rows=(1, 3), null={"gr"})]
    for f in faults:
        got, want = _call(**f, **kw), _call("gsr_backward_features", **f)
        assert got == want and got[0] == GSR_E_INVALID, (f, got, want)
        assert "gsr_backward_abs" not in got[1]
