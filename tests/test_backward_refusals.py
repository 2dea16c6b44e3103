"""CPU: what the seven backward entries (and gsr_forward_filtered, gsr_forward_features) refuse
before they touch the context, as (return code, gsr_last_error()) pairs held byte for byte against
tests/golden/backward_refusals.json.

The fixture was recorded from the library of the commit before the backward's entries were folded
into one request (`PYTHONPATH=. GSR_LIB=<that build's libgsr.so> python
tests/test_backward_refusals.py --record`); a build of the tree must reproduce it, the entry name of every message included.

Every case is one fault, or two applied in order, under one variant of an otherwise valid
request.  The context is a buffer that is never dereferenced: each case holds a fault that the
entry refuses before it locks the context, and nothing a second fault or a variant adds makes the
first one acceptable (a feature gradient makes a missing dL_dcolor acceptable: that pair is left
out)."""
import ctypes
import itertools
import json
import os
import sys

from gaussiansplattingviewer_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "backward_refusals.json")
PTR = 0x1000  # a device pointer's stand-in: the host never reads through it

# entry -> the optional structs it takes, in order, between its inputs and its gradients / stream
BACKWARD = {
    "gsr_backward": (),
    "gsr_backward_planes": ("planes",),
    "gsr_backward_camera": ("planes", "camera"),
    "gsr_backward_filtered": ("planes", "camera", "filter"),
    "gsr_backward_ordered": ("planes", "camera", "filter", "order"),
    "gsr_backward_strip": ("planes", "camera", "filter", "order"),
    "gsr_backward_features": ("planes", "camera", "filter", "order", "feat"),
}
FORWARD = {
    "gsr_forward_filtered": ("depth", "surface", "filter"),
    "gsr_forward_features": ("depth", "surface", "filter", "feat"),
}
TAKES_STRIP = ("gsr_backward_strip", "gsr_backward_features")
BAD_STRIPS = ((-1, 2), (0, 4), (2, 2), (2, 1), (3, 0))  # of a frame with 3 tile rows


def _request():
    """A valid request: 4 Gaussians with SHs, scales and rotations on a 40 x 40 frame."""
    return dict(null=set(), P=4, W=40, rows=(0, 0), shs=PTR, colors=None, scales=PTR,
                rotations=PTR, cov=None, dL_dcolor=PTR, planes=None, aa=None, det=None,
                feat=False, C=3, features=PTR)


def _set(**kw):
    return lambda r: r.update(kw)


def _null(name):
    return lambda r: r["null"].add(name)


def _feat(**kw):
    return lambda r: r.update(feat=True, **kw)


# fault -> (the struct an entry must take for it, or None; what it does to the request)
FAULTS = {
    **{f"null_{n}": (None, _null(n)) for n in ("ctx", "g", "st", "in", "gr")},
    "strip_refused": ("no strip", _set(rows=(1, 3))),
    **{f"bad_strip_{b}_{e}": (None, _set(rows=(b, e))) for b, e in BAD_STRIPS},
    "antialiasing_2": ("filter", _set(aa=2)),
    "deterministic_2": ("order", _set(det=2)),
    "deterministic_1_features": ("feat", _feat(det=1)),
    "C_0": ("feat", _feat(C=0)),
    "C_257": ("feat", _feat(C=257)),
    "features_null": ("feat", _feat(features=None)),
    "no_color_planes": ("planes", _set(dL_dcolor=None, planes="empty")),
    "no_color": (None, _set(dL_dcolor=None)),
    "sh_and_colors": (None, _set(shs=PTR, colors=PTR)),
    "no_sh_no_colors": (None, _set(shs=None, colors=None)),
    "cov_both": (None, _set(scales=PTR, cov=PTR)),
    "cov_neither": (None, _set(scales=None, cov=None)),
    "P_negative": (None, _set(P=-1)),
    "width_0": (None, _set(W=0)),
}
# the forwards check the scene under the context's lock: only these are refused before it
FORWARD_FAULTS = ("null_ctx", "null_g", "null_st", "null_gr", "antialiasing_2", "C_0", "C_257",
                  "features_null")
# variant -> (the struct an entry must take for it, what it does to the request)
VARIANTS = {
    "plain": (None, lambda r: None),
    "antialiasing": ("filter", _set(aa=1)),
    "deterministic": ("order", _set(det=1)),
    "strip": ("strip", _set(rows=(1, 3))),
    "features": ("feat", _feat()),
}


def _applies(entry, structs, needs):
    if needs is None:
        return True
    if needs == "no strip":
        return entry in BACKWARD and entry not in TAKES_STRIP
    if needs == "strip":
        return entry in TAKES_STRIP
    return needs in structs


def cases():
    """(key, entry, the request's mutations in order) of every case."""
    for entry, structs in {**BACKWARD, **FORWARD}.items():
        faults = [f for f, (needs, _) in FAULTS.items() if _applies(entry, structs, needs)
                  and (entry in BACKWARD or f in FORWARD_FAULTS)]
        for variant, (needs, vary) in VARIANTS.items():
            if not _applies(entry, structs, needs) or (entry in FORWARD and needs == "order"):
                continue
            for f in faults:
                if variant == "features" and f.startswith("no_color"):
                    continue  # a valid request: the feature gradient alone
                yield f"{entry}|{variant}|{f}", entry, (vary, FAULTS[f][1])
        for a, b in itertools.permutations(faults, 2):
            yield f"{entry}|plain|{a}+{b}", entry, (FAULTS[a][1], FAULTS[b][1])


def call(lib, ctx, entry, mutations):
    """(return code, message) of one case."""
    r = _request()
    for m in mutations:
        m(r)
    ref = lambda name, s: None if name in r["null"] else ctypes.byref(s)  # noqa: E731
    g = _lib.GsrGaussians(P=r["P"], D=0, M=1, scale_modifier=1.0, means3D=PTR, scales=r["scales"],
                          rotations=r["rotations"], opacities=PTR, shs=r["shs"],
                          colors_precomp=r["colors"], cov3D_precomp=r["cov"])
    st = _lib.GsrRasterSettings(image_width=r["W"], image_height=40, tanfovx=0.5, tanfovy=0.5,
                                viewmatrix=PTR, projmatrix=PTR, campos=PTR, bg=PTR,
                                tile_row_begin=r["rows"][0], tile_row_end=r["rows"][1])
    optional = {
        "planes": _lib.GsrPlaneGradients() if r["planes"] else None,
        "camera": None, "depth": None, "surface": None,
        "filter": None if r["aa"] is None else _lib.GsrFilterSettings(antialiasing=r["aa"]),
        "order": None if r["det"] is None else _lib.GsrBackwardOrder(deterministic=r["det"]),
    }
    backward = entry in BACKWARD
    if backward:
        first = _lib.GsrBackwardInputs(dL_dcolor=r["dL_dcolor"])
        last = _lib.GsrGradients(dL_dmeans3D=PTR)
        optional["feat"] = _lib.GsrFeatureGradients(
            C=r["C"], features=r["features"], dL_dfeature_map=PTR) if r["feat"] else None
    else:
        first = _lib.GsrOutputs(color=PTR, radii=PTR)
        optional["feat"] = _lib.GsrFeatureOutputs(
            C=r["C"], features=r["features"], feature_map=PTR) if r["feat"] else None
    structs = (BACKWARD if backward else FORWARD)[entry]
    args = [None if "ctx" in r["null"] else ctx, ref("g", g), ref("st", st)]
    if backward:
        args.append(ref("in", first))
    else:
        args.append(ref("gr", first))  # (gsr_outputs, the forward's fourth required pointer)
    args += [None if optional[s] is None else ctypes.byref(optional[s]) for s in structs]
    if backward:
        args.append(ref("gr", last))
    rc = getattr(lib, entry)(*args, None)
    return rc, lib.gsr_last_error().decode("latin-1")


def run_all(lib):
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    return {key: call(lib, ctx, entry, mutations) for key, entry, mutations in cases()}


def test_every_fault_meets_every_entry():
    keys = [k for k, _, _ in cases()]
    assert len(keys) == len(set(keys))
    for entry in BACKWARD:
        for n in ("ctx", "g", "st", "in", "gr"):
            assert f"{entry}|plain|null_{n}" in keys
        for f in ("no_color", "sh_and_colors", "no_sh_no_colors", "cov_both", "cov_neither",
                  "P_negative", "width_0", *(f"bad_strip_{b}_{e}" for b, e in BAD_STRIPS)):
            assert f"{entry}|plain|{f}" in keys
    assert "gsr_backward_strip|plain|strip_refused" not in keys
    assert "gsr_backward_ordered|deterministic|strip_refused" in keys
    assert "gsr_backward_features|plain|deterministic_1_features" in keys
    assert "gsr_forward_features|antialiasing|C_257" in keys


def test_refusals_match_the_recorded_ones():
    """Every (return code, message) is the fixture's, byte for byte."""
    with open(FIXTURE) as f:
        fixture = json.load(f)
    want = {k: tuple(fixture["messages"][i]) for k, i in fixture["cases"].items()}
    got = run_all(_lib.load_library())
    assert set(got) == set(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(got)} differ, e.g. {sorted(wrong.items())[:5]}"
    assert all(rc < 0 for rc, _ in got.values())


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: PYTHONPATH=. GSR_LIB=<libgsr.so to record from> python tests/test_backward_refusals.py "
                 "--record")
    got = run_all(_lib.load_library())
    assert all(rc < 0 for rc, _ in got.values()), [k for k, v in got.items() if v[0] >= 0]
    messages = sorted(set(got.values()))
    with open(FIXTURE, "w") as f:
        json.dump({"messages": messages,
                   "cases": {k: messages.index(v) for k, v in sorted(got.items())}}, f, indent=0)
        f.write("\n")
    print(f"{len(got)} cases, {len(messages)} distinct refusals from {_lib.LIB_PATH}")
