"""TEST INFRASTRUCTURE -- the scene file's specification restated in numpy (include/gsr.h "Scene
files"): a seeded raw scene, the column table and the header bytes.  Shared by
test_ply_scene_host.py and test_gpu_ply_scene.py; never imported by the product path.

Every comparison made with these is bit for bit: the writer and the raw reader copy words."""
from __future__ import annotations

import functools

import numpy as np

import ply_oracle

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
COEFFS = (1, 4, 9, 16, 25)

# Words a bit copy must keep and an arithmetic detour would not: a quiet and a signalling NaN with
# payloads, a negative NaN, both infinities, -0.0, the smallest and the largest denormal.
SPECIAL_BITS = np.array([0x7FC12345, 0x7F800001, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000,
                         0x00000001, 0x807FFFFF], dtype=np.uint32)


# The activated reader (load_ply) takes every float property through float64, as the reference's
# arithmetic does; that quiets a signalling NaN, which numpy's float32 xyz keeps.  The writer and
# the raw reader are held to it; a file meant for load_ply is made without it.
SIGNALLING_NAN = 0x7F800001


def row_words(M: int) -> int:
    """R: float32 words per file row for a file of M coefficients."""
    return 17 + 3 * (M - 1)


def shapes(P: int, M: int) -> dict:
    return {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, M - 1, 3), "opacity": (P, 1),
            "scaling": (P, 3), "rotation": (P, 4)}


@functools.lru_cache(maxsize=None)
def _scene(P: int, M: int, seed: int, special: bool, signalling: bool):
    rng = np.random.default_rng([seed, P, M])
    out = {}
    for name, shape in shapes(P, M).items():
        a = rng.normal(0.0, 1.5, shape).astype(np.float32)
        if special and a.size:
            w = a.reshape(-1).view(np.uint32)
            at = rng.choice(a.size, size=min(a.size, len(SPECIAL_BITS)), replace=False)
            w[at] = SPECIAL_BITS[:len(at)]
            if not signalling:
                w[w == SIGNALLING_NAN] = 0x7FC00001
        a.setflags(write=False)
        out[name] = a
    return out


def scene(P: int, M: int, seed: int = 0, special: bool = True, signalling: bool = True) -> dict:
    """A raw scene of P rows and M coefficients as numpy float32 arrays (read-only, cached: copy
    before handing one to code that might write).  special: some words of every tensor are
    SPECIAL_BITS; signalling=False: the signalling NaN among them is a quiet one with the same
    payload (for files that go through the activated reader, below)."""
    return dict(_scene(P, M, seed, special, signalling))


def copies(sc: dict) -> dict:
    return {k: v.copy() for k, v in sc.items()}


def rows(sc: dict, Mo: int | None = None) -> np.ndarray:
    """The file body, float32 [P, R]: the column table of include/gsr.h, in words."""
    P = sc["xyz"].shape[0]
    M = sc["f_rest"].shape[1] + 1
    Mo = M if Mo is None else Mo
    assert Mo >= M
    out = np.zeros((P, row_words(Mo)), np.uint32)  # +0.0: the normals and the padding
    w = {k: np.ascontiguousarray(v).view(np.uint32) for k, v in sc.items()}
    out[:, 0:3] = w["xyz"]
    out[:, 6:9] = w["f_dc"][:, 0, :]
    for c in range(3):
        for j in range(M - 1):
            out[:, 9 + c * (Mo - 1) + j] = w["f_rest"][:, j, c]
    at = 9 + 3 * (Mo - 1)
    out[:, at] = w["opacity"][:, 0]
    out[:, at + 1:at + 4] = w["scaling"]
    out[:, at + 4:at + 8] = w["rotation"]
    return out.view(np.float32)


def property_names(Mo: int) -> list:
    return (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
            + [f"f_rest_{i}" for i in range(3 * (Mo - 1))]
            + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])


def header(P: int, Mo: int) -> bytes:
    """What plyfile writes for upstream's save_ply: no comment, '\\n' line ends."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {P}"]
    lines += [f"property float {n}" for n in property_names(Mo)] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def file_bytes(sc: dict, Mo: int | None = None) -> bytes:
    M = sc["f_rest"].shape[1] + 1
    return header(sc["xyz"].shape[0], M if Mo is None else Mo) + rows(sc, Mo).tobytes()


def properties(sc: dict, Mo: int | None = None) -> dict:
    """{property name: float32 [P]} of the file: what a PLY reader returns, and what
    ply_oracle.write_ply takes."""
    M = sc["f_rest"].shape[1] + 1
    body = rows(sc, Mo)
    return {n: body[:, i].copy() for i, n in enumerate(property_names(M if Mo is None else Mo))}


def scene_of_properties(values: dict, M: int) -> dict:
    """The inverse of the column table on {property name: array of any dtype}: the raw scene as
    astype(float32) of the values."""
    f = {k: np.asarray(v).astype(np.float32) for k, v in values.items()}
    P = len(f["x"])
    rest = np.zeros((P, M - 1, 3), np.float32)
    for c in range(3):
        for j in range(M - 1):
            rest[:, j, c] = f[f"f_rest_{c * (M - 1) + j}"]
    return {"xyz": np.stack([f["x"], f["y"], f["z"]], axis=1),
            "f_dc": np.stack([f["f_dc_0"], f["f_dc_1"], f["f_dc_2"]], axis=1)[:, None, :],
            "f_rest": rest, "opacity": f["opacity"][:, None],
            "scaling": np.stack([f[f"scale_{i}"] for i in range(3)], axis=1),
            "rotation": np.stack([f[f"rot_{i}"] for i in range(4)], axis=1)}


def fixture(name, M, tmp_path, P=41):
    """(path, the values written): a file of ply_oracle.write_ply from a scene's properties."""
    finite = name in ("ascii", "doubles", "mixed")  # text and float64 detours: no NaN payloads
    values = properties(scene(P, M, seed=7, special=not finite))
    kw = {}
    if name == "big_endian":
        kw["fmt"] = "binary_big_endian"
    elif name == "ascii":
        kw["fmt"] = "ascii"
    elif name == "shuffled":
        order = list(values)
        np.random.default_rng(3).shuffle(order)
        kw["order"] = order
    elif name == "doubles":
        rng = np.random.default_rng(5)
        for n in "xyz":  # values float32 cannot hold: the cast must round them
            values[n] = values[n].astype(np.float64) + rng.normal(0, 1e-9, P)
        kw["types"] = {"x": "double", "y": "double", "z": "double"}
    elif name == "extra_uchar":
        values = dict(values, label=(np.arange(P) % 251).astype(np.uint8))
        order = list(values)
        order.insert(4, order.pop())  # in the middle of the row: the stride is odd
        kw["order"] = order
        kw["types"] = {"label": "uchar"}
    elif name == "no_normals":
        values = {k: v for k, v in values.items() if k not in ("nx", "ny", "nz")}
    elif name == "mixed":
        values["opacity"] = np.arange(P, dtype=np.int16) - 20
        values["scale_1"] = (np.arange(P) % 251).astype(np.uint8)
        values["rot_0"] = (np.arange(P, dtype=np.int32) - 7) * 100003
        values["f_dc_1"] = values["f_dc_1"].astype(np.float64) * (1 + 1e-10)
        kw["types"] = {"opacity": "short", "scale_1": "uchar", "rot_0": "int", "f_dc_1": "double"}
        kw["fmt"] = "binary_big_endian"
    else:
        raise KeyError(name)
    path = tmp_path / f"{name}.ply"
    ply_oracle.write_ply(path, values, **kw)
    return path, values


FIXTURES = ("big_endian", "ascii", "shuffled", "doubles", "extra_uchar", "no_normals", "mixed")


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_scene(got: dict, want: dict, what=""):
    assert set(got) == set(want) == set(NAMES), (what, sorted(got))
    for k in NAMES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, k)
