"""CPU: save_ply / load_scene_ply on host memory (csrc/ply_writer.hip, device == 0) against the
file's specification restated in numpy (ply_scene_reference.py) and the independent PLY reader
and writer (oracle/ply_oracle.py).  Every comparison is bit for bit: the feature copies words."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ply_oracle
import ply_scene_reference as ref
from gaussiansplattingviewer_amd import _lib, ply
from gaussiansplattingviewer_amd import load_scene_ply, save_ply

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr.h")
INVALID = -1   # GSR_E_INVALID
FAKE = 0x1000  # a non-NULL pointer nothing dereferences: every call it is passed to is refused


# ---- 1. the file's bytes ------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_rows", [None, 1, 100, 256])
@pytest.mark.parametrize("P", [0, 1, 2, 257])
@pytest.mark.parametrize("M", ref.COEFFS)
def test_file_bytes(M, P, chunk_rows, tmp_path):
    sc = ref.copies(ref.scene(P, M))
    path = tmp_path / "scene.ply"
    assert save_ply(path, sc, chunk_rows=chunk_rows) == P
    assert path.read_bytes() == ref.file_bytes(ref.scene(P, M))
    ref.assert_same_scene(sc, ref.scene(P, M), "the scene is only read")
    got = ply_oracle.read_vertex(path)
    want = ref.properties(ref.scene(P, M))
    assert list(got) == list(want)
    for name in want:
        assert got[name].dtype == np.float32
        assert np.array_equal(got[name].view(np.int32), want[name].view(np.int32)), name
    assert os.listdir(tmp_path) == ["scene.ply"]


def test_torch_host_tensors_parameters_and_an_optimizer(tmp_path):
    sc = ref.scene(57, 9)
    want = ref.file_bytes(sc)
    tensors = {k: torch.from_numpy(v.copy()) for k, v in sc.items()}
    save_ply(tmp_path / "t.ply", tensors)
    assert (tmp_path / "t.ply").read_bytes() == want
    params = {k: torch.nn.Parameter(t) for k, t in tensors.items()}
    save_ply(tmp_path / "p.ply", params)
    assert (tmp_path / "p.ply").read_bytes() == want
    # an optimizer: the groups are found by name, in any order, beside groups with other names
    groups = [{"params": [params[k]], "name": k} for k in reversed(ref.NAMES)]
    groups.append({"params": [torch.nn.Parameter(torch.zeros(3))], "name": "exposure"})
    opt = torch.optim.Adam(groups, lr=1e-3)
    assert save_ply(tmp_path / "o.ply", opt) == 57
    assert (tmp_path / "o.ply").read_bytes() == want


def test_degree_0_without_f_rest(tmp_path):
    sc = ref.scene(5, 1)
    without = {k: v.copy() for k, v in sc.items() if k != "f_rest"}
    save_ply(tmp_path / "a.ply", without)
    assert (tmp_path / "a.ply").read_bytes() == ref.file_bytes(sc)


# ---- 2. padding to a higher degree --------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:invalid value")  # the oracle's arithmetic on NaN words
@pytest.mark.parametrize("M", [1, 4, 9])
def test_padded_file_is_what_load_ply_accepts(M, tmp_path):
    sc = ref.scene(257, M, signalling=False)  # (ply_scene_reference.SIGNALLING_NAN)
    path = tmp_path / "padded.ply"
    save_ply(path, ref.copies(sc), sh_degree=3, chunk_rows=100)
    assert path.read_bytes() == ref.file_bytes(sc, 16)
    g, _, _ = ply.load_ply(str(path))
    xyz, _, _, _, sh, _, _ = ply_oracle.load_ply_reference(path)
    assert np.array_equal(ref.bits(g.xyz), ref.bits(xyz))
    assert np.array_equal(ref.bits(g.sh), ref.bits(sh))
    el = ply_oracle.read_vertex(path)
    for c in range(3):
        for j in range(M - 1, 15):
            assert not el[f"f_rest_{c * 15 + j}"].view(np.uint32).any(), (c, j)  # +0.0 bits
        for j in range(M - 1):
            assert np.array_equal(ref.bits(el[f"f_rest_{c * 15 + j}"]),
                                  ref.bits(sc["f_rest"][:, j, c]))
    back = load_scene_ply(path)
    assert back["f_rest"].shape == (257, 15, 3)
    assert np.array_equal(ref.bits(back["f_rest"][:, :M - 1]), ref.bits(sc["f_rest"]))
    assert not ref.bits(back["f_rest"][:, M - 1:]).any()


def test_padding_to_degree_4(tmp_path):
    sc = ref.scene(3, 16)
    save_ply(tmp_path / "p.ply", ref.copies(sc), sh_degree=4)
    assert (tmp_path / "p.ply").read_bytes() == ref.file_bytes(sc, 25)


# ---- 3. round trips -----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 1, 257])
@pytest.mark.parametrize("M", ref.COEFFS)
def test_round_trip(M, P, tmp_path):
    sc = ref.scene(P, M)
    path = tmp_path / "scene.ply"
    save_ply(path, ref.copies(sc), chunk_rows=100)
    back = load_scene_ply(path)
    ref.assert_same_scene(back, sc)
    assert {k: v.shape for k, v in back.items()} == ref.shapes(P, M)


@pytest.mark.parametrize("M", [1, 9, 16])
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_load_scene_of_foreign_files(name, M, tmp_path):
    path, values = ref.fixture(name, M, tmp_path)
    got = load_scene_ply(path)
    ref.assert_same_scene(got, ref.scene_of_properties(values, M), name)
    # and of the file as the independent reader sees it
    ref.assert_same_scene(got, ref.scene_of_properties(ply_oracle.read_vertex(path), M), name)


# ---- 4. a failure leaves nothing ---------------------------------------------------------------
def test_missing_directory(tmp_path):
    sc = ref.copies(ref.scene(3, 4))
    with pytest.raises(RuntimeError, match="cannot create"):
        save_ply(tmp_path / "nowhere" / "scene.ply", sc)
    ref.assert_same_scene(sc, ref.scene(3, 4))
    assert os.listdir(tmp_path) == []
    with pytest.raises(RuntimeError, match="cannot open"):
        load_scene_ply(tmp_path / "nowhere" / "scene.ply")


def test_failed_save_keeps_the_file_that_was_there(tmp_path):
    d = tmp_path / "d"
    d.mkdir()
    path = d / "scene.ply"
    save_ply(path, ref.copies(ref.scene(5, 4)))
    before = path.read_bytes()
    os.chmod(d, 0o555)
    try:
        if os.access(d, os.W_OK):
            # a user whom directory permissions do not bind (root): the save below would succeed
            pytest.skip("this user can write into a read-only directory")
        sc = ref.copies(ref.scene(7, 9))
        with pytest.raises(RuntimeError, match="cannot create"):
            save_ply(path, sc)
        ref.assert_same_scene(sc, ref.scene(7, 9))
        assert path.read_bytes() == before
        assert os.listdir(d) == ["scene.ply"] and not glob.glob(str(d / "*.tmp.*"))
    finally:
        os.chmod(d, 0o755)


def test_short_write_keeps_the_file_that_was_there(tmp_path):
    """A write that the file size limit cuts short (the kernel writes up to the limit, then refuses
    with EFBIG; Python ignores SIGXFSZ): binds every user, root too."""
    import resource
    path = tmp_path / "scene.ply"
    save_ply(path, ref.copies(ref.scene(5, 4)))
    before = path.read_bytes()
    sc = ref.copies(ref.scene(257, 16))
    soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
    resource.setrlimit(resource.RLIMIT_FSIZE, (30000, hard))  # header, one chunk and a bit
    try:
        with pytest.raises(RuntimeError, match="short write"):
            save_ply(path, sc, chunk_rows=100)
    finally:
        resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))
    ref.assert_same_scene(sc, ref.scene(257, 16))
    assert path.read_bytes() == before
    assert os.listdir(tmp_path) == ["scene.ply"]


def test_save_replaces_a_file_only_when_complete(tmp_path):
    path = tmp_path / "scene.ply"
    save_ply(path, ref.copies(ref.scene(5, 4)))
    save_ply(path, ref.copies(ref.scene(9, 16)))
    assert path.read_bytes() == ref.file_bytes(ref.scene(9, 16))
    assert os.listdir(tmp_path) == ["scene.ply"]


# ---- 5. refusals --------------------------------------------------------------------------------
def _bad(**changes):
    sc = ref.copies(ref.scene(6, 4))
    sc.update(changes)
    return sc


VALUE_ERRORS = {
    "missing": (lambda: {k: v for k, v in _bad().items() if k != "opacity"}, "no 'opacity'"),
    "float64": (lambda: _bad(xyz=np.zeros((6, 3))), "contiguous float32"),
    "not_contiguous": (lambda: _bad(xyz=np.zeros((6, 6), np.float32)[:, ::2]), "contiguous float32"),
    "shape": (lambda: _bad(rotation=np.zeros((6, 3), np.float32)), r"expected \(P, 4\)"),
    "f_dc_shape": (lambda: _bad(f_dc=np.zeros((6, 3), np.float32)), r"expected \(P, 1, 3\)"),
    "f_rest_shape": (lambda: _bad(f_rest=np.zeros((6, 9), np.float32)), r"expected \(P, M - 1, 3\)"),
    "rows": (lambda: _bad(scaling=np.zeros((5, 3), np.float32)), "5 rows"),
    "not_square": (lambda: _bad(f_rest=np.zeros((6, 4, 3), np.float32)), "M = 5 is not"),
    "mixed_kinds": (lambda: _bad(xyz="xyz"), "numpy array or a torch tensor"),
    "not_a_scene": (lambda: [1, 2, 3], "scene dict"),
}


@pytest.mark.parametrize("case", sorted(VALUE_ERRORS))
def test_value_errors(case, tmp_path):
    make, message = VALUE_ERRORS[case]
    with pytest.raises(ValueError, match=message):
        save_ply(tmp_path / "x.ply", make())
    assert os.listdir(tmp_path) == []


def test_value_errors_of_the_degree_and_the_optimizer(tmp_path):
    with pytest.raises(ValueError, match="below the scene's"):
        save_ply(tmp_path / "x.ply", ref.copies(ref.scene(6, 9)), sh_degree=1)
    with pytest.raises(ValueError, match="not in 0..4"):
        save_ply(tmp_path / "x.ply", ref.copies(ref.scene(6, 9)), sh_degree=5)
    params = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in ref.scene(6, 4).items()}
    groups = [{"params": [params[k]], "name": k} for k in ref.NAMES]
    twice = groups + [{"params": [torch.nn.Parameter(torch.zeros(6, 3))], "name": "xyz"}]
    with pytest.raises(ValueError, match="two param groups are named 'xyz'"):
        save_ply(tmp_path / "x.ply", torch.optim.Adam(twice, lr=1e-3))
    with pytest.raises(ValueError, match="no 'rotation'"):
        save_ply(tmp_path / "x.ply", torch.optim.Adam(groups[:-1], lr=1e-3))
    with pytest.raises(ValueError, match="HIP device"):
        load_scene_ply(tmp_path / "x.ply", device="cpu")
    assert os.listdir(tmp_path) == []


def test_mixed_devices_are_refused():
    sc = {k: torch.from_numpy(v.copy()) for k, v in ref.scene(6, 4).items()}
    sc["xyz"] = torch.empty((6, 3), dtype=torch.float32, device="meta")
    with pytest.raises(ValueError, match="HIP device or the CPU"):
        save_ply("unused.ply", sc)
    sc["xyz"] = np.zeros((6, 3), np.float32)  # numpy beside host tensors: one kind of memory
    assert ply._checked_scene(sc)[3] is None


def _c_scene(**kw):
    fields = dict(P=10, sh_coeffs=4, file_sh_coeffs=0, chunk_rows=0, xyz=FAKE, f_dc=FAKE,
                  f_rest=FAKE, opacity=FAKE, scaling=FAKE, rotation=FAKE)
    fields.update(kw)
    return _lib.GsrPlyScene(**fields)


# (what the scene is, the words the message must hold, whether gsr_ply_load_scene refuses it too)
REFUSALS = {
    "P_negative": (dict(P=-1), b"P < 0", True),
    "P_2_30": (dict(P=2 ** 30), b"P >= 2^30", True),
    "M_0": (dict(sh_coeffs=0), b"sh_coeffs 0", True),
    "M_5": (dict(sh_coeffs=5), b"sh_coeffs 5", True),
    "M_36": (dict(sh_coeffs=36), b"sh_coeffs 36", True),
    "Mo_12": (dict(file_sh_coeffs=12), b"file_sh_coeffs 12", False),
    "Mo_below_M": (dict(sh_coeffs=9, file_sh_coeffs=4), b"file_sh_coeffs 4 < sh_coeffs 9", False),
    "chunk_rows": (dict(chunk_rows=-1), b"chunk_rows < 0", True),
    "xyz": (dict(xyz=None), b"NULL tensor", True),
    "f_dc": (dict(f_dc=None), b"NULL tensor", True),
    "f_rest": (dict(f_rest=None), b"NULL f_rest", True),
    "opacity": (dict(opacity=None), b"NULL tensor", True),
    "scaling": (dict(scaling=None), b"NULL tensor", True),
    "rotation": (dict(rotation=None), b"NULL tensor", True),
}


@pytest.mark.parametrize("device", [0, 1])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_come_before_any_hip_call_and_before_the_file(case, device, tmp_path):
    """With device = 1 and pointers nothing may dereference, on a machine without a GPU: a call
    that reached HIP or the tensors would not come back with GSR_E_INVALID and this message."""
    lib = _lib.load_library()
    save, _, load = _lib.ply_scene_fns(lib)
    fields, words, load_too = REFUSALS[case]
    path = tmp_path / "scene.ply"
    assert lib.gsr_forward(None, None, None, None, None) < 0  # another entry's message
    assert save(os.fsencode(path), ctypes.byref(_c_scene(**fields)), device, None) == INVALID
    message = lib.gsr_last_error()
    assert b"gsr_ply_save" in message and words in message, message
    assert os.listdir(tmp_path) == []
    if load_too:
        assert lib.gsr_forward(None, None, None, None, None) < 0
        # (the path does not exist: the refusal comes before the file is opened)
        assert load(os.fsencode(path), ctypes.byref(_c_scene(**fields)), device, None) == INVALID
        message = lib.gsr_last_error()
        assert b"gsr_ply_load_scene" in message and words in message, message


def test_null_path_and_scene(tmp_path):
    lib = _lib.load_library()
    save, probe, load = _lib.ply_scene_fns(lib)
    sc = _c_scene()
    for device in (0, 1):
        assert save(None, ctypes.byref(sc), device, None) == INVALID
        assert b"gsr_ply_save: NULL path" in lib.gsr_last_error()
        assert save(b"x.ply", None, device, None) == INVALID
        assert b"gsr_ply_save: NULL scene" in lib.gsr_last_error()
        assert load(None, ctypes.byref(sc), device, None) == INVALID
        assert b"gsr_ply_load_scene: NULL path" in lib.gsr_last_error()
        assert load(b"x.ply", None, device, None) == INVALID
        assert b"gsr_ply_load_scene: NULL scene" in lib.gsr_last_error()
    assert probe(None, ctypes.byref(sc)) == INVALID and probe(b"x.ply", None) == INVALID
    assert b"gsr_ply_probe_scene: NULL argument" in lib.gsr_last_error()


def test_file_errors(tmp_path):
    lib = _lib.load_library()
    _, probe, load = _lib.ply_scene_fns(lib)
    good = tmp_path / "good.ply"
    save_ply(good, ref.copies(ref.scene(20, 4)))
    data = good.read_bytes()
    # a short file
    (tmp_path / "short.ply").write_bytes(data[:-5])
    with pytest.raises(RuntimeError, match="shorter than its vertex data"):
        load_scene_ply(tmp_path / "short.ply")
    # an f_rest count that is no 3 (M - 1)
    values = ref.properties(ref.scene(4, 4))
    del values["f_rest_8"]
    ply_oracle.write_ply(tmp_path / "rest.ply", values)
    with pytest.raises(RuntimeError, match=r"3 \(M - 1\) f_rest_\* properties.*found 8"):
        load_scene_ply(tmp_path / "rest.ply")
    # the probe's P and sh_coeffs are the only ones the load takes
    info = _lib.GsrPlyScene()
    assert probe(os.fsencode(good), ctypes.byref(info)) == 0
    assert (info.P, info.sh_coeffs) == (20, 4)
    out = {k: np.full(s, 7.0, np.float32) for k, s in ref.shapes(20, 4).items()}
    for wrong in (dict(P=19), dict(sh_coeffs=9), dict(sh_coeffs=1)):
        sc = ply._c_scene(out, 20, 4)
        for k, v in wrong.items():
            setattr(sc, k, v)
        assert load(os.fsencode(good), ctypes.byref(sc), 0, None) == INVALID
        assert b"are not the file's (20, 4)" in lib.gsr_last_error()
    assert all((v == 7.0).all() for v in out.values())  # nothing written


def test_the_entries_are_declared_exported_and_bound():
    lib = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = ("gsr_ply_save", "gsr_ply_probe_scene", "gsr_ply_load_scene")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
    fns = _lib.ply_scene_fns(lib)
    assert fns == tuple(getattr(lib, n) for n in names)
    assert [len(f.argtypes) for f in fns] == [4, 2, 4]
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4  # additive

    class Older:
        gsr_ply_load = object()

    with pytest.raises(RuntimeError, match="no gsr_ply_save"):
        _lib.ply_scene_fns(Older())


def test_struct_layout_matches_header(tmp_path):
    """gsr_ply_scene against include/gsr.h, with the gcc probe test_abi_host.py uses."""
    fields = [f for f, _ in _lib.GsrPlyScene._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsr_ply_scene));']
    lines += [f'printf("{f} %zu\\n", offsetof(gsr_ply_scene, {f}));' for f in fields]
    lines.append("return 0;}")
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(probe), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {l.split()[0]: int(l.split()[1]) for l in out.splitlines() if l}
    assert got.pop("size") == ctypes.sizeof(_lib.GsrPlyScene) == 72
    assert got == {f: getattr(_lib.GsrPlyScene, f).offset for f in fields}
    assert fields == ["P", "sh_coeffs", "file_sh_coeffs", "chunk_rows", "xyz", "f_dc", "f_rest",
                      "opacity", "scaling", "rotation"]
