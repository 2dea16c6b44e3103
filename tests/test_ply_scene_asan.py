"""CPU: the scene writer's and reader's host code (csrc/ply_writer.hip with csrc/ply_loader.hip)
under AddressSanitizer and UndefinedBehaviorSanitizer.

Host code only: the two sources are built a second time with `-Xarch_host
-fsanitize=address,undefined` into a stand-alone program (tools/asan/ply_scene_driver.cpp, its own
main, no Python and no preloaded runtime) that saves a scene of P = 257 rows and M = 16
coefficients in chunks of 100 rows from exactly-sized heap arrays, loads it back into
exactly-sized arrays and compares the words (also: padded to degree 4, degree 0 without f_rest,
an empty scene, two refused calls).  device == 0 makes no HIP call, so no GPU is needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(REPO, "gaussiansplattingviewer_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asan") / "ply_scene"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "include"), os.path.join(CSRC, "ply_writer.hip"),
           os.path.join(CSRC, "ply_loader.hip"),
           os.path.join(REPO, "tools", "asan", "ply_scene_driver.cpp"), "-o", str(out), "-lpthread"]
    subprocess.run(cmd, check=True, capture_output=True)
    return str(out)


def test_scene_writer_and_reader_under_asan_and_ubsan(driver, tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 5 and all(l.startswith("ok ") for l in lines), r.stdout
    assert os.listdir(tmp_path) == ["scene.ply"]
