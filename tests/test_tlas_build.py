"""The per-instance and per-node code of prt_rebuild_instances on the CPU (tests/cpp/tlas_build_check.cpp over
physically-based-ray-tracer_amd/csrc/prt_tlas_build.h, what the two device kernels run, and bvh_build.cpp's host
collapse, which emits the device builder's output format): the fat records' three-vertex bounds are the boxes bit for
bit -- random boxes, identical boxes, boxes at 1e6 scale, boxes without extent -- and the finish function makes of
build_blas8(fat, n, 1) a tree in build_tlas8's form whose bytes the refit of prt_update_instances reproduces; the same
under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program; the new entry point without a device.
The GPU side: tests/test_gpu_instance_rebuild.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import prt
from prt import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-ray-tracer_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "tlas_build_check.cpp"), os.path.join(CSRC, "bvh_build.cpp")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:halt_on_error=1:detect_leaks=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
COUNTS = [1, 2, 3, 9, 71, 301, 5000]
EXTENT = 40.0


def build_checker(exe, extra=("-O2",)):
    """tests/cpp/tlas_build_check.cpp, without FMA contraction as the library is built."""
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, *SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def run_checker(exe, *args, env=None):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=env)
    assert r.stdout.strip(), r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and out["ok"], (out, r.stderr[-2000:])
    return out


def random_boxes(n, seed, centre=0.0):
    """n boxes {lo, hi} scattered over a field of EXTENT around `centre`, sizes from a hundredth to a tenth of it."""
    rng = np.random.default_rng(seed)
    c = centre + rng.uniform(-0.5 * EXTENT, 0.5 * EXTENT, (n, 3))
    h = rng.uniform(0.005 * EXTENT, 0.05 * EXTENT, (n, 3))
    return np.concatenate([c - h, c + h], 1).astype(np.float32)


def flat_boxes(n, seed):
    """boxes without extent along one, two or all three axes (lo == hi there)"""
    b = random_boxes(n, seed)
    for i in range(n):
        for k in ((0,), (1, 2), (0, 1, 2))[i % 3]:
            b[i, 3 + k] = b[i, k]
    return b


def dump(a, path):
    np.ascontiguousarray(a, np.float32).tofile(path)
    return path


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("tlas_build") / "tlas_build_check"))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{name: boxes file}: the random sets of COUNTS, 71 identical boxes, 301 boxes a million units out (the spacing
    of float32 there is 1/16) and 71 boxes without extent."""
    d = tmp_path_factory.mktemp("tlas_build_boxes")
    sets = {f"random{n}": random_boxes(n, 11 + n) for n in COUNTS}
    sets["same71"] = np.tile(random_boxes(1, 3), (71, 1))
    sets["far301"] = random_boxes(301, 5, centre=1.0e6)
    sets["flat71"] = flat_boxes(71, 7)
    return {k: dump(b, str(d / f"{k}.bin")) for k, b in sets.items()}


CASES = [f"random{n}" for n in COUNTS] + ["same71", "far301", "flat71"]


@pytest.mark.parametrize("case", CASES)
def test_fat_records_bound_the_boxes_exactly(checker, files, case):
    out = run_checker(checker, "fat", files[case])
    assert out["boxes"] == os.path.getsize(files[case]) // 24


@pytest.mark.parametrize("case", CASES)
def test_finished_tree_has_the_host_form_and_the_refit_reproduces_it(checker, files, case):
    out = run_checker(checker, "build", files[case])
    n = os.path.getsize(files[case]) // 24
    assert out["instances"] == n and 1 <= out["nodes"] <= max(n, 1)
    if case in ("random1", "random2", "random3"):
        assert out["nodes"] == 1 and out["depth"] == 1
    if case == "random71":
        assert out["nodes"] > 1 and out["depth"] >= 2  # the smallest count with a multi-level tree
    if case == "random5000":
        assert out["depth"] >= 4


def _libasan():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_libasan() is None, reason="gcc's ASan runtime is not installed")
def test_clean_under_sanitizers(files, tmp_path):
    """The checker rebuilt with ASan + UBSan and run as a stand-alone program (nothing sanitized is loaded into
    Python): both modes on one node, the no-treelet sizes, a multi-level tree and the special boxes."""
    exe = build_checker(str(tmp_path / "tlas_build_check_asan"), SAN)
    for case in ("random1", "random2", "random3", "random71", "random301", "same71", "far301", "flat71"):
        run_checker(exe, "fat", files[case], env=SAN_ENV)
        run_checker(exe, "build", files[case], env=SAN_ENV)


def test_instance_rebuild_abi_without_a_device():
    """The symbol is exported with the header's signature; a NULL context and the builder argument are refused
    before anything else (no device needed)."""
    L = prt.load()
    assert hasattr(L, "prt_rebuild_instances") and "prt_rebuild_instances" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "prt.h")).read()
    assert ("int prt_rebuild_instances(prt_ctx* ctx, const float* transforms, int32_t count, uint32_t in_flags, "
            "int32_t builder);") in hdr
    xf = np.eye(4, dtype=np.float32).reshape(-1)
    assert L.prt_rebuild_instances(None, xf.ctypes.data, 1, 0, _lib.BUILDER_GPU_PLOC) == -1 and b"NULL" in L.prt_last_error()
    assert L.prt_rebuild_instances(None, None, 1, 0, _lib.BUILDER_GPU_LBVH) == -1
    assert L.prt_abi_version() == 10
