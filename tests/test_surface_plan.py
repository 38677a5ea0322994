"""The primary-surface record in the render plan, on the CPU (tests/cpp/surface_plan_check.cpp over csrc/prt_plan.h):
which calls carry the record, what iteration 0 of a dense pass, of a reusing pass with a stale record and of one with a
valid record does with it under the deferred and the per-iteration resolve, with the init fold on and off, whether the
pass then launches the wave init, that every later launch keeps its kernels, and how PRT_SURFACE_REUSE and PRT_INIT_FOLD
are parsed.  The GPU side: tests/test_gpu_surface_reuse.py."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-ray-tracer_amd", "csrc")
VARS = ("PRT_SURFACE_REUSE", "PRT_INIT_FOLD", "PRT_SHADOW_REUSE", "PRT_PRIMARY_REUSE")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("surface_plan") / "surface_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "surface_plan_check.cpp"), "-o", exe], check=True,
                   capture_output=True, text=True)
    return exe


def run(exe, mode, env=None):
    base = {k: v for k, v in os.environ.items() if k not in VARS}
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60, env=dict(base, **(env or {})))
    assert r.stdout.strip(), r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and out["ok"], (out, r.stderr[-3000:])
    return out


def test_which_calls_carry_the_record(checker):
    assert run(checker, "plan")["checked"] == 15


def test_iteration_0_takes_the_record_form_and_nothing_else_moves(checker):
    """11 passes x iters in {1, 2, 3} x every launch."""
    assert run(checker, "schedule")["checked"] == 11 * 9


@pytest.mark.parametrize("env,want", [
    ({}, (1, 1)),
    ({"PRT_SURFACE_REUSE": "0"}, (0, 1)),
    ({"PRT_SURFACE_REUSE": "1"}, (1, 1)),
    ({"PRT_SURFACE_REUSE": ""}, (0, 1)),  # (set, and atoi gives 0: as the sibling switches)
    ({"PRT_INIT_FOLD": "0"}, (1, 0)),
    ({"PRT_INIT_FOLD": "1"}, (1, 1)),
])
def test_the_switches(checker, env, want):
    out = run(checker, "tunables", env)
    assert (out["surface_reuse"], out["init_fold"]) == want


def test_the_variables_are_read_in_one_place():
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        for v in ("PRT_SURFACE_REUSE", "PRT_INIT_FOLD"):
            assert text.count(f'"{v}"') == (1 if name == "prt_plan.h" else 0), (name, v)
