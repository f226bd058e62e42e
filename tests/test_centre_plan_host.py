"""The centre plans of the map solvers (graphminer_amd/csrc/gm_centre_plan.h: the LDS ranges, which centres count there, the task lists of
rectangle / house / weighted 4-cycles and their order), checked on the host: tests/centre_plan_host_check.cc includes only that header,
runs hand-worked cases and properties on random inputs with tiny parameters, and is built with the address and undefined-behaviour
sanitizers of the host compiler.  The program is run on its own (nothing loaded into this interpreter is sanitized)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_centre_plan_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "centre_plan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "centre_plan_host_check.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith("centre plan ok"), (r.stdout, r.stderr)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
