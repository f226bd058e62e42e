"""The conversion from non-induced counts to induced graphlet orbits (graphminer_amd/csrc/gm_orbit.h, the one place gm_motif_local's
coefficient table lives), checked on the host: tests/orbit_host_check.cc includes only that header, counts for every vertex of each of the
six 4-vertex graphlets the spanning copies of every pattern by brute force over edge subsets, and asks the function for exactly the
vertex's own orbit.  Built with the address and undefined-behaviour sanitizers of the host compiler and run on its own (nothing loaded
into this interpreter is sanitized)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_orbit_table_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "orbit_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "orbit_host_check.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith("orbit table ok"), (r.stdout, r.stderr)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_the_finish_kernel_uses_the_one_table():
    """the device unit includes the header and calls the function; no second copy of the coefficients"""
    unit = open(os.path.join(ROOT, "graphminer_amd", "csrc", "gm_orbit_local.hip")).read()
    assert '#include "gm_orbit.h"' in unit
    assert "gm_orbits_from_noninduced(" in unit
