"""DevOwn<T> (graphminer_amd/csrc/gm_devown.h), the owner of every persistent device array, checked on the host: tests/devown_host_check.cc
includes only that header, stands counting malloc / free in for the library's allocator and is built with the address and undefined-behaviour
sanitizers of the host compiler.  The program is run on its own (nothing loaded into this interpreter is sanitized)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devown_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "devown_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "devown_host_check.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith("devown ok"), (r.stdout, r.stderr)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
