"""Once<T> (graphminer_amd/csrc/gm_once.h), the protocol by which a handle's lazily built structures are published, checked on the host:
tests/once_host_check.cc includes only that header and gm_devown.h, stands counting malloc / free in for the library's allocator and is
built twice with the host compiler -- address + undefined-behaviour sanitizers, then the thread sanitizer.  The program is run on its own
(nothing loaded into this interpreter is sanitized)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,flags", [
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]),
    ("tsan", ["-fsanitize=thread"]),
])
def test_once_under_host_sanitizers(tmp_path, name, flags):
    exe = str(tmp_path / ("once_host_check_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + flags +
                          ["-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "once_host_check.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith("once ok"), (r.stdout, r.stderr)
    assert "ERROR" not in r.stderr and "WARNING" not in r.stderr and "runtime error" not in r.stderr, r.stderr
