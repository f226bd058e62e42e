"""The rule by which launch_tch chooses the key addressing of tch_kernel's flattened pass (graphminer_amd/csrc/gm_tch_rule.h), checked on
the host: tests/tch_rule_host_check.cc includes only that header, forms the narrow form's 32-bit sum for the extreme indices of arrays on
either side of the threshold, and checks the threshold, the clamp of GM_TCH_WIDE_NE and that the extent of the array streamed from -- the
DAG's entries plus the task-major copies where a launch streams those -- decides.  Built with the address and undefined-behaviour
sanitizers of the host compiler and run on its own (nothing loaded into this interpreter is sanitized)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tch_rule_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "tch_rule_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "tch_rule_host_check.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith("tch rule ok"), (r.stdout, r.stderr)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_the_launch_passes_the_extent_of_the_copies():
    """the one place that swaps the view's col for the task-major copies sets their extent beside it, and launch_tch decides by it"""
    launch = open(os.path.join(ROOT, "graphminer_amd", "csrc", "gm_launch.hip")).read()
    i = launch.index("p.g.col = tl.colk;")
    assert "p.g.col_entries = (long long)g->ne + (long long)tl.n_copy_keys;" in launch[i:i + 300]
    assert launch.count("p.g.col = ") == 1
    tch = open(os.path.join(ROOT, "graphminer_amd", "csrc", "gm_tch.hip")).read()
    assert 'tch_wide_form(tch_key_entries(p.g.ne, p.g.col_entries), gm_opt("GM_TCH_WIDE_NE"))' in tch
