"""Which rows the LDS-ring layout peels off and how it deals the rest to the row blocks (csrc/mde_ring_rows.h, plan_rows):
a pure host function, so its invariants are checked by a stand-alone C++ program (tests/host/ring_rows_test.cpp) built
with the address and undefined-behaviour sanitizers and run as a child process.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_rows_invariants_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ring_rows_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "ring_rows_test.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases pass" in run.stdout
