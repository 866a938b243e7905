"""The pair index -> edge map of the edge sampler (csrc/mde_tri_index.h: host and device code, no HIP include) at
forced indices -- the first and last pairs and both sides of a spread of row boundaries, up to n = 2^31 - 1 -- against
128-bit integers, by a stand-alone C++ program (tests/host/tri_index_test.cpp) built with the address,
undefined-behaviour and float-cast-overflow sanitizers and run as a child process.  No GPU, nothing loaded into
Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tri_index_at_forced_indices_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tri_index_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "tri_index_test.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases pass" in run.stdout
    # the correction loops behind the double-precision square root: a bound of 64 steps (the program fails a
    # case above it); with the discriminant formed in integers they take a step or two
    assert int(re.search(r"at most (\d+) correction steps", run.stdout).group(1)) <= 64
