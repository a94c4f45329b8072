"""The scratch layout of the host drivers (multimesh_amd/csrc/mm_scratch_layout.h) on the CPU: a stand-alone program
(tests/host/scratch_layout_host.cpp, its own main, the layout header and no HIP; the context's pool is stubbed) is
compiled with g++ and run as a child process.  It checks that offsets are multiples of 256, follow the add order and do
not overlap; that the reservation is exactly the sum of the rounded sizes; that arrays which were not added stay null and
a zero-count entry gets a distinct slot; a nested contribution of the shape the GLL locate's visiting order has; sizes
beyond 4 GiB; that a guarded run is asked for exact byte counts; and the one error message with the site's code."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "scratch_layout_host.cpp")
HDR = os.path.join(ROOT, "multimesh_amd", "csrc", "mm_scratch_layout.h")
OUT = os.path.join(HERE, "host", "_build", "scratch_layout_host")


def test_scratch_layout_host():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "multimesh_amd", "csrc"), "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
