"""The fit of the search grid of mm_cutoff_distance and mm_surface_distance (multimesh_amd/csrc/mm_search_grid.h) on the
CPU: a stand-alone program (tests/host/search_grid_host.cpp, its own main, the header and no HIP) is compiled with g++ and
run as a child process.  It checks the cells and the number of x1.25 enlargements of eight grids -- uncapped, capped by the
cells in all, capped per axis, for both pads -- against values transcribed from the two loops the units had before they
shared the function; that inv_h is 1 / h; the grids of a box that is a point; and that an edge that fits is kept."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "search_grid_host.cpp")
HDR = os.path.join(ROOT, "multimesh_amd", "csrc", "mm_search_grid.h")
OUT = os.path.join(HERE, "host", "_build", "search_grid_host")


def test_search_grid_host():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                        os.path.join(ROOT, "multimesh_amd", "csrc"), "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
