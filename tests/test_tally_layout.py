"""The count-level kernels' per-wave LDS layouts (csrc/benor_tally_common.h):
the kernels take their region pointers and the host its sizes from one plain
C++ function.  tests/tally_layout_check.cpp, a host program over that header,
sweeps it: alignment, disjoint regions apart from the two documented aliases,
and every region inside what the size functions give the host.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ben-or-consensus-algorithm_amd", "csrc")


def test_layouts_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "tally_layout_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tally_layout_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 64 W x 7 caps x 2 launches x (1 Byzantine + 6 x 2 x 2 crash-family layouts), > 60 checks each
    assert int(r.stdout.split()[0]) >= 64 * 7 * 2 * 25 * 60 and " 0 failures" in r.stdout, r.stdout
