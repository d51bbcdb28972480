"""Host check of the device complex value type amgx_amd/csrc/cplx.h.

Builds tests/cplx_host_check.cpp (its own main, no HIP, no Python) with the
host C++ compiler and runs it: every cplx<R> operator against std::complex<R>
on a fixed table of values. A second build of the same program runs under
AddressSanitizer + UBSan."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "amgx_amd", "csrc")
SRC = os.path.join(HERE, "cplx_host_check.cpp")


def _host_cxx():
    """The host compiler the extension build uses; hipcc compiles plain C++
    as well, so a machine that can build this repository always has one."""
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "hipcc",
                "/opt/rocm/bin/hipcc"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no C++ compiler found (needed to build the "
                         "extension as well)")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = [_host_cxx(), "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, SRC,
           "-o", exe] + extra
    cp = subprocess.run(cmd, capture_output=True, text=True)
    assert cp.returncode == 0, f"compile failed:\n{cp.stderr}"
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, \
        f"{name} exit {run.returncode}:\n{run.stdout}\n{run.stderr}"
    assert "all cplx checks passed" in run.stdout


def test_cplx_operators_match_std_complex(tmp_path):
    _build_and_run(tmp_path, "cplx_check", [])


def test_cplx_operators_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "cplx_check_san",
                   ["-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"])
