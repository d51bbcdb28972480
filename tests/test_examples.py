"""Every shipped example runs end-to-end (reference examples/ are built and
run by its CI; here each is executed as a subprocess on the host path)."""

import os
import subprocess
import sys

import pytest

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)


def run_py(script, *args, timeout=180):
    return subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", script), *args],
        capture_output=True, text=True, timeout=timeout, cwd=REPO)


def two_rank_env():
    """Environment for a 2-rank launch: each rank takes the GPU of its local
    rank, so with a single GPU the ranks run on the host (gloo) path, as
    they do on a machine without one."""
    import torch
    env = dict(os.environ)
    if torch.cuda.is_available() and torch.cuda.device_count() < 2:
        env["HIP_VISIBLE_DEVICES"] = ""
        env["CUDA_VISIBLE_DEVICES"] = ""
    return env


def test_example_capi_matrix_mtx():
    """BASELINE config #1: matrix.mtx + FGMRES_AGGREGATION on the host
    path must converge in 1 iteration (reference README.md:126-129 shows
    the same run at 1 iteration / 1.6e-14)."""
    p = run_py("amgx_capi.py", "-m", "examples/matrix.mtx",
               "-c", "configs/FGMRES_AGGREGATION.json")
    assert p.returncode == 0, p.stderr[-800:]
    assert "iterations=1 " in p.stdout, p.stdout


def test_example_capi_poisson_default():
    p = run_py("amgx_capi.py")
    assert p.returncode == 0, p.stderr[-800:]
    assert "status=0" in p.stdout


def test_example_eigensolver():
    p = run_py("eigensolver_example.py")
    assert p.returncode == 0, p.stderr[-800:]
    assert "converged=True" in p.stdout


def test_example_pagerank():
    p = run_py("pagerank.py")
    assert p.returncode == 0, p.stderr[-800:]
    assert "top-5 pages" in p.stdout


def test_example_convert_roundtrip(tmp_path):
    b = str(tmp_path / "m.bin")
    m2 = str(tmp_path / "m2.mtx")
    p = run_py("convert.py", "examples/matrix.mtx", b)
    assert p.returncode == 0 and "NVAMGBinary" in p.stdout, p.stderr[-400:]
    p = run_py("convert.py", b, m2)
    assert p.returncode == 0, p.stderr[-400:]
    assert open(m2).readline().startswith("%%MatrixMarket")


def test_example_c_binary():
    """The compiled C client (built by __graft_entry__.build) solves
    matrix.mtx through libamgx_amd.so (reference examples/amgx_capi.c)."""
    exe = os.path.join(REPO, "examples", "amgx_capi")
    if not os.path.exists(exe):
        pytest.skip("C example not built")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=180,
                       cwd=REPO)  # config paths in the client are repo-relative
    assert p.returncode == 0, p.stderr[-800:]
    assert "AMGX_CAPI_OK" in p.stdout


def test_example_mpi_capi_two_ranks():
    """Distributed upload example at 2 gloo ranks via the exact torchrun
    invocation the docs give (reference examples/amgx_mpi_capi.c role)."""
    p = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29719", "examples/amgx_mpi_capi.py"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
        env=two_rank_env())
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-800:])
