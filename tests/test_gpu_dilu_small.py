"""The one-launch scalar DILU apply of small levels (dilu_small): split slabs,
one gathered vector, 1 or 8 lanes per row and several sweeps per launch,
against the host backend (ops/cpu.py) under the device coloring copied to the
host, and bit for bit against the full-slab form it replaced, between the
lane forms, and between one launch of three sweeps and three launches.

Conventions and tolerances are those of tests/test_dilu_split_gpu.py: rtol
1e-11 / atol 1e-12 in fp64, 1e-4 / 1e-5 with an fp32 matrix, 1e-12 / 1e-12 in
complex. The workgroup has 1024 threads, so a color of more than 1024 rows
(128 with 8 lanes) takes several rounds; the shapes cover fewer rows per color
than one round, several rounds, rows of one to six chunks of 8 entries with
ragged tails, and a halo tail. The routing boundary DILU_SMALL_ROWS was
measured at 1024 rows, under the several-round shapes, so every level names
form="small" and runs the kernel under test whatever its size; the routed
path at the boundary and the smoother's own calls have their own tests."""

import copy
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from amgx_amd import AMGConfig, CSRMatrix, create_solver
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import (poisson_2d, poisson_3d, poisson_3d_27pt,
                               random_laplacian)
from amgx_amd.resources import Resources

gpu = pytest.mark.gpu
DEV = "cuda:0"
F64 = dict(rtol=1e-11, atol=1e-12)
F32 = dict(rtol=1e-4, atol=1e-5)
C128 = dict(rtol=1e-12, atol=1e-12)
RELAX = 0.9
LANES = (1, 8)
SQUARE = ("p8", "p64", "rand", "27pt")
NAMES = SQUARE + ("halo",)
KINDS = ("f64", "f32A", "c128")


def core():
    from amgx_amd import _core
    return _core


def gpu_ops():
    from amgx_amd.ops import gpu
    return gpu


def ext(v, n_cols):
    """v with a halo tail of zeros up to n_cols entries."""
    out = torch.zeros(n_cols, dtype=v.dtype)
    out[:v.numel()] = v
    return out


def halo_matrix(P, n_rows):
    """The first n_rows rows of P; the remaining columns are a halo tail."""
    return CSRMatrix.from_scipy(P.to_scipy().tocsr()[:n_rows, :])


def make_level(A, seed):
    """Host matrix, device copy, the device coloring on both sides, and the
    host results every test compares with: x after each of three fused
    sweeps, and x after one and two plain applies from a zero and from a
    non-zero start."""
    Ag = A.to(DEV)
    colg = MatrixColoring.create(Ag)
    col = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    assert col.num_colors > 1
    g = torch.Generator().manual_seed(seed)
    b = ext(torch.rand(A.n_rows, generator=g, dtype=torch.float64), A.n_cols)
    x0 = ext(torch.rand(A.n_rows, generator=g, dtype=torch.float64) - 0.5,
             A.n_cols)
    einv = cpu_ops.dilu_setup(A, col)
    smooth, x = [], x0.clone()
    for _ in range(3):
        cpu_ops.dilu_solve(A, einv, col, cpu_ops.residual(A, x, b), RELAX, x)
        smooth.append(x.clone())
    plain = {}
    for start in ("zero", "nonzero"):
        x = torch.zeros_like(x0) if start == "zero" else x0.clone()
        plain[start] = []
        for _ in range(2):
            cpu_ops.dilu_solve(A, einv, col, b, RELAX, x)
            plain[start].append(x.clone())
    ro = A.row_offsets.long()
    per_color = torch.bincount(col.colors.long())
    return SimpleNamespace(A=A, Ag=Ag, colg=colg, col=col, b=b, x0=x0,
                           smooth=smooth, plain=plain, deg=ro[1:] - ro[:-1],
                           per_color=per_color)


@pytest.fixture(scope="module")
def levels():
    """Small levels shared by the tests; nothing here is modified."""
    out = {"p8": make_level(poisson_2d(8, 8), 41),
           "p64": make_level(poisson_2d(64, 64), 42),
           "rand": make_level(random_laplacian(3000, 12, seed=34), 43),
           "27pt": make_level(poisson_3d_27pt(12, 12, 12), 44),
           "halo": make_level(halo_matrix(poisson_2d(65, 64), 65 * 32), 45)}
    assert out["p8"].A.n_rows == 64            # under one round of 8 lanes
    assert out["p64"].A.n_rows == 4096
    assert int(out["p64"].per_color.max()) > 1024      # rounds at one lane
    d = out["rand"].deg                  # up to six chunks, ragged tails
    assert int(d.min()) < 8 and 40 < int(d.max()) <= 48
    assert bool((out["rand"].per_color % 128 != 0).any())   # ragged rounds
    assert out["halo"].A.n_cols == 2 * out["halo"].A.n_rows
    return out


def show(tag, got, ref):
    print(tag, "max dev", (got.cpu() - ref).abs().max().item())


def scratch(Ag, name, dtype):
    return gpu_ops()._scratch(Ag, name, Ag.n_cols, dtype)


def w_rows(Ag, dtype):
    """The rows of w; its halo tail is never written or read."""
    return scratch(Ag, "dilu_w", dtype)[:Ag.n_rows].clone()


def typed(L, kind):
    """(device matrix, b, x0) of the level in one of the type pairs."""
    A = L.A
    if kind == "f64":
        return L.Ag, L.b.to(DEV), L.x0.to(DEV)
    if kind == "f32A":
        Ag = CSRMatrix(A.row_offsets, A.col_indices,
                       A.values.to(torch.float32), n_cols=A.n_cols).to(DEV)
        return Ag, L.b.to(DEV), L.x0.to(DEV)
    va = A.values.to(torch.complex128) * (0.6 + 0.8j)
    Ag = CSRMatrix(A.row_offsets, A.col_indices, va, n_cols=A.n_cols).to(DEV)
    g = torch.Generator().manual_seed(46)
    im = torch.rand(2, A.n_cols, generator=g, dtype=torch.float64) - 0.3
    im[:, A.n_rows:] = 0                           # the halo tail stays zero
    return (Ag, torch.complex(L.b, im[0]).to(DEV),
            torch.complex(L.x0, im[1]).to(DEV))


def finite(x):
    return bool(torch.isfinite(torch.view_as_real(x) if x.is_complex()
                               else x).all())


# ---------------------------------------------------------------- host
@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", NAMES)
def test_fused_smoother_against_host(levels, name, lanes):
    """x carried through three sweeps from a non-zero start."""
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    assert e_gpu.va_u is not None              # U is built at setup
    x, bg = L.x0.to(DEV), L.b.to(DEV)
    for sweep in range(3):
        assert G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, x, RELAX, lanes=lanes,
                             form="small") is True
        show(f"sweep {sweep}", x, L.smooth[sweep])
        assert torch.allclose(x.cpu(), L.smooth[sweep], **F64)
    assert not bool(x[L.A.n_rows:].any())         # the halo tail stays zero


@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("start", ["zero", "nonzero"])
@pytest.mark.parametrize("name", NAMES)
def test_plain_apply_against_host(levels, name, start, lanes):
    """dilu_solve accumulates into x; the second apply finds the first
    apply's z in w. The L values are gathered by the first plain apply."""
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    assert e_gpu.va_l is None
    x = (torch.zeros_like(L.x0) if start == "zero" else L.x0.clone()).to(DEV)
    for k in range(2):
        G.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, x, lanes=lanes,
                     form="small")
        show(f"apply {k}", x, L.plain[start][k])
        assert torch.allclose(x.cpu(), L.plain[start][k], **F64)
    assert e_gpu.va_l is not None


@gpu
@pytest.mark.parametrize("name", SQUARE)
def test_complex_against_host(levels, name):
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, "c128")
    Ah = CSRMatrix(Ag.row_offsets.cpu(), Ag.col_indices.cpu(),
                   Ag.values.cpu(), n_cols=Ag.n_cols)
    e_ref = cpu_ops.dilu_setup(Ah, L.col)
    b = bg.cpu()
    fused, x1 = [], x0.cpu()
    for _ in range(3):
        cpu_ops.dilu_solve(Ah, e_ref, L.col, cpu_ops.residual(Ah, x1, b),
                           RELAX, x1)
        fused.append(x1.clone())
    y1 = x0.cpu()
    cpu_ops.dilu_solve(Ah, e_ref, L.col, b, RELAX, y1)
    e_gpu = G.dilu_setup(Ag, L.colg)
    for lanes in LANES:
        x2 = x0.clone()
        for sweep in range(3):
            assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x2, RELAX,
                                 lanes=lanes, form="small") is True
            show(f"lanes {lanes} sweep {sweep}", x2, fused[sweep])
            assert torch.allclose(x2.cpu(), fused[sweep], **C128)
        y2 = x0.clone()
        G.dilu_solve(Ag, e_gpu, L.colg, bg, RELAX, y2, lanes=lanes,
                     form="small")
        assert torch.allclose(y2.cpu(), y1, **C128)


@gpu
@pytest.mark.parametrize("name", ["rand", "p64"])
def test_fp32_matrix_against_host(levels, name):
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, "f32A")
    e_gpu = G.dilu_setup(Ag, L.colg)
    assert e_gpu.va_u.dtype == torch.float32
    for lanes in LANES:
        x = x0.clone()
        for sweep in range(3):
            assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x, RELAX,
                                 lanes=lanes, form="small") is True
            show(f"lanes {lanes} sweep {sweep}", x, L.smooth[sweep])
            assert torch.allclose(x.cpu(), L.smooth[sweep], **F32)
        assert x.dtype == torch.float64
        y = x0.clone()
        G.dilu_solve(Ag, e_gpu, L.colg, bg, RELAX, y, lanes=lanes,
                     form="small")
        assert torch.allclose(y.cpu(), L.plain["nonzero"][0], **F32)


# ---------------------------------------------------------------- bitwise
def trail_of(L, kind, **how):
    """x after each of three fused sweeps and two plain applies, and w after
    each, for one way of running them."""
    G = gpu_ops()
    Ag, bg, x0 = typed(L, kind)
    e_gpu = G.dilu_setup(Ag, L.colg)
    x, xs, ws = x0.clone(), [], []
    for _ in range(3):
        assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x, RELAX, **how) is True
        xs.append(x.clone())
        ws.append(w_rows(Ag, x.dtype))
    for _ in range(2):
        G.dilu_solve(Ag, e_gpu, L.colg, bg, RELAX, x, **how)
        xs.append(x.clone())
        ws.append(w_rows(Ag, x.dtype))
    assert x.dtype == x0.dtype and finite(x)
    return xs, ws


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_new_form_equals_full_slab_form_bitwise(levels, name, kind):
    """The split-slab kernel against the retained full-slab kernel: the terms
    dropped are exact zeros and the sums keep their order, so x holds the
    same bits after every apply. (w differs: the old form keeps z apart.)"""
    L = levels[name]
    old, _ = trail_of(L, kind, form="small_full")
    for lanes in LANES:
        new, _ = trail_of(L, kind, form="small", lanes=lanes)
        for step, (a, b) in enumerate(zip(old, new)):
            assert torch.equal(a, b), f"lanes {lanes} step {step}"


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_lane_forms_agree_bitwise(levels, name, kind):
    L = levels[name]
    one = trail_of(L, kind, form="small", lanes=1)
    eight = trail_of(L, kind, form="small", lanes=8)
    for a, b in zip(one[0] + one[1], eight[0] + eight[1]):
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_launch_equals_per_color_path_bitwise(levels, name):
    """The same slabs through dilu_split: same x and same w."""
    L = levels[name]
    small = trail_of(L, "f64", form="small")
    split = trail_of(L, "f64", form="split")
    for a, b in zip(small[0] + small[1], split[0] + split[1]):
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_three_sweeps_in_one_launch_bitwise(levels, name, fused, kind):
    """sweeps=3 in one launch against three launches of sweeps=1."""
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, kind)
    e_gpu = G.dilu_setup(Ag, L.colg)

    def run(x, **how):
        if fused:
            assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x, RELAX,
                                 form="small", **how) is True
        else:
            G.dilu_solve(Ag, e_gpu, L.colg, bg, RELAX, x, form="small",
                         **how)
    for lanes in LANES:
        x1, x3 = x0.clone(), x0.clone()
        for _ in range(3):
            run(x1, lanes=lanes, sweeps=1)
        w1 = w_rows(Ag, x1.dtype)
        run(x3, lanes=lanes, sweeps=3)
        assert finite(x3) and not torch.equal(x3, x0)
        assert torch.equal(x1, x3)
        assert torch.equal(w1, w_rows(Ag, x1.dtype))
    if fused and kind == "f64":
        assert torch.allclose(x3.cpu(), L.smooth[2], **F64)


@gpu
def test_smoother_sweep_passes_the_count(levels):
    """MulticolorDILUSolver.sweep(b, x, 3) on a small level: one call of the
    backend with sweeps=3, the bits of three solve_iteration calls."""
    from amgx_amd.config import ConfigScope
    from amgx_amd.solvers.dilu import MulticolorDILUSolver
    L, G = levels["p8"], gpu_ops()
    assert L.A.n_rows <= core().DILU_SMALL_ROWS
    A = L.A.to(DEV)
    s = MulticolorDILUSolver(ConfigScope(None, {}), Resources(DEV))
    s.setup(A)
    bg = L.b.to(DEV)
    x1, x3 = L.x0.to(DEV), L.x0.to(DEV)
    for _ in range(3):
        s.solve_iteration(bg, x1)
    calls = []
    real = G.dilu_smooth

    def counting(*args, **kwargs):
        calls.append(kwargs.get("sweeps", 1))
        return real(*args, **kwargs)
    G.dilu_smooth = counting
    try:
        s.sweep(bg, x3, 3)
    finally:
        G.dilu_smooth = real
    assert calls == [3]
    assert torch.equal(x1, x3)


# ---------------------------------------------------------------- scratch
@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["rand", "halo"])
def test_stale_scratch_is_not_read(levels, name, fused, lanes):
    """w and y full of NaN before the call: neither is zeroed, so a value
    read before this launch wrote it would reach x."""
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    x = L.x0.to(DEV)
    for vec in ("dilu_w", "dilu_y"):
        scratch(L.Ag, vec, x.dtype).fill_(float("nan"))
    if fused:
        assert G.dilu_smooth(L.Ag, e_gpu, L.colg, L.b.to(DEV), x, RELAX,
                             lanes=lanes, form="small") is True
        want = L.smooth[0]
    else:
        G.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, x, lanes=lanes,
                     form="small")
        want = L.plain["nonzero"][0]
    assert bool(torch.isfinite(x).all())
    assert torch.allclose(x.cpu(), want, **F64)
    assert not bool(x[L.A.n_rows:].any())


# ---------------------------------------------------------------- boundary
@gpu
@pytest.mark.parametrize("over", [0, 1])
def test_routing_at_the_boundary(over):
    """A 1D Laplacian of exactly DILU_SMALL_ROWS rows takes the one-launch
    apply and one of one row more the per-color path: the binding of the
    other path refuses the level, and both agree with the host."""
    G, C = gpu_ops(), core()
    assert C.DILU_SMALL_ROWS <= C.SMALL_LEVEL_ROWS == 16384
    n = C.DILU_SMALL_ROWS + over
    T = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)],
                 [-1, 0, 1]).tocsr()
    A = CSRMatrix.from_scipy(T)
    L = make_level(A, 47 + over)
    assert G._split_path(L.Ag) == bool(over)
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    x, bg = L.x0.to(DEV), L.b.to(DEV)
    for sweep in range(3):
        assert G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, x, RELAX) is True
        assert torch.allclose(x.cpu(), L.smooth[sweep], **F64)
    y = L.x0.to(DEV)
    G.dilu_solve(L.Ag, e_gpu, L.colg, bg, RELAX, y)
    assert torch.allclose(y.cpu(), L.plain["nonzero"][0], **F64)
    # routed and named forms are the same kernel
    z = L.x0.to(DEV)
    G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, z, RELAX, sweeps=3,
                  form="split" if over else "small")
    assert torch.equal(z, x)
    st = G._slabs(L.Ag, L.colg)
    ro_u, ci_u, _ = G._slab_part(st, True)
    w, yv = scratch(L.Ag, "dilu_w", x.dtype), scratch(L.Ag, "dilu_y", x.dtype)
    args = (st.ro_s, st.ci_s, e_gpu.va_s, ro_u, ci_u, e_gpu.va_u,
            e_gpu.einv_s, L.colg.rows_sorted, L.colg.bounds,
            L.colg.bounds_dev, bg, w, z, RELAX, True, 0, yv)
    if over:
        with pytest.raises(RuntimeError, match="run dilu_split"):
            C.dilu_small(*args)
    else:
        C.dilu_small(*args)                        # within the bound: runs
        assert torch.allclose(z.cpu(), cpu_next(L, x.cpu()), **F64)


def cpu_next(L, x):
    x = x.clone()
    cpu_ops.dilu_solve(L.A, cpu_ops.dilu_setup(L.A, L.col), L.col,
                       cpu_ops.residual(L.A, x, L.b), RELAX, x)
    return x


@gpu
def test_arguments_are_checked(levels):
    L, G, C = levels["p8"], gpu_ops(), core()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    bg = L.b.to(DEV)
    with pytest.raises(RuntimeError):
        G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, L.x0.to(DEV), RELAX, lanes=4,
                      form="small")
    with pytest.raises(RuntimeError):
        G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, L.x0.to(DEV), RELAX, sweeps=0,
                      form="small")
    with pytest.raises(ValueError):
        G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, L.x0.to(DEV), RELAX,
                      form="other")
    st = G._slabs(L.Ag, L.colg)
    ro_u, ci_u, _ = G._slab_part(st, True)
    x = L.x0.to(DEV)
    w = torch.empty_like(x)
    with pytest.raises(RuntimeError, match="needs y"):   # nothing allocated
        C.dilu_small(st.ro_s, st.ci_s, e_gpu.va_s, ro_u, ci_u, e_gpu.va_u,
                     e_gpu.einv_s, L.colg.rows_sorted, L.colg.bounds,
                     L.colg.bounds_dev, bg, w, x, RELAX, True)
    assert torch.equal(x, L.x0.to(DEV))


# ---------------------------------------------------------------- graph
@gpu
def test_graph_replay_equals_eager():
    """The flagship configuration on a 24^3 cube, every level at or under
    SMALL_LEVEL_ROWS: the V-cycle captured and replayed, then eager. The
    one-launch applies sit inside the captured graph and allocate nothing."""
    from bench import FGMRES_AGG
    A = poisson_3d(24, 24, 24, device=DEV)
    assert A.n_rows == 13824 <= core().SMALL_LEVEL_ROWS
    g = torch.Generator().manual_seed(48)
    b = torch.rand(A.n_rows, generator=g, dtype=torch.float64).to(DEV)
    out = {}
    for use_graph in (1, 0):
        cfg = copy.deepcopy(FGMRES_AGG)
        cfg["solver"]["preconditioner"]["use_hip_graph"] = use_graph
        s = create_solver(AMGConfig.from_dict(cfg).root_scope(),
                          resources=Resources(DEV))
        s.setup(A)
        x = torch.zeros_like(b)
        st = s.solve(b, x, zero_initial_guess=True)
        amg = s.precond
        assert (amg._graph is not None) == bool(use_graph)
        assert not amg._graph_failed
        small = [lv.A.n_rows <= core().DILU_SMALL_ROWS
                 for lv in amg.hierarchy.levels[:-1]]
        assert sum(small) >= 2
        out[use_graph] = (x.clone(), st.iterations)
    assert bool(torch.isfinite(out[1][0]).all())
    assert out[0][1] == out[1][1]
    assert torch.equal(out[0][0], out[1][0])
