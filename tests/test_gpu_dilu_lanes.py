"""Scalar per-color DILU with one gathered vector (y = x + w) in the fused
forward sweep and with 1 or 8 lanes per row, against the host backend
(ops/cpu.py) under the device coloring copied to the host, and the two lane
forms against each other bit for bit.

Conventions and tolerances are those of tests/test_dilu_split_gpu.py: rtol
1e-11 / atol 1e-12 in fp64, 1e-4 / 1e-5 with an fp32 matrix, 1e-12 / 1e-12 in
complex. Every matrix has just over SMALL_LEVEL_ROWS rows, the smallest size
that takes the per-color path; the rows span whole chunks of 8 entries,
ragged tails and rows shorter than one chunk."""

import copy
from types import SimpleNamespace

import pytest
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
SQUARE = ("rand", "27pt", "7pt")
NAMES = SQUARE + ("halo",)


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
    assert A.n_rows > core().SMALL_LEVEL_ROWS
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
    deg = ro[1:] - ro[:-1]
    return SimpleNamespace(A=A, Ag=Ag, colg=colg, col=col, b=b, x0=x0,
                           smooth=smooth, plain=plain, deg=deg)


@pytest.fixture(scope="module")
def levels():
    """Per-color levels shared by the tests; nothing here is modified."""
    out = {"rand": make_level(random_laplacian(16500, 12, seed=11), 31),
           "27pt": make_level(poisson_3d_27pt(26, 26, 26), 32),
           "7pt": make_level(poisson_3d(26, 26, 26), 33),
           "halo": make_level(halo_matrix(poisson_2d(129, 256), 129 * 128),
                              34)}
    d = out["rand"].deg                  # up to six chunks, ragged tails
    assert int(d.min()) < 8 and 40 < int(d.max()) <= 48
    assert sorted(set(out["27pt"].deg.tolist())) == [8, 12, 18, 27]
    assert int(out["7pt"].deg.max()) == 7   # rows shorter than a chunk
    assert out["halo"].A.n_cols == 2 * out["halo"].A.n_rows
    return out


def show(tag, got, ref):
    print(tag, "max dev", (got.cpu() - ref).abs().max().item())


def scratch(Ag, name, dtype):
    return gpu_ops()._scratch(Ag, name, Ag.n_cols, dtype)


# ---------------------------------------------------------------- host
@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", NAMES)
def test_fused_smoother_against_host(levels, name, lanes):
    """x carried through three sweeps; y is rewritten by every apply."""
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    x, bg = L.x0.to(DEV), L.b.to(DEV)
    for sweep in range(3):
        assert G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, x, RELAX,
                             lanes=lanes) is True
        show(f"sweep {sweep}", x, L.smooth[sweep])
        assert torch.allclose(x.cpu(), L.smooth[sweep], **F64)
    assert not bool(x[L.A.n_rows:].any())         # the halo tail stays zero


@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("start", ["zero", "nonzero"])
@pytest.mark.parametrize("name", NAMES)
def test_plain_apply_against_host(levels, name, start, lanes):
    """dilu_solve accumulates into x; the second apply finds the first
    apply's z in w."""
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    x = (torch.zeros_like(L.x0) if start == "zero" else L.x0.clone()).to(DEV)
    for k in range(2):
        G.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, x, lanes=lanes)
        show(f"apply {k}", x, L.plain[start][k])
        assert torch.allclose(x.cpu(), L.plain[start][k], **F64)


# ---------------------------------------------------------------- bitwise
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
    g = torch.Generator().manual_seed(35)
    im = torch.rand(2, A.n_cols, generator=g, dtype=torch.float64) - 0.3
    return (Ag, torch.complex(L.b, im[0]).to(DEV),
            torch.complex(L.x0, im[1]).to(DEV))


@gpu
@pytest.mark.parametrize("kind", ["f64", "f32A", "c128"])
@pytest.mark.parametrize("name", SQUARE)
def test_lane_forms_agree_bitwise(levels, name, kind):
    """Two fused sweeps and two plain applies with lanes=1 and lanes=8: x
    and the scratch vector w hold the same bits after each."""
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, kind)
    e_gpu = G.dilu_setup(Ag, L.colg)
    assert e_gpu.va_u.dtype == Ag.values.dtype
    got = {}
    for lanes in LANES:
        x, trail = x0.clone(), []
        for _ in range(2):
            assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x, RELAX,
                                 lanes=lanes) is True
            trail += [x.clone(), scratch(Ag, "dilu_w", x.dtype).clone()]
        for _ in range(2):
            G.dilu_solve(Ag, e_gpu, L.colg, bg, RELAX, x, lanes=lanes)
            trail += [x.clone(), scratch(Ag, "dilu_w", x.dtype).clone()]
        got[lanes] = trail
    assert x.dtype == x0.dtype and bool(torch.isfinite(
        torch.view_as_real(x) if x.is_complex() else x).all())
    for step, (one, eight) in enumerate(zip(got[1], got[8])):
        assert torch.equal(one, eight), f"step {step}"


@gpu
@pytest.mark.parametrize("name", SQUARE)
def test_complex_against_host(levels, name):
    """The complex instantiation of both lane forms against the host."""
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, "c128")
    Ah = CSRMatrix(Ag.row_offsets.cpu(), Ag.col_indices.cpu(),
                   Ag.values.cpu(), n_cols=Ag.n_cols)
    e_ref = cpu_ops.dilu_setup(Ah, L.col)
    b, x1 = bg.cpu(), x0.cpu()
    cpu_ops.dilu_solve(Ah, e_ref, L.col, cpu_ops.residual(Ah, x1, b), RELAX,
                       x1)
    e_gpu = G.dilu_setup(Ag, L.colg)
    for lanes in LANES:
        x2 = x0.clone()
        assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x2, RELAX,
                             lanes=lanes) is True
        show(f"lanes {lanes}", x2, x1)
        assert torch.allclose(x2.cpu(), x1, **C128)


@gpu
def test_fp32_matrix_against_host(levels):
    L, G = levels["rand"], gpu_ops()
    Ag, bg, x0 = typed(L, "f32A")
    e_gpu = G.dilu_setup(Ag, L.colg)
    for lanes in LANES:
        x = x0.clone()
        for sweep in range(3):
            assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x, RELAX,
                                 lanes=lanes) is True
        assert x.dtype == torch.float64
        show(f"lanes {lanes}", x, L.smooth[2])
        assert torch.allclose(x.cpu(), L.smooth[2], **F32)


# ---------------------------------------------------------------- scratch
@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", ["rand", "halo"])
def test_stale_scratch_is_not_read(levels, name, lanes):
    """w and y full of NaN before a fused apply: neither is zeroed any more,
    so a value read before this apply wrote it would reach x."""
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    x = L.x0.to(DEV)
    for vec in ("dilu_w", "dilu_y"):
        scratch(L.Ag, vec, x.dtype).fill_(float("nan"))
    assert G.dilu_smooth(L.Ag, e_gpu, L.colg, L.b.to(DEV), x, RELAX,
                         lanes=lanes) is True
    assert bool(torch.isfinite(x).all())
    assert torch.allclose(x.cpu(), L.smooth[0], **F64)
    assert not bool(x[L.A.n_rows:].any())


# ---------------------------------------------------------------- routing
@gpu
def test_routing(levels):
    """lanes=0 takes the form dilu_lanes names for the slab's entries per
    row: 8 lanes on the full slab of the random graph, one on the 7-point
    matrix. The split parts L and U carry about half a row and route by
    their own figure and their own threshold."""
    G, pick = gpu_ops(), core().dilu_lanes
    assert pick(7.0) == 1 and pick(12.7) == 8
    # L / U: one lane measured faster at 2.98 entries per row, 8 from 4.57
    assert pick(2.98, split=True) == 1 and pick(4.57, split=True) == 8
    want = {"rand": 8, "7pt": 1}
    for name, lanes in want.items():
        L = levels[name]
        n = L.A.n_rows
        assert pick(L.A.nnz / n) == lanes
        e_gpu = G.dilu_setup(L.Ag, L.colg)
        st = G._slabs(L.Ag, L.colg)
        assert st.ci_s.numel() == L.A.nnz
        # U holds half of the off-diagonal entries: its own, smaller figure
        nnz_u = G._slab_part(st, True)[1].numel()
        assert 2 * nnz_u == L.A.nnz - n
        assert pick(nnz_u / n, split=True) == lanes
        out = []
        for la in (0, lanes):
            x = L.x0.to(DEV)
            assert G.dilu_smooth(L.Ag, e_gpu, L.colg, L.b.to(DEV), x, RELAX,
                                 lanes=la) is True
            G.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, x,
                         lanes=la)
            out.append(x)
        assert torch.equal(out[0], out[1])
    L = levels["7pt"]
    with pytest.raises(RuntimeError):
        G.dilu_solve(L.Ag, G.dilu_setup(L.Ag, L.colg), L.colg, L.b.to(DEV),
                     RELAX, L.x0.to(DEV), lanes=4)


@gpu
def test_positional_call_without_lanes_and_y(levels):
    """_core.dilu_split with the 14 positional arguments it had before lanes
    and y: routed, y allocated by the binding, same bits as dilu_smooth."""
    L, G = levels["27pt"], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    st = G._slabs(L.Ag, L.colg)
    ro_u, ci_u, _ = G._slab_part(st, True)
    bg, x1, x2 = L.b.to(DEV), L.x0.to(DEV), L.x0.to(DEV)
    assert G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, x1, RELAX) is True
    w = torch.full_like(x2, float("nan"))
    core().dilu_split(st.ro_s, st.ci_s, e_gpu.va_s, ro_u, ci_u, e_gpu.va_u,
                      e_gpu.einv_s, L.colg.rows_sorted, L.colg.bounds, bg, w,
                      x2, RELAX, True)
    assert torch.equal(x1, x2)
    assert torch.equal(w, scratch(L.Ag, "dilu_w", x1.dtype))


# ---------------------------------------------------------------- graph
@gpu
def test_graph_replay_equals_eager():
    """One flagship V-cycle, captured and replayed, then eager: the y pass
    and both lane forms sit inside the captured graph and allocate nothing."""
    from bench import FGMRES_AGG
    A = poisson_3d(40, 40, 40, device=DEV)
    g = torch.Generator().manual_seed(36)
    b = torch.rand(A.n_rows, generator=g, dtype=torch.float64).to(DEV)
    out = {}
    for use_graph in (1, 0):
        cfg = copy.deepcopy(FGMRES_AGG)
        cfg["solver"]["preconditioner"]["use_hip_graph"] = use_graph
        s = create_solver(AMGConfig.from_dict(cfg).root_scope(),
                          resources=Resources(DEV))
        s.setup(A)
        amg = s.precond
        x = torch.full_like(b, 7.0)      # a zero guess ignores what x holds
        amg.solve(b, x, zero_initial_guess=True)
        assert (amg._graph is not None) == bool(use_graph)
        assert not amg._graph_failed
        per_color = [lv.A.n_rows > core().SMALL_LEVEL_ROWS
                     for lv in amg.hierarchy.levels]
        assert sum(per_color) >= 2
        out[use_graph] = x.clone()
    assert bool(torch.isfinite(out[1]).all())
    assert torch.equal(out[0], out[1])
