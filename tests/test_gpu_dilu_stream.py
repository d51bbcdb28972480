"""Stream form of the scalar per-color DILU sweeps (slab_row_dot_stream: 64
rows per wave, their entries streamed through a wave-private LDS window)
against the forced one-lane form, bit for bit, for the fused smoother and the
plain apply; the complex and fp32-matrix instantiations also against the host
backend with the tolerances of tests/test_gpu_dilu_lanes.py.

The matrices are the two 26^3 lattices and the random graph of that file, an
arrow-type matrix whose rows meet every window edge, and a small multipartite
graph whose colors have 1, 63, 64, 65 and 257 rows."""

import copy
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from amgx_amd import AMGConfig, CSRMatrix, create_solver
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.ops import cpu as cpu_ops
from amgx_amd.problems import poisson_3d, poisson_3d_27pt, random_laplacian
from amgx_amd.resources import Resources

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32 = dict(rtol=1e-4, atol=1e-5)
C128 = dict(rtol=1e-12, atol=1e-12)
RELAX = 0.9
GROUP = 64          # hub rows per color of the arrow matrix: one wave
COLOR_SIZES = (1, 63, 64, 65, 257)


def core():
    from amgx_amd import _core
    return _core


def gpu_ops():
    from amgx_amd.ops import gpu
    return gpu


def symmetric_dominant(n, pairs, seed):
    """Symmetric matrix with the given off-diagonal pairs (i, j), negative
    values, and a diagonal of the row's absolute sum plus one."""
    g = np.random.default_rng(seed)
    i, j = np.asarray(pairs, dtype=np.int64).T
    v = -(0.1 + g.random(i.size))
    off = sp.coo_matrix((np.r_[v, v], (np.r_[i, j], np.r_[j, i])),
                        shape=(n, n)).tocsr()
    assert off.nnz == 2 * i.size, "a pair is listed twice"
    diag = np.asarray(abs(off).sum(axis=1)).ravel() + 1.0
    return CSRMatrix.from_scipy((off + sp.diags(diag)).tocsr())


def arrow_matrix(W):
    """Hub rows coupled to leaf rows only, so the hubs of a group share a
    color. Colors: early leaves 0, groups A, B, C 1..3, late leaves 4. The
    64 hubs of a group are one wave of their color, and `part` below gives
    the length of hub h's row in the slab the group is built for: the full
    slab for A (diagonal included), U for B (late leaves), L for C (early
    leaves). In that slab, counted from the wave's first entry, hub 0 spans
    three windows, hub 1 ends exactly at 3 W, hub 2 fills [3 W, 4 W - 1), hub
    3 starts at the last slot of that window and crosses into the next, and
    hubs 4..7 are empty (the diagonal alone in the full slab)."""
    part = [2 * W + 5, W - 5, W - 1, 9, 0, 0, 0, 0]
    g = np.random.default_rng(5)
    part += g.integers(0, 13, GROUP - len(part)).tolist()
    pool = 2 * W + 8
    early = np.arange(pool)
    late = pool + np.arange(pool)
    both = np.r_[early, late]
    n = 2 * pool + 3 * GROUP
    colors = np.zeros(n, dtype=np.int32)
    colors[late] = 4
    pairs = []
    for grp in range(3):
        for h, p in enumerate(part):
            row = 2 * pool + grp * GROUP + h
            colors[row] = 1 + grp
            if grp == 0:
                cols = both[:max(p, 1) - 1]
            elif grp == 1:
                cols = np.r_[late[:p], early[h:h + 2]]
            else:
                cols = np.r_[early[:p], late[h:h + 2]]
            pairs += [(row, int(c)) for c in cols]
    return symmetric_dominant(n, pairs, 6), colors, part


def sized_colors_matrix():
    """Rows in colors of COLOR_SIZES rows, coupled at random to rows of other
    colors."""
    colors = np.repeat(np.arange(len(COLOR_SIZES)), COLOR_SIZES)
    n = colors.size
    g = np.random.default_rng(7)
    pairs = set()
    for i in range(n):
        for j in g.integers(0, n, 5).tolist():
            if colors[i] != colors[j]:
                pairs.add((min(i, j), max(i, j)))
    colors = colors.astype(np.int32)
    return symmetric_dominant(n, sorted(pairs), 8), colors


def make_level(A, seed, colors=None):
    """Device copy, coloring (the device's own, or the given colors) on both
    sides, fixed b and x0."""
    Ag = A.to(DEV)
    if colors is None:
        colg = MatrixColoring.create(Ag)
    else:
        colg = MatrixColoring(torch.from_numpy(colors).to(DEV),
                              int(colors.max()) + 1)
    col = MatrixColoring(colg.colors.cpu(), colg.num_colors)
    g = torch.Generator().manual_seed(seed)
    b = torch.rand(A.n_rows, generator=g, dtype=torch.float64)
    x0 = torch.rand(A.n_rows, generator=g, dtype=torch.float64) - 0.5
    return SimpleNamespace(A=A, Ag=Ag, colg=colg, col=col, b=b, x0=x0)


@pytest.fixture(scope="module")
def levels():
    """Levels shared by the tests; nothing here is modified."""
    W = core().dilu_stream_window(16)
    arrow, arrow_colors, _ = arrow_matrix(W)
    sized, sized_colors = sized_colors_matrix()
    one = CSRMatrix.from_scipy(sp.csr_matrix(np.array([[4.0]])))
    out = {"7pt": make_level(poisson_3d(26, 26, 26), 41),
           "27pt": make_level(poisson_3d_27pt(26, 26, 26), 42),
           "rand": make_level(random_laplacian(16500, 12, seed=11), 43),
           "arrow": make_level(arrow, 44, arrow_colors),
           "sized": make_level(sized, 45, sized_colors),
           "one": make_level(one, 46, np.zeros(1, dtype=np.int32))}
    assert abs(arrow.n_rows - (4 * W + 200)) <= 16
    assert [e - s for s, e in zip(out["sized"].colg.bounds[:-1],
                                  out["sized"].colg.bounds[1:])] \
        == list(COLOR_SIZES)
    return out


NAMES = ("7pt", "27pt", "rand", "arrow", "sized", "one")


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
    g = torch.Generator().manual_seed(47)
    im = torch.rand(2, A.n_cols, generator=g, dtype=torch.float64) - 0.3
    return (Ag, torch.complex(L.b, im[0]).to(DEV),
            torch.complex(L.x0, im[1]).to(DEV))


def trail(G, Ag, e_gpu, colg, bg, x0, **how):
    """x and the scratch vector w after each of two fused sweeps and two
    plain applies."""
    x, out = x0.clone(), []
    for _ in range(2):
        assert G.dilu_smooth(Ag, e_gpu, colg, bg, x, RELAX, **how) is True
        out += [x.clone(), G._scratch(Ag, "dilu_w", Ag.n_cols, x.dtype)
                .clone()]
    for _ in range(2):
        G.dilu_solve(Ag, e_gpu, colg, bg, RELAX, x, **how)
        out += [x.clone(), G._scratch(Ag, "dilu_w", Ag.n_cols, x.dtype)
                .clone()]
    return out


def finite(x):
    return bool(torch.isfinite(torch.view_as_real(x) if x.is_complex()
                               else x).all())


# ---------------------------------------------------------------- bitwise
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_stream_equals_one_lane(levels, name):
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, "f64")
    e_gpu = G.dilu_setup(Ag, L.colg)
    one = trail(G, Ag, e_gpu, L.colg, bg, x0, lanes=1, form="split")
    got = trail(G, Ag, e_gpu, L.colg, bg, x0, form="stream")
    assert finite(got[-2])
    for step, (a, b) in enumerate(zip(one, got)):
        assert torch.equal(a, b), f"step {step}"


@gpu
def test_arrow_rows_meet_the_window_edges(levels):
    """The construction does what arrow_matrix says, read off the slabs."""
    L, G = levels["arrow"], gpu_ops()
    W = core().dilu_stream_window(16)
    st = G._slabs(L.Ag, L.colg)
    bounds = L.colg.bounds
    assert [bounds[c + 1] - bounds[c] for c in (1, 2, 3)] == [GROUP] * 3
    slabs = {1: st.ro_s, 2: G._slab_part(st, True)[0],
             3: G._slab_part(st, False)[0]}
    for color, ro in slabs.items():
        s = bounds[color]
        off = (ro[s:s + GROUP + 1] - ro[s]).cpu().tolist()
        assert off[1] > 2 * W                      # three windows
        assert off[2] == 3 * W                     # ends at an edge
        assert off[3] == 4 * W - 1                 # next starts at base+W-1
        assert off[4] > 4 * W                      # and crosses the edge
        assert off[8] - off[4] == (4 if color == 1 else 0)   # empty rows
    # the last color's U rows are all empty
    ro_u = slabs[2]
    assert int(ro_u[bounds[5]] - ro_u[bounds[4]]) == 0


@gpu
@pytest.mark.parametrize("kind", ["f32A", "c128"])
@pytest.mark.parametrize("name", ["rand", "arrow"])
def test_value_types(levels, name, kind):
    """The fp32-matrix and complex instantiations (windows of 512 and 256
    entries): one fused sweep against the host, then bitwise against one
    lane."""
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, kind)
    Ah = CSRMatrix(Ag.row_offsets.cpu(), Ag.col_indices.cpu(),
                   Ag.values.cpu().to(x0.dtype), n_cols=Ag.n_cols)
    e_ref = cpu_ops.dilu_setup(Ah, L.col)
    b, x1 = bg.cpu(), x0.cpu()
    cpu_ops.dilu_solve(Ah, e_ref, L.col, cpu_ops.residual(Ah, x1, b), RELAX,
                       x1)
    e_gpu = G.dilu_setup(Ag, L.colg)
    x2 = x0.clone()
    assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x2, RELAX,
                         form="stream") is True
    print(name, kind, "max dev", (x2.cpu() - x1).abs().max().item())
    assert x2.dtype == x0.dtype
    assert torch.allclose(x2.cpu(), x1, **(F32 if kind == "f32A" else C128))
    one = trail(G, Ag, e_gpu, L.colg, bg, x0, lanes=1, form="split")
    got = trail(G, Ag, e_gpu, L.colg, bg, x0, form="stream")
    assert finite(got[-2])
    for step, (a, c) in enumerate(zip(one, got)):
        assert torch.equal(a, c), f"step {step}"


# ---------------------------------------------------------------- scratch
@gpu
@pytest.mark.parametrize("name", ["rand", "arrow"])
def test_stale_scratch_is_not_read(levels, name):
    """w and y full of NaN before the fused apply: the result is unchanged."""
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    bg, want = L.b.to(DEV), L.x0.to(DEV)
    assert G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, want, RELAX,
                         form="stream") is True
    for vec in ("dilu_w", "dilu_y"):
        G._scratch(L.Ag, vec, L.Ag.n_cols, want.dtype).fill_(float("nan"))
    x = L.x0.to(DEV)
    assert G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, x, RELAX,
                         form="stream") is True
    assert finite(x) and torch.equal(x, want)


@gpu
@pytest.mark.parametrize("name", ["27pt", "arrow"])
def test_three_sweeps_equal_three_calls(levels, name):
    L, G = levels[name], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    bg, x1, x3 = L.b.to(DEV), L.x0.to(DEV), L.x0.to(DEV)
    for _ in range(3):
        G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, x1, RELAX, form="stream")
    G.dilu_smooth(L.Ag, e_gpu, L.colg, bg, x3, RELAX, sweeps=3,
                  form="stream")
    assert torch.equal(x1, x3)


# ---------------------------------------------------------------- routing
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_routed_equals_forced_forms(levels, name):
    L, G = levels[name], gpu_ops()
    Ag, bg, x0 = typed(L, "f64")
    e_gpu = G.dilu_setup(Ag, L.colg)
    out = []
    for how in (dict(), dict(form="stream"), dict(lanes=1, form="split"),
                dict(lanes=8, form="split")):
        x = x0.clone()
        assert G.dilu_smooth(Ag, e_gpu, L.colg, bg, x, RELAX, **how) is True
        G.dilu_solve(Ag, e_gpu, L.colg, bg, RELAX, x, **how)
        out.append(x)
    for x in out[1:]:
        assert torch.equal(out[0], x)


@gpu
def test_stream_form_takes_no_lanes(levels):
    L, G = levels["7pt"], gpu_ops()
    e_gpu = G.dilu_setup(L.Ag, L.colg)
    with pytest.raises(RuntimeError):
        G.dilu_solve(L.Ag, e_gpu, L.colg, L.b.to(DEV), RELAX, L.x0.to(DEV),
                     lanes=8, form="stream")
    with pytest.raises(RuntimeError):
        G.dilu_smooth(L.Ag, e_gpu, L.colg, L.b.to(DEV), L.x0.to(DEV), RELAX,
                      lanes=4)


@gpu
def test_routing_rule():
    """The rule at the points of its table (profiles/NOTES.md, "DILU stream
    form"): every slab class measured takes the stream form where its colors
    have 43.7 k rows, and none at 13.5 k or 5.7 k rows per color (the
    boundary of 16384 rows is on the safe side of the measured tie); an empty
    slab never does."""
    C = core()
    pick = C.dilu_stream
    assert C.DILU_STREAM_ROWS == 64 and C.DILU_STREAM_WINDOW == 512
    assert C.dilu_stream_window(16) == 512      # fp64
    assert C.dilu_stream_window(12) == 512      # fp32 matrix, fp64 vectors
    assert C.dilu_stream_window(32) == 256      # complex128
    assert C.DILU_STREAM_MIN_ROWS_FULL == C.DILU_STREAM_MIN_ROWS_SPLIT == 16384
    for epr in (6.97, 10.14, 12.63):
        assert pick(epr, 43691) and pick(epr, 2147844)
        assert not pick(epr, 13475) and not pick(epr, 5744)
    for epr in (2.98, 4.57, 5.82):
        assert pick(epr, 43691, split=True)
        assert not pick(epr, 13475, split=True)
    assert pick(7.0, 16384) and not pick(7.0, 16383)
    assert not pick(0.0, 1 << 20, split=True)


# ---------------------------------------------------------------- graph
@gpu
def test_graph_replay_equals_eager():
    """One flagship V-cycle with the fine level's colors routed to the stream
    form, captured and replayed, then eager."""
    from bench import FGMRES_AGG
    A = poisson_3d(40, 40, 40, device=DEV)
    g = torch.Generator().manual_seed(48)
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
        fine = amg.hierarchy.levels[0].A
        assert fine.n_rows == A.n_rows
        bounds = fine.coloring.bounds
        routed = [core().dilu_stream(fine.nnz / fine.n_rows, e - s_)
                  for s_, e in zip(bounds[:-1], bounds[1:])]
        assert any(routed) and not all(routed)     # both forms in the graph
        out[use_graph] = x.clone()
    assert bool(torch.isfinite(out[1]).all())
    assert torch.equal(out[0], out[1])
