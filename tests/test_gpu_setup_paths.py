"""The native setup paths against their yardsticks, exactly.

Colours and matching roots against the numpy replays of
``tests/test_setup_replay.py``, for every number k of rounds per read-back;
the root renumbering, the colour order, the aggregate-membership CSR and the
slab structure against the torch expressions they replace, evaluated here; the
Galerkin product with and without the handed-over aggregate CSR; and the
hierarchy of a whole setup under k = 1 and the default k."""

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from amgx_amd import AMGConfig, CSRMatrix, create_solver, ops
from amgx_amd.amg.coloring import MatrixColoring
from amgx_amd.problems import poisson_3d
from amgx_amd.resources import Resources
from tests.test_setup_replay import (COLORING, MATCHING, renumber,
                                     replay_coloring, replay_matching)

DEV = "cuda:0"
BATCHES = [1, 3, 0]     # rounds per read-back; 0 = the default rule


def gpu():
    from amgx_amd.ops import gpu as g
    return g


def to_matrix(g, diag=4.0, off=-1.0, device=DEV):
    """the graph as a matrix with one diagonal and one off-diagonal value"""
    rows = np.repeat(np.arange(g.n), np.diff(g.ro))
    va = np.where(g.ci == rows, diag, off).astype(np.float64)
    return CSRMatrix(torch.from_numpy(g.ro).to(device),
                     torch.from_numpy(g.ci).to(device),
                     torch.from_numpy(va).to(device), n_cols=g.n_cols)


_replays = {}


def replay(kind, name):
    """one replay per graph, shared by the cases"""
    key = (kind, name)
    if key not in _replays:
        _replays[key] = replay_coloring(COLORING[name])[0] \
            if kind == "color" else replay_matching(MATCHING[name])[0]
    return _replays[key]


# ==================================================================== colouring
@pytest.mark.parametrize("batch", BATCHES, ids=["k1", "k3", "kdef"])
@pytest.mark.parametrize("name", list(COLORING))
def test_colors_equal_replay(name, batch):
    g = COLORING[name]
    colors, num = gpu().color_matrix(to_matrix(g), batch=batch)
    want = replay("color", name)
    assert colors.dtype == torch.int32
    assert np.array_equal(colors.cpu().numpy(), want)
    assert num == int(want.max()) + 1


def test_colors_seeded_and_multihash_are_batch_invariant():
    """seeds of the other schemes, and MULTI_HASH rounds ahead of the greedy
    ones: a surplus round of either kind copies the colours"""
    A = to_matrix(COLORING["chords-513"])
    for kw in ({"seed": 7}, {"seed": 11, "multihash_rounds": 7}):
        ref = gpu().color_matrix(A, batch=1, **kw)
        for batch in (3, 0):
            got = gpu().color_matrix(A, batch=batch, **kw)
            assert got[1] == ref[1] and torch.equal(got[0], ref[0])
    want, _ = replay_coloring(COLORING["chords-513"], seed=7)
    assert np.array_equal(
        gpu().color_matrix(A, seed=7)[0].cpu().numpy(), want)


# ===================================================================== matching
@pytest.mark.parametrize("batch", BATCHES, ids=["k1", "k3", "kdef"])
@pytest.mark.parametrize("name", list(MATCHING))
def test_matching_equals_replay(name, batch):
    g = MATCHING[name]
    A = to_matrix(g)
    roots = gpu().size2_roots(A, batch=batch)
    want = replay("match", name)
    assert roots.dtype == torch.int32
    assert np.array_equal(roots.cpu().numpy(), want)
    assert torch.equal(gpu().size2_roots(A, batch=batch, weights=True), roots)
    agg, num = gpu().size2_matching(A, batch=batch)
    uniq, inv = torch.unique(roots, sorted=True, return_inverse=True)
    assert agg.dtype == torch.int32 and num == int(uniq.numel())
    assert torch.equal(agg, inv.to(torch.int32))
    assert (np.array_equal(agg.cpu().numpy(), renumber(want)[0])
            and num == renumber(want)[1])


def test_matching_general_weights_is_batch_invariant():
    A = poisson_3d(6, 6, 6, device=DEV)
    g = torch.Generator().manual_seed(6)
    bump = 1.0 + 0.5 * torch.rand(A.n_rows, generator=g, dtype=torch.float64)
    va = A.values.clone()
    didx = ops.compute_diag_index(A).long()
    va[didx] = va[didx] * bump.to(DEV)
    A = CSRMatrix(A.row_offsets, A.col_indices, va, n_cols=A.n_cols)
    ref = gpu().size2_roots(A, batch=1)
    for batch in (3, 0):
        assert torch.equal(gpu().size2_roots(A, batch=batch), ref)
        # edge weights computed once per call: the same bits, the same ties
        assert torch.equal(gpu().size2_roots(A, batch=batch, weights=True),
                           ref)
        agg, num = gpu().size2_matching(A, batch=batch)
        uniq, inv = torch.unique(ref, sorted=True, return_inverse=True)
        assert num == int(uniq.numel())
        assert torch.equal(agg, inv.to(torch.int32))


# ================================================================== key orders
def torch_order(keys, nkeys):
    k64 = keys.to(torch.int64)
    order = torch.argsort(k64, stable=True).to(torch.int32)
    counts = torch.bincount(k64, minlength=nkeys)
    off = torch.zeros(nkeys + 1, dtype=torch.int64, device=keys.device)
    off[1:] = torch.cumsum(counts, 0)
    return order, off.to(torch.int32)


def _rand_keys(n, nkeys, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, nkeys, (n,), generator=g).to(torch.int32).to(DEV)


COLOR_INPUTS = {
    "one-color": (torch.zeros(700, dtype=torch.int32), 1),
    "65-colors": (None, 65),
    "empty-class": (None, 9),
    "n1": (torch.zeros(1, dtype=torch.int32), 1),
}


@pytest.mark.parametrize("name", list(COLOR_INPUTS))
def test_color_order_equals_torch(name):
    colors, num = COLOR_INPUTS[name]
    if name == "65-colors":
        colors = _rand_keys(1500, 65, 65)
        colors[:65] = torch.arange(65, dtype=torch.int32, device=DEV)
    elif name == "empty-class":
        colors = _rand_keys(1000, 9, 9)
        colors[colors == 4] = 5         # class 4 is empty, as is the last
        colors[colors == 8] = 0
    colors = colors.to(DEV)
    col = MatrixColoring(colors, num)
    order, off = torch_order(colors, num)
    assert col.rows_sorted.dtype == torch.int32
    assert torch.equal(col.rows_sorted, order)
    assert col.bounds == off.cpu().tolist()
    assert col.bounds_dev.dtype == torch.int32
    assert torch.equal(col.bounds_dev, off)
    assert col.num_colors == num and len(col.bounds) == num + 1
    for c in range(num):
        assert torch.equal(col.rows_of(c), order[off[c]:off[c + 1]])


def _aggregates(name):
    if name == "singletons-and-pairs":
        agg = torch.arange(400, dtype=torch.int32).repeat_interleave(2)[:650]
        agg[300:] = torch.arange(150, 500, dtype=torch.int32)
        return agg, 500
    if name == "one-of-300":
        agg = torch.arange(40, dtype=torch.int32).repeat_interleave(2)
        return torch.cat([agg[:30], torch.full((300,), 15, dtype=torch.int32),
                          agg[30:]]), 40
    agg = _rand_keys(1000, 333, 3).cpu()     # not monotone in the row
    agg[:333] = torch.arange(332, -1, -1, dtype=torch.int32)
    return agg, 333


@pytest.mark.parametrize("name", ["singletons-and-pairs", "one-of-300",
                                  "not-monotone"])
def test_aggregate_csr_equals_torch(name):
    agg, num = _aggregates(name)
    agg = agg.to(DEV)
    off, fids = gpu().aggregate_csr(agg, num)
    order, want_off = torch_order(agg, num)
    assert off.dtype == torch.int32 and fids.dtype == torch.int32
    assert torch.equal(fids, order) and torch.equal(off, want_off)


def test_galerkin_with_and_without_structure():
    A = poisson_3d(9, 8, 7, device=DEV)
    agg, num = ops.size2_matching(A)
    structure = gpu().aggregate_csr(agg, num)
    a = ops.galerkin_aggregation(A, agg, num)
    b = ops.galerkin_aggregation(A, agg, num, structure=structure)
    assert torch.equal(a.row_offsets, b.row_offsets)
    assert torch.equal(a.col_indices, b.col_indices)
    assert torch.equal(a.values, b.values)
    assert a.n_rows == num and a.n_cols == b.n_cols


# ======================================================================== slabs
def torch_slabs(A, rows_sorted):
    n = A.n_rows
    perm = rows_sorted.to(torch.int64)
    ro64 = A.row_offsets.to(torch.int64)
    counts = (ro64[1:] - ro64[:-1])[perm]
    ro_s = torch.zeros(n + 1, dtype=torch.int32, device=A.device)
    csum = torch.cumsum(counts, 0)
    ro_s[1:] = csum.to(torch.int32)
    nzmap = (torch.repeat_interleave(ro64[perm], counts)
             + torch.arange(int(A.nnz), device=A.device, dtype=torch.int64)
             - torch.repeat_interleave(csum - counts, counts))
    slot = torch.empty(n, dtype=torch.int32, device=A.device)
    slot[perm] = torch.arange(n, dtype=torch.int32, device=A.device)
    return ro_s, A.col_indices[nzmap], nzmap, slot


def _slab_matrix(name):
    rng = np.random.default_rng(5)
    if name == "n1":
        lens = [1]
    elif name == "width-8":
        lens = [8] * 300
    elif name == "width-9":
        lens = [9] * 300
    else:   # empty rows, one row of 300 entries
        lens = rng.integers(0, 12, 520).tolist()
        lens[::7] = [0] * len(lens[::7])
        lens[257] = 300
    n = len(lens)
    n_cols = max(n, 320)
    rows = [np.sort(rng.choice(n_cols, k, replace=False)) for k in lens]
    ro = np.zeros(n + 1, dtype=np.int32)
    ro[1:] = np.cumsum(lens)
    ci = np.concatenate(rows).astype(np.int32) if sum(lens) else \
        np.zeros(0, dtype=np.int32)
    va = rng.standard_normal(ci.size)
    A = CSRMatrix(torch.from_numpy(ro).to(DEV), torch.from_numpy(ci).to(DEV),
                  torch.from_numpy(va).to(DEV), n_cols=n_cols)
    colors = torch.from_numpy(rng.integers(0, 5, n).astype(np.int32)).to(DEV)
    return A, colors


@pytest.mark.parametrize("lanes", [0, 1, 8])
@pytest.mark.parametrize("name", ["general", "width-8", "width-9", "n1"])
def test_slab_structure_equals_torch(name, lanes):
    from amgx_amd import _core
    A, colors = _slab_matrix(name)
    col = MatrixColoring(colors, 5)     # rows by colour: not the identity
    if A.n_rows > 1:
        assert not torch.equal(col.rows_sorted.long(),
                               torch.arange(A.n_rows, device=DEV))
    got = _core.slab_structure(A.row_offsets, A.col_indices, col.rows_sorted,
                               lanes)
    want = torch_slabs(A, col.rows_sorted)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32
        assert torch.equal(g.to(w.dtype), w)
    if lanes == 0:
        st = gpu()._slabs(A, col)
        assert torch.equal(st.ro_s, want[0]) and torch.equal(st.ci_s, want[1])
        assert torch.equal(st.nzmap.long(), want[2])
        assert torch.equal(st.slot_of_row, want[3])
        assert torch.equal(st.perm, col.rows_sorted.long())
        assert torch.equal(gpu()._gather_nz(A.values, st.nzmap),
                           A.values[want[2]])


def test_slab_structure_rejects_a_non_permutation():
    from amgx_amd import _core
    A, _ = _slab_matrix("general")
    rows = torch.zeros(A.n_rows, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        _core.slab_structure(A.row_offsets, A.col_indices, rows, 0)


# =================================================================== end to end
def test_hierarchy_is_batch_invariant(monkeypatch):
    from bench import FGMRES_AGG
    A = poisson_3d(12, 12, 12, device=DEV)
    b = torch.ones(A.n_rows, dtype=torch.float64, device=DEV)
    out = {}
    for batch in (1, 0):
        monkeypatch.setattr(gpu(), "ROUND_BATCH", batch)
        s = create_solver(AMGConfig.from_dict(copy.deepcopy(FGMRES_AGG))
                          .root_scope(), resources=Resources(DEV))
        s.setup(A)
        x = torch.zeros_like(b)
        st = s.solve(b, x, zero_initial_guess=True)
        levels = s.precond.hierarchy.levels
        out[batch] = ([lv.A.n_rows for lv in levels],
                      [lv.A.coloring.colors.clone() for lv in levels
                       if lv.A.coloring is not None],
                      [lv.aggregates.clone() for lv in levels[:-1]],
                      x.clone(), st.iterations)
    assert len(out[0][0]) >= 3 and out[0][0] == out[1][0]
    assert len(out[0][1]) >= 2 and len(out[0][1]) == len(out[1][1])
    for i in (1, 2):
        for p, q in zip(out[0][i], out[1][i]):
            assert torch.equal(p, q)
    assert out[0][4] == out[1][4] and torch.equal(out[0][3], out[1][3])


def test_smoke_runs():
    import __graft_entry__ as entry
    entry.smoke()
