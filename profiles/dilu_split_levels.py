#!/usr/bin/env python3
"""Per-level shapes of the flagship hierarchy (256^3 Poisson, bench.py's
FGMRES_AGG) and the scalar DILU byte model summed over the levels that take
the per-color path: bytes of one smoother apply for the fused forward sweep,
the in-place backward sweep over U (bwd_split), the full-slab backward sweep
it replaced (bwd_full), the z memset and the trailing axpy, plus one residual
per level (csrmv). Then the cold build time of the fine level's U part.

    python profiles/dilu_split_levels.py
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from amgx_amd import AMGConfig, _core, create_solver  # noqa: E402
from amgx_amd.ops import gpu as G  # noqa: E402
from amgx_amd.problems import poisson_3d  # noqa: E402
from amgx_amd.resources import Resources  # noqa: E402
from bench import FGMRES_AGG  # noqa: E402

dev = "cuda:0"
A = poisson_3d(256, 256, 256, device=dev)
s = create_solver(AMGConfig.from_dict(FGMRES_AGG).root_scope(),
                  resources=Resources(dev))
s.setup(A)
torch.cuda.synchronize()
hier = s.precond.hierarchy
tot = {"fwd": 0, "bwd_split": 0, "bwd_full": 0, "memset": 0, "axpy": 0,
       "colors": 0, "csrmv": 0}
for i, lvl in enumerate(hier.levels[:-1]):
    M = lvl.A
    n, nnz = M.n_rows, M.nnz
    split = n > _core.DILU_SMALL_ROWS
    rec = {"level": i, "n": n, "nnz": nnz, "colors": M.coloring.num_colors,
           "per_color_path": split}
    if split:
        st = G._slabs(M, M.coloring)
        nnz_u = st.upper[1].numel()
        rec["nnz_u"] = nnz_u
        sweep = n * 16 + 4          # offsets + rows_sorted + Einv
        tot["fwd"] += nnz * 12 + sweep + n * 32       # b, x, w read; w write
        tot["bwd_split"] += nnz_u * 12 + sweep + n * 32   # w rw, x rw
        tot["bwd_full"] += nnz * 12 + sweep + n * 24      # w, z read; z write
        tot["memset"] += n * 8
        tot["axpy"] += n * 24
        tot["colors"] += M.coloring.num_colors
    tot["csrmv"] += nnz * 12 + (n + 1) * 4 + n * 24
    print(json.dumps(rec))
print(json.dumps({"bytes_per_apply_per_color_levels": tot}))
# cold build of the fine level's U structure and value gather
st = G._slabs(A, A.coloring)
for rep in range(2):
    st.upper = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    part = G._slab_part(st, True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    G._gather_part(s.precond.hierarchy.levels[0].smoother.Einv.va_s, part)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(json.dumps({"fine_U_structure_ms": (t1 - t0) * 1e3,
                      "fine_U_value_gather_ms": (t2 - t1) * 1e3}))
