"""Rank grades and the Spearman rank correlation matrix (kernel K24).

Spearman's rho is Pearson's r on mid-ranks, and mid-ranks on a fine grid
of cells need no sort:

1. `rank_grid`: per column, ascending cutoffs c_0 < ... < c_{q-1} from the
   quantile sketch at j / cells. A value x lies in cell(x) = #{j : c_j < x}
   (right-closed cells, the placement of the binning kernel K6).
2. `grade_counts`: one read-only pass counts the rows of every cell; the
   counts merge across ranks with one int64 all-reduce.
3. `grade_tables`: every cell gets the centred, scaled mid-rank of its rows,
   grade = (midrank - (m + 1) / 2) / m in (-1/2, 1/2), m = non-null rows.
4. `grade_columns`: one transform pass writes the f32 grade of every row
   into a reused slab, which feeds the Gram kernel of the Pearson path (K8).

- HIP path: ops/hip/grades.hip (`grade_counts`, `grade_apply`).
- torch path (CPU; also the tests' reference): torch.bucketize on fp64,
  bincount, gather.

Rows inside one cell are tied: the result is Spearman's rho of the data
tied on the grid. Columns with at most `cells` distinct values, or at most
`cells` rows, get a cell per value and the exact rho.
"""

from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from anovos_amd.core import dist
from anovos_amd.ops import backend
from anovos_amd.ops import histogram as hist_ops
from anovos_amd.ops import stats as stats_ops

# cells of a column's grid the kernel stages in LDS: GRADE_MAX_CELLS of
# ops/hip/anovos_kernels.h
GRADE_MAX_CELLS = 4096

# f32 grade scratch of one row slab of spearman_matrix. The Gram kernel
# sizes its grid to one wave of resident blocks, so slabs must stay large;
# tools/bench_spearman.py times 1, 4 and 16 GiB.
SLAB_BYTES = 4 << 30


def _predecessor(v: float, dtype: torch.dtype) -> float:
    """The next value below v that the column's dtype can hold."""
    if dtype == torch.float32:
        return float(np.nextafter(np.float32(v), np.float32(-np.inf)))
    return float(np.nextafter(np.float64(v), -np.inf))


def _grid_from_quantiles(q: Sequence[float], dtype: torch.dtype, cells: int) -> np.ndarray:
    """Drop NaN, deduplicate, and put one cutoff just below every value that
    came back for two or more probabilities: such a value holds at least
    1 / cells of the rows, and without the extra cutoff its cell would also
    take the few rows between the previous cutoff and the value itself.
    Every repeat freed a slot, so the grid stays within cells - 1 cutoffs."""
    q = np.asarray(q, dtype=np.float64)
    q = q[~np.isnan(q)]
    vals, reps = np.unique(q, return_counts=True)
    extra = [p for p in (_predecessor(v, dtype) for v in vals[reps >= 2]) if not math.isnan(p)]
    grid = np.unique(np.concatenate([vals, np.asarray(extra, dtype=np.float64)]))
    return grid[: cells - 1]


def rank_grid(idf, cols: List[str], cells: int) -> List[np.ndarray]:
    """Global (rank-identical) grid cutoffs of every column: fp64 arrays,
    strictly ascending, at most cells - 1 entries each; empty for an
    all-null column. Quantiles at j / cells, j = 1 .. cells - 1. Columns
    that take an exact quantile path (at most EXACT_N_THRESHOLD non-null
    rows, integral with a range below 4096, or holding infinities) are
    queried with rel_err = 1 / (2 cells): the default 0.01 folds each 1 %
    tail of an exact path into a single cell. Sketch columns keep the
    default, a tighter tolerance there costs refinement reads. Collective."""
    cols = list(cols)
    probs = [j / cells for j in range(1, cells)]
    tight = 1.0 / (2.0 * cells)
    moments = stats_ops.frame_moments(idf, cols) if cols else {}
    small, integral, sketch = [], [], []
    for c in cols:
        m = moments[c]
        if not m.n > 0 or m.min != m.min:
            continue  # all-null: empty grid
        if m.n <= hist_ops.EXACT_N_THRESHOLD or math.isinf(m.min) or math.isinf(m.max):
            small.append(c)
        elif m.integral and 0 < (m.max - m.min) < 4096:
            integral.append(c)
        else:
            sketch.append(c)
    q = {}
    # the exact paths are called directly: approx_quantiles keys its value
    # cache by probability alone, and values queried at another rel_err
    # must not land in it
    if small:
        q.update(hist_ops._exact_quantiles(idf, small, probs, moments, rel_err=tight))
    if integral:
        q.update(hist_ops._exact_integral_quantiles(idf, integral, probs, moments, rel_err=tight))
    if sketch:
        q.update(hist_ops.approx_quantiles(idf, sketch, probs, moments=moments))
    return [
        _grid_from_quantiles(q[c], idf.col(c).data.dtype, cells) if c in q else np.zeros(0, dtype=np.float64)
        for c in cols
    ]


def grade_tables(counts, m: Optional[int] = None) -> np.ndarray:
    """fp64 grade of every cell from its global row count n_j, on the host
    (the kernel takes them rounded to f32): before_j = sum_{i<j} n_i,
    midrank_j = before_j + (n_j + 1) / 2, grade_j = (midrank_j - (m + 1) / 2)
    / m with m = sum n_j. The grades weighted by n_j sum to zero and lie in
    (-1/2, 1/2). All zeros when m = 0."""
    n = np.asarray(counts, dtype=np.float64)
    if m is None:
        m = n.sum()
    m = float(m)
    if m <= 0:
        return np.zeros(n.shape, dtype=np.float64)
    before = np.cumsum(n) - n
    midrank = before + (n + 1.0) / 2.0
    return (midrank - (m + 1.0) / 2.0) / m


def _as_f64(c) -> torch.Tensor:
    return torch.as_tensor(np.asarray(c, dtype=np.float64) if not torch.is_tensor(c) else c).to(torch.float64)


def _cells_torch(t: torch.Tensor, cuts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cell index, null mask) of one column: the torch path."""
    null = torch.isnan(t)
    cell = torch.bucketize(t.to(torch.float64), cuts.to(t.device), right=False)
    return cell, null


def _grades_torch(t: torch.Tensor, cuts: torch.Tensor, table: torch.Tensor, null_grade: float) -> torch.Tensor:
    """table[cell(x)] in the table's dtype, null_grade for NaN: the torch path."""
    cell, null = _cells_torch(t, cuts)
    g = table.to(t.device)[cell]
    return torch.where(null, torch.full_like(g, float(null_grade)), g)


def grade_counts(tensors: Sequence[torch.Tensor], cutoffs: Sequence) -> torch.Tensor:
    """int64 [ncols, max_ncut + 2] LOCAL counts on the columns' device:
    slot 0 = nulls (NaN), slot 1 + j = rows of cell j = #{c : c < x}."""
    cuts = [_as_f64(c).contiguous() for c in cutoffs]
    if tensors and tensors[0].is_cuda and backend.use_hip(tensors[0]):
        return backend.hip_ext().grade_counts([t.contiguous() for t in tensors], cuts)
    stride = max([int(c.numel()) + 2 for c in cuts] + [2])
    dev = tensors[0].device if tensors else torch.device("cpu")
    out = torch.zeros(len(tensors), stride, dtype=torch.int64, device=dev)
    for i, (t, c) in enumerate(zip(tensors, cuts)):
        cell, null = _cells_torch(t, c)
        slot = torch.where(null, torch.zeros_like(cell), cell + 1)
        out[i] = torch.bincount(slot.reshape(-1), minlength=stride)
    return out


def grade_columns(
    tensors: Sequence[torch.Tensor],
    cutoffs: Sequence,
    tables: Sequence,
    null_grade: float = 0.0,
    outs: Optional[Sequence[torch.Tensor]] = None,
) -> List[torch.Tensor]:
    """Per column the f32 tensor tables[i][cell(x)], null_grade for NaN.
    `outs`, when given, are dense f32 tensors of the columns' lengths that
    receive the result (a scratch slab reused across calls)."""
    cuts = [_as_f64(c).contiguous() for c in cutoffs]
    tabs = [torch.as_tensor(np.asarray(t, dtype=np.float32) if not torch.is_tensor(t) else t).to(torch.float32)
            for t in tables]
    if tensors and tensors[0].is_cuda and backend.use_hip(tensors[0]):
        res = backend.hip_ext().grade_apply(
            [t.contiguous() for t in tensors], cuts, tabs, float(null_grade),
            list(outs) if outs is not None else None,
        )
        return list(res)
    res = []
    for i, (t, c, tab) in enumerate(zip(tensors, cuts, tabs)):
        g = _grades_torch(t, c, tab, null_grade)
        if outs is not None:
            outs[i].copy_(g)
            g = outs[i]
        res.append(g)
    return res


def column_grades(idf, cols: List[str], cells: int):
    """[(grid fp64, table fp64)] of every column, from
    Column.cache[("grades", cells)] where present; the others take the
    quantile query, one counting pass and one int64 all-reduce together.
    Collective."""
    key = ("grades", cells)
    todo = [c for c in dict.fromkeys(cols) if key not in idf.col(c).cache]
    if todo:
        grids = rank_grid(idf, todo, cells)
        local = grade_counts([idf.col(c).data for c in todo], grids)
        counts = dist.all_reduce_(local, "sum").cpu().numpy()
        for i, c in enumerate(todo):
            n = counts[i, 1 : len(grids[i]) + 2]
            idf.col(c).cache[key] = (grids[i], grade_tables(n, int(n.sum())))
    return [idf.col(c).cache[key] for c in cols]


def spearman_matrix(idf, cols: List[str], cells: int = 1024, use_bf16: bool = True) -> np.ndarray:
    """Global Spearman rank correlation matrix over numeric columns:
    Pearson's r of the columns' grades on a grid of `cells` cells.

    Null convention of the Pearson path: ranks are taken among a column's
    non-null rows, and a null takes the mean rank, so it contributes zero.
    With no nulls the result is Spearman's rho of the grid-tied data. The
    diagonal is 1; a column without variance (constant, all-null) gives 0
    off the diagonal. Grid and grade tables are cached per column, so a
    second call goes straight to the transform pass. Collective."""
    cols = list(cols)
    k = len(cols)
    grades = column_grades(idf, cols, cells)
    grids = [g for g, _ in grades]
    tables = [t for _, t in grades]
    tensors = [idf.col(c).data for c in cols]
    dev = tensors[0].device
    n = int(tensors[0].shape[0])
    on_gpu = dev.type == "cuda" and backend.use_hip(tensors[0])
    gram = torch.zeros(k, k, dtype=torch.float64, device=dev)
    # rows of one slab: a multiple of four keeps every scratch row on a
    # 16-byte line
    rows = max(4, (SLAB_BYTES // (4 * k)) & ~3)
    if on_gpu:
        ext = backend.hip_ext()
        tensors = [t.contiguous() for t in tensors]
        scratch = torch.empty(k, min(rows, max(n, 1)), dtype=torch.float32, device=dev)
        zero_means = torch.zeros(k, dtype=torch.float32, device=dev)
    for start in range(0, n, rows):
        stop = min(n, start + rows)
        slab = [t[start:stop] for t in tensors]
        if on_gpu:
            outs = [scratch[i, : stop - start] for i in range(k)]
            grade_columns(slab, grids, tables, 0.0, outs=outs)
            if use_bf16:
                g = ext.centered_gram_bf16(outs, zero_means)
            else:
                X = scratch[:, : stop - start]
                g = X @ X.T
        else:
            # fp64 grades: exact rho where every value has a cell of its own
            X = torch.stack([_grades_torch(t, torch.from_numpy(c), torch.from_numpy(tab), 0.0)
                             for t, c, tab in zip(slab, grids, tables)])
            g = X @ X.T
        gram += g.to(torch.float64)
    if dist.is_dist():
        dist.all_reduce_(gram, "sum")
    g = gram.cpu().numpy()
    # X @ X.T goes through a general matrix product, which on some hosts
    # leaves g[i, j] and g[j, i] an ulp apart; a symmetric g stays as it is
    g = 0.5 * (g + g.T)
    d = np.sqrt(np.clip(np.diag(g), 1e-300, None))
    corr = g / np.outer(d, d)
    np.fill_diagonal(corr, 1.0)
    return np.clip(corr, -1.0, 1.0)
