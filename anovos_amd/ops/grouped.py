"""Moments of numerical columns grouped by a categorical column (kernel K23).

A categorical column is a tensor of int32 dictionary codes; a code outside
[0, dictionary size) — NULL_CODE included — takes the null slot after the
last category. For a pair (categorical c, numerical v) every slot gets
(n, s1, s2) = (#rows, sum d, sum d^2) with d = x - a_v over its rows whose
x is not NaN, where the shift a_v is the global mean of v (rank-identical,
from the cached frame moments). The triples merge across ranks with one
all-reduce and are converted on the host in fp64.

- HIP path: ops/hip/grouped_moments.hip — value columns that share a code
  column are packed into one work item, per-thread private LDS
  accumulators, a deterministic two-stage reduce, no floating-point atomic.
- torch path (CPU; also the reference inside the tests and the
  benchmark's baseline): bincount for n, index_add_ over fp64 d and d^2.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from anovos_amd.core import dist
from anovos_amd.ops import backend, stats
from anovos_amd.ops.groupby import align_dictionaries

# Dictionaries with more slots (categories + null slot) than this take the
# torch path on the GPU as well: the kernel reads a pair's two columns once
# per window of GRP_CELLS slots, the torch path a fixed number of times.
# Measured on 1x MI355X, f32, 4M rows (profiles/bench_grouped_moments_k23.log,
# docs/BENCHMARKS.md): no crossover up to the largest dictionary timed — at
# 32 768 slots the kernel takes 5.8 ms per pair, the torch path 1.1 s (its
# fp64 index_add_ costs 0.5 - 2.8 s per pair at every size from 16 slots
# up). The kernel's time grows by about 0.18 us per slot and pair, so the
# limit stays at the largest size that was measured.
KERNEL_MAX_SLOTS = 32768

# fp64 triples of one launch: bounds the flat buffer that is allocated,
# all-reduced and copied to the host at once
LAUNCH_OUT_BYTES = 256 << 20


def _slots(codes: torch.Tensor, size: int) -> torch.Tensor:
    c = codes.to(torch.int64)
    return torch.where((c >= 0) & (c < size), c, torch.full_like(c, size))


def grouped_sums_torch(codes: torch.Tensor, size: int, x: torch.Tensor, shift: float) -> torch.Tensor:
    """[size + 1, 3] fp64 (n, s1, s2) of one pair: the torch path."""
    slot = _slots(codes, size)
    ok = ~torch.isnan(x)
    slot = slot[ok]
    d = x[ok].to(torch.float64) - shift
    out = torch.zeros(size + 1, 3, dtype=torch.float64, device=x.device)
    out[:, 0] = torch.bincount(slot, minlength=size + 1).to(torch.float64)
    out[:, 1].index_add_(0, slot, d)
    out[:, 2].index_add_(0, slot, d * d)
    return out


def _launches(cells: Sequence[int], budget_bytes: int) -> List[Tuple[int, int]]:
    """[start, stop) ranges of consecutive pairs whose blocks together stay
    within the budget; a block larger than the budget goes alone."""
    out, start, used = [], 0, 0
    for q, c in enumerate(cells):
        if q > start and used + 24 * c > budget_bytes:
            out.append((start, q))
            start, used = q, 0
        used += 24 * c
    if len(cells) > start:
        out.append((start, len(cells)))
    return out


def grouped_moments(
    idf, cat_cols: List[str], num_cols: List[str], pairs: Optional[List[Tuple[str, str]]] = None
) -> Dict[Tuple[str, str], np.ndarray]:
    """Global per-group moments of every pair: {(cat, num): float64 array
    [len(dict) + 1, 3]} with rows (n, mean, M2) in dictionary order, the
    null slot last, M2 = sum (x - mean_g)^2; slots without a row hold NaN
    for mean and M2. pairs=None means every (cat, num). Collective: every
    rank calls it with the same columns and pairs."""
    cat_cols, num_cols = list(cat_cols), list(num_cols)
    for c in cat_cols:
        if idf.col(c).kind != "categorical":
            raise TypeError(f"grouped_moments needs categorical group columns, got '{c}'")
    for c in num_cols:
        if idf.col(c).kind != "numerical":
            raise TypeError(f"grouped_moments needs numerical value columns, got '{c}'")
    if pairs is None:
        pairs = [(c, v) for c in cat_cols for v in num_cols]
    pairs = [tuple(p) for p in pairs]
    # the slot layout keys off dictionary sizes: they must be rank-identical
    align_dictionaries(idf, cat_cols)
    cpos = {c: k for k, c in enumerate(cat_cols)}
    vpos = {v: k for k, v in enumerate(num_cols)}
    sizes = [len(idf.col(c).dictionary or []) for c in cat_cols]
    mom = stats.frame_moments(idf, num_cols) if num_cols else {}
    shifts = []
    for v in num_cols:
        a = mom[v].mean
        shifts.append(float(a) if np.isfinite(a) else 0.0)  # all-null (or non-finite) column: 0
    pc = [cpos[c] for c, _ in pairs]
    pv = [vpos[v] for _, v in pairs]
    cells = [sizes[c] + 1 for c in pc]
    codes = [idf.col(c).data for c in cat_cols]
    values = [idf.col(v).data for v in num_cols]
    dev = codes[0].device if codes else idf.device

    on_gpu = bool(codes) and bool(values) and all(t.is_cuda for t in codes + values) and backend.use_hip(codes[0])
    if on_gpu:
        ext = backend.hip_ext()
        codes = [t.contiguous() if t.dtype == torch.int32 else t.to(torch.int32).contiguous() for t in codes]
        values = [t.contiguous() if t.dtype in (torch.float32, torch.float64) else t.to(torch.float64).contiguous()
                  for t in values]

    out: Dict[Tuple[str, str], np.ndarray] = {}
    for start, stop in _launches(cells, LAUNCH_OUT_BYTES):
        qs = range(start, stop)
        kern = [q for q in qs if on_gpu and cells[q] <= KERNEL_MAX_SLOTS]
        parts: Dict[int, torch.Tensor] = {}
        if kern:
            flat = ext.grouped_moments(codes, sizes, values, shifts, [pc[q] for q in kern], [pv[q] for q in kern])
            off = 0
            for q in kern:
                parts[q] = flat[off : off + 3 * cells[q]]
                off += 3 * cells[q]
        for q in qs:
            if q not in parts:
                parts[q] = grouped_sums_torch(codes[pc[q]], sizes[pc[q]], values[pv[q]], shifts[pv[q]]).reshape(-1)
        flat = torch.cat([parts[q] for q in qs]) if len(qs) else torch.zeros(0, dtype=torch.float64, device=dev)
        host = dist.all_reduce_(flat, "sum").cpu().numpy()  # one collective, one copy per launch
        off = 0
        for q in qs:
            t = host[off : off + 3 * cells[q]].reshape(cells[q], 3)
            off += 3 * cells[q]
            n, s1, s2 = t[:, 0], t[:, 1], t[:, 2]
            res = np.full((cells[q], 3), np.nan, dtype=np.float64)
            res[:, 0] = n
            has = n > 0
            with np.errstate(invalid="ignore", over="ignore"):
                res[has, 1] = shifts[pv[q]] + s1[has] / n[has]
                m2 = s2[has] - s1[has] * s1[has] / n[has]
                res[has, 2] = np.where(m2 < 0, 0.0, m2)  # NaN (from infinities) stays NaN
            out[pairs[q]] = res
    return out
