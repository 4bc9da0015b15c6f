"""Fused row-wise scans (kernel K10): per-row null count, per-row outlier
flags, row filters over a columnar layout.

Reference: nullRows_detection UDF (quality_checker.py:248-258) counts
nulls per row; the GPU kernel streams every column once, accumulating
per-row counters staged in LDS (rows x 2B), instead of a per-row Python
UDF.

Null lane masks (K10m): the first analyzer pass over a column (fused
moments+HLL for f32, code counts for dictionary codes) has already tested
every value for null and can write the result out at one bit per value.
A column whose ``Column.cache`` holds such a mask is counted from it —
1/32 of the bytes — and the rest of the columns take the column scan."""

from __future__ import annotations

import os
from typing import List

import torch

from anovos_amd.ops import backend

# Column.cache key of (mask tensor, (n, nchunks, per)); dropped with the
# rest of the cache by clear_stats_cache
NULL_MASK_KEY = "null_mask"


def null_masks_enabled() -> bool:
    """ANOVOS_NULL_MASKS=0 turns mask emission off (A/B runs, shards with
    no memory to spare: a mask is 1/32 of its column)."""
    return os.environ.get("ANOVOS_NULL_MASKS", "1") != "0"


def store_null_masks(idf, cols: List[str], masks, parts) -> None:
    """Cache what a producer binding returned for `cols` (None / [] for a
    column it emitted no mask for)."""
    for c, m, p in zip(cols, masks, parts):
        if m is not None:
            idf.col(c).cache[NULL_MASK_KEY] = (m, tuple(int(v) for v in p))


def row_null_counts(idf, cols: List[str]) -> torch.Tensor:
    """int32 tensor [local_rows] of null counts across the given columns."""
    n = idf.local_rows()
    dev = idf.device
    first = idf.col(cols[0]).data if cols else None
    if first is not None and first.is_cuda and backend.use_hip(first):
        ext = backend.hip_ext()
        # mask groups: columns with a cached null mask of this shard, by
        # the partition it was made with (one K10m launch per partition)
        groups = {}
        scan = []
        for c in cols:
            hit = idf.col(c).cache.get(NULL_MASK_KEY)
            if hit is not None and hit[1][0] == n and hit[0].device == first.device:
                groups.setdefault(hit[1], []).append(hit[0])
            else:
                scan.append(c)
        # one fused launch covers numeric (NaN) AND categorical (-1 code)
        # columns; timestamps (INT64_MIN null) use the eager fallback
        fused = [idf.col(c).data.contiguous() for c in scan
                 if idf.col(c).kind == "numerical" or idf.col(c).data.dtype == torch.int32]
        rest = [c for c in scan
                if not (idf.col(c).kind == "numerical" or idf.col(c).data.dtype == torch.int32)]
        out = torch.zeros(n, dtype=torch.int32, device=dev)
        for part, masks in groups.items():
            ext.row_null_counts_masked(masks, list(part), out)
        if fused:
            ext.row_null_counts_num(fused, out)
        for c in rest:
            out += idf.col(c).null_mask().to(torch.int32)
        return out
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    for c in cols:
        out += idf.col(c).null_mask().to(torch.int32)
    return out
