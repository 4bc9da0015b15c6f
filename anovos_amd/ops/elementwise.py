"""Fused elementwise column ops (kernel K11): (x-a)*b scaling and NaN
fill across many columns in one launch — the apply halves of
z/IQR/min-max standardization and MMM imputation."""

from __future__ import annotations

from typing import List, Sequence

import torch

from anovos_amd.ops import backend


def fill_code_columns(tensors: Sequence[torch.Tensor], fills: Sequence[int]) -> List[torch.Tensor]:
    """out_i = (codes_i == NULL_CODE) ? fill_i : codes_i — categorical
    mode imputation, one fused launch for all columns (the torch
    fallback's eq/full_like/where chain costs ~5x the traffic)."""
    from anovos_amd.core.dtypes import NULL_CODE

    if tensors and tensors[0].is_cuda and backend.use_hip(tensors[0]):
        ext = backend.hip_ext()
        return ext.fill_code_columns([t.contiguous() for t in tensors], [int(f) for f in fills])
    return [torch.where(t == NULL_CODE, torch.full_like(t, int(f)), t) for t, f in zip(tensors, fills)]


def scale_columns(tensors: Sequence[torch.Tensor], a: Sequence[float], b: Sequence[float]) -> List[torch.Tensor]:
    """out_i = float32((float64(x_i) - a_i) * b_i); NaN propagates.

    The column is centred in double, with a_i and b_i as the doubles they
    were fitted as, and the product is rounded to float32 once. The HIP
    kernel (K11) and the torch path below compute this same formula for
    float32 and float64 columns alike, so a column whose mean is large
    against its spread keeps its signal, and min-max output stays inside
    [0, 1]."""
    if tensors and tensors[0].is_cuda and backend.use_hip(tensors[0]):
        ext = backend.hip_ext()
        return ext.scale_columns(
            [t.contiguous() for t in tensors],
            torch.tensor(list(a), dtype=torch.float64),
            torch.tensor(list(b), dtype=torch.float64),
        )
    return [((t.to(torch.float64) - float(ai)) * float(bi)).to(torch.float32) for t, ai, bi in zip(tensors, a, b)]


def fill_nan_columns(tensors: Sequence[torch.Tensor], fills: Sequence[float]) -> List[torch.Tensor]:
    """out_i = isnan(x_i) ? fill_i : x_i (dtype preserved)."""
    if tensors and tensors[0].is_cuda and backend.use_hip(tensors[0]):
        ext = backend.hip_ext()
        return ext.fill_nan_columns(
            [t.contiguous() for t in tensors], torch.tensor(list(fills), dtype=torch.float64)
        )
    # NaN only, as the kernel does: nan_to_num would also replace +-inf
    # (with the dtype's largest finite value)
    return [torch.where(torch.isnan(t), torch.full_like(t, float(f)), t) for t, f in zip(tensors, fills)]
