"""Linear projection of standardized columns (kernel K27): the scores of
PCA, one contiguous f32 tensor per component.

    z_j = isnan(x_j) ? 0 : (x_j - shift_j) * scale_j
    y_c = sum_j W[c][j] z_j          c < r,  W [r, k]

- HIP path (ops/hip/project_columns.hip): split-bf16 MFMA, three products,
  fp32 accumulation, standardization and null handling fused into the one
  read of the frame; every component is written to a tensor of its own.
- CPU backend: fp64 torch in row slabs of a bounded scratch, each component
  written into its own tensor.

Neither path allocates an [n, k] or [n, r] block of the whole frame, and a
latent column owns its memory like any other column of the store. A null
counts as z = 0, the column mean once shift is the mean.
"""

from __future__ import annotations

from typing import List

import numpy as np
import torch

from anovos_amd.ops import backend

# Most columns of one projection: ROWQUAD_MAX_COLS of ops/hip/anovos_kernels.h
# (the CPU path keeps the same limit, so a model fits either backend).
PROJECT_MAX_COLS = 256
# Scratch of one row slab of the CPU path (the fp64 Z block and its image
# under W).
PROJECT_SLAB_BYTES = 1 << 28


def project_columns(idf, cols: List[str], shift, scale, W) -> List[torch.Tensor]:
    """The r = W.shape[0] score columns of every local row, contiguous f32
    on the frame's device. `shift`, `scale` [k] and `W` [r, k] are fp64
    arrays on the host."""
    cols = list(cols)
    k = len(cols)
    shift = np.asarray(shift, dtype=np.float64).reshape(-1)
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    W = np.ascontiguousarray(W, dtype=np.float64)
    if k > PROJECT_MAX_COLS:
        raise ValueError(f"project_columns: {k} columns, at most {PROJECT_MAX_COLS}")
    if shift.shape != (k,) or scale.shape != (k,) or W.ndim != 2 or W.shape[1] != k:
        raise ValueError("project_columns: shift, scale and W do not match the columns")
    r = W.shape[0]
    if not 1 <= r <= k:
        raise ValueError(f"project_columns: W has {r} rows, expected 1 .. {k}")
    dev = idf.device
    tensors = [idf.col(c).data for c in cols]
    n = int(tensors[0].shape[0])
    if dev.type == "cuda" and backend.use_hip(tensors[0]):
        ext = backend.hip_ext()
        # f64 columns are centred in f64 before the downcast (NaN kept), as
        # in mahalanobis_d2: at |mean| >> spread the cast would lose the signal
        f32, kshift = [], []
        for t, m in zip(tensors, shift):
            if t.dtype == torch.float32:
                f32.append(t.contiguous())
                kshift.append(float(m))
            else:
                f32.append((t.to(torch.float64) - float(m)).to(torch.float32).contiguous())
                kshift.append(0.0)
        shift_t = torch.tensor(kshift, dtype=torch.float64).to(torch.float32).to(dev)
        scale_t = torch.tensor(scale, dtype=torch.float64).to(torch.float32).to(dev)
        W_t = torch.tensor(W, dtype=torch.float64).to(torch.float32).to(dev).contiguous()
        return ext.project_columns_bf16x2(f32, shift_t, scale_t, W_t)
    shift_t = torch.tensor(shift, dtype=torch.float64, device=dev)
    scale_t = torch.tensor(scale, dtype=torch.float64, device=dev)
    Wt = torch.tensor(W, dtype=torch.float64, device=dev).T.contiguous()  # [k, r]
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(r)]
    rows = max(1, PROJECT_SLAB_BYTES // (8 * (k + r)))
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        Z = torch.stack([t[r0:r1].to(torch.float64) for t in tensors], dim=1)
        Z = (Z - shift_t) * scale_t
        Z = torch.where(torch.isnan(Z), torch.zeros_like(Z), Z)
        Y = Z @ Wt
        for c in range(r):
            outs[c][r0:r1] = Y[:, c].to(torch.float32)
    return outs
