"""Three-layer ReLU MLP of standardized columns (kernel K30): the encoder of
the autoencoder, one contiguous f32 tensor per output.

    z_j = isnan(x_j) ? 0 : (x_j - shift_j) * scale_j
    y   = W3 relu(W2 relu(W1 z + b1) + b2) + b3

- HIP path (ops/hip/mlp_encode.hip): split-bf16 MFMA, three products, fp32
  accumulation; standardization, null handling and both hidden layers fused
  into the one read of the frame, the hidden activations kept in registers;
  every output is written to a tensor of its own.
- CPU backend, and shapes beyond the kernel's limits: f32 torch in row slabs
  of a bounded scratch, each output written into its own tensor.

Neither path allocates a block of the whole frame.
"""

from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from anovos_amd.ops import backend

# Limits of the kernel: MLP_MAX_COLS and mlp_widths_ok of ops/hip/anovos_kernels.h
MLP_MAX_COLS = 160
# Rows of one slab of the library path (the f32 Z block and its three images)
MLP_SLAB_ROWS = 65536


def kernel_takes(d: int, widths: Sequence[int]) -> bool:
    """Whether K30 serves d columns and the layer widths (n1, n2, n3)."""
    ks = (d + 31) // 32
    n1, n2, n3 = widths
    return 1 <= d <= MLP_MAX_COLS and 1 <= n1 <= 64 * ks and 1 <= n2 <= 32 * ks and 1 <= n3 <= 32 * ks


def mlp_encode(idf, cols: List[str], shift, scale, layers: Sequence[Tuple]) -> List[torch.Tensor]:
    """The n3 output columns of every local row, contiguous f32 on the
    frame's device. `shift`, `scale` [d] are fp64 arrays on the host;
    `layers` is three (weight, bias) pairs of f32 tensors, weight [out, in]
    as torch.nn.Linear stores it."""
    cols = list(cols)
    d = len(cols)
    shift = np.asarray(shift, dtype=np.float64).reshape(-1)
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    if len(layers) != 3:
        raise ValueError(f"mlp_encode: {len(layers)} layers, expected 3")
    if shift.shape != (d,) or scale.shape != (d,):
        raise ValueError("mlp_encode: shift and scale do not match the columns")
    width = d
    for W, b in layers:
        if W.ndim != 2 or W.shape[1] != width or b.shape != (W.shape[0],):
            raise ValueError("mlp_encode: layer shapes do not chain")
        width = W.shape[0]
    dev = idf.device
    tensors = [idf.col(c).data for c in cols]
    n = int(tensors[0].shape[0])
    params = [t.detach().to(device=dev, dtype=torch.float32).contiguous() for Wb in layers for t in Wb]
    if dev.type == "cuda" and backend.use_hip(tensors[0]) and kernel_takes(d, [W.shape[0] for W, _ in layers]):
        ext = backend.hip_ext()
        # f64 columns are centred in f64 before the downcast (NaN kept), as
        # in project_columns
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
        return ext.mlp_encode_bf16x2(f32, shift_t, scale_t, *params)
    shift_t = torch.tensor(shift, dtype=torch.float64).to(torch.float32).to(dev)
    scale_t = torch.tensor(scale, dtype=torch.float64).to(torch.float32).to(dev)
    plain = not shift.any() and bool((scale == 1.0).all())
    W1, b1, W2, b2, W3, b3 = params
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(W3.shape[0])]
    for r0 in range(0, n, MLP_SLAB_ROWS):
        r1 = min(n, r0 + MLP_SLAB_ROWS)
        Z = torch.stack([t[r0:r1].to(torch.float32) for t in tensors], dim=1)
        if not plain:
            Z = (Z - shift_t) * scale_t
        Z = torch.nan_to_num(Z, nan=0.0)
        F = torch.nn.functional
        Y = F.linear(F.relu(F.linear(F.relu(F.linear(Z, W1, b1)), W2, b2)), W3, b3)
        for c in range(len(outs)):
            outs[c][r0:r1] = Y[:, c]
    return outs
