"""Mahalanobis distance of every row (kernel K26): whiten-then-square.

Beyond the reference, whose outlier detection is univariate. For k
numerical columns with mean mu and covariance Sigma (n - 1 denominator),

    d2(x) = (x - mu)^T Sigma^+ (x - mu)

is computed in whitening form. With sd = sqrt(diag Sigma), the correlation
matrix C = Sigma / (sd sd^T) = V Lambda V^T (numpy.linalg.eigh, fp64) and
the r eigenvalues above rank_tol * lambda_max kept,

    W = Lambda_r^(-1/2) V_r^T          [r, k]
    z = (x - mu) / sd
    d2 = |W z|^2

which is the pseudo-inverse form: a column that is a linear combination of
others adds a zero eigenvalue and is projected out. Working on C keeps the
spectrum free of the columns' scales.

- fit_whitening: mu, sd, W, r from ops/corr.covariance_matrix (fp64, one
  all-reduce under torch.distributed, so every rank gets the same model).
- mahalanobis_d2: per-row f32 tensor. HIP path (ops/hip/row_quadform.hip):
  split-bf16 MFMA, three products, fp32 accumulation. CPU backend: fp64
  torch in row slabs.

A null counts as the column mean (z = 0), the convention of
correlation_matrix on a frame with remaining nulls.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

from anovos_amd.ops import backend
from anovos_amd.ops import corr as corr_ops
from anovos_amd.ops import stats as stats_ops

# Most columns of one model: ROWQUAD_MAX_COLS of ops/hip/anovos_kernels.h
# (the CPU path keeps the same limit, so a model fits either backend).
ROWQUAD_MAX_COLS = 256
# Scratch of one row slab of the CPU path (the fp64 Z block and its image
# under W).
MAHA_SLAB_BYTES = 1 << 28


@dataclass
class WhiteningModel:
    columns: List[str]          # the k columns W applies to, in order
    mean: np.ndarray            # [k] fp64
    sd: np.ndarray              # [k] fp64, ddof = 1
    W: np.ndarray               # [r, k] fp64
    rank: int
    excluded: List[str] = field(default_factory=list)  # zero / non-finite variance


def whitening_from_covariance(cov: np.ndarray, rank_tol: float = 1e-6):
    """(sd, W, r) of a covariance matrix whose diagonal is positive and
    finite."""
    cov = np.asarray(cov, dtype=np.float64)
    sd = np.sqrt(np.diag(cov))
    C = cov / np.outer(sd, sd)
    C = (C + C.T) / 2
    np.fill_diagonal(C, 1.0)
    lam, V = np.linalg.eigh(C)
    keep = lam > rank_tol * lam[-1]
    keep &= lam > 0
    lam, V = lam[keep][::-1], V[:, keep][:, ::-1]  # descending
    W = (V / np.sqrt(lam)).T
    return sd, np.ascontiguousarray(W), int(lam.size)


def fit_whitening(idf, cols: List[str], moments=None, rank_tol: float = 1e-6) -> WhiteningModel:
    """Means, standard deviations (ddof = 1) and the whitening matrix of the
    columns. Columns with zero or non-finite variance are left out of the
    model and listed in `excluded`."""
    cols = list(cols)
    if moments is None:
        moments = stats_ops.frame_moments(idf, cols)
    cov = corr_ops.covariance_matrix(idf, cols, moments=moments)
    var = np.diag(cov)
    ok = np.isfinite(var) & (var > 0)
    # a column without a finite mean (all null) has no finite variance either
    ok &= np.array([np.isfinite(moments[c].mean) for c in cols], dtype=bool)
    used = [c for c, g in zip(cols, ok) if g]
    excluded = [c for c, g in zip(cols, ok) if not g]
    mean = np.array([moments[c].mean for c in used], dtype=np.float64)
    if len(used) < 1:
        return WhiteningModel(used, mean, np.zeros(0), np.zeros((0, 0)), 0, excluded)
    sub = cov[np.ix_(ok, ok)]
    if not np.all(np.isfinite(sub)):
        raise ValueError("fit_whitening: covariance matrix is not finite")
    sd, W, r = whitening_from_covariance(sub, rank_tol)
    return WhiteningModel(used, mean, sd, W, r, excluded)


def mahalanobis_d2(idf, cols: List[str], model: WhiteningModel) -> torch.Tensor:
    """d2 of every local row, f32 on the frame's device. `cols` are the
    frame's columns that stand for model.columns, in the model's order."""
    cols = list(cols)
    k = len(cols)
    if k != len(model.mean) or model.W.shape != (model.rank, k) or model.rank < 1:
        raise ValueError("mahalanobis_d2: model does not match the columns")
    dev = idf.device
    tensors = [idf.col(c).data for c in cols]
    n = int(tensors[0].shape[0])
    if dev.type == "cuda" and backend.use_hip(tensors[0]):
        ext = backend.hip_ext()
        # f64 columns are centred in f64 before the downcast (NaN kept), as
        # in pearson_matrix: at |mean| >> spread the cast would lose the signal
        f32, shift = [], []
        for t, m in zip(tensors, model.mean):
            if t.dtype == torch.float32:
                f32.append(t.contiguous())
                shift.append(float(m))
            else:
                f32.append((t.to(torch.float64) - float(m)).to(torch.float32).contiguous())
                shift.append(0.0)
        shift_t = torch.tensor(shift, dtype=torch.float64).to(torch.float32).to(dev)
        scale_t = torch.tensor(1.0 / model.sd, dtype=torch.float64).to(torch.float32).to(dev)
        W_t = torch.tensor(model.W, dtype=torch.float64).to(torch.float32).to(dev)
        return ext.row_quadform_bf16x2(f32, shift_t, scale_t, W_t)
    mean = torch.tensor(model.mean, dtype=torch.float64, device=dev)
    inv_sd = torch.tensor(1.0 / model.sd, dtype=torch.float64, device=dev)
    Wt = torch.tensor(model.W, dtype=torch.float64, device=dev).T.contiguous()  # [k, r]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    rows = max(1, MAHA_SLAB_BYTES // (8 * (k + model.rank)))
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        Z = torch.stack([t[r0:r1].to(torch.float64) for t in tensors], dim=1)
        Z = (Z - mean) * inv_sd
        Z = torch.where(torch.isnan(Z), torch.zeros_like(Z), Z)
        Y = Z @ Wt
        out[r0:r1] = (Y * Y).sum(dim=1).to(torch.float32)
    return out
