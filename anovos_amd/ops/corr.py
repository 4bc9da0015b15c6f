"""Correlation / covariance matrix (kernel K8): standardize-then-Gram.

Reference: association_evaluator.correlation_matrix (:118-123) assembles
a vector column and calls MLlib Correlation.corr (one JVM pass). Here the
Pearson matrix is computed from a single fused pass producing the Gram
matrix X^T X of the (mean-centered) column block:

- HIP path: hand-written bf16 MFMA tile kernel with on-the-fly
  standardization (ops/hip/corr_mfma.hip), fp32 accumulate; per-GPU
  partial Gram matrices merged with one RCCL all-reduce.
- Library path (sanctioned): torch.matmul (rocBLAS) on the centered
  block, also the CPU backend.

Null handling matches the reference: correlation_matrix is run on an
imputed frame (workflow imputes MMM first); any remaining NaN is treated
as the column mean (contributes zero to covariance).

For a raw frame (beyond the reference): pairwise_sums and
pairwise_pearson_matrix take every entry over the rows where both columns
are present, from the masked MFMA Gram kernel K25
(ops/hip/pairwise_gram.hip) or the same sums by library matmuls.
"""

from __future__ import annotations

from typing import List

import numpy as np
import torch

from anovos_amd.core import dist
from anovos_amd.ops import backend
from anovos_amd.ops import stats as stats_ops


def pearson_matrix(idf, cols: List[str], moments=None, use_bf16: bool = True) -> np.ndarray:
    """Global Pearson correlation matrix over numeric columns."""
    if moments is None:
        moments = stats_ops.frame_moments(idf, cols)
    dev = idf.device
    n = idf.count()
    tensors = [idf.col(c).data for c in cols]
    col_means = [m if m == m else 0.0 for m in (moments[c].mean for c in cols)]
    if dev.type == "cuda" and backend.use_hip(tensors[0]) and use_bf16:
        ext = backend.hip_ext()
        # f32 columns: the kernel centers in-register (subtraction of
        # nearby f32 values is exact, error = storage quantization).
        # f64 columns MUST center in f64 BEFORE the downcast: casting
        # raw values loses the whole signal when |mean| >> spread
        # (f32 spacing at 1e8 is 8.0).
        f32, kmeans = [], []
        for t, m in zip(tensors, col_means):
            if t.dtype == torch.float32:
                f32.append(t.contiguous())
                kmeans.append(m)
            else:
                f32.append((t - m).to(torch.float32).contiguous())
                kmeans.append(0.0)
        means = torch.tensor(kmeans, dtype=torch.float32, device=dev)
        gram = ext.centered_gram_bf16(f32, means)  # [k,k] fp32
    else:
        # center in f64, then downcast; NaN contributes zero (== mean)
        X = torch.stack(
            [torch.nan_to_num((t.to(torch.float64) - m).to(torch.float32), nan=0.0)
             for t, m in zip(tensors, col_means)],
            dim=1,
        )
        gram = X.T @ X
    gram = gram.to(torch.float64)
    if dist.is_dist():
        dist.all_reduce_(gram, "sum")
    g = gram.cpu().numpy()
    d = np.sqrt(np.clip(np.diag(g), 1e-300, None))
    corr = g / np.outer(d, d)
    np.fill_diagonal(corr, 1.0)
    return np.clip(corr, -1.0, 1.0)


# Scratch of one row slab of pairwise_sums' library path (the Z, Z*Z and M
# planes): three planes of a 100 GB frame do not fit beside it.
PAIR_SLAB_BYTES = 1 << 30
# An f32 matmul counts the rows of a slab exactly only below 2^24.
PAIR_SLAB_MAX_ROWS = 1 << 23

# pairwise_pearson_matrix reports r as undefined where a conditional
# variance Q - S^2 / n is not above tol * Q (Q is the raw second moment about
# the global mean, so the ratio is free of scale):
# - fp64 sums: 1e-12, the cancellation error of the two terms.
# - f32 matmul: the fp32 summation of Q and of S leaves a relative error of
#   about sqrt(rows) * 2^-24 (at most rows * 2^-24) in each; 1e-4 covers
#   slabs of 2^23 rows.
# - bf16 kernel: the square plane is bf16(zb * zb), rounded to 2^-9
#   relative, so a column that is constant on a partner's rows leaves
#   |Q - S^2 / n| up to 2^-9 Q instead of 0; 2^-8 is twice that. What it
#   also drops is a pair whose conditional mean lies more than 16
#   conditional standard deviations from the column's global mean.
PAIR_TOL_F64 = 1e-12
PAIR_TOL_F32 = 1e-4
PAIR_TOL_BF16 = 2.0 ** -8


def _pairwise_path(idf, cols, use_bf16):
    dev = idf.device
    if dev.type == "cuda" and backend.use_hip(idf.col(cols[0]).data):
        return "bf16" if use_bf16 else "f32"
    return "f64"


def pairwise_sums(idf, cols: List[str], moments=None, use_bf16: bool = True) -> np.ndarray:
    """The sums a pairwise-complete Pearson r needs, fp64 [4, k, k] =
    (N, P, S, Q). With m = 1 where a value is present (else 0) and
    z = x - mean on present rows (else 0), mean the global column mean:

    N[i][j] = sum m_i m_j     rows where both are present
    P[i][j] = sum z_i z_j
    S[i][j] = sum z_i m_j     sum of i over the rows where j is present
    Q[i][j] = sum z_i^2 m_j

    HIP path (K25, ops/hip/pairwise_gram.hip): bf16 MFMA Gram of
    [Z | Z^2 | M] formed in registers from one read of x. Library path
    (use_bf16=False, and the CPU backend): four matmuls per row slab of at
    most PAIR_SLAB_BYTES, f32 on the GPU and fp64 on the CPU, slab sums
    added in fp64. All four are plain sums over rows: ranks merge with one
    all-reduce."""
    if moments is None:
        moments = stats_ops.frame_moments(idf, cols)
    dev = idf.device
    k = len(cols)
    tensors = [idf.col(c).data for c in cols]
    n = int(tensors[0].shape[0])  # rows of this shard
    col_means = [m if m == m else 0.0 for m in (moments[c].mean for c in cols)]
    path = _pairwise_path(idf, cols, use_bf16)
    if path == "bf16":
        ext = backend.hip_ext()
        # f64 columns are centred in f64 before the downcast (NaN kept), as
        # in pearson_matrix
        f32, kmeans = [], []
        for t, m in zip(tensors, col_means):
            if t.dtype == torch.float32:
                f32.append(t.contiguous())
                kmeans.append(m)
            else:
                f32.append((t - m).to(torch.float32).contiguous())
                kmeans.append(0.0)
        means = torch.tensor(kmeans, dtype=torch.float32, device=dev)
        sums = ext.pairwise_gram_bf16(f32, means)  # [4,k,k] fp64
    else:
        work = torch.float32 if path == "f32" else torch.float64
        itemsize = 4 if path == "f32" else 8
        rows = max(1, min(PAIR_SLAB_BYTES // (3 * k * itemsize), PAIR_SLAB_MAX_ROWS))
        sums = torch.zeros(4, k, k, dtype=torch.float64, device=dev)
        for r0 in range(0, n, rows):
            r1 = min(n, r0 + rows)
            # planes as [k, rows]: every column is written as one dense row
            Z = torch.empty(k, r1 - r0, dtype=work, device=dev)
            M = torch.empty(k, r1 - r0, dtype=work, device=dev)
            for j, (t, m) in enumerate(zip(tensors, col_means)):
                v = t[r0:r1].to(torch.float64)
                present = ~torch.isnan(v)
                Z[j] = torch.where(present, v - m, torch.zeros_like(v)).to(work)
                M[j] = present.to(work)
            ZZ = Z * Z
            sums[0] += (M @ M.T).to(torch.float64)
            sums[1] += (Z @ Z.T).to(torch.float64)
            sums[2] += (Z @ M.T).to(torch.float64)
            sums[3] += (ZZ @ M.T).to(torch.float64)
            del Z, M, ZZ
        # a BLAS need not return Z Z^T symmetric to the last bit; r is
        sums[1] = (sums[1] + sums[1].T) / 2
    if dist.is_dist():
        dist.all_reduce_(sums, "sum")
    return sums.cpu().numpy()


def pairwise_pearson_matrix(idf, cols: List[str], moments=None, use_bf16: bool = True,
                            min_periods: int = 2, return_counts: bool = False):
    """Pearson's r over the rows where both columns of a pair are present
    (pandas `DataFrame.corr`, R `use="pairwise.complete.obs"`), from
    pairwise_sums in fp64. With n = N[i][j]:

    cov = P[i][j] - S[i][j] S[j][i] / n
    v_i = Q[i][j] - S[i][j]^2 / n,   v_j = Q[j][i] - S[j][i]^2 / n
    r   = cov / sqrt(v_i v_j), clipped to [-1, 1]

    An entry, diagonal included, is NaN where n < max(min_periods, 2) or a
    conditional variance is not above tol times its Q (PAIR_TOL_*: 1e-12
    on the fp64 path, 1e-4 on the f32 matmul path, 2^-8 on the bf16 kernel
    path); elsewhere the diagonal is exactly 1.0. return_counts=True also
    returns N as int64."""
    N, P, S, Q = pairwise_sums(idf, cols, moments=moments, use_bf16=use_bf16)
    path = _pairwise_path(idf, cols, use_bf16)
    tol = {"f64": PAIR_TOL_F64, "f32": PAIR_TOL_F32, "bf16": PAIR_TOL_BF16}[path]
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = np.where(N > 0, N, np.nan)
        cov = P - S * S.T / nn
        vi = Q - S * S / nn
        vj = vi.T
        ok = (N >= max(int(min_periods), 2)) & (vi > tol * Q) & (vj > tol * Q.T)
        r = np.clip(cov / np.sqrt(vi * vj), -1.0, 1.0)
    r = np.where(ok, r, np.nan)
    d = np.diag(ok)
    r[np.diag_indices_from(r)] = np.where(d, 1.0, np.nan)
    if return_counts:
        return r, np.rint(N).astype(np.int64)
    return r


def covariance_matrix(idf, cols: List[str], moments=None) -> np.ndarray:
    """Global covariance matrix (n-1 denominator, Spark RowMatrix
    computeCovariance semantics — reference association_eval_varclus.py:71-84)."""
    if moments is None:
        moments = stats_ops.frame_moments(idf, cols)
    tensors = [idf.col(c).data for c in cols]
    col_means = [m if m == m else 0.0 for m in (moments[c].mean for c in cols)]
    # center in f64 before any precision loss; NaN contributes zero
    Xc = torch.stack(
        [torch.nan_to_num(t.to(torch.float64) - m, nan=0.0) for t, m in zip(tensors, col_means)],
        dim=1,
    )
    gram = Xc.T @ Xc
    if dist.is_dist():
        dist.all_reduce_(gram, "sum")
    n = idf.count()
    return (gram / max(n - 1, 1)).cpu().numpy()
