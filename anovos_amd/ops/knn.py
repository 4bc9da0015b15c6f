"""The apply step of KNN imputation (kernel K29): sklearn's
KNNImputer.transform on the device.

With target columns x_0 .. x_{m-1} (NaN = null), donors F [s, m] (the
model's _fit_X), mx = !isnan(x), mf = !isnan(F):

    ov = sum_c mx_c mf_c
    sq = sum_c mx_c mf_c (x_c - F_c)^2
    d2 = m * sq / ov            ov > 0, else +inf

A task is (row i, column j) with x_j[i] null. Its donors are the rows of F
with column j present and finite d2; its estimate is the plain mean of
column j over the k nearest, fewer if fewer exist, the donor column mean if
there is none. Neighbours are the k smallest under the total order
(d2, donor index) on either path.

- knn_impute_fp64: fp64 torch, four GEMMs per row batch and a top-k per
  column - the CPU backend, and the default of imputation_sklearn.
- knn_impute: one K29 call per column that has nulls
  (ops/hip/knn_impute.hip: split-bf16 MFMA filter pass, candidates kept in
  registers, exact f32 re-rank); the fp64 code on the CPU backend and beyond
  the kernel's limits.
"""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from anovos_amd.ops import backend

# KNN_MAX_COLS, KNN_MAX_K, KNN_MAX_DONORS of ops/hip/anovos_kernels.h
KNN_MAX_COLS = 128
KNN_MAX_K = 8
KNN_MAX_DONORS = 65536

APPLY_PRECISIONS = ("fp64", "bf16x2")


def check_apply_precision(apply_precision):
    if apply_precision not in APPLY_PRECISIONS:
        raise ValueError(
            f"Invalid input for apply_precision: one of {APPLY_PRECISIONS}, got {apply_precision!r}")


def KNN_FILTER_GAMMA(m_pad: int) -> float:
    """Bound of K29's filter pass: |sq_filter - sq| <= gamma * sum_overlap
    (|zx| + |zf|)^2 with z the centred values. 2^-18 for each operand's
    split residual and for the dropped lo * lo term of the cross product,
    2^-18 + 2^-24 on the squares, and the fp32 sum of the 7 * m_pad products
    of one accumulator (derivation in ops/hip/knn_impute.hip)."""
    return 3 * 2.0 ** -18 + (7 * int(m_pad) + 1) * 2.0 ** -24


def knn_impute_fp64(B: torch.Tensor, F: torch.Tensor, k: int, batch: int = 16384) -> torch.Tensor:
    """sklearn KNNImputer.transform semantics on device: nan-euclidean
    distances dist^2 = m/|overlap| * sum_overlap (x-f)^2 via three GEMMs
    per batch, per-column donor selection (non-missing target, finite
    distance), uniform-weight mean of the k nearest, column-mean
    fallback when no donor exists."""
    m = B.shape[1]
    Mf = (~torch.isnan(F)).to(F.dtype)
    Fv = torch.nan_to_num(F)
    col_mean = Fv.sum(0) / Mf.sum(0).clamp(min=1.0)
    F2 = (Fv * Fv) * Mf
    out = B.clone()
    for s in range(0, B.shape[0], batch):
        b = B[s : s + batch]
        Mx = (~torch.isnan(b)).to(b.dtype)
        Xv = torch.nan_to_num(b)
        S1 = (Xv * Xv * Mx) @ Mf.T
        S2 = Mx @ F2.T
        S3 = (Xv * Mx) @ (Fv * Mf).T
        overlap = Mx @ Mf.T  # [b, s]
        sq = (S1 + S2 - 2 * S3).clamp(min=0.0)
        d2 = torch.where(overlap > 0, m * sq / overlap.clamp(min=1.0), torch.full_like(sq, float("inf")))
        miss = torch.isnan(b)
        for j in range(m):
            rows = miss[:, j].nonzero(as_tuple=True)[0]
            if not rows.numel():
                continue
            # donors: fitted rows with col j present and finite distance
            dj = d2[rows] + torch.where(Mf[:, j] > 0, torch.zeros(1, device=B.device), torch.full((1,), float("inf"), device=B.device))
            kk = min(k, int((Mf[:, j] > 0).sum()))
            if kk == 0:
                out[s + rows, j] = col_mean[j]
                continue
            vals, idx = torch.topk(dj, kk, dim=1, largest=False)
            # topk leaves open which of several donors AT the k-th distance
            # it returns: those rows take the (d2, index) order from a stable sort
            last = vals[:, -1:]
            tied = (torch.isfinite(last[:, 0]) & ((dj <= last).sum(1) > kk)).nonzero(as_tuple=True)[0]
            if tied.numel():
                sv, si = torch.sort(dj[tied], dim=1, stable=True)
                vals[tied] = sv[:, :kk]
                idx[tied] = si[:, :kk]
            donor = Fv[:, j][idx]  # [r, kk]
            ok = torch.isfinite(vals)
            cnt = ok.sum(1).clamp(min=1)
            est = (donor * ok).sum(1) / cnt
            est = torch.where(ok.any(1), est, col_mean[j].expand_as(est))
            out[s + rows, j] = est
    return out


def kernel_serves(idf, cols: List[str], donors: np.ndarray, k: int) -> bool:
    """True where knn_impute runs K29: the HIP backend, within the limits."""
    t = idf.col(cols[0]).data
    if not (idf.device.type == "cuda" and backend.use_hip(t)):
        return False
    return len(cols) <= KNN_MAX_COLS and 1 <= k <= KNN_MAX_K and 1 <= donors.shape[0] <= KNN_MAX_DONORS


def knn_impute(idf, cols: List[str], donors, k: int) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Imputed values of the columns that have nulls: {column: (rows,
    values)}, `rows` the int64 indices of its null rows and `values` fp64,
    both on the frame's device. `donors` is the fitted fp64 [s, m] array in
    the order of `cols`."""
    cols = list(cols)
    k = int(k)
    F = np.ascontiguousarray(donors, dtype=np.float64)
    if F.ndim != 2 or F.shape[1] != len(cols):
        raise ValueError("knn_impute: donors do not match the columns")
    dev = idf.device
    tensors = [idf.col(c).data for c in cols]
    out: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
    if not kernel_serves(idf, cols, F, k):
        nan_any = torch.zeros(tensors[0].shape[0], dtype=torch.bool, device=dev)
        for t in tensors:
            nan_any |= torch.isnan(t)
        nan_rows = nan_any.nonzero(as_tuple=True)[0]
        if not nan_rows.numel():
            return out
        B = torch.stack([t[nan_rows].to(torch.float64) for t in tensors], dim=1)
        filled = knn_impute_fp64(B, torch.from_numpy(F).to(dev), k)
        for j, c in enumerate(cols):
            sub = torch.isnan(B[:, j])
            if bool(sub.any()):
                out[c] = (nan_rows[sub], filled[:, j][sub])
        return out

    ext = backend.hip_ext()
    present = ~np.isnan(F)
    col_mean = np.where(present, F, 0.0).sum(0) / np.maximum(present.sum(0), 1)
    # f64 columns are centred in f64 before the downcast (NaN kept), donors
    # alike, and take centre 0, as in ops/project.py
    f32, center, Fc = [], [], F.copy()
    for j, t in enumerate(tensors):
        if t.dtype == torch.float32:
            f32.append(t.contiguous())
            center.append(float(col_mean[j]))
        else:
            f32.append((t.to(torch.float64) - float(col_mean[j])).to(torch.float32).contiguous())
            center.append(0.0)
            Fc[:, j] -= col_mean[j]
    donors_t = torch.from_numpy(Fc).to(torch.float32).to(dev).contiguous()
    center_t = torch.tensor(center, dtype=torch.float64)
    for j, (c, t) in enumerate(zip(cols, tensors)):
        rows = torch.isnan(t).nonzero(as_tuple=True)[0]
        if not rows.numel():
            continue
        est, _, _ = ext.knn_impute_bf16x2(f32, rows, center_t, donors_t, j, k)
        vals = est.to(torch.float64)
        if t.dtype != torch.float32:
            vals = vals + float(col_mean[j])
        out[c] = (rows, torch.where(torch.isnan(vals), torch.full_like(vals, float(col_mean[j])), vals))
    return out
