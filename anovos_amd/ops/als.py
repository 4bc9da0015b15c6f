"""Matrix-factorization imputation by alternating least squares with weighted
regularisation (ALS-WR), kernel K32 (ops/hip/als_sweep.hip).

The method. Per column j: mu_j and sd_j over the non-null rows (ddof = 1);
where sd_j is 0, NaN, or there are fewer than two observations, sd_j = 1;
s_j = 1 / sd_j.

    m_rj = !isnan(x_rj)
    z_rj = m_rj ? (x_rj - mu_j) * s_j : 0        (a subtract, then a multiply)
    k    = min(rank, m), 1 <= k <= ALS_MAX_RANK;  reg > 0
    n_r  = sum_j m_rj;  n_j = sum_r m_rj over all ranks

    row half, given V [m, k]:
        u_r = (sum_j m_rj v_j v_j^T + reg max(n_r, 1) I)^-1 sum_j z_rj v_j
    column half, given U:
        H_j = sum_r m_rj u_r u_r^T,  g_j = sum_r z_rj u_r
        v_j = (H_j + reg max(n_j, 1) I)^-1 g_j

The fit: V <- V0; max_iter times U <- rows(V), V <- cols(U); then U <- rows(V)
once more. The value of a null entry is (u_r . v_j) sd_j + mu_j; a row with no
observed column gets u = 0 and therefore mu_j. V0 is the top-k eigenvectors,
by descending eigenvalue, of D G D, G the centred Gram matrix of
corr.covariance_matrix(precision="bf16x2") (K28) and D = diag(s), each
eigenvector signed so that its largest component is positive.

- als_fit_fp64: the fit in fp64 numpy - the definition the tests hold K32 to.
- als_v0: V0 from the cached moments and K28.
- als_impute: the driver. On the HIP backend within the kernel's limits the
  row half and the column half run on K32 and the m small solves on the host;
  elsewhere the fp64 definition runs in row slabs, without an [n, m] copy.
"""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from anovos_amd.core import dist
from anovos_amd.ops import backend
from anovos_amd.ops import corr as corr_ops
from anovos_amd.ops import stats as stats_ops

# ALS_MAX_RANK, ALS_MAX_COLS of ops/hip/anovos_kernels.h
ALS_MAX_RANK = 16
ALS_MAX_COLS = 160
# rows of one slab of the fp64 path
SLAB_ROWS = 1 << 16


def als_kr(rank: int) -> int:
    """The rank padded to the kernel's KR in {4, 8, 12, 16}."""
    return (int(rank) + 3) // 4 * 4


def als_tri(kr: int) -> int:
    return kr * (kr + 1) // 2


def ALS_GAMMA_RHS(m_pad: int) -> float:
    """Row half, right-hand side: K26's bound, |b - b*| <= gamma sum_j |z_j| |v_j|
    with the columns padded to m_pad (a multiple of 32): operand splits and the
    dropped lo.lo term, 3 * 2^-18, the fp32 sum of 3 m_pad products, and the
    forming of z."""
    return 3 * 2.0 ** -18 + (3 * int(m_pad) + 1) * 2.0 ** -24


def ALS_GAMMA_A(m_pad: int) -> float:
    """Row half, matrix: |A - A*| <= gamma sum_j m_j |v_ja v_jb|. The product
    v_ja v_jb is rounded once to f32 (2^-24); hi + lo of it leaves a residual
    of 2^-18 (M is exact, so there is no second operand to split); the fp32 sum
    has 2 m_pad terms."""
    return 2.0 ** -18 + 2.0 ** -24 + (2 * int(m_pad) + 1) * 2.0 ** -24


# Column half, derived in K28's manner with its flush rule (an fp32
# accumulator takes the products of 64 rows, everything beyond is fp64).
# gamma_H on sum_r m |u_a u_b|: the rounding of the f32 product (2^-24), one
# split residual (2^-18) and the chain of 2 * 64 terms. gamma_g on sum_r
# |z| |u|: K28's figure - splits on either side and the dropped lo.lo term,
# the chain of 3 * 64 terms, the subtractions and the multiply that form z.
ALS_FLUSH_ROWS = 64
ALS_GAMMA_H = 2.0 ** -18 + 2.0 ** -24 + (2 * ALS_FLUSH_ROWS + 1) * 2.0 ** -24
ALS_GAMMA_G = 3 * 2.0 ** -18 + (3 * ALS_FLUSH_ROWS + 4) * 2.0 ** -24


def unpack_normal(packed: np.ndarray, kr: int) -> Tuple[np.ndarray, np.ndarray]:
    """([.., kr, kr] symmetric, [.., kr]) of K32's packed [.., T + kr]."""
    packed = np.asarray(packed)
    a, b = np.tril_indices(kr)
    H = np.zeros(packed.shape[:-1] + (kr, kr), dtype=packed.dtype)
    H[..., a, b] = packed[..., : als_tri(kr)]
    H[..., b, a] = packed[..., : als_tri(kr)]
    return H, packed[..., als_tri(kr):]


def _rows_fp64(Z, M, V, reg):
    A = np.einsum("rj,ja,jb->rab", M, V, V) + (reg * np.maximum(M.sum(1), 1.0))[:, None, None] * np.eye(V.shape[1])
    return np.linalg.solve(A, (Z @ V)[:, :, None])[:, :, 0]


def _cols_solve(H, g, n_cols, reg):
    A = H + (reg * np.maximum(np.asarray(n_cols, dtype=np.float64), 1.0))[:, None, None] * np.eye(H.shape[1])
    return np.linalg.solve(A, g[:, :, None])[:, :, 0]


def als_fit_fp64(X, mu, sd, V0, max_iter: int, reg: float):
    """The fit on X [n, m] (NaN = null) in fp64 numpy from V0 [m, k]: (X with
    every null replaced by its value, U [n, k], V [m, k])."""
    X = np.asarray(X, dtype=np.float64)
    mu, sd, V = (np.asarray(a, dtype=np.float64) for a in (mu, sd, V0))
    mask = ~np.isnan(X)
    M = mask.astype(np.float64)
    Z = np.where(mask, (X - mu) * (1.0 / sd), 0.0)
    for _ in range(int(max_iter)):
        U = _rows_fp64(Z, M, V, reg)
        V = _cols_solve(np.einsum("rj,ra,rb->jab", M, U, U), Z.T @ U, M.sum(0), reg)
    U = _rows_fp64(Z, M, V, reg)
    return np.where(mask, X, (U @ V.T) * sd + mu), U, V


def column_scales(idf, cols: List[str]):
    """(mu, sd, n) per column from the cached moments, with the method's
    defaults: sd = 1 where it is 0, NaN or there are fewer than two values."""
    moments = stats_ops.frame_moments(idf, cols)
    mu = np.array([moments[c].mean if moments[c].n > 0 else 0.0 for c in cols], dtype=np.float64)
    sd = np.array([moments[c].stddev for c in cols], dtype=np.float64)
    sd = np.where(np.isnan(sd) | (sd == 0), 1.0, sd)
    return mu, sd, np.array([moments[c].n for c in cols], dtype=np.float64)


def als_v0(idf, cols: List[str], sd, k: int) -> np.ndarray:
    """V0 [m, k]: the existing initialisation (top right singular vectors of
    the zero-filled standardized matrix) from K28's Gram matrix."""
    moments = stats_ops.frame_moments(idf, cols)
    G = corr_ops.covariance_matrix(idf, cols, moments=moments, precision="bf16x2") * max(idf.count() - 1, 1)
    s = 1.0 / np.asarray(sd, dtype=np.float64)
    _, evecs = np.linalg.eigh(G * s[:, None] * s[None, :])
    V = evecs[:, ::-1][:, :k].copy()
    top = np.abs(V).argmax(0)
    return V * np.sign(V[top, np.arange(k)] + (V[top, np.arange(k)] == 0))


def kernel_serves(idf, cols: List[str], rank: int) -> bool:
    """True where als_impute runs K32: the HIP backend, within its limits, every
    column 16-byte aligned (the kernels read four rows per load; a column
    that is an offset view of a wider tensor may not be; f64 and strided
    columns go to the kernels as fresh f32 copies)."""
    return (idf.device.type == "cuda" and backend.use_hip(idf.col(cols[0]).data)
            and len(cols) <= ALS_MAX_COLS and 1 <= min(rank, len(cols)) <= ALS_MAX_RANK
            and all(t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 == 0
                    for t in (idf.col(c).data for c in cols)))


def _fit_kernel(idf, cols, mu, sd, n_cols, V, max_iter, reg, clones):
    ext = backend.hip_ext()
    if ext.ALS_MAX_RANK != ALS_MAX_RANK or ext.ALS_MAX_COLS != ALS_MAX_COLS:
        raise RuntimeError("the limits of the extension and of ops/als.py differ")
    dev = idf.device
    k = V.shape[1]
    kr = als_kr(k)
    f32, outs, center, wide = [], [], [], []
    for j, c in enumerate(cols):
        t = idf.col(c).data
        if t.dtype == torch.float32:
            f32.append(t.contiguous())
            outs.append(clones[c])
            center.append(float(mu[j]))
        else:
            # centred in fp64 before the downcast, as ops/chain.py
            f32.append((t.to(torch.float64) - float(mu[j])).to(torch.float32).contiguous())
            outs.append(torch.zeros_like(f32[-1]))
            center.append(0.0)
            wide.append(j)
    center_t = torch.tensor(center, dtype=torch.float64)
    scale_t, sd_t = torch.from_numpy(1.0 / sd), torch.from_numpy(sd)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    n = idf.local_rows()
    for _ in range(int(max_iter)):
        if n:
            U, _ = ext.als_row_solve_bf16x2(f32, center_t, scale_t, sd_t, to_dev(V), float(reg))
            packed = ext.als_col_normal_bf16x2(f32, center_t, scale_t, U)
            del U
        else:
            packed = torch.zeros(len(cols), als_tri(kr) + kr, dtype=torch.float64, device=dev)
        dist.all_reduce_(packed, "sum")  # the one collective of a sweep
        H, g = unpack_normal(packed.cpu().numpy(), kr)
        V = _cols_solve(H[:, :k, :k], g[:, :k], n_cols, reg)
    if n:
        ext.als_row_solve_bf16x2(f32, center_t, scale_t, sd_t, to_dev(V), float(reg), outs=outs, want_u=False)
    for j in wide:
        clone = clones[cols[j]]
        null = torch.isnan(f32[j])
        clone[null] = (outs[j][null].to(torch.float64) + float(mu[j])).to(clone.dtype)


def _fit_slabs(idf, cols, mu, sd, n_cols, V, max_iter, reg, clones):
    """The fp64 definition in row slabs, torch fp64 on the frame's device."""
    dev = idf.device
    n, m, k = idf.local_rows(), len(cols), V.shape[1]
    mu_t, s_t, sd_t = (torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev) for a in (mu, 1.0 / sd, sd))
    eye = torch.eye(k, dtype=torch.float64, device=dev)

    def slabs(Vn):
        Vt = torch.from_numpy(np.ascontiguousarray(Vn, dtype=np.float64)).to(dev)
        VV = (Vt[:, :, None] * Vt[:, None, :]).reshape(m, k * k)
        for r0 in range(0, n, SLAB_ROWS):
            X = torch.stack([idf.col(c).data[r0:r0 + SLAB_ROWS].to(torch.float64) for c in cols], dim=1)
            mask = ~torch.isnan(X)
            M = mask.to(torch.float64)
            Z = torch.where(mask, (X - mu_t) * s_t, torch.zeros_like(X))
            A = (M @ VV).reshape(-1, k, k) + (reg * M.sum(1).clamp(min=1.0)).view(-1, 1, 1) * eye
            U = torch.linalg.solve(A, (Z @ Vt).unsqueeze(2)).squeeze(2)
            yield r0, mask, M, Z, U, Vt

    for _ in range(int(max_iter)):
        packed = torch.zeros(m, k * k + k, dtype=torch.float64, device=dev)
        for _, _, M, Z, U, _ in slabs(V):
            packed[:, : k * k] += M.T @ (U[:, :, None] * U[:, None, :]).reshape(-1, k * k)
            packed[:, k * k:] += Z.T @ U
        dist.all_reduce_(packed, "sum")
        P = packed.cpu().numpy()
        V = _cols_solve(P[:, : k * k].reshape(m, k, k), P[:, k * k:], n_cols, reg)
    for r0, mask, _, _, U, Vt in slabs(V):
        pred = (U @ Vt.T) * sd_t + mu_t
        for j, c in enumerate(cols):
            null = ~mask[:, j]
            view = clones[c][r0:r0 + SLAB_ROWS]
            view[null] = pred[:, j][null].to(view.dtype)


def als_impute(idf, cols: List[str], rank: int, max_iter: int, reg: float,
               clones: Dict[str, torch.Tensor], V0=None) -> np.ndarray:
    """Writes the value of every null entry of the columns `cols` into
    clones[c] (a copy of the column, in its dtype); nothing else of the clones
    changes. Every rank fits the same V: one all-reduce per sweep. Returns
    the V0 [m, k] the fit started from (V0, if given)."""
    if not reg > 0:
        raise ValueError("reg must be positive")
    cols = list(cols)
    k = min(int(rank), len(cols))
    if k < 1:
        raise ValueError("rank must be at least 1")
    mu, sd, n_cols = column_scales(idf, cols)
    V0 = als_v0(idf, cols, sd, k) if V0 is None else np.asarray(V0, dtype=np.float64)
    fit = _fit_kernel if kernel_serves(idf, cols, rank) else _fit_slabs
    fit(idf, cols, mu, sd, n_cols, V0, max_iter, reg, clones)
    return V0
