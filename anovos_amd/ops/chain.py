"""The apply step of regression imputation (kernel K31): sklearn's
IterativeImputer.transform with linear estimators, as a row-local chain.

The fitted model is: initial statistics s_j, R = n_iter_ rounds, one visiting
order order[p] (p < m_s <= m) shared by the rounds, per step (r, p)
coefficients c_{r,p} over its neighbour columns (zero elsewhere and at its
own target), an intercept b_{r,p}, and clip bounds [min_j, max_j].

All work is in centred space, where a null and its initial fill are both 0:

    z0_i       = isnan(x_i) ? 0 : x_i - s_i
    beta_{r,p} = b_{r,p} + c_{r,p} . s - s_{order[p]}
    for r < R, p < m_s, j = order[p] null in the row (Omega = its nulls):
        z_j <- clip(beta_{r,p} + sum_i C[r,p,i] z_i, min_j - s_j, max_j - s_j)

with z = z0 on the observed columns and the chain state on Omega; the value
of a null entry is z_j + s_j. Steps whose target is observed do nothing.

- chain_model: the model in this form, fp64, or None where it has no such form.
- chain_replay_fp64: the recurrence in fp64 numpy - the definition the kernel
  tests hold K31 to.
- chain_impute: K31 (ops/hip/chain_impute.hip) over the frame's columns,
  writing only the null entries of caller-owned clones.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from anovos_amd.ops import backend

# CHAIN_MAX_COLS, CHAIN_MAX_ROUNDS of ops/hip/anovos_kernels.h
CHAIN_MAX_COLS = 160
CHAIN_MAX_ROUNDS = 32

ChainModel = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]


def CHAIN_GAMMA(m_pad: int) -> float:
    """Bound of K31's observed part, |P_kernel - P| <= gamma * sum_i |C_i| |z0_i|,
    the figure of K26 - K30. K31 multiplies all four split products: each
    operand's hi + lo residual is at most 2^-17, together 2^-16 < 3 * 2^-18 +
    97 * 2^-24, which leaves the rest for the fp32 sum of the products and the
    intercept (derivation in ops/hip/chain_impute.hip)."""
    return 3 * 2.0 ** -18 + (3 * int(m_pad) + 1) * 2.0 ** -24


def chain_model(model, m: int) -> Optional[ChainModel]:
    """(s [m], order [m_s], C [R, m_s, m], beta [R, m_s], lo [m], hi [m]) of a
    fitted IterativeImputer over m columns, fp64, lo / hi in centred space;
    None - use the step-by-step path - when a step's estimator is not linear,
    the rounds do not share one visiting order, a feature was dropped at fit,
    the sequence is empty or the kernel's limits are exceeded."""
    s = np.asarray(model.initial_imputer_.statistics_, dtype=np.float64).reshape(-1)
    seq = list(getattr(model, "imputation_sequence_", []))
    R = int(getattr(model, "n_iter_", 0))
    if s.shape != (m,) or np.isnan(s).any() or R < 1 or not seq or len(seq) % R:
        return None
    m_s = len(seq) // R
    if not (2 <= m <= CHAIN_MAX_COLS and R <= CHAIN_MAX_ROUNDS and 1 <= m_s <= m):
        return None
    order = np.array([int(t.feat_idx) for t in seq[:m_s]], dtype=np.int64)
    if len(set(order.tolist())) != m_s:
        return None
    C = np.zeros((R, m_s, m), dtype=np.float64)
    b = np.zeros((R, m_s), dtype=np.float64)
    for i, t in enumerate(seq):
        r, p = divmod(i, m_s)
        if int(t.feat_idx) != order[p] or not hasattr(t.estimator, "coef_"):
            return None
        nb = np.asarray(t.neighbor_feat_idx, dtype=np.int64)
        C[r, p, nb] = np.asarray(t.estimator.coef_, dtype=np.float64).reshape(-1)
        C[r, p, order[p]] = 0.0
        b[r, p] = float(np.asarray(t.estimator.intercept_).reshape(-1)[0])
    beta = b + C @ s - s[order][None, :]
    lo = np.broadcast_to(np.asarray(getattr(model, "_min_value", -np.inf), dtype=np.float64), (m,)) - s
    hi = np.broadcast_to(np.asarray(getattr(model, "_max_value", np.inf), dtype=np.float64), (m,)) - s
    return s, order, C, beta, lo, hi


def chain_replay_fp64(X, center, order, C, beta, lo, hi) -> np.ndarray:
    """The recurrence on X [n, m] (NaN = null) in fp64: X with every null of a
    column in `order` replaced by z_j + center_j; other entries as they are."""
    X = np.asarray(X, dtype=np.float64)
    center, C, beta = (np.asarray(a, dtype=np.float64) for a in (center, C, beta))
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    miss = np.isnan(X)
    z = np.where(miss, 0.0, X - center)
    for r in range(C.shape[0]):
        for p, j in enumerate(np.asarray(order).tolist()):
            c = C[r, p].copy()
            c[j] = 0.0
            z[:, j] = np.where(miss[:, j], np.clip(beta[r, p] + z @ c, lo[j], hi[j]), z[:, j])
    out = X.copy()
    targets = np.zeros(X.shape[1], dtype=bool)
    targets[np.asarray(order)] = True
    fill = miss & targets[None, :]
    out[fill] = (z + center)[fill]
    return out


def chain_error_bound(z0, order, C, beta, lo, hi, m_pad: int, e0=0.0, u_c: float = 0.0):
    """(z, e): the fp64 replay on centred values z0 [n, m] (NaN = null; z is z0
    on observed entries and the final state on nulls) and K31's bound on the
    error of every null's state, the same recurrence run on errors:

        e_j <- (gamma + u_c) sum_obs |C_i| |z0_i| + sum_obs |C_i| e0_i
               + u (|beta| + sum_obs |C_i| |z0_i| + sum_Omega |C_i| (|z_i| + e_i)) (|Omega| + 2)
               + sum_Omega |C_i| e_i

    gamma = CHAIN_GAMMA(m_pad), u = 2^-24: the rounding of beta + P and of
    each of the |Omega| + 1 sums of the chain step; clipping is 1-Lipschitz.
    e0 [n, m] is the error z0 already carries, u_c a relative error of C."""
    z0 = np.asarray(z0, dtype=np.float64)
    miss = np.isnan(z0)
    z = np.where(miss, 0.0, z0)
    zobs, e, u = np.abs(z), np.zeros(z.shape), 2.0 ** -24
    e0 = np.where(miss, 0.0, np.broadcast_to(e0, z.shape))
    for r in range(C.shape[0]):
        for p, j in enumerate(np.asarray(order).tolist()):
            a = np.abs(C[r, p])
            obs = zobs @ a
            mag = abs(beta[r, p]) + obs + (miss * (np.abs(z) + e)) @ a
            ej = (CHAIN_GAMMA(m_pad) + u_c) * obs + e0 @ a + u * mag * (miss.sum(1) + 2) + (miss * e) @ a
            zj = np.clip(beta[r, p] + z @ C[r, p], lo[j], hi[j])
            z[:, j], e[:, j] = np.where(miss[:, j], zj, z[:, j]), np.where(miss[:, j], ej, 0.0)
    return z, e


def kernel_serves(idf, cols: List[str]) -> bool:
    """True where chain_impute runs K31: the HIP backend."""
    return idf.device.type == "cuda" and backend.use_hip(idf.col(cols[0]).data)


def chain_impute(idf, cols: List[str], cm: ChainModel, clones: Dict[str, torch.Tensor]) -> None:
    """Writes the imputed value of every null entry of the columns `cols`
    into clones[c] (a copy of the column, in its dtype); nothing else of the
    clones changes. f32 columns go to the kernel as they are with centre s_j
    and are written in place; f64 columns are centred in fp64 before the
    downcast, take centre 0, and get their results added back in fp64."""
    s, order, C, beta, lo, hi = cm
    cols = list(cols)
    dev = idf.device
    ext = backend.hip_ext()
    f32, outs, center, wide = [], [], [], []
    for j, c in enumerate(cols):
        t = idf.col(c).data
        if t.dtype == torch.float32:
            f32.append(t.contiguous())
            outs.append(clones[c])
            center.append(float(s[j]))
        else:
            f32.append((t.to(torch.float64) - float(s[j])).to(torch.float32).contiguous())
            outs.append(torch.zeros_like(f32[-1]))
            center.append(0.0)
            wide.append(j)
    as_f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.float32).to(dev)
    ext.chain_impute_bf16x2(f32, torch.tensor(center, dtype=torch.float64),
                            torch.from_numpy(np.asarray(order, dtype=np.int32)), as_f32(C), as_f32(beta),
                            as_f32(lo), as_f32(hi), outs)
    for j in sorted(set(range(len(cols))) - set(np.asarray(order).tolist())):
        # never a target: its nulls keep the initial fill
        clone = clones[cols[j]]
        clone.masked_fill_(torch.isnan(clone), float(s[j]))
    for j in wide:
        if j not in set(np.asarray(order).tolist()):
            continue
        clone = clones[cols[j]]
        null = torch.isnan(f32[j])
        clone[null] = (outs[j][null].to(torch.float64) + float(s[j])).to(clone.dtype)
