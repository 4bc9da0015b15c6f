"""imputation_sklearn(method_type="KNN", apply_precision=...): the fp64 torch
apply and the K29 kernel path (ops/knn.py). GPU test against sklearn's own
transform of the same model: 0 of 4 800 imputed entries are fp64 ties (k-th /
(k + 1)-th gap below 1e-6 relative; reference alone; at most 0.1 % may be).
"""

import os
import pickle
import tempfile

import numpy as np
import pandas as pd
import pytest
import torch
from sklearn.impute import KNNImputer
from sklearn.metrics.pairwise import nan_euclidean_distances

from anovos_amd.core.frame import AnovosFrame
from anovos_amd.data_analyzer.quality_checker import nullColumns_detection
from anovos_amd.data_transformer import transformers_advanced as TA
from anovos_amd.shared.context import init_context

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


def _frame(n, seed, wide=False):
    rng = np.random.default_rng(seed)
    a = rng.normal(1e4, 3e3, n)
    pdf = pd.DataFrame({
        "a": a.astype(np.float32),
        "b": (a * 0.5 + rng.normal(0, 300, n)).astype(np.float32),
        "c": rng.normal(0, 1e3, n).astype(np.float32),
        "d": rng.normal(1e5, 2e3, n),  # float64
    })
    if wide:
        # spreads of thousands: sklearn's own fp64 |x|^2 + |f|^2 - 2 x f is off by ~4 at 1e8
        pdf["e"] = (1e8 + 8 * rng.integers(-400, 400, n)).astype(np.float32)
        pdf["f"] = (rng.normal(-5e3, 2e3, n) + 0.2 * a).astype(np.float32)
    for c in pdf.columns:
        pdf.loc[rng.choice(n, n // 25, replace=False), c] = np.nan
    return pdf


def _values(odf, cols):
    return np.column_stack([odf.col(c).data.cpu().numpy().astype(np.float64) for c in cols])


def test_cpu_apply_precision():
    pdf = _frame(3000, 1)
    ctx, idf, cols = init_context("cpu"), AnovosFrame.from_pandas(pdf, device="cpu"), list(pdf.columns)
    kw = dict(method_type="KNN", sample_size=1000, sample_seed=42)
    default = _values(TA.imputation_sklearn(ctx, idf, cols, **kw), cols)
    fp64 = _values(TA.imputation_sklearn(ctx, idf, cols, apply_precision="fp64", **kw), cols)
    split = _values(TA.imputation_sklearn(ctx, idf, cols, apply_precision="bf16x2", **kw), cols)
    assert not np.isnan(default).any()
    assert np.array_equal(default, fp64) and np.array_equal(fp64, split)
    with pytest.raises(ValueError, match="apply_precision"):
        TA.imputation_sklearn(ctx, idf, cols, apply_precision="fp16", **kw)
    TA.imputation_sklearn(ctx, idf, cols, method_type="regression", apply_precision="fp16", sample_size=1000)  # ignored
    # nullColumns_detection forwards the key
    cfg = {"sample_size": 1000, "apply_precision": "bf16x2"}
    odf, _ = nullColumns_detection(ctx, idf, "all", treatment=True, treatment_method="KNN", treatment_configs=cfg)
    assert np.array_equal(_values(odf, cols), default)
    with pytest.raises(ValueError, match="apply_precision"):
        nullColumns_detection(ctx, idf, "all", treatment=True, treatment_method="KNN",
                              treatment_configs={**cfg, "apply_precision": "fp16"})


def _true_ties(model, X, k):
    """imputed entries whose k-th / (k + 1)-th fp64 distances differ < 1e-6 relative"""
    F = model._fit_X
    ties = np.zeros(X.shape, dtype=bool)
    for j in range(X.shape[1]):
        rows = np.flatnonzero(np.isnan(X[:, j]))
        d = nan_euclidean_distances(X[rows], F[~np.isnan(F[:, j])], squared=True)
        d = np.sort(np.where(np.isnan(d), np.inf, d), axis=1)
        ties[rows, j] = d[:, k] - d[:, k - 1] < 1e-6 * d[:, k]
    return ties


@requires_gpu
@pytest.mark.gpu
def test_gpu_bf16x2_matches_sklearn_transform():
    pdf = _frame(20000, 3, wide=True)
    cols = list(pdf.columns)
    X = pdf.to_numpy(dtype=np.float64)
    mp = tempfile.mkdtemp(prefix="knn_bf16x2_")
    model = KNNImputer(n_neighbors=5).fit(X[:4000])
    with open(os.path.join(mp, "imputation_sklearn.pkl"), "wb") as f:
        pickle.dump(model, f)
    truth = model.transform(X)
    ties = _true_ties(model, X, 5)
    nulls = np.isnan(X)
    assert ties.sum() <= 1e-3 * nulls.sum()
    ctx, idf = init_context("cuda"), AnovosFrame.from_pandas(pdf, device="cuda")
    out = TA.imputation_sklearn(ctx, idf, cols, method_type="KNN", apply_precision="bf16x2",
                                pre_existing_model=True, model_path=mp)
    got = _values(out, cols)
    assert np.array_equal(got[~nulls], X[~nulls])
    check = nulls & ~ties
    close = np.isclose(got[check], truth[check], rtol=2e-4, atol=2e-3)
    assert close.all(), (int((~close).sum()), float(np.abs(got[check] - truth[check]).max()))
