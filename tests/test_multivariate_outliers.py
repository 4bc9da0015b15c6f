"""Multivariate outlier detection: ops/mahalanobis.py and
quality_checker.multivariate_outlier_detection.

The squared Mahalanobis distance d2 = (x - mu)^T Sigma^+ (x - mu) is
computed in whitening form from the eigen-decomposition of the correlation
matrix. Checked here on the CPU (fp64) path against scikit-learn's
EmpiricalCovariance and a direct pseudo-inverse, on a rank-deficient frame,
on planted rows that no univariate detector sees, and through the public
function's return, model and workflow contracts. One gpu-marked copy runs
the planted-rows case through the MFMA kernel K26.
"""

import numpy as np
import pandas as pd
import pytest
import torch
import yaml
from scipy.stats import chi2

from anovos_amd.core.frame import AnovosFrame
from anovos_amd.data_analyzer import quality_checker as qc
from anovos_amd.ops import mahalanobis as maha
from anovos_amd.shared.context import AnovosContext


@pytest.fixture(scope="module")
def cctx():
    return AnovosContext("cpu")


def _cols(k):
    return [f"x{i:02d}" for i in range(k)]


def _frame(X, names=None, device="cpu"):
    names = names or _cols(X.shape[1])
    return AnovosFrame.from_pandas(pd.DataFrame(X, columns=names), device=device)


def _stat(stats, metric):
    return stats.loc[stats["metric"] == metric, "value"].iloc[0]


# ---------------------------------------------------------------- mahalanobis_d2

def test_d2_matches_sklearn_and_pinv():
    from sklearn.covariance import EmpiricalCovariance

    rng = np.random.default_rng(5)
    n, k = 5000, 12
    X = rng.standard_normal((n, 3)) @ rng.standard_normal((3, k)) + 0.5 * rng.standard_normal((n, k))
    X = X * np.linspace(0.5, 50, k) + np.linspace(-100, 100, k)
    idf = _frame(X)
    model = maha.fit_whitening(idf, _cols(k))
    assert model.rank == k and model.excluded == []
    np.testing.assert_allclose(model.mean, X.mean(0), rtol=1e-12)
    np.testing.assert_allclose(model.sd, X.std(0, ddof=1), rtol=1e-12)
    # the fp64 whitening form itself (the function returns f32)
    Z = (X - model.mean) / model.sd
    d2 = ((Z @ model.W.T) ** 2).sum(1)
    sk = EmpiricalCovariance().fit(X).mahalanobis(X) * (n - 1) / n  # ML covariance -> ddof = 1
    Xc = X - X.mean(0)
    direct = np.einsum("ij,jk,ik->i", Xc, np.linalg.pinv(np.cov(X, rowvar=False)), Xc)
    scale = d2.max()
    assert np.abs(d2 - sk).max() <= 1e-9 * scale
    assert np.abs(d2 - direct).max() <= 1e-9 * scale
    got = maha.mahalanobis_d2(idf, _cols(k), model)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
    # the f32 rounding of the result is all that separates them
    assert np.abs(got.double().numpy() - d2).max() <= 2.0 ** -23 * scale
    assert np.abs(got.double().numpy() - sk).max() <= 1e-9 * scale + 2.0 ** -23 * scale


def test_d2_row_slabs_and_nulls(monkeypatch):
    """several CPU slabs give what one gives; a null counts as the mean"""
    rng = np.random.default_rng(6)
    X = rng.standard_normal((1000, 5)) @ rng.standard_normal((5, 5))
    X[rng.random(X.shape) < 0.1] = np.nan
    X[7] = np.nan
    idf = _frame(X)
    model = maha.fit_whitening(idf, _cols(5))
    one = maha.mahalanobis_d2(idf, _cols(5), model)
    monkeypatch.setattr(maha, "MAHA_SLAB_BYTES", 8 * 10 * 64)  # 64 rows
    many = maha.mahalanobis_d2(idf, _cols(5), model)
    assert torch.equal(one, many)
    assert float(one[7]) == 0.0
    Z = np.nan_to_num((X - model.mean) / model.sd, nan=0.0)
    np.testing.assert_allclose(one.numpy(), ((Z @ model.W.T) ** 2).sum(1), rtol=1e-6)


def test_rank_deficiency_and_constant_column(cctx):
    rng = np.random.default_rng(8)
    n = 4000
    B = rng.standard_normal((n, 5)) @ rng.standard_normal((5, 5)) + np.array([3.0, -20.0, 0.0, 100.0, 7.0])
    names = ["a", "b", "c", "d", "e"]
    full = pd.DataFrame(B, columns=names)
    full["lin"] = 2.0 * full["a"] - 0.5 * full["c"]  # exact linear combination
    full["const"] = 4.25
    cols = names + ["lin", "const"]
    idf = AnovosFrame.from_pandas(full[cols])
    model = maha.fit_whitening(idf, cols)
    assert model.excluded == ["const"]
    assert model.columns == names + ["lin"]
    assert model.rank == len(cols) - 2
    d2 = maha.mahalanobis_d2(idf, model.columns, model).double().numpy()
    base = AnovosFrame.from_pandas(full[names])
    bm = maha.fit_whitening(base, names)
    assert bm.rank == 5
    ref = maha.mahalanobis_d2(base, names, bm).double().numpy()
    assert np.abs(d2 - ref).max() <= 1e-6 * ref.max()
    with pytest.warns(UserWarning, match="const"):
        _, stats = qc.multivariate_outlier_detection(cctx, idf, list_of_cols=cols)
    assert _stat(stats, "excluded_constant_attributes") == "const"
    assert _stat(stats, "rank") == 5.0 and _stat(stats, "attributes_count") == 6.0


# ---------------------------------------------------------------- planted rows

N_REG, N_PLANT, K_PLANT = 20000, 20, 20


@pytest.fixture(scope="module")
def planted():
    """20 000 regular rows of a 3-factor model in 20 columns on very
    different scales, and 20 planted rows whose every coordinate is an
    independent draw within +-1.5 sd: ordinary one by one, impossible
    together."""
    rng = np.random.default_rng(7)
    n, k = N_REG, K_PLANT
    f = rng.standard_normal((n, 3))
    L = rng.standard_normal((3, k))
    X = f @ L + 0.3 * rng.standard_normal((n, k))
    X = X * rng.uniform(0.5, 50, k) + rng.uniform(-100, 100, k)
    mu, sd = X.mean(0), X.std(0, ddof=1)
    P = mu + sd * rng.uniform(-1.5, 1.5, (N_PLANT, k))
    Xa = np.vstack([X, P])
    # the fp64 reference, computed once and left unchanged
    Z = (Xa - Xa.mean(0)) / Xa.std(0, ddof=1)
    lam, V = np.linalg.eigh(np.corrcoef(Xa, rowvar=False))
    W = (V / np.sqrt(lam)).T
    d2 = ((Z @ W.T) ** 2).sum(1)
    return {"X": Xa, "d2": d2, "threshold": float(chi2.ppf(0.999, k))}


def test_planted_rows_are_found_and_univariate_misses_them(cctx, planted):
    Xa, thr = planted["X"], planted["threshold"]
    assert abs(thr - 45.3) < 0.05
    idf = _frame(Xa)
    odf, stats = qc.multivariate_outlier_detection(cctx, idf, append_distance=True)
    assert odf.local_rows() == len(Xa)
    d2 = odf.col("mahalanobis_d2").data.double().numpy()
    assert np.abs(d2 - planted["d2"]).max() <= 2.0 ** -22 * planted["d2"].max()
    assert _stat(stats, "threshold") == pytest.approx(thr, rel=1e-12)
    assert _stat(stats, "rank") == float(K_PLANT)
    flag = d2 > thr
    assert flag[N_REG:].all(), "every planted row is flagged"
    assert d2[N_REG:].min() > 100
    regular = int(flag[:N_REG].sum())
    print(f"regular rows flagged: {regular} (chi-square expectation 20)")
    assert regular <= 60  # a cap: three times the expectation
    assert _stat(stats, "outlier_rows") == float(regular + N_PLANT)
    assert _stat(stats, "rows_count") == float(len(Xa))
    assert _stat(stats, "outlier_pct") == round((regular + N_PLANT) / len(Xa), 4)
    assert _stat(stats, "max_distance") == pytest.approx(float(d2.max()), rel=1e-6)
    # the univariate 3-sigma detector changes none of the planted rows
    uni, ustats = qc.outlier_detection(
        cctx, idf, detection_side="both",
        detection_configs={"stdev_lower": 3.0, "stdev_upper": 3.0, "min_validation": 1},
        treatment=True, treatment_method="value_replacement")
    for c in _cols(K_PLANT):
        assert torch.equal(uni.col(c).data[N_REG:], idf.col(c).data[N_REG:]), c
    assert int(ustats["lower_outliers"].sum() + ustats["upper_outliers"].sum()) > 0


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_planted_rows_gpu_matches_cpu_flags(planted):
    """The same case through K26. A flag may differ from the fp64 one only
    where the fp64 d2 lies within the kernel's derived error bound of the
    threshold; at most 5 such rows are allowed (the reference has none
    within 1e-3 of the threshold on this seed)."""
    from anovos_amd.shared.context import init_context

    Xa, thr, ref = planted["X"], planted["threshold"], planted["d2"]
    assert int((np.abs(ref - thr) < 1e-3).sum()) == 0
    ctx = init_context("cuda:0")
    # f32 columns: the kernel reads them as they are
    idf = _frame(Xa.astype(np.float32), device="cuda:0")
    odf, stats = qc.multivariate_outlier_detection(ctx, idf, append_distance=True)
    d2 = odf.col("mahalanobis_d2").data
    assert d2.dtype == torch.float32 and d2.is_cuda
    d2 = d2.double().cpu().numpy()
    # the derived bound of tests/test_row_quadform_kernel.py, on the fp64
    # model of the f32 frame, plus the f32 rounding of z (3 * 2^-24)
    X32 = Xa.astype(np.float32).astype(np.float64)
    mu, sd = X32.mean(0), X32.std(0, ddof=1)
    Z = (X32 - mu) / sd
    lam, V = np.linalg.eigh(np.corrcoef(X32, rowvar=False))
    W = (V / np.sqrt(lam)).T
    Y = Z @ W.T
    ref32 = (Y ** 2).sum(1)
    eps = (3 * 2.0 ** -18 + 3 * 32 * 2.0 ** -24 + 3 * 2.0 ** -24) * (np.abs(Z) @ np.abs(W).T)
    bound = (2 * np.abs(Y) * eps + eps ** 2).sum(1) + K_PLANT * 2.0 ** -24 * ref32
    ratio = np.abs(d2 - ref32) / bound
    print(f"planted rows on the GPU: max |d2 - ref|/bound = {ratio.max():.4f}")
    assert ratio.max() <= 1
    near = np.abs(ref32 - thr) <= bound
    assert int(near.sum()) <= 5
    flag_gpu, flag_ref = d2 > thr, ref32 > thr
    assert np.array_equal(flag_gpu[~near], flag_ref[~near])
    assert flag_gpu[N_REG:].all()
    assert _stat(stats, "outlier_rows") == float(flag_gpu.sum())


# ---------------------------------------------------------------- contracts

@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(9)
    n = 3000
    X = rng.standard_normal((n, 2)) @ rng.standard_normal((2, 4)) + 0.2 * rng.standard_normal((n, 4))
    X[:5] = X.std(0) * np.array([2.0, -2.0, 2.0, -2.0]) * rng.uniform(0.8, 1.2, (5, 4))
    pdf = pd.DataFrame(X, columns=["p", "q", "r", "s"])
    pdf["label"] = rng.choice(["u", "v"], n)
    return pdf


def test_treatment_and_append_distance(cctx, small):
    idf = AnovosFrame.from_pandas(small)
    same, stats = qc.multivariate_outlier_detection(cctx, idf, confidence=0.99)
    assert same is idf
    assert list(stats.columns) == ["metric", "value"]
    assert list(stats["metric"]) == ["rows_count", "attributes_count", "rank", "threshold", "outlier_rows",
                                     "outlier_pct", "max_distance", "excluded_constant_attributes"]
    assert _stat(stats, "attributes_count") == 4.0  # the categorical column is not taken
    assert _stat(stats, "threshold") == pytest.approx(chi2.ppf(0.99, 4))
    n_out = int(_stat(stats, "outlier_rows"))
    assert 5 <= n_out < 200
    app, _ = qc.multivariate_outlier_detection(cctx, idf, confidence=0.99, append_distance=True, distance_col="dist2")
    assert app.columns == idf.columns + ["dist2"]
    col = app.col("dist2")
    assert col.data.dtype == torch.float32 and col.dtype == "float"
    flag = col.data.double() > float(_stat(stats, "threshold"))
    assert int(flag.sum()) == n_out
    cut, cstats = qc.multivariate_outlier_detection(cctx, idf, confidence=0.99, treatment=True, append_distance=True)
    assert cut.local_rows() == len(small) - n_out
    keep = (~flag).nonzero(as_tuple=True)[0]
    for c in idf.columns:
        assert torch.equal(cut.col(c).data, idf.col(c).data[keep]), c
    assert torch.equal(cut.col("mahalanobis_d2").data, col.data[keep])
    assert _stat(cstats, "outlier_rows") == float(n_out)
    # an explicit threshold overrides the chi-square one
    _, tstats = qc.multivariate_outlier_detection(cctx, idf, threshold=2.5)
    assert _stat(tstats, "threshold") == 2.5
    assert _stat(tstats, "outlier_rows") == float(int((col.data.double() > 2.5).sum()))


def test_model_round_trip(cctx, small, tmp_path):
    idf = AnovosFrame.from_pandas(small)
    mp = str(tmp_path / "model")
    a, sa = qc.multivariate_outlier_detection(cctx, idf, confidence=0.995, append_distance=True, model_path=mp)
    dfm = pd.read_parquet(tmp_path / "model" / "outlier_multivariate" / "part-00000.parquet")
    assert list(dfm["attribute"]) == ["p", "q", "r", "s"]
    assert {"mean", "sd", "W", "rank", "threshold"} <= set(dfm.columns)
    # applied to other rows, the saved model - not a refit - decides
    other = AnovosFrame.from_pandas(small.iloc[::-1].reset_index(drop=True).iloc[:1500])
    b, sb = qc.multivariate_outlier_detection(cctx, other, append_distance=True, pre_existing_model=True, model_path=mp)
    assert _stat(sb, "threshold") == _stat(sa, "threshold")
    da = a.col("mahalanobis_d2").data
    db = b.col("mahalanobis_d2").data
    assert torch.equal(db, da.flip(0)[:1500])
    thr = float(_stat(sa, "threshold"))
    assert _stat(sb, "outlier_rows") == float(int((da.flip(0)[:1500].double() > thr).sum()))
    # a column the model names and the frame lacks
    with pytest.raises(TypeError, match="not in the frame"):
        qc.multivariate_outlier_detection(cctx, other.drop(["q"]), pre_existing_model=True, model_path=mp)


@pytest.mark.parametrize("kwargs", [
    {"confidence": 0}, {"confidence": 1}, {"confidence": 1.5}, {"confidence": "high"},
    {"threshold": 0}, {"threshold": -3.0},
    {"rank_tol": -1e-9}, {"rank_tol": 1}, {"rank_tol": "tiny"},
    {"append_distance": True, "distance_col": "p"},
    {"treatment": "maybe"},
    {"list_of_cols": ["p"]},
    {"list_of_cols": ["p", "label"]},
])
def test_invalid_arguments(cctx, small, kwargs):
    idf = AnovosFrame.from_pandas(small)
    with pytest.raises(TypeError):
        qc.multivariate_outlier_detection(cctx, idf, **kwargs)


def test_too_few_and_too_many_columns(cctx):
    rng = np.random.default_rng(10)
    one_live = pd.DataFrame({"a": rng.standard_normal(50), "b": np.ones(50), "c": np.full(50, 2.0)})
    with pytest.raises(TypeError, match="fewer than 2"):
        qc.multivariate_outlier_detection(cctx, AnovosFrame.from_pandas(one_live))
    wide = _frame(rng.standard_normal((8, maha.ROWQUAD_MAX_COLS + 1)),
                  names=[f"w{i}" for i in range(maha.ROWQUAD_MAX_COLS + 1)])
    with pytest.raises(TypeError, match=str(maha.ROWQUAD_MAX_COLS)):
        qc.multivariate_outlier_detection(cctx, wide)


def test_fit_runs_on_a_sample_distance_on_the_full_frame(cctx, small):
    idf = AnovosFrame.from_pandas(small)
    odf, stats = qc.multivariate_outlier_detection(cctx, idf, sample_size=1000, append_distance=True)
    assert odf.local_rows() == len(small) and _stat(stats, "rows_count") == float(len(small))
    full, _ = qc.multivariate_outlier_detection(cctx, idf, append_distance=True)
    a, b = odf.col("mahalanobis_d2").data, full.col("mahalanobis_d2").data
    assert not torch.equal(a, b)                      # another fit ...
    assert float(((a - b).abs() / (1 + b)).max()) < 0.5  # ... of the same population


def test_reachable_from_a_workflow_config(tmp_path):
    from anovos_amd import workflow

    rng = np.random.default_rng(11)
    n = 1500
    u = rng.standard_normal(n)
    pdf = pd.DataFrame({"id": [f"r{i}" for i in range(n)], "u": u,
                        "v": 3 * u + 0.1 * rng.standard_normal(n) + 50,
                        "w": rng.standard_normal(n)})
    pdf.loc[0, ["u", "v"]] = [1.5, 50 - 4.5]  # ordinary coordinates, impossible pair
    src = tmp_path / "in.csv"
    pdf.to_csv(src, index=False)
    rep = str(tmp_path / "report")
    cfg = {
        "input_dataset": {"read_dataset": {"file_path": str(src), "file_type": "csv",
                                           "file_configs": {"header": True, "inferSchema": True}}},
        "quality_checker": {"multivariate_outlier_detection": {"list_of_cols": "all", "treatment": True}},
        "report_preprocessing": {"master_path": rep},
    }
    cfg_path = tmp_path / "cfg.yaml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f, sort_keys=False)
    df = workflow.run(str(cfg_path))
    stats = pd.read_csv(tmp_path / "report" / "multivariate_outlier_detection.csv")
    removed = int(float(_stat(stats, "outlier_rows")))
    assert removed >= 1 and df.local_rows() == n - removed
    assert "r0" not in set(df.to_pandas()["id"])
