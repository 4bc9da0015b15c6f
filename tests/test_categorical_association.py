"""categorical_association_matrix and pair_contingency_tables against
pandas / scipy / scikit-learn and plain-numpy formulas.

The statistics are fp64 host code over integer tables of fewer than 10^4
cells with values in [0, 1] (V, U) or below ln r (MI): both sides round at
about 1e-12, so reference values are compared at 1e-9 absolute and exact
identities (a recoded column, a removed null row) at 1e-12."""

import math
import warnings

import numpy as np
import pandas as pd
import pytest
import torch
import yaml

from anovos_amd.core.frame import AnovosFrame
from anovos_amd.data_analyzer import association_evaluator as ae
from anovos_amd.ops.contingency import pair_contingency_tables

REF_TOL = 1e-9
EXACT_TOL = 1e-12


# ------------------------------------------------------------------ tables
def test_tables_match_pandas_crosstab(income_frame, income_pdf):
    cols = ["workclass", "education", "income"]
    tables = pair_contingency_tables(income_frame, cols)
    assert set(tables) == {("workclass", "education"), ("workclass", "income"), ("education", "income")}
    for (a, b), got in tables.items():
        da, db = income_frame.col(a).dictionary, income_frame.col(b).dictionary
        ct = pd.crosstab(income_pdf[a], income_pdf[b], dropna=False)
        want = ct.reindex(index=list(da) + [np.nan], columns=list(db) + [np.nan], fill_value=0).to_numpy()
        assert got.dtype == np.int64 and got.shape == (len(da) + 1, len(db) + 1)
        np.testing.assert_array_equal(got, want)
        assert got.sum() == len(income_pdf)
    # the fixture has 10 null workclass values and none elsewhere
    assert tables[("workclass", "education")][-1].sum() == 10
    assert tables[("education", "income")][-1].sum() == 0


def test_tables_explicit_pairs_and_orientation(income_frame):
    cols = ["workclass", "education"]
    t = pair_contingency_tables(income_frame, cols, [("education", "workclass"), ("workclass", "workclass")])
    u = pair_contingency_tables(income_frame, cols)
    np.testing.assert_array_equal(t[("education", "workclass")], u[("workclass", "education")].T)
    d = t[("workclass", "workclass")]
    np.testing.assert_array_equal(d, np.diag(np.diag(d)))


# -------------------------------------------------------- reference values
@pytest.fixture(scope="module")
def assoc_pdf():
    rng = np.random.default_rng(2024)
    n = 500
    a = rng.choice(["a0", "a1", "a2", "a3"], n, p=[0.4, 0.3, 0.2, 0.1]).astype(object)
    # b follows a half of the time
    b = np.where(rng.random(n) < 0.5, np.char.replace(a.astype(str), "a", "b"), rng.choice(["b0", "b1", "b2", "b7", "b9"], n)).astype(object)
    b[rng.choice(n, 37, replace=False)] = None
    c = rng.choice(["u", "v", "w"], n).astype(object)
    x = rng.normal(0, 1, n) + (a == "a0") * 1.5
    x[rng.choice(n, 11, replace=False)] = np.nan
    return pd.DataFrame({"a": a, "b": b, "c": c, "x": x})


@pytest.fixture(scope="module")
def assoc_frame(assoc_pdf):
    return AnovosFrame.from_pandas(assoc_pdf)


@pytest.fixture(scope="module")
def assoc_labels(ctx, assoc_frame, assoc_pdf):
    """The frame as plain label columns: categoricals as they are, x as
    its equal-frequency bin label (NaN stays null)."""
    from anovos_amd.data_transformer.transformers import attribute_binning

    binned = attribute_binning(ctx, assoc_frame.select(["x"]), ["x"], [], "equal_frequency", 10,
                               "numerical", False, "NA", "replace")
    lab = assoc_pdf.copy()
    lab["x"] = binned.col("x").data.cpu().numpy().astype(np.float64)
    return lab


COLS = ["a", "b", "c", "x"]
PAIRS = [(p, q) for i, p in enumerate(COLS) for q in COLS[i + 1:]]


def _matrix(odf):
    assert list(odf.columns) == ["attribute"] + sorted(odf["attribute"])
    return odf.set_index("attribute")


def _complete(lab, p, q):
    sub = lab[[p, q]].dropna()
    return sub[p].to_numpy(), sub[q].to_numpy()


def _crosstab(lab, p, q):
    x, y = _complete(lab, p, q)
    return pd.crosstab(pd.Series(x), pd.Series(y)).to_numpy().astype(np.float64)


def test_cramers_v_matches_scipy(ctx, assoc_frame, assoc_labels):
    from scipy.stats.contingency import association

    m = _matrix(ae.categorical_association_matrix(ctx, assoc_frame, method_type="cramers_v"))
    for p, q in PAIRS:
        want = association(_crosstab(assoc_labels, p, q).astype(np.int64), method="cramer")
        assert abs(m.loc[p, q] - want) <= REF_TOL, (p, q, m.loc[p, q], want)
        assert m.loc[p, q] == m.loc[q, p]
    for p in COLS:
        assert abs(m.loc[p, p] - 1.0) <= EXACT_TOL


def test_mutual_info_matches_sklearn(ctx, assoc_frame, assoc_labels):
    from sklearn.metrics import mutual_info_score

    m = _matrix(ae.categorical_association_matrix(ctx, assoc_frame, method_type="mutual_info"))
    for p, q in PAIRS:
        x, y = _complete(assoc_labels, p, q)
        want = mutual_info_score(x.astype(str), y.astype(str))
        assert abs(m.loc[p, q] - want) <= REF_TOL, (p, q, m.loc[p, q], want)
        assert m.loc[p, q] == m.loc[q, p]
    for p in COLS:
        v = assoc_labels[p].dropna()
        pr = v.value_counts().to_numpy() / len(v)
        assert abs(m.loc[p, p] - float(-(pr * np.log(pr)).sum())) <= REF_TOL


def _entropy(counts):
    pr = counts[counts > 0] / counts.sum()
    return float(-(pr * np.log(pr)).sum())


def _mi(t):
    n = t.sum()
    outer = np.outer(t.sum(axis=1), t.sum(axis=0))
    nz = t > 0
    return float((t[nz] / n * np.log(t[nz] * n / outer[nz])).sum())


def test_theils_u_matches_formula(ctx, assoc_frame, assoc_labels):
    m = _matrix(ae.categorical_association_matrix(ctx, assoc_frame, method_type="theils_u"))
    for p, q in PAIRS:
        t = _crosstab(assoc_labels, p, q)
        want_pq = _mi(t) / _entropy(t.sum(axis=1))  # [row p, column q] = MI / H(p)
        want_qp = _mi(t) / _entropy(t.sum(axis=0))
        assert abs(m.loc[p, q] - want_pq) <= REF_TOL, (p, q, m.loc[p, q], want_pq)
        assert abs(m.loc[q, p] - want_qp) <= REF_TOL, (q, p, m.loc[q, p], want_qp)
    for p in COLS:
        assert abs(m.loc[p, p] - 1.0) <= EXACT_TOL


def test_bias_corrected_v_matches_formula(ctx, assoc_frame, assoc_labels):
    m = _matrix(ae.categorical_association_matrix(ctx, assoc_frame, method_type="cramers_v", bias_correction=True))
    plain = _matrix(ae.categorical_association_matrix(ctx, assoc_frame, method_type="cramers_v"))
    for p, q in PAIRS:
        t = _crosstab(assoc_labels, p, q)
        n = t.sum()
        r, c = t.shape
        e = np.outer(t.sum(axis=1), t.sum(axis=0)) / n
        phi2 = ((t - e) ** 2 / e).sum() / n
        phi2c = max(0.0, phi2 - (r - 1) * (c - 1) / (n - 1))
        rt = r - (r - 1) ** 2 / (n - 1)
        ct = c - (c - 1) ** 2 / (n - 1)
        want = math.sqrt(phi2c / min(rt - 1, ct - 1))
        assert abs(m.loc[p, q] - want) <= REF_TOL, (p, q, m.loc[p, q], want)
        assert m.loc[p, q] <= plain.loc[p, q]
    assert m.loc["a", "b"] > 0.3  # a real association survives the correction


# --------------------------------------------------------------- properties
def _frame(**cols):
    return AnovosFrame.from_pandas(pd.DataFrame(cols))


def test_bijective_recoding_is_perfect(ctx):
    rng = np.random.default_rng(5)
    x = rng.choice(["p", "q", "r", "s", "t"], 300, p=[0.5, 0.2, 0.15, 0.1, 0.05]).astype(object)
    y = np.array([{"p": "E", "q": "A", "r": "D", "s": "B", "t": "C"}[v] for v in x], dtype=object)
    idf = _frame(x=x, y=y)
    for method in ("cramers_v", "theils_u"):
        m = _matrix(ae.categorical_association_matrix(ctx, idf, method_type=method))
        assert np.abs(m.to_numpy(dtype=np.float64) - 1.0).max() <= EXACT_TOL, method


def test_constant_column_gives_nan_not_an_exception(ctx):
    rng = np.random.default_rng(6)
    idf = _frame(k=np.array(["only"] * 200, dtype=object),
                 x=rng.choice(["a", "b", "c"], 200).astype(object),
                 y=rng.choice(["u", "v"], 200).astype(object))
    v = _matrix(ae.categorical_association_matrix(ctx, idf, method_type="cramers_v"))
    assert v.loc["k"].isna().all() and v["k"].isna().all()
    assert not v.loc[["x", "y"], ["x", "y"]].isna().any().any()
    u = _matrix(ae.categorical_association_matrix(ctx, idf, method_type="theils_u"))
    assert u.loc["k"].isna().all()  # H(k) = 0
    mi = _matrix(ae.categorical_association_matrix(ctx, idf, method_type="mutual_info"))
    assert math.isnan(mi.loc["k", "k"])


def test_all_null_pair_gives_nan(ctx):
    idf = _frame(x=np.array(["a", "b", None, None], dtype=object),
                 y=np.array([None, None, "u", "v"], dtype=object))
    for method in ("cramers_v", "mutual_info", "theils_u"):
        m = _matrix(ae.categorical_association_matrix(ctx, idf, method_type=method))
        assert math.isnan(m.loc["x", "y"]) and math.isnan(m.loc["y", "x"])
        assert not math.isnan(m.loc["x", "x"])
    bc = _matrix(ae.categorical_association_matrix(ctx, idf, bias_correction=True))
    assert math.isnan(bc.loc["x", "y"])


def test_symmetry_and_asymmetry(ctx, assoc_frame):
    for method in ("cramers_v", "mutual_info"):
        m = _matrix(ae.categorical_association_matrix(ctx, assoc_frame, method_type=method)).to_numpy(dtype=np.float64)
        np.testing.assert_array_equal(m, m.T)
    # a column and a coarsening of it: the fine column determines the
    # coarse one, not the other way round
    rng = np.random.default_rng(8)
    fine = rng.choice(["a1", "a2", "b1", "b2", "b3"], 400).astype(object)
    coarse = np.array([v[0] for v in fine], dtype=object)
    u = _matrix(ae.categorical_association_matrix(ctx, _frame(coarse=coarse, fine=fine), method_type="theils_u"))
    assert abs(u.loc["coarse", "fine"] - 1.0) <= EXACT_TOL  # MI / H(coarse): coarse is known from fine
    assert u.loc["fine", "coarse"] < 0.9


def test_nulls_equal_rows_removed(ctx, assoc_frame, assoc_pdf):
    sub = AnovosFrame.from_pandas(assoc_pdf.dropna(subset=["a", "b"]).reset_index(drop=True)[["a", "b"]])
    for method in ("cramers_v", "mutual_info", "theils_u"):
        full = _matrix(ae.categorical_association_matrix(ctx, assoc_frame, ["a", "b"], method_type=method))
        cut = _matrix(ae.categorical_association_matrix(ctx, sub, ["a", "b"], method_type=method))
        for p, q in (("a", "b"), ("b", "a")):
            assert abs(full.loc[p, q] - cut.loc[p, q]) <= EXACT_TOL, (method, p, q)


def test_max_categories_drops_and_warns(ctx, income_frame):
    with pytest.warns(UserWarning, match="ifa"):
        m = _matrix(ae.categorical_association_matrix(ctx, income_frame, ["ifa", "workclass", "education"],
                                                      max_categories=50))
    assert list(m.index) == ["education", "workclass"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = _matrix(ae.categorical_association_matrix(ctx, income_frame, ["workclass", "education"],
                                                      max_categories=5))
    assert list(m.index) == ["education", "workclass"]
    with pytest.warns(UserWarning, match="education"):
        with pytest.raises(TypeError):
            ae.categorical_association_matrix(ctx, income_frame, ["education"], max_categories=4)


def test_invalid_inputs(ctx, income_frame):
    with pytest.raises(TypeError):
        ae.categorical_association_matrix(ctx, income_frame, method_type="pearson")
    with pytest.raises(TypeError):
        ae.categorical_association_matrix(ctx, income_frame, ["workclass", "no_such_column"])
    with pytest.raises(TypeError):
        ae.categorical_association_matrix(ctx, income_frame, ["workclass"], drop_cols=["workclass"])


def test_all_columns_and_single_column(ctx, income_frame):
    m = _matrix(ae.categorical_association_matrix(ctx, income_frame, drop_cols=["ifa"]))
    assert list(m.index) == sorted(["age", "fnlwgt", "hours_per_week", "workclass", "education", "income"])
    assert np.abs(np.diag(m.to_numpy(dtype=np.float64)) - 1.0).max() <= EXACT_TOL
    one = _matrix(ae.categorical_association_matrix(ctx, income_frame, ["workclass"], method_type="mutual_info"))
    cnt = income_frame.col("workclass").to_pandas_series().value_counts().to_numpy()
    assert abs(one.loc["workclass", "workclass"] - _entropy(cnt.astype(np.float64))) <= REF_TOL


# ----------------------------------------------------------------- workflow
def test_workflow_writes_csv(tmp_path, income_pdf):
    from anovos_amd import workflow

    data = tmp_path / "income.csv"
    income_pdf.to_csv(data, index=False)
    rep = tmp_path / "report"
    cfg = {
        "input_dataset": {
            "read_dataset": {"file_path": str(data), "file_type": "csv",
                             "file_configs": {"header": True, "inferSchema": True}},
        },
        "association_evaluator": {
            "categorical_association_matrix": {"list_of_cols": "all", "drop_cols": ["ifa"],
                                               "method_type": "theils_u"},
        },
        "report_preprocessing": {"master_path": str(rep)},
    }
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f, sort_keys=False)
    workflow.run(str(tmp_path / "cfg.yaml"), device="cpu")
    out = pd.read_csv(rep / "categorical_association_matrix.csv")
    want = sorted(["age", "fnlwgt", "hours_per_week", "workclass", "education", "income"])
    assert list(out.columns) == ["attribute"] + want
    assert list(out["attribute"]) == want
    vals = out[want].to_numpy(dtype=np.float64)
    assert np.isfinite(vals).all() and (vals >= 0).all() and (vals <= 1 + EXACT_TOL).all()


# ---------------------------------------------------------------------- gpu
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_gpu_equals_cpu(assoc_pdf):
    from anovos_amd.shared.context import AnovosContext

    rng = np.random.default_rng(31)
    pdf = pd.concat([assoc_pdf] * 3, ignore_index=True)
    pdf["y"] = rng.integers(0, 7, len(pdf)).astype(np.float64)
    cpu = AnovosFrame.from_pandas(pdf, device="cpu")
    gpu = AnovosFrame.from_pandas(pdf, device="cuda:0")
    cats = ["a", "b", "c"]
    tc = pair_contingency_tables(cpu, cats)
    tg = pair_contingency_tables(gpu, cats)
    assert set(tc) == set(tg)
    for k in tc:
        np.testing.assert_array_equal(tg[k], tc[k])
    ctx_c, ctx_g = AnovosContext("cpu"), AnovosContext("cuda:0")  # the session's context stays as it is
    for method in ("cramers_v", "mutual_info", "theils_u"):
        mc = ae.categorical_association_matrix(ctx_c, cpu, method_type=method)
        mg = ae.categorical_association_matrix(ctx_g, gpu, method_type=method)
        assert list(mc.columns) == list(mg.columns) and list(mc["attribute"]) == list(mg["attribute"])
        names = list(mc["attribute"])
        np.testing.assert_array_equal(mg[names].to_numpy(dtype=np.float64), mc[names].to_numpy(dtype=np.float64))
