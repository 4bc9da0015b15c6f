"""numerical_categorical_association and ops.grouped.grouped_moments
against pandas / scipy / scikit-learn and plain-numpy formulas.

The statistics are fp64 host code over per-group moments of a few hundred
rows with values of O(1) (eta in [0, 1], F of order 1 to 100): both sides
round near 1e-13, so reference values are compared at 1e-9 (absolute for
eta, relative for F) and exact identities (an affine map of x, recoded
categories) at 1e-12 — the reasoning of tests/test_categorical_association.py."""

import math
import warnings

import numpy as np
import pandas as pd
import pytest
import torch
import yaml

from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.data_analyzer import association_evaluator as ae
from anovos_amd.ops.grouped import grouped_moments

REF_TOL = 1e-9
EXACT_TOL = 1e-12


# ----------------------------------------------------------------- moments
def test_grouped_moments_match_pandas_groupby(income_frame, income_pdf):
    """Every (categorical, numerical) pair of the income fixture, with the
    null slot (10 null workclass values), NaN values (20 null ages) and a
    category without a row (an unused dictionary entry)."""
    edu = income_frame.col("education")
    wide = Column("education", "string", edu.data, list(edu.dictionary) + ["Unused"])
    idf = AnovosFrame({"workclass": income_frame.col("workclass"), "education": wide,
                       "age": income_frame.col("age"), "hours_per_week": income_frame.col("hours_per_week"),
                       "fnlwgt": income_frame.col("fnlwgt")}, income_frame.device)
    cats, nums = ["workclass", "education"], ["age", "hours_per_week", "fnlwgt"]
    res = grouped_moments(idf, cats, nums)
    assert set(res) == {(c, v) for c in cats for v in nums}
    for (c, v), got in res.items():
        labels = list(idf.col(c).dictionary)
        assert got.dtype == np.float64 and got.shape == (len(labels) + 1, 3)
        agg = income_pdf.groupby(c, dropna=False)[v].agg(["count", "mean", "var"])
        for s, lab in enumerate(labels + [np.nan]):
            hit = [k for k in agg.index if (k == lab) or (k != k and lab != lab)]
            if not hit or agg.loc[hit[0], "count"] == 0:
                assert got[s, 0] == 0 and math.isnan(got[s, 1]) and math.isnan(got[s, 2]), (c, v, lab)
                continue
            cnt, mean, var = agg.loc[hit[0]]
            assert got[s, 0] == cnt
            assert abs(got[s, 1] - mean) <= REF_TOL * max(1.0, abs(mean)), (c, v, lab)
            m2 = var * (cnt - 1) if cnt > 1 else 0.0
            assert abs(got[s, 2] - m2) <= REF_TOL * max(1.0, m2), (c, v, lab)
    assert res[("workclass", "hours_per_week")][-1, 0] == 10  # the null slot
    assert res[("education", "age")][-2, 0] == 0  # the unused entry
    assert res[("education", "age")][:, 0].sum() == income_pdf["age"].notna().sum()


def test_grouped_moments_explicit_pairs_and_refusals(income_frame):
    res = grouped_moments(income_frame, ["workclass", "education"], ["age", "fnlwgt"],
                          [("education", "fnlwgt"), ("workclass", "age")])
    full = grouped_moments(income_frame, ["workclass", "education"], ["age", "fnlwgt"])
    assert list(res) == [("education", "fnlwgt"), ("workclass", "age")]
    for k in res:
        np.testing.assert_array_equal(res[k], full[k])
    with pytest.raises(TypeError):
        grouped_moments(income_frame, ["age"], ["fnlwgt"])
    with pytest.raises(TypeError):
        grouped_moments(income_frame, ["workclass"], ["education"])


# -------------------------------------------------------- reference values
@pytest.fixture(scope="module")
def anova_pdf():
    rng = np.random.default_rng(2025)
    n = 600
    a = rng.choice(["a0", "a1", "a2", "a3"], n, p=[0.4, 0.3, 0.2, 0.1]).astype(object)
    b = rng.choice(["u", "v", "w"], n).astype(object)
    b[rng.choice(n, 31, replace=False)] = None
    x = rng.normal(0, 1, n) + (a == "a0") * 1.5 - (a == "a3") * 0.7
    x[rng.choice(n, 17, replace=False)] = np.nan
    y = rng.normal(5, 2, n) + (b == "w") * 0.4
    z = 1000.0 + rng.normal(0, 0.5, n) + (a == "a1") * 0.3  # |mean| >> sigma
    return pd.DataFrame({"a": a, "b": b, "x": x, "y": y, "z": z})


@pytest.fixture(scope="module")
def anova_frame(anova_pdf):
    return AnovosFrame.from_pandas(anova_pdf)


CATS, NUMS = ["a", "b"], ["x", "y", "z"]


def _matrix(odf, cats=CATS, nums=NUMS):
    assert list(odf.columns) == ["attribute"] + sorted(nums)
    assert list(odf["attribute"]) == sorted(cats)
    return odf.set_index("attribute")


def _groups(pdf, c, v):
    sub = pdf[[c, v]].dropna()
    return [g[v].to_numpy(dtype=np.float64) for _, g in sub.groupby(c)]


def test_anova_f_matches_scipy_and_sklearn(ctx, anova_frame, anova_pdf):
    from scipy.stats import f_oneway
    from sklearn.feature_selection import f_classif

    m = _matrix(ae.numerical_categorical_association(ctx, anova_frame, method_type="anova_f"))
    for c in CATS:
        for v in NUMS:
            want = float(f_oneway(*_groups(anova_pdf, c, v)).statistic)
            assert abs(m.loc[c, v] - want) <= REF_TOL * abs(want), (c, v, m.loc[c, v], want)
            if v == "z":
                # f_classif takes SSB from raw sums of squares: at mean 1000 it
                # cancels n * mean^2 * 2^-53 = 7e-8 against an SSB below 1, so it
                # is no reference at 1e-9 for this column (f_oneway centres first)
                continue
            sub = anova_pdf[[c, v]].dropna()
            f_sk = float(f_classif(sub[[v]].to_numpy(), sub[c].to_numpy().astype(str))[0][0])
            assert abs(m.loc[c, v] - f_sk) <= REF_TOL * abs(f_sk), (c, v, m.loc[c, v], f_sk)


def test_eta_matches_formula_and_f(ctx, anova_frame, anova_pdf):
    eta2 = _matrix(ae.numerical_categorical_association(ctx, anova_frame, method_type="eta_squared"))
    eta = _matrix(ae.numerical_categorical_association(ctx, anova_frame))  # correlation_ratio is the default
    f = _matrix(ae.numerical_categorical_association(ctx, anova_frame, method_type="anova_f"))
    for c in CATS:
        for v in NUMS:
            groups = _groups(anova_pdf, c, v)
            allv = np.concatenate(groups)
            mu = allv.mean()
            ssb = sum(g.size * (g.mean() - mu) ** 2 for g in groups)
            sst = float(((allv - mu) ** 2).sum())
            assert abs(eta2.loc[c, v] - ssb / sst) <= REF_TOL, (c, v)
            assert abs(eta.loc[c, v] - math.sqrt(ssb / sst)) <= REF_TOL, (c, v)
            k, n = len(groups), allv.size
            fk = f.loc[c, v] * (k - 1)
            assert abs(eta2.loc[c, v] - fk / (fk + n - k)) <= REF_TOL, (c, v)
    assert eta.loc["a", "x"] > 0.4 and eta.loc["b", "x"] < 0.2  # a drives x, b does not


# --------------------------------------------------------------- properties
def _frame(**cols):
    return AnovosFrame.from_pandas(pd.DataFrame(cols))


def _eta(ctx, idf, cat="c", num="x", method="correlation_ratio"):
    odf = ae.numerical_categorical_association(ctx, idf, [cat, num], method_type=method)
    return float(odf.set_index("attribute").loc[cat, num])


def test_eta_invariant_under_affine_map_and_recoding(ctx):
    rng = np.random.default_rng(9)
    c = rng.choice(["p", "q", "r", "s"], 300, p=[0.4, 0.3, 0.2, 0.1]).astype(object)
    x = rng.normal(0, 1, 300) + (c == "p") * 0.8
    base = _eta(ctx, _frame(c=c, x=x))
    assert 0.1 < base < 0.9
    # powers of two scale exactly; the shift moves every deviation by rounding only
    for alpha, beta in ((4.0, 0.0), (-0.5, 0.0), (2.0, 3.0), (-8.0, 100.0)):
        assert abs(_eta(ctx, _frame(c=c, x=alpha * x + beta)) - base) <= EXACT_TOL, (alpha, beta)
    recoded = np.array([{"p": "Z", "q": "A", "r": "M", "s": "B"}[v] for v in c], dtype=object)
    assert abs(_eta(ctx, _frame(c=recoded, x=x)) - base) <= EXACT_TOL


def test_eta_is_one_when_x_is_a_function_of_the_category(ctx):
    rng = np.random.default_rng(10)
    c = rng.choice(["p", "q", "r"], 200).astype(object)
    x = np.array([{"p": 1.5, "q": -2.25, "r": 7.0}[v] for v in c])
    idf = _frame(c=c, x=x)
    assert abs(_eta(ctx, idf) - 1.0) <= EXACT_TOL
    assert abs(_eta(ctx, idf, method="eta_squared") - 1.0) <= EXACT_TOL
    assert _eta(ctx, idf, method="anova_f") > 1e12  # SSW is rounding only
    # deviations from the global mean (2) that are exact: SSW = 0 < SSB gives +inf
    idf = _frame(c=np.array(["p"] * 100 + ["q"] * 100, dtype=object), x=np.array([1.0] * 100 + [3.0] * 100))
    assert _eta(ctx, idf, method="anova_f") == float("inf")
    assert _eta(ctx, idf) == 1.0


def test_undefined_cases_are_nan(ctx):
    rng = np.random.default_rng(11)
    c = rng.choice(["p", "q", "r"], 200).astype(object)
    x = rng.normal(0, 1, 200)
    for method in ("correlation_ratio", "eta_squared", "anova_f"):
        # a constant x (SST = 0; for F, SSW = SSB = 0) and a constant category (k = 1)
        assert math.isnan(_eta(ctx, _frame(c=c, x=np.full(200, 3.7)), method=method)), method
        assert math.isnan(_eta(ctx, _frame(c=np.array(["only"] * 200, dtype=object), x=x), method=method)), method
        # no pairwise-complete row
        idf = _frame(c=np.array(["a", "b", None, None], dtype=object), x=np.array([np.nan, np.nan, 1.0, 2.0]))
        assert math.isnan(_eta(ctx, idf, method=method)), method
        # a non-finite value among the rows used
        xi = x.copy()
        xi[5] = np.inf
        assert math.isnan(_eta(ctx, _frame(c=c, x=xi), method=method)), method
    # N <= k: every group has one row — F is undefined, eta is 1
    idf = _frame(c=np.array(["a", "b", "c"], dtype=object), x=np.array([1.0, 2.0, 4.0]))
    assert math.isnan(_eta(ctx, idf, method="anova_f"))
    assert abs(_eta(ctx, idf) - 1.0) <= EXACT_TOL
    # an infinity in a row that is not used (null category) does no harm
    cn = c.copy()
    cn[5] = None
    xi = x.copy()
    xi[5] = -np.inf
    assert not math.isnan(_eta(ctx, _frame(c=cn, x=xi)))


def test_nulls_equal_rows_removed(ctx, anova_frame, anova_pdf):
    """Pairwise-complete rows: nulls on the categorical side (b) and on the
    numerical side (x) — the same as dropping those rows first."""
    sub = AnovosFrame.from_pandas(anova_pdf.dropna(subset=["b", "x"]).reset_index(drop=True)[["b", "x"]])
    for method in ("correlation_ratio", "eta_squared", "anova_f"):
        full = _matrix(ae.numerical_categorical_association(ctx, anova_frame, ["b", "x"], method_type=method), ["b"], ["x"])
        cut = _matrix(ae.numerical_categorical_association(ctx, sub, method_type=method), ["b"], ["x"])
        want = cut.loc["b", "x"]
        assert abs(full.loc["b", "x"] - want) <= REF_TOL * max(1.0, abs(want)), method


def test_max_categories_drops_and_warns(ctx, income_frame):
    with pytest.warns(UserWarning, match="ifa"):
        m = ae.numerical_categorical_association(ctx, income_frame, ["ifa", "workclass", "education", "age"],
                                                 max_categories=50)
    assert list(m["attribute"]) == ["education", "workclass"] and list(m.columns) == ["attribute", "age"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = ae.numerical_categorical_association(ctx, income_frame, ["workclass", "education", "age"], max_categories=5)
    assert list(m["attribute"]) == ["education", "workclass"]
    with pytest.warns(UserWarning, match="education"):
        with pytest.raises(TypeError):
            ae.numerical_categorical_association(ctx, income_frame, ["education", "age"], max_categories=4)


def test_invalid_inputs(ctx, income_frame):
    with pytest.raises(TypeError, match="method_type"):
        ae.numerical_categorical_association(ctx, income_frame, method_type="pearson")
    with pytest.raises(TypeError, match="Column"):
        ae.numerical_categorical_association(ctx, income_frame, ["workclass", "no_such_column"])
    with pytest.raises(TypeError, match="Column"):
        ae.numerical_categorical_association(ctx, income_frame, ["workclass", "education"])  # no numerical column
    with pytest.raises(TypeError, match="Column"):
        ae.numerical_categorical_association(ctx, income_frame, ["age", "fnlwgt"])  # no categorical column
    with pytest.raises(TypeError, match="Column"):
        ae.numerical_categorical_association(ctx, income_frame, ["workclass", "age"], drop_cols=["age"])


def test_all_columns_string_arguments_and_no_rounding(ctx, income_frame):
    m = ae.numerical_categorical_association(ctx, income_frame, drop_cols=["ifa"])
    assert list(m.columns) == ["attribute", "age", "fnlwgt", "hours_per_week"]
    assert list(m["attribute"]) == ["education", "income", "workclass"]
    vals = m[["age", "fnlwgt", "hours_per_week"]].to_numpy(dtype=np.float64)
    assert np.isfinite(vals).all() and (vals >= 0).all() and (vals <= 1).all()
    assert not np.array_equal(vals, vals.round(4))  # not rounded
    s = ae.numerical_categorical_association(ctx, income_frame, "workclass|age|fnlwgt", drop_cols="fnlwgt")
    assert list(s.columns) == ["attribute", "age"] and list(s["attribute"]) == ["workclass"]
    assert s.loc[0, "age"] == m.set_index("attribute").loc["workclass", "age"]


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
            "numerical_categorical_association": {"list_of_cols": "all", "drop_cols": ["ifa"],
                                                  "method_type": "eta_squared"},
        },
        "report_preprocessing": {"master_path": str(rep)},
    }
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f, sort_keys=False)
    workflow.run(str(tmp_path / "cfg.yaml"), device="cpu")
    out = pd.read_csv(rep / "numerical_categorical_association.csv")
    assert list(out.columns) == ["attribute", "age", "fnlwgt", "hours_per_week"]
    assert list(out["attribute"]) == ["education", "income", "workclass"]
    vals = out[["age", "fnlwgt", "hours_per_week"]].to_numpy(dtype=np.float64)
    assert np.isfinite(vals).all() and (vals >= 0).all() and (vals <= 1).all()


# ---------------------------------------------------------------------- gpu
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
def test_gpu_equals_cpu(anova_pdf, monkeypatch):
    """Device frame (HIP kernel; column `wide` has more slots than one
    window, `huge` more than KERNEL_MAX_SLOTS — lowered for this test — and
    takes the torch path on the device) against the CPU frame. The sums
    differ in order only: n is exact, mean / M2 and the statistics agree
    at 1e-9 relative."""
    from anovos_amd.ops import grouped
    from anovos_amd.shared.context import AnovosContext

    monkeypatch.setattr(grouped, "KERNEL_MAX_SLOTS", 64)
    rng = np.random.default_rng(33)
    pdf = pd.concat([anova_pdf] * 3, ignore_index=True)
    pdf["wide"] = np.char.add("w", rng.integers(0, 45, len(pdf)).astype(str)).astype(object)
    pdf["huge"] = np.char.add("h", rng.integers(0, 150, len(pdf)).astype(str)).astype(object)
    pdf["x32"] = pdf["x"].astype(np.float32)
    cpu = AnovosFrame.from_pandas(pdf, device="cpu")
    gpu = AnovosFrame.from_pandas(pdf, device="cuda:0")
    cats, nums = ["a", "b", "wide", "huge"], ["x", "y", "z", "x32"]
    mc = grouped_moments(cpu, cats, nums)
    mg = grouped_moments(gpu, cats, nums)
    assert list(mc) == list(mg)
    for k in mc:
        np.testing.assert_array_equal(mg[k][:, 0], mc[k][:, 0])
        np.testing.assert_allclose(mg[k][:, 1], mc[k][:, 1], rtol=REF_TOL, atol=0, equal_nan=True)
        np.testing.assert_allclose(mg[k][:, 2], mc[k][:, 2], rtol=REF_TOL, atol=REF_TOL, equal_nan=True)
    ctx_c, ctx_g = AnovosContext("cpu"), AnovosContext("cuda:0")  # the session's context stays as it is
    for method in ("correlation_ratio", "eta_squared", "anova_f"):
        oc = ae.numerical_categorical_association(ctx_c, cpu, method_type=method, max_categories=10_000)
        og = ae.numerical_categorical_association(ctx_g, gpu, method_type=method, max_categories=10_000)
        assert list(oc.columns) == list(og.columns) and list(oc["attribute"]) == list(og["attribute"])
        names = [c for c in oc.columns if c != "attribute"]
        np.testing.assert_allclose(og[names].to_numpy(dtype=np.float64), oc[names].to_numpy(dtype=np.float64),
                                   rtol=REF_TOL, atol=REF_TOL, equal_nan=True)
