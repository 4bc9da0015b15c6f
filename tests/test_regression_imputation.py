"""imputation_sklearn(method_type="regression", apply_precision="bf16x2"): the
fitted IterativeImputer in chain form (ops/chain.py) and its apply through the
K31 kernel, against sklearn's own transform."""

import os
import pickle
import tempfile

import numpy as np
import pandas as pd
import pytest
import torch
from sklearn.experimental import enable_iterative_imputer  # noqa: F401
from sklearn.impute import IterativeImputer

from anovos_amd.core.frame import AnovosFrame
from anovos_amd.data_analyzer.quality_checker import nullColumns_detection
from anovos_amd.data_transformer import transformers_advanced as TA
from anovos_amd.ops.chain import chain_error_bound, chain_model, chain_replay_fp64
from anovos_amd.shared.context import init_context

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


def _frame(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(1e4, 3e3, n)
    pdf = pd.DataFrame({
        "a": a.astype(np.float32),
        "b": (a * 0.5 + rng.normal(0, 300, n)).astype(np.float32),
        "c": rng.normal(0, 1e3, n).astype(np.float32),
        "d": rng.normal(1e5, 2e3, n) + a,  # float64
        "e": (1e8 + 8 * rng.integers(-400, 400, n)).astype(np.float32),
        "f": (rng.normal(-5e3, 2e3, n) + 0.2 * a).astype(np.float32),
    })
    for c in pdf.columns:
        pdf.loc[rng.choice(n, n * 15 // 100, replace=False), c] = np.nan
    pdf.iloc[7] = np.nan  # an all-null row
    return pdf


def _values(odf, cols):
    return np.column_stack([odf.col(c).data.cpu().numpy().astype(np.float64) for c in cols])


def test_cpu_apply_precision_and_chain_form():
    pdf = _frame(3000, 1)
    ctx, idf, cols = init_context("cpu"), AnovosFrame.from_pandas(pdf, device="cpu"), list(pdf.columns)
    kw = dict(method_type="regression", sample_size=1000, sample_seed=42)
    default = _values(TA.imputation_sklearn(ctx, idf, cols, **kw), cols)
    assert not np.isnan(default).any()
    for value in ("bf16x2", "fp16"):  # the CPU backend keeps the fp64 path; other strings are ignored
        assert np.array_equal(_values(TA.imputation_sklearn(ctx, idf, cols, apply_precision=value, **kw), cols), default)
    X = pdf.to_numpy(dtype=np.float64)
    model = IterativeImputer(max_iter=4, tol=0, random_state=42).fit(X[:1000])  # tol = 0: every round runs
    cm = chain_model(model, X.shape[1])
    assert cm is not None and cm[2].shape[0] == model.n_iter_
    truth = model.transform(X)
    assert np.abs(chain_replay_fp64(X, *cm) - truth).max() <= 1e-9 * np.abs(truth).max()
    # a visiting order drawn per round has no chain form; the apply still runs
    mp = tempfile.mkdtemp(prefix="reg_random_")
    shuffled = IterativeImputer(max_iter=3, tol=0, random_state=0, imputation_order="random").fit(X[:1000])
    assert chain_model(shuffled, X.shape[1]) is None and chain_model(model, X.shape[1] + 1) is None
    with open(os.path.join(mp, "imputation_sklearn.pkl"), "wb") as f:
        pickle.dump(shuffled, f)
    out = TA.imputation_sklearn(ctx, idf, cols, apply_precision="bf16x2", pre_existing_model=True, model_path=mp, **kw)
    old = shuffled.transform(X)  # the frame stores f32: one rounding of each value
    assert (np.abs(_values(out, cols) - old) <= 2.0 ** -23 * np.abs(old) + 1e-9 * np.abs(old).max()).all()


@requires_gpu
@pytest.mark.gpu
def test_gpu_bf16x2_matches_sklearn_transform():
    """20 000 rows x 6 columns, one f64 and one 1e8 off zero, a model loaded from disk:
    within the derived bound of tests/test_chain_impute_kernel.py (run here on sklearn's
    own values) plus one f32 rounding of the stored value; f64 columns: of the centred one."""
    pdf = _frame(20000, 3)
    cols = list(pdf.columns)
    X = pdf.to_numpy(dtype=np.float64)
    mp = tempfile.mkdtemp(prefix="reg_bf16x2_")
    model = IterativeImputer(max_iter=10, tol=0, random_state=42).fit(X[:4000])  # tol = 0: all ten rounds
    with open(os.path.join(mp, "imputation_sklearn.pkl"), "wb") as f:
        pickle.dump(model, f)
    truth = model.transform(X)
    ctx, idf = init_context("cuda"), AnovosFrame.from_pandas(pdf, device="cuda")
    out = TA.imputation_sklearn(ctx, idf, cols, method_type="regression", apply_precision="bf16x2",
                                pre_existing_model=True, model_path=mp)
    got = _values(out, cols)
    miss = np.isnan(X)
    assert np.array_equal(got[~miss], X[~miss])
    s, order, C, beta, lo, hi = chain_model(model, len(cols))
    u, z0 = 2.0 ** -24, np.where(miss, np.nan, X - s)
    # e0: centring in f32 (x - f32(s) is exact near s, the second subtraction rounds); u_c: C as f32
    _, e = chain_error_bound(z0, order, C, beta, lo, hi, 32, e0=u * np.abs(z0), u_c=u)
    # + the stored value's rounding, and 64 fp64 roundings of the reference's own sums
    bound = e + 2 * u * (np.abs(truth) + e) + 2.0 ** -47 * np.abs(truth).max()
    ratio = (np.abs(got - truth) / bound)[miss]
    print(f"regression bf16x2 vs sklearn: max error / bound = {ratio.max():.4f}")
    assert (ratio <= 1).all(), (int((ratio > 1).sum()), float(ratio.max()))
    cfg = {"pre_existing_model": True, "model_path": mp, "apply_precision": "bf16x2"}
    odf, _ = nullColumns_detection(ctx, idf, "all", treatment=True, treatment_method="regression", treatment_configs=cfg)
    assert np.array_equal(_values(odf, cols), got)


@requires_gpu
@pytest.mark.gpu
def test_gpu_peak_memory():
    """2^21 rows x 20 f32 columns: beyond the output clones the bf16x2 apply allocates the
    coefficient image and tables (< 0.2 MB); the fp64 path's stacked rows alone are 335 MB."""
    n, m = 2 ** 21, 20
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.randn(n, 3, device="cuda", generator=g)
    cols = [f"c{j}" for j in range(m)]
    data = {}
    for j, c in enumerate(cols):
        t = base[:, j % 3] * (1 + j) + torch.randn(n, device="cuda", generator=g)
        t[torch.rand(n, device="cuda", generator=g) < 0.05] = float("nan")
        data[c] = t
    sample = np.column_stack([data[c][:4000].cpu().numpy().astype(np.float64) for c in cols])
    mp = tempfile.mkdtemp(prefix="reg_mem_")
    with open(os.path.join(mp, "imputation_sklearn.pkl"), "wb") as f:
        pickle.dump(IterativeImputer(max_iter=3, tol=0, random_state=0).fit(sample), f)
    ctx, idf = init_context("cuda"), AnovosFrame({c: TA.Column(c, "float", data[c]) for c in cols}, "cuda:0")
    del base, data
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = TA.imputation_sklearn(ctx, idf, cols, method_type="regression", apply_precision="bf16x2",
                                pre_existing_model=True, model_path=mp)
    extra = torch.cuda.max_memory_allocated() - before - n * m * 4
    assert not any(bool(torch.isnan(out.col(c).data).any()) for c in cols)
    assert extra < 4 * 2 ** 20, f"{extra / 2 ** 20:.1f} MiB beyond the output clones"
