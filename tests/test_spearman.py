"""correlation_matrix(method="spearman") against scipy.stats.spearmanr.

Spearman's rho is computed as Pearson's r of mid-ranks on a grid of
`rank_cells` cells per column (ops/rank.py). Where every distinct value has
a cell of its own (at most `rank_cells` rows, or at most `rank_cells`
distinct values) the grid ties nothing and the CPU path, which keeps the
grades in fp64, must agree with scipy to rounding (1e-12). Elsewhere rows
inside a cell are tied, and the deviation from scipy depends on the sample,
about 1 / (cells * sqrt(n)) times a small constant.

Measured deviation of the CPU path from scipy on `_frame(n)` (seed 5,
columns normal / skew / rounded / spike / ties14), 1024 cells, largest
entry over all pairs:

    n =   5 000:  2.08e-5      asserted: 4 x = 8.3e-5
    n = 300 000:  4.44e-6      asserted: 4 x = 1.8e-5

and from the null-convention reference (`nulls` column included), held to
the same bounds:

    n =   5 000:  2.17e-5      n = 300 000:  4.44e-6

The factor 4 covers the sample dependence. A measurement above 1e-4 at
1024 cells would mean a wrong grid or wrong mid-ranks, not a tight bound.

GPU against CPU at n = 300 000 (two f32 columns, `nulls` included):

    use_bf16=False: measured 1.15e-5 in one slab and 4.6e-6 in three,
    asserted 4 x the larger = 4.6e-5 (the grades are rounded to f32 and the
    Gram is accumulated in f32 by rocBLAS: 300 000 products of magnitude
    up to 1/4 at 2^-24 relative each);
    use_bf16=True: measured 1.27e-4, asserted the bf16 Gram bound of
    correlation_matrix's docstring, 1e-2.
"""

import numpy as np
import pandas as pd
import pytest
import scipy.stats as ss
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

# 4 x the measured deviations in the module docstring
BOUND = {5000: 4 * 2.08e-5, 300000: 4 * 4.44e-6}
BOUND_GPU_F32 = 4 * 1.15e-5
BOUND_GPU_BF16 = 1e-2


@pytest.fixture(scope="module")
def cpu_ctx():
    from anovos_amd.shared.context import AnovosContext

    return AnovosContext("cpu")


def _frame(n, seed=5, nulls=False):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=n)
    d = {
        "normal": z,
        "skew": np.exp(0.7 * z + 0.7 * rng.normal(size=n)),
        "rounded": (z + rng.normal(size=n)).round(1),
        "spike": np.where(rng.random(n) < 0.6, 0.0, rng.exponential(size=n)),
        "ties14": np.where(rng.random(n) < 0.14, 1.25, z + rng.normal(size=n)),
    }
    if nulls:
        v = z + 0.5 * rng.normal(size=n)
        v[rng.random(n) < 0.1] = np.nan
        d["nulls"] = v
    return pd.DataFrame(d)


def _spearman(ctx, pdf, device="cpu", **kw):
    """(matrix in the frame's column order, frame)"""
    from anovos_amd.core.frame import AnovosFrame
    from anovos_amd.data_analyzer import association_evaluator as ae

    idf = AnovosFrame.from_pandas(pdf, device=device)
    m = ae.correlation_matrix(ctx, idf, method="spearman", **kw)
    assert list(m.columns) == ["attribute"] + sorted(pdf.columns)
    assert list(m["attribute"]) == sorted(pdf.columns)
    m = m.set_index("attribute")
    return m.loc[list(pdf.columns), list(pdf.columns)].to_numpy(dtype=np.float64), idf


def _scipy(pdf):
    if pdf.shape[1] == 2:
        r = ss.spearmanr(pdf.iloc[:, 0], pdf.iloc[:, 1]).statistic
        return np.array([[1.0, r], [r, 1.0]])
    return np.asarray(ss.spearmanr(pdf.to_numpy()).statistic)


def _null_convention_reference(pdf):
    """numpy Pearson of pandas mid-ranks, NaN replaced by the mean rank."""
    r = pdf.rank(method="average")
    r = r.fillna(r.mean())
    return np.corrcoef(r.to_numpy(dtype=np.float64), rowvar=False)


@pytest.mark.parametrize("n", [2, 3, 700, 1024])
def test_exact_small_columns_with_ties(cpu_ctx, n):
    rng = np.random.default_rng(n)
    pdf = pd.DataFrame({
        "few": rng.integers(0, max(2, n // 3), n) + 0.5,      # heavy ties
        "ints": rng.integers(-5, 6, n).astype(np.float64),
        "round": rng.normal(size=n).round(1),
        "cont": rng.normal(size=n),
        "f32": rng.normal(size=n).astype(np.float32),
    })
    if n <= 3:
        # no constant column (scipy gives NaN there): distinct values in
        # different orders, one tie at n = 3
        pdf = pd.DataFrame({"a": [1.0, 2.0, 3.0][:n], "b": [3.5, 1.5, 2.5][:n], "c": [0.1, 0.7, 0.7][:n] if n == 3 else [0.7, 0.1]})
    got, _ = _spearman(cpu_ctx, pdf, rank_cells=1024)
    dev = np.abs(got - _scipy(pdf)).max()
    print(f"n={n}: deviation from scipy {dev:.3e}")
    assert dev <= 1e-12


def test_exact_eight_values_on_the_sketch_path(cpu_ctx):
    """n = 300 000 is past the exact-quantile threshold; eight equiprobable
    values, integral (dense-histogram path) and non-integral (sketch path),
    each get a cell of their own."""
    n = 300_000
    rng = np.random.default_rng(8)
    a = rng.integers(0, 8, n)
    b = (a + rng.integers(0, 4, n)) % 8
    c = rng.integers(0, 8, n)
    pdf = pd.DataFrame({
        "int_a": a.astype(np.float64),
        "frac_b": b * 0.37 + 0.1,
        "frac_c": np.where(c > 3, a, c) * 1.13 - 2.9,
        "int_c32": c.astype(np.float32),
    })
    got, _ = _spearman(cpu_ctx, pdf, rank_cells=1024)
    dev = np.abs(got - _scipy(pdf)).max()
    print(f"eight values: deviation from scipy {dev:.3e}")
    assert dev <= 1e-12


@pytest.mark.parametrize("n", [5000, 300000])
def test_grid_tied_columns_against_scipy(cpu_ctx, n):
    pdf = _frame(n)
    got, _ = _spearman(cpu_ctx, pdf, rank_cells=1024)
    dev = np.abs(got - _scipy(pdf))
    print(f"n={n}: largest deviation from scipy {dev.max():.3e}; per column {dev.max(axis=0)}")
    assert dev.max() <= BOUND[n]


@pytest.mark.parametrize("n", [5000, 300000])
def test_nulls_take_the_mean_rank(cpu_ctx, n):
    pdf = _frame(n, nulls=True)
    got, _ = _spearman(cpu_ctx, pdf, rank_cells=1024)
    dev = np.abs(got - _null_convention_reference(pdf))
    print(f"n={n}: largest deviation from the null-convention reference {dev.max():.3e}")
    assert dev.max() <= BOUND[n]


def test_degenerate_columns(cpu_ctx):
    n = 500
    rng = np.random.default_rng(3)
    x = rng.normal(size=n)
    pdf = pd.DataFrame({"x": x, "const": np.full(n, 4.5), "null": np.full(n, np.nan), "y": x + rng.normal(size=n)})
    got, _ = _spearman(cpu_ctx, pdf)
    np.testing.assert_array_equal(np.diag(got), np.ones(4))
    for c in (1, 2):
        off = np.delete(got[c], c)
        np.testing.assert_array_equal(off, np.zeros(3))
        np.testing.assert_array_equal(np.delete(got[:, c], c), np.zeros(3))
    assert abs(got[0, 3] - ss.spearmanr(pdf["x"], pdf["y"]).statistic) <= 1e-12


def test_zero_rows(cpu_ctx):
    pdf = pd.DataFrame({"a": np.zeros(0), "b": np.zeros(0), "c": np.zeros(0, dtype=np.float32)})
    got, _ = _spearman(cpu_ctx, pdf)
    np.testing.assert_array_equal(got, np.eye(3))


def test_matrix_properties_and_arguments(cpu_ctx):
    from anovos_amd.core.frame import AnovosFrame
    from anovos_amd.data_analyzer import association_evaluator as ae

    pdf = _frame(3000, seed=9, nulls=True)
    idf = AnovosFrame.from_pandas(pdf, device="cpu")
    plain = ae.correlation_matrix(cpu_ctx, idf, use_bf16=False)
    named = ae.correlation_matrix(cpu_ctx, idf, use_bf16=False, method="pearson")
    pd.testing.assert_frame_equal(plain, named, check_exact=True)
    for cells in (2, 7, 1024, 4096):
        m = ae.correlation_matrix(cpu_ctx, idf, method="spearman", rank_cells=cells)
        assert list(m.columns) == list(plain.columns) and list(m["attribute"]) == list(plain["attribute"])
        v = m[list(m["attribute"])].to_numpy(dtype=np.float64)
        np.testing.assert_array_equal(v, v.T)
        assert np.all(v >= -1.0) and np.all(v <= 1.0) and not np.isnan(v).any()
        np.testing.assert_array_equal(np.diag(v), np.ones(len(v)))
    with pytest.raises(TypeError):
        ae.correlation_matrix(cpu_ctx, idf, method="kendall")
    with pytest.raises(TypeError):
        ae.correlation_matrix(cpu_ctx, idf, method=None)
    for bad in (1, 0, -3, 4097, 10.5, "1024", None, True):
        with pytest.raises(TypeError):
            ae.correlation_matrix(cpu_ctx, idf, method="spearman", rank_cells=bad)


def test_second_call_reads_the_grade_cache(cpu_ctx, monkeypatch):
    from anovos_amd.ops import histogram, rank

    pdf = _frame(4000, seed=10, nulls=True)
    first, idf = _spearman(cpu_ctx, pdf, rank_cells=256)
    for c in pdf.columns:
        grid, table = idf.col(c).cache[("grades", 256)]
        assert grid.dtype == np.float64 and np.all(np.diff(grid) > 0) and len(grid) <= 255
        assert len(table) == len(grid) + 1 and np.all(np.abs(table) <= 0.5)  # an empty cell can sit on the end
        assert ("grades", 1024) not in idf.col(c).cache

    def forbidden(*a, **k):
        raise AssertionError("a warm call must not query quantiles or count")

    monkeypatch.setattr(rank, "rank_grid", forbidden)
    monkeypatch.setattr(rank, "grade_counts", forbidden)
    monkeypatch.setattr(histogram, "approx_quantiles", forbidden)
    monkeypatch.setattr(histogram, "_exact_quantiles", forbidden)
    from anovos_amd.data_analyzer import association_evaluator as ae

    m = ae.correlation_matrix(cpu_ctx, idf, method="spearman", rank_cells=256).set_index("attribute")
    second = m.loc[list(pdf.columns), list(pdf.columns)].to_numpy(dtype=np.float64)
    np.testing.assert_array_equal(first, second)


def test_row_slabs_add_up(cpu_ctx, monkeypatch):
    """Three slabs with a partial last one give the one-slab result."""
    from anovos_amd.ops import rank

    pdf = _frame(5000, seed=11, nulls=True)
    whole, _ = _spearman(cpu_ctx, pdf)
    monkeypatch.setattr(rank, "SLAB_BYTES", 2000 * 4 * pdf.shape[1])
    sliced, _ = _spearman(cpu_ctx, pdf)
    assert np.abs(sliced - whole).max() <= 1e-12


def test_grade_tables_are_centred_midranks():
    from anovos_amd.ops import rank

    n = np.array([3, 0, 1, 5, 2])
    t = rank.grade_tables(n, 11)
    assert t.dtype == np.float64
    midrank = np.array([2.0, 3.5, 4.0, 7.0, 10.5])
    np.testing.assert_allclose(t, (midrank - 6.0) / 11.0, rtol=0, atol=1e-16)
    assert abs((n * t).sum()) < 1e-15 and np.all(np.abs(t) < 0.5)
    np.testing.assert_array_equal(rank.grade_tables(np.zeros(4, dtype=np.int64), 0), np.zeros(4))


def test_grid_gets_a_cutoff_below_a_repeated_quantile():
    from anovos_amd.ops import rank

    q = [0.5, 1.25, 1.25, 1.25, float("nan"), 2.0, 3.0, 3.0]
    g32 = rank._grid_from_quantiles(q, torch.float32, 16)
    g64 = rank._grid_from_quantiles(q, torch.float64, 16)
    p32 = [float(np.nextafter(np.float32(v), np.float32(-np.inf))) for v in (1.25, 3.0)]
    p64 = [float(np.nextafter(v, -np.inf)) for v in (1.25, 3.0)]
    np.testing.assert_array_equal(g32, [0.5, p32[0], 1.25, 2.0, p32[1], 3.0])
    np.testing.assert_array_equal(g64, [0.5, p64[0], 1.25, 2.0, p64[1], 3.0])
    assert len(rank._grid_from_quantiles(np.full(7, np.nan), torch.float64, 8)) == 0


# ---------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def gpu_case(cpu_ctx):
    """The n = 300 000 x 6 frame with two f32 columns, and its CPU result:
    computed once, shared by the GPU tests, never modified."""
    pdf = _frame(300_000, nulls=True)
    pdf["skew"] = pdf["skew"].astype(np.float32)
    pdf["spike"] = pdf["spike"].astype(np.float32)
    want, _ = _spearman(cpu_ctx, pdf, rank_cells=1024)
    want.setflags(write=False)
    return pdf, want


@pytest.fixture(scope="module")
def gpu_ctx():
    from anovos_amd.shared.context import AnovosContext

    return AnovosContext("cuda:0")


@requires_gpu
@pytest.mark.gpu
def test_gpu_f32_gram_matches_cpu(gpu_ctx, gpu_case):
    pdf, want = gpu_case
    got, _ = _spearman(gpu_ctx, pdf, device="cuda", rank_cells=1024, use_bf16=False)
    dev = np.abs(got - want).max()
    print(f"GPU f32 Gram against CPU: {dev:.3e}")
    assert dev <= BOUND_GPU_F32
    again, _ = _spearman(gpu_ctx, pdf, device="cuda", rank_cells=1024, use_bf16=False)
    np.testing.assert_array_equal(got, again)


@requires_gpu
@pytest.mark.gpu
def test_gpu_bf16_gram_within_its_bound_and_repeatable(gpu_ctx, gpu_case):
    pdf, want = gpu_case
    got, idf = _spearman(gpu_ctx, pdf, device="cuda", rank_cells=1024)
    dev = np.abs(got - want).max()
    print(f"GPU bf16 Gram against CPU: {dev:.3e}")
    assert dev <= BOUND_GPU_BF16
    np.testing.assert_array_equal(got, got.T)
    from anovos_amd.data_analyzer import association_evaluator as ae

    warm = ae.correlation_matrix(gpu_ctx, idf, method="spearman").set_index("attribute")
    np.testing.assert_array_equal(warm.loc[list(pdf.columns), list(pdf.columns)].to_numpy(), got)
    cold, _ = _spearman(gpu_ctx, pdf, device="cuda", rank_cells=1024)
    np.testing.assert_array_equal(cold, got)


@requires_gpu
@pytest.mark.gpu
def test_gpu_three_slabs_with_a_partial_last_one(gpu_ctx, gpu_case, monkeypatch):
    from anovos_amd.ops import rank

    pdf, want = gpu_case
    k, n = pdf.shape[1], len(pdf)
    rows = 120_000  # 120 000 + 120 000 + 60 000
    monkeypatch.setattr(rank, "SLAB_BYTES", rows * 4 * k)
    assert -(-n // rows) == 3 and n % rows != 0
    got, _ = _spearman(gpu_ctx, pdf, device="cuda", rank_cells=1024, use_bf16=False)
    dev = np.abs(got - want).max()
    print(f"GPU f32 Gram in three slabs against CPU: {dev:.3e}")
    assert dev <= BOUND_GPU_F32
    got16, _ = _spearman(gpu_ctx, pdf, device="cuda", rank_cells=1024)
    assert np.abs(got16 - want).max() <= BOUND_GPU_BF16
