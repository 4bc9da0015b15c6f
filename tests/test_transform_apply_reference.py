"""The apply half of scaling and outlier treatment against plain float64.

Every kernel on this path has a bit-exact test of its own, but those
compare the kernel with the same formula written in torch. Here the
reference is numpy float64 arithmetic written in this file, which never
calls the code under test, and the code under test is what a user calls:
`ops.elementwise.scale_columns`, the three public scaling functions with
fitted and with pre-existing parameters, and `outlier_detection` with a
hand-written model. Each test runs on the torch path (cpu) and, with
`-m gpu`, on the HIP kernels.

The scaling contract, for a finite x and ref = (float64(x) - a) * b:

    |out - ref| <= 4 * 2**-24 * |ref| + 2**-44 * (|x| + |a|) * |b|

The first term is a few float32 roundings of the result, the second the
rounding of a and of the difference in double (or a two-float split of
a). Double arithmetic rounded once to float32 stays below 0.25 of it.

Lengths: 1, 3, 5, 4 099 (one chunk) and 65 539 (two chunks with an
unaligned boundary). From length 5 on every column holds about 3 % NaN,
one +inf, one -inf and one -0.0.
"""

import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.data_analyzer import quality_checker as qc
from anovos_amd.data_transformer import transformers as T
from anovos_amd.ops import elementwise
from test_quantile_contract import DEVICES, requires_gpu

LENGTHS = [1, 3, 5, 4_099, 65_539]
NAN, INF = float("nan"), float("inf")
# f32 and f64 interleaved
NAMES = ["f64_epoch", "f32_grid", "f64_cents", "f32_year", "f64_bigint", "f32_normal", "f64_normal", "f32_big",
         "f64_tiny"]
SCALERS = ["z_standardization", "IQR_standardization", "normalization"]


# -------------------------------------------------------------------- data
def _raw_columns(n):
    rng = np.random.default_rng(7001 + n)
    f32 = np.float32
    return rng, {
        "f64_epoch": 1.6e9 + rng.normal(0.0, 50.0, n),
        "f64_cents": 1e6 + rng.integers(0, 100_000, n) / 100.0,
        "f64_bigint": rng.integers(2**52, 2**53, n).astype(np.float64),
        "f64_normal": rng.normal(0.0, 1.0, n),
        "f64_tiny": 1e-30 * rng.normal(0.0, 1.0, n),
        "f32_grid": (2**24 + 2 * rng.integers(0, 50, n)).astype(f32),
        "f32_year": (2000 + rng.integers(0, 25, n)).astype(f32),
        "f32_normal": rng.normal(0.0, 1.0, n).astype(f32),
        "f32_big": rng.normal(3e30, 1e29, n).astype(f32),
    }


@functools.lru_cache(maxsize=None)
def _columns(n, infinities=True):
    """name -> read-only numpy column. `infinities=False` leaves out the
    two infinite rows (NaN and -0.0 stay): a column that holds +-inf has
    no finite mean or range to fit."""
    rng, cols = _raw_columns(n)
    for name in sorted(cols):
        x = cols[name]
        if n >= 5:
            k = max(1, round(0.03 * n))
            pos = rng.permutation(n)
            x[pos[:k]] = NAN
            if infinities:
                x[pos[k]] = INF
                x[pos[k + 1]] = -INF
            x[pos[k + 2]] = -0.0
        x.flags.writeable = False
    return cols


def _with_degenerate(cols, n):
    """The columns plus one constant and one all-NaN column."""
    out = dict(cols)
    const = np.full(n, 7.25)
    if n >= 5:
        const[1] = NAN
    out["constant"] = const
    out["all_nan"] = np.full(n, NAN)
    return out


def _frame(cols, device):
    """A fresh frame (cold caches) over copies of the shared columns."""
    return AnovosFrame(
        {c: Column(c, "float" if x.dtype == np.float32 else "double", torch.from_numpy(x.copy()).to(device))
         for c, x in cols.items()},
        device=device,
    )


def _need_kernels(device):
    if device == "cuda":
        from anovos_amd.ops import backend

        assert backend.require_hip() is not None, "HIP extension must be loadable on the GPU box"


# --------------------------------------------------------------- reference
def _finite64(x):
    v = x.astype(np.float64)
    return v[np.isfinite(v)]


def _z_ab(x):
    """(a, b) of z-scoring over the finite values; b = 1 where there is no
    spread to divide by (the direct kernel test still runs then)."""
    f = _finite64(x)
    sd = float(f.std(ddof=1)) if f.size > 1 else NAN
    return float(f.mean()), (1.0 / sd if sd == sd and sd > 0 else 1.0)


def _minmax_ab(x):
    f = _finite64(x)
    lo, hi = float(f.min()), float(f.max())
    return lo, (1.0 / (hi - lo) if hi > lo else 1.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _assert_same_bits(t, x, what):
    got = t.cpu().numpy()
    assert got.dtype == x.dtype and got.shape == x.shape, what
    assert np.array_equal(_bits(got), _bits(x)), what


def _scale_bound(x, a, b):
    """(finite mask, ref, bound) of the contract in the module docstring."""
    xd = x.astype(np.float64)
    fin = np.isfinite(xd)
    ref = (xd[fin] - a) * b
    bound = 4 * 2.0**-24 * np.abs(ref) + 2.0**-44 * (np.abs(xd[fin]) + abs(a)) * abs(b)
    return fin, ref, bound


def _assert_scaled(out, x, a, b, what):
    """float32 output; NaN exactly where x is NaN; +-inf with the sign
    sign(x) * sign(b) where x is infinite; the bound on every finite row."""
    if isinstance(out, torch.Tensor):
        assert out.dtype == torch.float32, what
        out = out.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == x.shape, what
    g = out.astype(np.float64)
    xd = x.astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(xd)), (what, "NaN rows")
    inf = np.isinf(xd)
    assert np.array_equal(g[inf], np.sign(xd[inf]) * np.sign(b) * INF), (what, "infinite rows", g[inf])
    fin, ref, bound = _scale_bound(x, a, b)
    err = np.abs(g[fin] - ref)
    ratio = np.divide(err, bound, out=np.where(err > 0, INF, 0.0), where=bound > 0)
    worst = int(np.argmax(ratio)) if ratio.size else -1
    if worst >= 0:
        print(f"{what}: worst error {err[worst]:.3e} = {ratio[worst]:.3g} of the bound (ref {ref[worst]!r})")
    assert np.all(err <= bound), (what, "worst error/bound", float(ratio[worst]), "got", g[fin][worst],
                                  "ref", ref[worst], "x", xd[fin][worst], "a", a, "b", b)


# ------------------------------------------------- 1. scale_columns direct
PARAM_SETS = {
    "z": _z_ab,
    "minmax": _minmax_ab,
    "z_negated": lambda x: (_z_ab(x)[0], -_z_ab(x)[1]),  # the sign of an infinite row follows b
}


@pytest.mark.parametrize("params", list(PARAM_SETS))
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("device", DEVICES)
def test_scale_columns_against_float64(device, n, params):
    """All nine columns, f32 and f64 interleaved, in one call."""
    _need_kernels(device)
    cols = _columns(n)
    ab = [PARAM_SETS[params](cols[c]) for c in NAMES]
    outs = elementwise.scale_columns(
        [torch.from_numpy(cols[c].copy()).to(device) for c in NAMES], [a for a, _ in ab], [b for _, b in ab]
    )
    assert len(outs) == len(NAMES)
    for c, (a, b), out in zip(NAMES, ab, outs):
        _assert_scaled(out, cols[c], a, b, f"{params} {c} n={n}")


@pytest.mark.parametrize("device", DEVICES)
def test_scale_columns_mixed_lengths_one_call(device):
    """Every column at every length in one call: the launch is sized by
    the longest column and each one must still end at its own length."""
    _need_kernels(device)
    specs = [(c, n) for n in LENGTHS for c in NAMES]
    ab = [_z_ab(_columns(n)[c]) for c, n in specs]
    outs = elementwise.scale_columns(
        [torch.from_numpy(_columns(n)[c].copy()).to(device) for c, n in specs], [a for a, _ in ab], [b for _, b in ab]
    )
    for (c, n), (a, b), out in zip(specs, ab, outs):
        _assert_scaled(out, _columns(n)[c], a, b, f"mixed {c} n={n}")


# ------------------------------------- 2. public functions, fixed parameters
def _fixed_row(fn, x):
    """The model row of one column from numpy float64 over its finite
    values, as a dict, NaN where the column has none."""
    f = _finite64(x)
    if fn == "z_standardization":
        return {"mean": float(f.mean()) if f.size else NAN, "stddev": float(f.std(ddof=1)) if f.size > 1 else NAN}
    if fn == "IQR_standardization":
        q = np.quantile(f, [0.25, 0.5, 0.75]) if f.size else [NAN] * 3
        return {"p25": float(q[0]), "p50": float(q[1]), "p75": float(q[2])}
    return {"min": float(f.min()) if f.size else NAN, "max": float(f.max()) if f.size else NAN}


def _ab_of_row(fn, row):
    """(a, b, excluded) from a model row, by the rules the functions
    document: no spread (to five decimals for z and IQR) or no values."""
    if fn == "z_standardization":
        a, s = row["mean"], row["stddev"]
        spread = s
        excluded = not (s == s) or round(s, 5) == 0.0
    elif fn == "IQR_standardization":
        a, spread = row["p50"], row["p75"] - row["p25"]
        excluded = not (spread == spread) or round(spread, 5) == 0.0
    else:
        a, spread = row["min"], row["max"] - row["min"]
        excluded = not (spread == spread) or spread == 0.0
    return a, (NAN if excluded else 1.0 / spread), excluded


def _write_model(fn, cols, root):
    rows = [{"feature": c, **_fixed_row(fn, x)} for c, x in cols.items()]
    path = os.path.join(root, fn)
    os.makedirs(path, exist_ok=True)
    pd.DataFrame(rows).to_parquet(os.path.join(path, "part-00000.parquet"))
    return {r["feature"]: r for r in rows}


def _call(fn, ctx, idf, **kw):
    f = getattr(T, fn)
    return f(idf, **kw) if fn == "normalization" else f(ctx, idf, **kw)


_FIXED = {}


def _fixed_outputs(ctx, tmp_path_factory, fn, device, n, mode):
    """(columns, model rows, output frame as name -> numpy), once per case."""
    key = (fn, device, n, mode)
    if key not in _FIXED:
        _need_kernels(device)
        cols = _with_degenerate(_columns(n), n)
        root = str(tmp_path_factory.mktemp("fixed_model"))
        rows = _write_model(fn, cols, root)
        with pytest.warns(UserWarning, match="excluded from"):
            odf = _call(fn, ctx, _frame(cols, device), pre_existing_model=True, model_path=root, output_mode=mode)
        _FIXED[key] = (cols, rows, {c: odf.col(c).data.cpu().numpy() for c in odf.columns})
    return _FIXED[key]


@pytest.mark.parametrize("mode", ["replace", "append"])
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("fn", SCALERS)
@pytest.mark.parametrize("device", DEVICES)
def test_scalers_with_fixed_parameters(ctx, tmp_path_factory, device, fn, n, mode):
    """The constant and the all-NaN column are excluded with a warning and
    left untouched, and so is whatever else the model gives no spread
    (every column at n = 1; f64_tiny for z and IQR, whose spread rounds
    to zero at five decimals)."""
    cols, rows, out = _fixed_outputs(ctx, tmp_path_factory, fn, device, n, mode)
    applied = 0
    for c, x in cols.items():
        a, b, excluded = _ab_of_row(fn, rows[c])
        assert excluded == (c in ("constant", "all_nan") or n == 1 or (c == "f64_tiny" and fn != "normalization")), c
        if excluded or mode == "append":  # the input column stays as it was
            assert np.array_equal(_bits(out[c]), _bits(x)) and out[c].dtype == x.dtype, (fn, c, "input changed")
        if excluded:
            assert c + "_scaled" not in out, (fn, c)
            continue
        applied += 1
        _assert_scaled(out[c + "_scaled" if mode == "append" else c], x, a, b, f"{fn} {mode} {c} n={n}")
    assert applied == (0 if n == 1 else len(NAMES) - (fn != "normalization"))
    assert len(out) == len(cols) + (applied if mode == "append" else 0)


# ------------------------------------------- 3. public functions, fitted
def _rel_close(got, want, rel):
    """pytest.approx(want, rel=rel) as the moments tests of test_dist use
    it, and without approx's absolute floor of 1e-12, which would pass
    anything on a column of tiny values."""
    if want != want:
        return got != got
    return got == pytest.approx(want, rel=rel) and abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("fn", SCALERS)
@pytest.mark.parametrize("device", DEVICES)
def test_scalers_fitted(ctx, tmp_path, device, fn, n):
    """Fitted on the columns without their infinite rows. Mean within
    rel 1e-12 and stddev within rel 1e-3, the tolerances of the offset
    moments test in test_dist (the mean's taken against max(|mean|,
    stddev): a mean near zero has no relative accuracy to ask for);
    min and max exact. The outputs follow the saved parameters within the
    scaling bound, and applying the saved model gives the same bits."""
    _need_kernels(device)
    cols = _with_degenerate(_columns(n, infinities=False), n)
    root = str(tmp_path)
    with pytest.warns(UserWarning, match="excluded from"):
        fit = _call(fn, ctx, _frame(cols, device), model_path=root)
    saved = pd.read_parquet(os.path.join(root, fn, "part-00000.parquet"))
    assert list(saved["feature"]) == list(cols)
    rows = {r["feature"]: r for r in saved.to_dict("records")}
    for c, x in cols.items():
        want, got = _fixed_row(fn, x), rows[c]
        if fn == "z_standardization":
            sd = want["stddev"]
            scale = max(abs(want["mean"]), sd if sd == sd else 0.0)
            assert (got["mean"] != got["mean"]) if want["mean"] != want["mean"] else (
                got["mean"] == pytest.approx(want["mean"], rel=1e-12) and abs(got["mean"] - want["mean"]) <= 1e-12 * scale
            ), (c, got["mean"], want["mean"])
            assert _rel_close(got["stddev"], sd, 1e-3), (c, got["stddev"], sd)
        elif fn == "normalization":
            for k in ("min", "max"):
                assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (c, k, got[k], want[k])
    with pytest.warns(UserWarning, match="excluded from"):
        again = _call(fn, ctx, _frame(cols, device), pre_existing_model=True, model_path=root)
    assert fit.columns == again.columns == list(cols)
    for c, x in cols.items():
        a, b, excluded = _ab_of_row(fn, rows[c])
        if excluded:
            _assert_same_bits(fit.col(c).data, x, (fn, c, "excluded column changed"))
        else:
            _assert_scaled(fit.col(c).data, x, a, b, f"{fn} fitted {c} n={n}")
        assert fit.col(c).data.dtype == again.col(c).data.dtype
        _assert_same_bits(again.col(c).data, fit.col(c).data.cpu().numpy(), (fn, c, "saved model applies differently"))
    if n > 1:
        assert not _ab_of_row(fn, rows["f64_epoch"])[2] and not _ab_of_row(fn, rows["f32_year"])[2]


# ----------------------------------------------------------- 4. min-max range
def _assert_unit_range(out, x, what):
    g = out.astype(np.float64)
    xd = x.astype(np.float64)
    fin = np.isfinite(xd)
    assert np.array_equal(np.isfinite(g), fin), what
    lo, hi = xd[fin].min(), xd[fin].max()
    assert hi > lo, what
    assert g[fin].min() >= 0.0 and g[fin].max() <= 1.0, (what, g[fin].min(), g[fin].max())
    assert np.all(g[xd == lo] == 0.0), (what, "minimum row", g[xd == lo])
    assert np.all(g[xd == hi] == 1.0), (what, "maximum row", g[xd == hi])


@pytest.mark.parametrize("n", LENGTHS[1:])
@pytest.mark.parametrize("device", DEVICES)
def test_normalization_range_fixed_model(ctx, tmp_path_factory, device, n):
    """With the finite minimum and maximum as the model, infinite rows
    present: every finite output in [0, 1], the minimum row exactly 0.0
    and the maximum row exactly 1.0. (At n = 1 there is no range.)"""
    cols, _, out = _fixed_outputs(ctx, tmp_path_factory, "normalization", device, n, "replace")
    for c in NAMES:
        _assert_unit_range(out[c], cols[c], f"normalization {c} n={n}")


@pytest.mark.parametrize("n", LENGTHS[1:])
@pytest.mark.parametrize("device", DEVICES)
def test_normalization_range_fitted(device, n):
    """The same with minimum and maximum fitted by the moments pass."""
    _need_kernels(device)
    cols = _columns(n, infinities=False)
    odf = T.normalization(_frame(cols, device))
    for c in NAMES:
        _assert_unit_range(odf.col(c).data.cpu().numpy(), cols[c], f"fitted normalization {c} n={n}")


# ------------------------------------------------------ 5. outlier bounds
BOUNDS = {"a": (-1.1, 1234567.89), "b": (16777217.0, 3.5e38)}  # none of them a float32
OUTLIER_COLS = [("a", np.float32), ("a", np.float64), ("b", np.float32), ("b", np.float64)]
SIDES = ["lower", "upper", "both"]
TREATMENTS = ["value_replacement", "null_replacement", "row_removal", "detect_only"]


def _oname(pair, dt):
    return f"{pair}_{np.dtype(dt).name}"


@functools.lru_cache(maxsize=None)
def _outlier_column(pair, dt, n):
    """Around each bound: the bound rounded to the dtype and its two
    neighbours in the dtype; for float64 also float32(bound) and its two
    float64 neighbours. Then NaN and +-inf, then ordinary values on both
    sides of both bounds. A length too short for all of them takes the
    first n, the two bounds alternating."""
    rng = np.random.default_rng(9001 + n + 17 * len(pair + np.dtype(dt).name))
    groups = []
    with np.errstate(over="ignore"):
        for bound in BOUNDS[pair]:
            r = dt(bound)
            g = [r, np.nextafter(r, dt(-INF)), np.nextafter(r, dt(INF))]
            if dt is np.float64:
                r32 = np.float64(np.float32(bound))
                g += [r32, np.nextafter(r32, -INF), np.nextafter(r32, INF)]
            groups.append(g)
    special = [v for both in zip(*groups) for v in both] + [NAN, INF, -INF]
    if n <= len(special):
        x = np.array(special[:n], dtype=dt)
    else:
        if pair == "a":
            x = rng.normal(0.0, 1e6, n)
        else:
            x = np.where(rng.random(n) < 0.5, 16777217.0 + rng.integers(-40, 41, n), rng.uniform(1e30, 3.3e38, n))
        x = x.astype(dt)
        x[rng.permutation(n)[: len(special)]] = np.array(special, dtype=dt)
    x.flags.writeable = False
    return x


def _outlier_flags(pair, dt, n, side):
    """The reference verdicts: float64(x) < lo, float64(x) > hi."""
    lo, hi = BOUNDS[pair]
    xd = _outlier_column(pair, dt, n).astype(np.float64)
    with np.errstate(invalid="ignore"):
        lower = (xd < lo) if side in ("lower", "both") else np.zeros(n, dtype=bool)
        upper = (xd > hi) if side in ("upper", "both") else np.zeros(n, dtype=bool)
    return lower, upper


def _outlier_frame(n, device):
    cols = {_oname(p, dt): _outlier_column(p, dt, n) for p, dt in OUTLIER_COLS}
    cols["rowid"] = np.arange(n, dtype=np.float64)  # not in the model: passes through
    return _frame(cols, device)


def _outlier_model(root):
    path = os.path.join(root, "outlier_numcols")
    os.makedirs(path, exist_ok=True)
    pd.DataFrame(
        {"attribute": [_oname(p, dt) for p, dt in OUTLIER_COLS],
         "parameters": [[str(v) for v in BOUNDS[p]] for p, _ in OUTLIER_COLS]}
    ).to_parquet(os.path.join(path, "part-00000.parquet"))


def _run_outliers(ctx, root, device, n, side, treatment):
    kw = dict(treatment=True, treatment_method=treatment)
    if treatment == "detect_only":
        kw = dict(treatment=False, print_impact=True)
    return qc.outlier_detection(
        ctx, _outlier_frame(n, device), [_oname(p, dt) for p, dt in OUTLIER_COLS], detection_side=side,
        pre_existing_model=True, model_path=root, **kw,
    )


def _count_table(stats):
    return {r["attribute"]: (int(r["lower_outliers"]), int(r["upper_outliers"]), int(r["excluded_due_to_skewness"]))
            for r in stats.to_dict("records")}


def test_outlier_fixture_straddles_the_bounds():
    """The columns tell the three comparisons apart: the float64 verdict
    differs from the verdict against the bound rounded to float32, and, on
    float32 columns, from the verdict of a float32 comparison."""
    for pair, dt in OUTLIER_COLS:
        lo, hi = BOUNDS[pair]
        x = _outlier_column(pair, dt, LENGTHS[-1])
        lower, upper = _outlier_flags(pair, dt, LENGTHS[-1], "both")
        with np.errstate(invalid="ignore", over="ignore"):
            rounded = x.astype(np.float64) < float(np.float32(lo))
            assert int(lower.sum()) != int(rounded.sum()), (pair, dt)
            if dt is np.float64 and pair == "a":
                assert int(upper.sum()) != int((x > float(np.float32(hi))).sum())
        assert 0 < lower.sum() < x.size and 0 < upper.sum() < x.size


@pytest.mark.parametrize("treatment", TREATMENTS)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("device", DEVICES)
def test_outlier_bounds_against_float64(ctx, tmp_path, capsys, device, n, side, treatment):
    """Counts equal the float64 reference exactly; value_replacement puts
    the bound rounded to the column's dtype at exactly the flagged rows
    and leaves every other row bit-identical; null_replacement puts NaN
    there; row_removal keeps exactly the rows no column flags. On the GPU
    the replacements and the count-only run take the fused kernel,
    row_removal the torch path."""
    _need_kernels(device)
    root = str(tmp_path)
    _outlier_model(root)
    odf, stats = _run_outliers(ctx, root, device, n, side, treatment)
    flags = {_oname(p, dt): _outlier_flags(p, dt, n, side) for p, dt in OUTLIER_COLS}
    want = {c: (int(lo.sum()), int(hi.sum()), 0) for c, (lo, hi) in flags.items()}
    assert _count_table(stats) == want
    if treatment == "detect_only":
        printed = capsys.readouterr().out
        assert all(c in printed for c in want), printed
    keep = np.ones(n, dtype=bool)
    for lower, upper in flags.values():
        keep &= ~(lower | upper)
    assert odf.columns == [_oname(p, dt) for p, dt in OUTLIER_COLS] + ["rowid"]
    for pair, dt in OUTLIER_COLS:
        c = _oname(pair, dt)
        x = _outlier_column(pair, dt, n)
        lower, upper = flags[c]
        expect = x.copy()
        if treatment == "row_removal":
            expect = expect[keep]
        elif treatment != "detect_only":
            with np.errstate(over="ignore"):
                lo_v, hi_v = (dt(v) for v in BOUNDS[pair]) if treatment == "value_replacement" else (dt(NAN), dt(NAN))
            expect[lower] = lo_v
            expect[upper] = hi_v
        got = odf.col(c).data.cpu().numpy()
        assert got.dtype == x.dtype and got.shape == expect.shape, (c, got.shape, expect.shape)
        if treatment == "null_replacement":
            flagged = lower | upper
            assert np.all(np.isnan(got[flagged])), c
            assert np.array_equal(_bits(got[~flagged]), _bits(x[~flagged])), c
        else:
            bad = np.nonzero(_bits(got) != _bits(expect))[0]
            assert bad.size == 0, (c, "rows", bad[:5], got[bad[:5]], expect[bad[:5]])
    rowid = np.arange(n, dtype=np.float64)
    _assert_same_bits(odf.col("rowid").data, rowid[keep] if treatment == "row_removal" else rowid, "rowid")


# ------------------------------------------------- 6. cross-device agreement
@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_outlier_counts_agree_across_devices(ctx, tmp_path, capsys, n):
    root = str(tmp_path)
    _outlier_model(root)
    for side in SIDES:
        for treatment in TREATMENTS:
            cpu = _count_table(_run_outliers(ctx, root, "cpu", n, side, treatment)[1])
            gpu = _count_table(_run_outliers(ctx, root, "cuda", n, side, treatment)[1])
            assert cpu == gpu, (side, treatment)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS[1:])
@pytest.mark.parametrize("fn", SCALERS)
def test_scaled_outputs_agree_across_devices(ctx, tmp_path_factory, fn, n):
    """Both sides lie within the bound of the float64 reference, so they
    differ by no more than twice the bound."""
    cols, rows, cpu = _fixed_outputs(ctx, tmp_path_factory, fn, "cpu", n, "replace")
    _, _, gpu = _fixed_outputs(ctx, tmp_path_factory, fn, "cuda", n, "replace")
    assert list(cpu) == list(gpu)
    for c, x in cols.items():
        a, b, excluded = _ab_of_row(fn, rows[c])
        if excluded:
            assert np.array_equal(_bits(cpu[c]), _bits(gpu[c])), c
            continue
        fin, _, bound = _scale_bound(x, a, b)
        assert np.array_equal(cpu[c][~fin], gpu[c][~fin], equal_nan=True), c
        diff = np.abs(cpu[c][fin].astype(np.float64) - gpu[c][fin].astype(np.float64))
        print(f"{fn} {c} n={n}: largest cpu/gpu difference {diff.max():.3e}")
        assert np.all(diff <= 2 * bound), (fn, c, float((diff / np.maximum(bound, 1e-300)).max()))
