"""The rank contract of ops.histogram.approx_quantiles, taken literally.

The docstring promises "a value whose rank is within rel_err*n of prob*n".
Every test here checks exactly that against a CPU fp64 sort of the column's
non-NaN values — never against the code under test, and with no allowance
for a neighbouring data value. The exact order statistic meets the
contract for every input below, so the contract is always satisfiable;
where a single value holds more rows than the tolerance (a spike), it
forces that value itself.

Sizes: 300 001 rows take the sketch path natively; 70 001 rows with
EXACT_N_THRESHOLD patched to 0 give two chunks with an unaligned boundary
on the GPU. Each (device, size, rel_err) combination is computed once, in
one call over one frame that mixes columns needing no refinement with
columns needing several passes, and shared by the per-column tests."""

import functools

import numpy as np
import pytest
import torch

from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.ops import histogram as hist_ops

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="cuda", marks=[requires_gpu, pytest.mark.gpu])]
SIZES = [300_001, 70_001]
REL_ERRS = [1e-2, 1e-4]
PROBS = [0.0, 0.001, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999, 1.0]
NAN = float("nan")
INF = float("inf")


# ------------------------------------------------------------------ helper
def assert_rank_contract(vs, probs, got, rel_err, what=""):
    """vs: sorted fp64 CPU tensor of the non-NaN values; got[j] answers
    probs[j]. Rank of q within rel_err*n (+1: ceil(p*n) vs p*(n-1) rank
    conventions) of p*n, q inside the data's range, non-decreasing in p."""
    n = vs.numel()
    tol = rel_err * n + 1
    assert len(got) == len(probs), what
    prev = -INF
    for p, q in zip(probs, got):
        assert q == q, (what, p, q)
        qt = torch.tensor(q, dtype=torch.float64)
        below = int(torch.searchsorted(vs, qt, right=False))  # count(vs < q)
        upto = int(torch.searchsorted(vs, qt, right=True))  # count(vs <= q)
        assert below <= p * n + tol, (what, p, q, "count(vs < q)", below, "p*n", p * n, "tol", tol)
        assert upto >= p * n - tol, (what, p, q, "count(vs <= q)", upto, "p*n", p * n, "tol", tol)
        assert float(vs[0]) <= q <= float(vs[-1]), (what, p, q, float(vs[0]), float(vs[-1]))
        assert q >= prev, (what, "not monotone in p", p, q, prev)
        prev = q


def _sorted_valid(x):
    v = x.to(torch.float64)
    return torch.sort(v[~torch.isnan(v)])[0]


# -------------------------------------------------------------------- data
def _plant(x, g, values):
    """Overwrite distinct random positions with the given values."""
    pos = torch.randperm(x.numel(), generator=g)[: len(values)]
    x[pos] = torch.tensor(values, dtype=x.dtype)
    return x


@functools.lru_cache(maxsize=None)
def _columns(n):
    """name -> CPU tensor, f32 unless noted, about 2 % NaN."""
    g = torch.Generator().manual_seed(1009 + n)
    f32, f64 = torch.float32, torch.float64

    def randn(dtype=f32):
        return torch.randn(n, generator=g, dtype=dtype)

    def rand():
        return torch.rand(n, generator=g)

    cols = {
        "normal": randn() * 7 + 3,
        "lognormal": randn().exp() * 10,
        "cap_high": (rand() * 100).clamp(max=80.0),
        "cap_low": (rand() * 100).clamp(min=30.0),
        "few_1e6": _plant(randn(), g, [1e6] * 5),
        "pm_1e9": _plant(randn(), g, [-1e9] * 5 + [1e9] * 5),
        "two_values": torch.where(rand() < 0.5, torch.tensor(0.25), torch.tensor(7.75)),
        "spike90": torch.where(rand() < 0.9, torch.tensor(0.1), rand()),
        "zeros97": torch.where(rand() < 0.97, torch.tensor(0.0), randn() * 5),
        "half_int": torch.randint(0, 20, (n,), generator=g).to(f32) + 0.5,
        "int_5000": torch.randint(0, 5000, (n,), generator=g).to(f32),  # range >= 4096: generic path
        "int_20": torch.randint(0, 20, (n,), generator=g).to(f32),  # dense integral path
        "constant": torch.full((n,), 3.3),
        "f64_1e9": 1e9 + 1e-3 * randn(f64),
        "tiny": 1e-30 * randn(),
    }
    for x in cols.values():
        x[rand() < 0.02] = NAN
    cols["all_nan"] = torch.full((n,), NAN)
    cols["empty"] = torch.empty(0)
    return cols


@functools.lru_cache(maxsize=None)
def _reference(n):
    return {name: _sorted_valid(x) for name, x in _columns(n).items()}


NAMES = list(_columns.__wrapped__(64))
VALUED = [c for c in NAMES if c not in ("all_nan", "empty")]


def _frame(data, device, names=None):
    """A fresh frame (cold caches) over the shared CPU tensors."""
    names = list(data) if names is None else names
    return AnovosFrame({c: Column(c, "float", data[c].to(device)) for c in names}, device=device)


def _sketch(monkeypatch, n):
    if n <= hist_ops.EXACT_N_THRESHOLD:
        monkeypatch.setattr(hist_ops, "EXACT_N_THRESHOLD", 0)


_RESULTS = {}


def _full_call(monkeypatch, device, n, rel_err):
    """approx_quantiles over the whole frame, computed once per combination."""
    _sketch(monkeypatch, n)
    key = (device, n, rel_err)
    if key not in _RESULTS:
        idf = _frame(_columns(n), device)
        _RESULTS[key] = (idf, hist_ops.approx_quantiles(idf, NAMES, PROBS, rel_err=rel_err))
    return _RESULTS[key]


# ---------------------------------------------------------------- contract
@pytest.mark.parametrize("column", VALUED)
@pytest.mark.parametrize("rel_err", REL_ERRS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_rank_contract(monkeypatch, device, n, rel_err, column):
    _, got = _full_call(monkeypatch, device, n, rel_err)
    assert_rank_contract(_reference(n)[column], PROBS, got[column], rel_err, column)


@pytest.mark.parametrize("rel_err", REL_ERRS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_spikes_resolve_to_the_spike_value(monkeypatch, device, n, rel_err):
    """A value that holds more rows than the tolerance is the only answer
    the contract admits for the probabilities inside its rank block."""
    _, got = _full_call(monkeypatch, device, n, rel_err)
    q = {c: dict(zip(PROBS, got[c])) for c in NAMES}
    assert q["cap_high"][0.95] == 80.0 and q["cap_high"][0.99] == 80.0 and q["cap_high"][1.0] == 80.0
    assert q["cap_low"][0.0] == 30.0 and q["cap_low"][0.05] == 30.0 and q["cap_low"][0.25] == 30.0
    assert q["zeros97"][0.05] == 0.0 and q["zeros97"][0.5] == 0.0 and q["zeros97"][0.95] == 0.0
    assert q["two_values"][0.25] == 0.25 and q["two_values"][0.75] == 7.75
    spike = float(torch.tensor(0.1))  # the f32 value
    assert q["spike90"][0.25] == spike and q["spike90"][0.5] == spike and q["spike90"][0.75] == spike
    assert got["constant"] == [float(torch.tensor(3.3))] * len(PROBS)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_all_nan_and_empty_columns_return_nan(monkeypatch, device, n):
    _, got = _full_call(monkeypatch, device, n, 1e-2)
    for c in ("all_nan", "empty"):
        assert len(got[c]) == len(PROBS) and all(v != v for v in got[c]), (c, got[c])


# --------------------------------------------------------------- infinities
@pytest.mark.parametrize("rel_err", REL_ERRS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_infinite_values(monkeypatch, device, n, rel_err):
    """Three +inf and two -inf in N(0,1): no exception, the contract at
    every probability whose exact order statistic is finite, -+inf at
    p = 0 and p = 1, where the order statistic itself is infinite."""
    _sketch(monkeypatch, n)
    g = torch.Generator().manual_seed(77 + n)
    data = {}
    for name, dtype in (("inf32", torch.float32), ("inf64", torch.float64)):
        x = torch.randn(n, generator=g, dtype=dtype)
        x[torch.rand(n, generator=g) < 0.02] = NAN
        data[name] = _plant(x, g, [INF] * 3 + [-INF] * 2)
    got = hist_ops.approx_quantiles(_frame(data, device), list(data), PROBS, rel_err=rel_err)
    for name, x in data.items():
        vs = _sorted_valid(x)
        assert got[name][0] == -INF and got[name][-1] == INF, (name, got[name])
        assert_rank_contract(vs, PROBS[1:-1], got[name][1:-1], rel_err, name)


# -------------------------------------------------------------- consistency
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_second_call_returns_identical_floats(monkeypatch, device, n):
    """The second call is served by the ("q", p) cache; a call with other
    probabilities reuses the ("hist", nbins) cache and must agree with a
    cold frame."""
    idf, first = _full_call(monkeypatch, device, n, 1e-4)
    again = hist_ops.approx_quantiles(idf, NAMES, PROBS, rel_err=1e-4)
    other = [0.1, 0.5, 0.9]
    warm = hist_ops.approx_quantiles(idf, VALUED, other, rel_err=1e-4)
    cold = hist_ops.approx_quantiles(_frame(_columns(n), device), VALUED, other, rel_err=1e-4)
    for c in NAMES:
        assert np.array_equal(np.array(first[c]), np.array(again[c]), equal_nan=True), c
    for c in VALUED:
        assert warm[c] == cold[c], c
        assert warm[c][1] == first[c][PROBS.index(0.5)], c


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("device", DEVICES)
def test_subset_of_probabilities_on_a_fresh_frame(monkeypatch, device, n):
    _, full = _full_call(monkeypatch, device, n, 1e-4)
    sub = [0.05, 0.5, 0.999]
    got = hist_ops.approx_quantiles(_frame(_columns(n), device), VALUED, sub, rel_err=1e-4)
    for c in VALUED:
        assert got[c] == [full[c][PROBS.index(p)] for p in sub], c


# ------------------------------------------------------------- frame level
@pytest.mark.parametrize("device", DEVICES)
def test_outlier_detection_on_capped_and_mostly_zero_columns(ctx, device):
    """The cap is the 95th percentile itself, so no row lies above it; the
    97 %-zeros column has p5 == p95 and is excluded as skewed — what the
    exact path gives below 250 000 rows."""
    from anovos_amd.data_analyzer import quality_checker as qc

    n = SIZES[0]
    idf = _frame(_columns(n), device, ["cap_high", "zeros97", "normal"])
    _, stats = qc.outlier_detection(
        ctx, idf, ["cap_high", "zeros97", "normal"], detection_side="both",
        detection_configs={"pctile_lower": 0.05, "pctile_upper": 0.95, "min_validation": 1},
        treatment=False, print_impact=True,
    )
    stats = stats.set_index("attribute")
    assert int(stats.loc["cap_high", "upper_outliers"]) == 0
    assert int(stats.loc["cap_high", "excluded_due_to_skewness"]) == 0
    assert int(stats.loc["zeros97", "excluded_due_to_skewness"]) == 1
    # the smooth column next to them: 5 % on each side, within the sketch's 1 %
    nn = _reference(n)["normal"].numel()
    for side in ("lower_outliers", "upper_outliers"):
        assert abs(int(stats.loc["normal", side]) - 0.05 * nn) <= 0.01 * nn + 1


# -------------------------------------------------------------- cost guard
class _Calls:
    """Counts pass-1 histogram launches and records the column indices of
    the brackets handed to each refinement pass and each masked min/max
    (every read of a column after pass 1)."""

    def __init__(self, monkeypatch):
        self.hist = 0
        self.refined_cols = []
        real_hist, real_refine = hist_ops.global_histograms, hist_ops._refine_pass
        real_extrema = hist_ops._bracket_extrema

        def hist(*a, **kw):
            self.hist += 1
            return real_hist(*a, **kw)

        def refine(tensors, cols, brackets, *a, **kw):
            self.refined_cols.append(sorted({k[0] for k in brackets}))
            return real_refine(tensors, cols, brackets, *a, **kw)

        def extrema(tensors, brackets):
            self.refined_cols.append(sorted({k[0] for k in brackets}))
            return real_extrema(tensors, brackets)

        monkeypatch.setattr(hist_ops, "global_histograms", hist)
        monkeypatch.setattr(hist_ops, "_refine_pass", refine)
        monkeypatch.setattr(hist_ops, "_bracket_extrema", extrema)


@pytest.mark.parametrize("device", DEVICES)
def test_smooth_columns_cost_one_pass(monkeypatch, device):
    """normal*7+3 needs no refinement at rel_err 1e-2: one pass-1 launch,
    nothing else. lognormal*10 cannot be served by pass 1 alone: the
    2048-bin grid over its range (up to about 1100) puts 3.5 % of the rows
    into the modal bin, above the 1 % tolerance, so it gets exactly one
    refinement pass over its own brackets — and never a read of the column
    next to it. A column that needs several passes changes none of that."""
    n = SIZES[0]
    data = _columns(n)
    calls = _Calls(monkeypatch)
    alone = hist_ops.approx_quantiles(_frame(data, device, ["normal"]), ["normal"], PROBS, rel_err=1e-2)
    assert calls.hist == 1 and calls.refined_cols == []
    calls = _Calls(monkeypatch)
    smooth = ["normal", "lognormal"]
    got = hist_ops.approx_quantiles(_frame(data, device, smooth), smooth, PROBS, rel_err=1e-2)
    assert calls.hist == 1 and calls.refined_cols == [[1]]
    assert got["normal"] == alone["normal"]
    # a column that needs several passes next to them adds no read of theirs
    mixed = ["normal", "pm_1e9", "lognormal"]
    calls = _Calls(monkeypatch)
    got3 = hist_ops.approx_quantiles(_frame(data, device, mixed), mixed, PROBS, rel_err=1e-2)
    assert calls.hist == 1
    assert calls.refined_cols[0] == [1, 2]
    assert all(cols == [1] for cols in calls.refined_cols[1:]), calls.refined_cols
    assert 2 <= len(calls.refined_cols) <= 2 * hist_ops.MAX_REFINE_PASSES
    for c in smooth:
        assert got3[c] == got[c], c
