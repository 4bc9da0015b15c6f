"""Bin counts emitted by the binning kernel and their reuse by the drift
frequency pass; reuse of the cached dense integer histogram by
approx_quantiles.

CPU tests compare the cached-count path of batched_bin_frequencies with
the histogram path (forced by clearing the stats cache) — results must be
identical. GPU tests compare the counting kernel with the plain one
(bit-identical outputs) and its counts with torch.bincount of the labels
it produced; counts are integers and placement is deterministic, so every
comparison is exact."""

import numpy as np
import pandas as pd
import pytest
import torch

from anovos_amd.core.frame import AnovosFrame
from anovos_amd.data_transformer import transformers as T
from anovos_amd.drift_stability import drift_detector as dd
from anovos_amd.ops import histogram as hist_ops

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

KEY = ("bincounts",)


# ---------------------------------------------------------------- CPU ----
def _frame(n=997, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 3, n)
    a[rng.choice(n, 37, replace=False)] = np.nan
    b = rng.integers(0, 50, n).astype("float64")
    c = rng.exponential(2.0, n)
    c[:5] = np.nan
    const = np.full(n, 4.25)
    return AnovosFrame.from_pandas(pd.DataFrame({"a": a, "b": b, "c": c, "const": const}))


class _HistCalls:
    def __init__(self, monkeypatch):
        self.n = 0
        real = hist_ops.global_histograms

        def counted(*args, **kw):
            self.n += 1
            return real(*args, **kw)

        monkeypatch.setattr(hist_ops, "global_histograms", counted)


def _cached_then_histogram(binned, cols, total, max_bin, calls):
    """(cached-path result, histogram-path result); checks which path ran."""
    assert all(KEY in binned.col(c).cache for c in cols)
    before = calls.n
    cached = dd.batched_bin_frequencies(binned, cols, total, max_bin=max_bin)
    assert calls.n == before, "cached counts must not launch a histogram"
    binned.clear_stats_cache()
    plain = dd.batched_bin_frequencies(binned, cols, total, max_bin=max_bin)
    assert calls.n == before + 1
    return cached, plain


@pytest.mark.parametrize("max_bin", [10, 0])
def test_cached_counts_match_histogram_path(ctx, monkeypatch, max_bin):
    idf = _frame()
    calls = _HistCalls(monkeypatch)
    binned = T.attribute_binning(ctx, idf, ["a", "b", "c", "const"], bin_size=10, output_mode="append")
    cols = [c + "_binned" for c in ["a", "b", "c", "const"]]
    cached, plain = _cached_then_histogram(binned, cols, idf.count(), max_bin, calls)
    assert cached == plain
    # the constant column (all cutoffs equal) lands in one bin; nulls keyed -1
    assert cached["const_binned"] == (["1"], [1.0])
    assert cached["a_binned"][0][0] == "-1"
    assert cached["a_binned"][1][0] == 37 / idf.count()


def test_cached_counts_survive_replace_mode(ctx, monkeypatch):
    idf = _frame()
    calls = _HistCalls(monkeypatch)
    binned = T.attribute_binning(ctx, idf, ["a", "c"], bin_size=10)  # output_mode="replace"
    cached, plain = _cached_then_histogram(binned, ["a", "c"], idf.count(), 10, calls)
    assert cached == plain


@pytest.mark.parametrize("max_bin", [10, 0])
def test_cached_counts_fold_longer_model_and_all_null(ctx, monkeypatch, tmp_path, max_bin):
    """A pre-existing model with 19 cutoffs read with max_bin=10: labels
    11..20 fold into the edge bin, as the histogram path clamps them. The
    same model applied to an all-null column gives only the null key."""
    src = _frame()
    T.attribute_binning(ctx, src, ["a", "c"], bin_size=20, model_path=str(tmp_path), output_mode="append")
    n = src.count()
    tgt = AnovosFrame.from_pandas(pd.DataFrame({
        "a": src.col("a").data.numpy().astype("float64"),
        "c": np.full(n, np.nan),  # all-null target column
    }))
    calls = _HistCalls(monkeypatch)
    binned = T.attribute_binning(ctx, tgt, ["a", "c"], bin_size=10, pre_existing_model=True,
                                 model_path=str(tmp_path), output_mode="append")
    assert float(torch.nan_to_num(binned.col("a_binned").data, nan=0.0).max()) > 10
    cached, plain = _cached_then_histogram(binned, ["a_binned", "c_binned"], n, max_bin, calls)
    assert cached == plain
    assert cached["c_binned"] == (["-1"], [1.0])
    if max_bin:
        assert max(int(k) for k in cached["a_binned"][0]) == 10
    else:
        assert max(int(k) for k in cached["a_binned"][0]) == 20


def test_one_column_without_counts_falls_back_for_all(ctx, monkeypatch):
    idf = _frame()
    calls = _HistCalls(monkeypatch)
    binned = T.attribute_binning(ctx, idf, ["a", "b", "c"], bin_size=10, output_mode="append")
    cols = ["a_binned", "b_binned", "c_binned"]
    del binned.col("b_binned").cache[KEY]
    mixed = dd.batched_bin_frequencies(binned, cols, idf.count(), max_bin=10)
    assert calls.n == 1, "a column without counts sends every column through the histogram"
    binned.clear_stats_cache()
    plain = dd.batched_bin_frequencies(binned, cols, idf.count(), max_bin=10)
    assert mixed == plain


def test_single_column_frequencies_use_cached_counts(ctx):
    idf = _frame()
    binned = T.attribute_binning(ctx, idf, ["a", "const"], bin_size=10, output_mode="append")
    cached = {c: dd._bin_frequencies(binned, c, idf.count()) for c in ["a_binned", "const_binned"]}
    binned.clear_stats_cache()
    plain = {c: dd._bin_frequencies(binned, c, idf.count()) for c in ["a_binned", "const_binned"]}
    assert cached == plain


def test_counts_wrapper_torch_fallback():
    from anovos_amd.ops import bucketize as bk

    x = torch.tensor([float("nan"), -1.0, 0.0, 0.5, 1.0, 7.0, float("inf")])
    y = torch.tensor([2.0, float("nan")], dtype=torch.float64)
    outs, counts = bk.bucketize_columns_float_counts(
        [x, y], [torch.tensor([0.0, 1.0], dtype=torch.float64), torch.empty(0, dtype=torch.float64)]
    )
    ref = bk.bucketize_columns_float([x, y], [torch.tensor([0.0, 1.0]), torch.empty(0)])
    for o, r in zip(outs, ref):
        assert torch.equal(o.view(torch.int32), r.view(torch.int32))
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (2, 4)
    assert counts.tolist() == [[1, 2, 2, 2], [1, 1, 0, 0]]


def test_integer_quantiles_reuse_dense_histogram(monkeypatch):
    """A second probability list on bounded integer columns returns what a
    cold cache returns, without another histogram over those columns."""
    monkeypatch.setattr(hist_ops, "EXACT_N_THRESHOLD", 100)  # take the sketch path at test size
    rng = np.random.default_rng(11)
    n = 5000
    pdf = pd.DataFrame({
        "i1": rng.integers(-3, 40, n).astype("float64"),
        "i2": rng.poisson(6.0, n).astype("float64"),
    })
    pdf.loc[:17, "i2"] = np.nan
    cols = ["i1", "i2"]
    p1 = [0.01, 0.25, 0.5, 0.75, 0.99]
    p2 = [j / 10 for j in range(1, 10)]

    cold1 = hist_ops.approx_quantiles(AnovosFrame.from_pandas(pdf), cols, p1)
    cold2 = hist_ops.approx_quantiles(AnovosFrame.from_pandas(pdf), cols, p2)

    idf = AnovosFrame.from_pandas(pdf)
    calls = _HistCalls(monkeypatch)
    warm1 = hist_ops.approx_quantiles(idf, cols, p1)
    assert calls.n == 1
    assert all(("inthist",) in idf.col(c).cache for c in cols)
    warm2 = hist_ops.approx_quantiles(idf, cols, p2)
    assert calls.n == 1, "cached dense counts must serve the second probability list"
    assert warm1 == cold1
    assert warm2 == cold2


# ---------------------------------------------------------------- GPU ----
@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


# 1, 3: below one vector; 2047/2053: around one two-vector trip of 256
# threads (2 * 256 * 4 = 2048); 65 539: first length with two chunks (chunk
# boundary 32 770 is no multiple of 4); 300 001: several chunks plus a tail
LENGTHS = [1, 3, 2047, 2053, 65_536 + 3, 300_001]


@pytest.fixture(scope="module")
def gpu_inputs():
    g = torch.Generator().manual_seed(17)
    cols = []
    for n in LENGTHS:
        x = torch.randn(n, generator=g) * 2.0
        x[torch.rand(n, generator=g) < 0.03] = float("nan")
        cols.append(x)
    cols.append(torch.randn(70_001, generator=g).double() * 2.0)  # f64 column
    cols[-1][::13] = float("nan")
    return [c.cuda() for c in cols]


def _cuts(ncut):
    # strictly increasing over the data's range; exact f32 values so some
    # data points can be made to sit exactly on a cutoff
    return torch.linspace(-3.0, 3.0, ncut, dtype=torch.float64) if ncut else torch.empty(0, dtype=torch.float64)


def _check(ext, cols, cuts):
    outs, counts = ext.bucketize_columns_float_counts(cols, cuts)
    ref = ext.bucketize_columns_float(cols, cuts)
    stride = max(int(c.numel()) for c in cuts) + 2
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (len(cols), stride)
    counts = counts.cpu()
    for i, (o, r) in enumerate(zip(outs, ref)):
        o, r = o.cpu(), r.cpu()
        assert o.dtype == torch.float32 and o.shape == cols[i].shape
        # bit-identical, NaN positions included
        assert torch.equal(o.view(torch.int32), r.view(torch.int32)), f"column {i}"
        want = torch.bincount(torch.nan_to_num(o, nan=0.0).to(torch.long), minlength=stride)
        assert torch.equal(counts[i], want), f"column {i}: {counts[i].tolist()} vs {want.tolist()}"
        assert int(counts[i, 0]) == int(torch.isnan(cols[i]).sum())
        assert int(counts[i, cuts[i].numel() + 2:].sum()) == 0
    return outs, counts


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("ncut", [0, 1, 9, 16, 17, 33])
def test_counts_kernel_lengths_dtypes_cutoff_counts(ext, gpu_inputs, ncut):
    """All lengths and the f64 column in one call. ncut <= 15 runs the
    private counters, 16..32 the shared atomics with the linear scan, 33
    the shared atomics with the binary search."""
    _check(ext, gpu_inputs, [_cuts(ncut) for _ in gpu_inputs])


@requires_gpu
@pytest.mark.gpu
def test_counts_kernel_mixed_cutoff_counts_in_one_call(ext, gpu_inputs):
    ncuts = [0, 1, 9, 16, 17, 33, 9]
    _check(ext, gpu_inputs, [_cuts(k) for k in ncuts])
    # every column within the private-counter limit, different lengths
    _check(ext, gpu_inputs, [_cuts(k) for k in [9, 0, 15, 1, 9, 3, 15]])


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 20])
def test_counts_kernel_special_values(ext, pad):
    """Values on a cutoff, +-inf, duplicated cutoffs, a NaN cutoff, an
    all-NaN column; pad > 0 repeats it on the shared-atomics path."""
    inf = float("inf")
    base = [0.0, 0.5, 0.5, 1.0, 2.0]
    cuts = torch.tensor(base + [2.0 + 0.25 * (k + 1) for k in range(pad)], dtype=torch.float64)
    nan_cuts = cuts.clone()
    nan_cuts[1] = float("nan")
    g = torch.Generator().manual_seed(23)
    vals = torch.tensor([0.0, 0.5, 1.0, 2.0, -inf, inf, float("nan"), -0.0, 0.25, 0.75, 1e30, -1e30,
                         float(np.nextafter(np.float32(0.5), np.float32(1.0))),
                         float(np.nextafter(np.float32(0.5), np.float32(0.0)))])
    x = torch.cat([vals, torch.rand(3001, generator=g) * 3 - 0.5, vals])
    allnan = torch.full((2051,), float("nan"))
    cols = [x.cuda(), x.double().cuda(), allnan.cuda(), x.cuda()]
    outs, counts = _check(ext, cols, [cuts, cuts, cuts, nan_cuts])
    assert counts[2].tolist() == [2051] + [0] * (cuts.numel() + 1)
    # right-closed bins: a value equal to a cutoff stays at or below it
    o = outs[0].cpu()
    assert o[0] == 1.0 and o[1] == 2.0 and o[2] == 4.0 and o[3] == 5.0
    assert o[4] == 1.0 and o[5] == float(cuts.numel() + 1) and torch.isnan(o[6])
    # the f64 pass places the same values the same way
    assert torch.equal(outs[1].cpu().view(torch.int32), o.view(torch.int32))


@pytest.fixture(scope="module")
def label_inputs():
    # 4096: whole vectors, no tail; 4099: vector tail; 65 539: two chunks
    # with an unaligned boundary; 300 001: several chunks plus a tail.
    # Integer-valued data, so many values sit exactly on a cutoff.
    g = torch.Generator().manual_seed(31)
    out = {}
    for n in [4096, 4099, 65_536 + 3, 300_001]:
        cols = []
        for _ in range(3):
            x = torch.randint(-2, 20, (n,), generator=g).float() * 0.5
            x[torch.rand(n, generator=g) < 0.02] = float("nan")
            cols.append(x.cuda())
        lab = (torch.rand(n, generator=g) < 0.3).to(torch.uint8).cuda()
        out[n] = (cols, lab)
    return out


def _short_cuts(k, dup=False, nan=False):
    c = torch.arange(k, dtype=torch.float64) * 0.5
    if dup and k >= 3:
        c[2] = c[1]
    if nan and k >= 4:
        c[3] = float("nan")
    return c


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 4099, 65_536 + 3, 300_001])
@pytest.mark.parametrize("ncuts", [(9, 4, 0), (13, 9, 12), (16, 10, 1)])
def test_label_counts_register_cutoffs_match_lds_scan(ext, label_inputs, n, ncuts):
    """Launches whose longest cutoff list has <= 9 / <= 16 entries keep
    the cutoffs in registers. Padding every list to 17 entries with +inf
    (a cutoff no value exceeds) sends the same columns through the LDS
    scan; counts must be equal. (9,4,0) -> 9 registers, (13,9,12) -> 16
    registers with private counters, (16,10,1) -> 16 with shared atomics."""
    cols, lab = label_inputs[n]
    cuts = [_short_cuts(k, dup=(i == 1), nan=(i == 2)) for i, k in enumerate(ncuts)]
    sizes = [k + 3 for k in ncuts]
    padded = [torch.cat([c, torch.full((17 - c.numel(),), float("inf"), dtype=torch.float64)]) for c in cuts]
    got = ext.bucketize_label_counts(cols, cuts, lab, sizes).cpu()
    want = ext.bucketize_label_counts(cols, padded, lab, sizes).cpu()
    assert torch.equal(got, want)
    # and against torch: slot 0 nulls, bin b -> slot b + 1
    from anovos_amd.ops import bucketize as bk

    off = 0
    for x, c, sz in zip(cols, cuts, sizes):
        if bool(torch.isnan(c).any()):  # torch.bucketize needs sorted boundaries
            off += 2 * sz
            continue
        lbl = bk.bucketize_columns_float([x.cpu()], [c])[0]
        slot = torch.where(torch.isnan(lbl), torch.zeros_like(lbl), lbl + 1).to(torch.long)
        tot = torch.bincount(slot, minlength=sz)
        evt = torch.bincount(slot[lab.cpu() != 0], minlength=sz)
        assert torch.equal(got[off:off + sz], tot) and torch.equal(got[off + sz:off + 2 * sz], evt)
        off += 2 * sz


@requires_gpu
@pytest.mark.gpu
def test_binning_then_frequencies_on_gpu_match_histogram_path(ctx):
    g = torch.Generator().manual_seed(29)
    n = 70_003
    pdf = pd.DataFrame({
        "a": (torch.randn(n, generator=g) * 5).numpy(),
        "b": torch.randint(0, 30, (n,), generator=g).float().numpy(),
    })
    pdf.loc[::17, "a"] = np.nan
    idf = AnovosFrame.from_pandas(pdf, device="cuda:0")
    binned = T.attribute_binning(ctx, idf, ["a", "b"], bin_size=10, output_mode="append")
    cols = ["a_binned", "b_binned"]
    assert all(binned.col(c).cache[KEY].is_cuda for c in cols)
    cached = dd.batched_bin_frequencies(binned, cols, n, max_bin=10)
    cached0 = dd.batched_bin_frequencies(binned, cols, n, max_bin=0)
    binned.clear_stats_cache()
    assert cached == dd.batched_bin_frequencies(binned, cols, n, max_bin=10)
    assert cached0 == dd.batched_bin_frequencies(binned, cols, n, max_bin=0)
