"""Device quantile queries (K3q) and the device-cutoff IV/IG launch.

Everything is compared on fp64 bit patterns: the query kernel has to give
the bits of ops/histogram.host_quantile_query (hist mode) and of
_exact_integral_quantiles' rule (dense integer mode), and the analyzer has
to return the same results with ANOVOS_DEVICE_QUANTILES on and off.
"""

import math

import numpy as np
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
NAN = float("nan")
REL_ERR = 0.01
BENCH_PROBS = [0.01, 0.05, 0.10, 0.25, 0.50, 0.75, 0.90, 0.95, 0.99]


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _f64(v):
    return torch.tensor(np.asarray(v, dtype=np.float64), device=DEV)


def _check_hist_query(ext, hist, lo, hi, n, probs, rel_err=REL_ERR):
    """Kernel == host on values (bits), flags and largest bin; returns the host's."""
    from anovos_amd.ops.histogram import host_quantile_query

    hist = np.asarray(hist, dtype=np.int64)
    want_v, want_f, want_m = host_quantile_query(hist, lo, hi, n, probs, rel_err)
    v, f, m = ext.hist_quantile_query(torch.from_numpy(hist).to(DEV), _f64(lo), _f64(hi), _f64(n),
                                      list(probs), rel_err)
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(want_v))
    assert np.array_equal(f.cpu().numpy().astype(bool), want_f)
    assert np.array_equal(m.cpu().numpy(), want_m.astype(np.int64))
    return want_v, want_f, want_m


# --------------------------------------------------- kernel against the host
@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("nbins", [8, 2048])
@pytest.mark.parametrize("ncols", [1, 3, 150])
def test_hist_query_random(ext, ncols, nbins):
    rng = np.random.default_rng(1000 * ncols + nbins)
    # dense, sparse (bins of 0 and 1 counts) and mixed columns
    hist = rng.integers(0, 1000, (ncols, nbins))
    hist[rng.random((ncols, nbins)) < 0.3] = 0
    hist[rng.random((ncols, nbins)) < 0.1] = 1
    hist[:, 0] += 1  # no column is empty
    lo = rng.normal(0, 100, ncols)
    hi = lo + rng.random(ncols) * 10.0 ** rng.integers(-3, 6, ncols)
    n = hist.sum(axis=1).astype(np.float64)
    for probs in ([0.0], [1.0], [0.5], BENCH_PROBS):  # P = 1 and P = 9
        _check_hist_query(ext, hist, lo, hi, n, probs)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("nbins", [8, 2048])
def test_hist_query_special_columns(ext, nbins):
    probs = [0.0, 1.0, 0.5] + BENCH_PROBS
    big = 2 ** 31 + 7
    rows, lo, hi, n = [], [], [], []

    def add(h, l, u):
        rows.append(h)
        lo.append(l)
        hi.append(u)
        n.append(float(sum(h)))

    one_bin = [0] * nbins
    one_bin[nbins // 2] = 100_000
    add(one_bin, -3.0, 5.0)  # 0: all mass in one bin
    last = [0] * nbins
    last[-1] = 4321
    add(last, 0.3, 0.9)  # 1: mass only in the last bin (whose bound rounds above hi at 8 bins)
    add([0] * nbins, NAN, NAN)  # 2: empty column
    add([5] + [0] * (nbins - 1), NAN, NAN)  # 3: NaN range
    add([77] + [0] * (nbins - 1), 2.5, 2.5)  # 4: hi == lo
    single = [0] * nbins
    single[3] = 1
    add(single, 0.0, 1.0)  # 5: n == 1
    huge = [0] * nbins
    huge[1], huge[nbins - 2], huge[nbins // 2] = 2 ** 30, 2 ** 30, 7
    add(huge, -1.0, 1.0)  # 6: n == 2^31 + 7
    assert n[6] == big
    smooth = [50] * nbins
    add(smooth, 0.0, 1.0)  # 7: 50 of 50 * nbins per bin: flagged at 8 bins only
    vals, flags, maxbin = _check_hist_query(ext, rows, lo, hi, n, probs)
    assert flags[0].all() and maxbin[0] == 100_000
    assert flags[1].all() and maxbin[1] == 4321
    assert np.isnan(vals[2]).all() and np.isnan(vals[3]).all()
    assert (vals[4] == 2.5).all() and not flags[2:5].any()
    assert flags[7].all() == (nbins == 8)
    assert maxbin[6] == 2 ** 30


# --------------------------------------------------------- dense integer mode
def _integral_rule(counts, cmin, n, R, probs, rel_err):
    """_exact_integral_quantiles' query of one column."""
    cdf = np.cumsum(counts[:R])
    vals = []
    for p in probs:
        if p <= rel_err:
            r = 1
        elif p >= 1 - rel_err:
            r = n
        else:
            r = min(max(int(math.ceil(p * n)), 1), n)
        b = int(np.searchsorted(cdf, r, side="left"))
        vals.append(float(cmin + min(b, R - 1)))
    return vals


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["ones", "random", "gaps"])
def test_inthist_query(ext, pattern):
    rng = np.random.default_rng(5)
    Rs = [1, 2, 4095, 4095, 2]
    M = 4095
    counts = np.zeros((len(Rs), M), dtype=np.int64)
    for i, R in enumerate(Rs):
        if pattern == "ones":  # every rank is a cdf step
            counts[i, :R] = 1
        elif pattern == "random":
            counts[i, :R] = rng.integers(1, 50, R)
        else:  # empty integers inside the range; the ends are occupied
            counts[i, :R] = rng.integers(0, 3, R) * rng.integers(0, 2, R)
            counts[i, 0], counts[i, R - 1] = 3, 2
    counts[4, :2] = [5, 5]  # p = 0.5 -> r = 5 == cdf[0]
    cmin = np.array([-7.0, 0.0, 1000.0, -4094.0, 3.0])
    n = counts.sum(axis=1)
    up, dn = (lambda x: float(np.nextafter(x, 2.0))), (lambda x: float(np.nextafter(x, -1.0)))
    hi_p = 1 - REL_ERR
    probs = [0.0, dn(REL_ERR), REL_ERR, up(REL_ERR), 0.25, 0.5, 0.75, dn(hi_p), hi_p, up(hi_p), 1.0]
    got = ext.inthist_quantile_query(torch.from_numpy(counts).to(DEV), _f64(cmin), _f64(n),
                                     _f64(Rs), probs, REL_ERR).cpu().numpy()
    want = np.array([_integral_rule(counts[i], cmin[i], int(n[i]), Rs[i], probs, REL_ERR)
                     for i in range(len(Rs))])
    assert np.array_equal(_bits(got), _bits(want))
    if pattern == "ones":
        assert want[4][5] == 3.0  # the rank on the cdf step stays in the first integer


# ------------------------------------ device cutoffs into the counting kernel
@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 255, 1025, 65_537])
def test_bucketize_label_counts_dev_matches_host_cutoffs(ext, rows):
    g = torch.Generator().manual_seed(rows)
    cols = []
    for i in range(4):
        x = torch.randn(rows, generator=g, dtype=torch.float64 if i == 2 else torch.float32) * (i + 1)
        x[torch.rand(rows, generator=g) < 0.05] = NAN
        cols.append(x.to(DEV))
    label = (torch.rand(rows, generator=g) < 0.3).to(torch.uint8).to(DEV)
    cuts = torch.sort(torch.randn(4, 9, generator=g, dtype=torch.float64) * 2, dim=1).values
    cuts[3, 4] = NAN  # an all-null column gives NaN cutoffs
    sizes = [11] * 4
    want = ext.bucketize_label_counts(cols, [cuts[i] for i in range(4)], label, sizes)
    got = ext.bucketize_label_counts_dev(cols, cuts.to(DEV), label, sizes)
    assert torch.equal(got, want)
    assert int(got.sum()) > 0


# ------------------------------------------------------------------ end to end
N_E2E = 250_001  # just above EXACT_N_THRESHOLD
NUM = ["normal", "lognormal", "ints", "spike", "const", "allnull", "withinf"]
SMOOTH = ["normal", "ints", "const", "allnull"]  # served by the device cutoffs
CAT = ["c0", "c1"]


@pytest.fixture(scope="module")
def e2e_frame():
    from anovos_amd.core.frame import AnovosFrame, Column

    n = N_E2E
    g = torch.Generator().manual_seed(11)
    data = {}
    data["normal"] = torch.randn(n, generator=g) * 3 + 1  # no nulls: n stays above the threshold
    data["lognormal"] = torch.exp(torch.randn(n, generator=g))
    data["ints"] = torch.randint(0, 80, (n,), generator=g).to(torch.float32)
    x = torch.randn(n, generator=g)
    x[torch.rand(n, generator=g) < 0.6] = 1.25
    data["spike"] = x
    data["const"] = torch.full((n,), 3.5)
    data["allnull"] = torch.full((n,), NAN)
    x = torch.randn(n, generator=g)
    x[17] = float("inf")
    data["withinf"] = x
    for c in ("lognormal", "ints", "spike"):
        data[c][torch.rand(n, generator=g) < 0.01] = NAN
    cols = {c: Column(c, "float", data[c].to(torch.float32).to(DEV)) for c in NUM}
    for i, c in enumerate(CAT):
        codes = torch.randint(0, 5 + i, (n,), generator=g).to(torch.int32)
        codes[torch.rand(n, generator=g) < 0.02] = -1
        cols[c] = Column(c, "string", codes.to(DEV), [f"v{j}" for j in range(5 + i)])
    lab = (torch.rand(n, generator=g) < 0.25).to(torch.int32)
    cols["label"] = Column("label", "string", lab.to(DEV), ["no", "yes"])
    return AnovosFrame(cols, torch.device(DEV))


def _quantiles(idf, monkeypatch, switch, cols=NUM, probs=BENCH_PROBS):
    from anovos_amd.ops import histogram as hist_ops

    monkeypatch.setenv("ANOVOS_DEVICE_QUANTILES", switch)
    idf.clear_stats_cache()
    return hist_ops.approx_quantiles(idf, cols, probs)


@requires_gpu
@pytest.mark.gpu
def test_approx_quantiles_same_with_switch_on_and_off(e2e_frame, monkeypatch):
    idf = e2e_frame
    off = _quantiles(idf, monkeypatch, "0")
    assert all(("hist_dev", 2048) not in idf.col(c).cache and ("inthist_dev",) not in idf.col(c).cache
               for c in NUM)
    on = _quantiles(idf, monkeypatch, "1")
    for c in NUM:
        assert np.array_equal(_bits(on[c]), _bits(off[c])), c
    cache = {c: idf.col(c).cache for c in NUM}
    thr = {c: REL_ERR * 0.5 * (N_E2E if c in ("normal", "const") else 0.99 * N_E2E) for c in NUM}
    # the spike column was flagged and went through the host path: its
    # histogram row was fetched; the smooth column's stayed on the device
    assert cache["spike"][("hist_maxbin", 2048)] > thr["spike"]
    assert ("hist", 2048) in cache["spike"]
    assert cache["normal"][("hist_maxbin", 2048)] <= thr["normal"]
    assert ("hist_dev", 2048) in cache["normal"] and ("hist", 2048) not in cache["normal"]
    # +inf: sorted, never binned; integers: dense counts, on the device too
    assert ("hist_dev", 2048) not in cache["withinf"] and ("hist", 2048) not in cache["withinf"]
    assert ("inthist_dev",) in cache["ints"] and ("inthist",) in cache["ints"]
    assert on["spike"][4] == 1.25 and on["const"] == [3.5] * 9
    assert all(math.isnan(v) for v in on["allnull"])


@requires_gpu
@pytest.mark.gpu
def test_iv_ig_same_with_switch_on_and_off(e2e_frame, ext, monkeypatch):
    from anovos_amd.data_analyzer import association_evaluator as ae
    from anovos_amd.data_transformer import transformers as T
    from anovos_amd.shared.context import init_context

    ctx = init_context(DEV + ":0")
    idf = e2e_frame
    seen = []
    launch = ext.bucketize_label_counts_dev

    def spy(cols, cut_matrix, label, sizes):
        seen.append(cut_matrix.cpu().numpy().copy())
        return launch(cols, cut_matrix, label, sizes)

    monkeypatch.setattr(ext, "bucketize_label_counts_dev", spy)

    def run(switch, cols):
        _quantiles(idf, monkeypatch, switch)  # the analyzer's quantile section comes first
        iv = ae.IV_calculation(ctx, idf, list_of_cols=cols, label_col="label", event_label="yes")
        ig = ae.IG_calculation(ctx, idf, list_of_cols=cols, label_col="label", event_label="yes")
        return iv, ig

    for cols, device_cutoffs in ((NUM + CAT, False), (SMOOTH + CAT, True)):
        iv0, ig0 = run("0", cols)
        assert not seen
        host_cuts = T.compute_bin_cutoffs(ctx, idf, [c for c in cols if c in NUM], "equal_frequency", 10)[1]
        iv1, ig1 = run("1", cols)
        assert list(iv1["attribute"]) == list(iv0["attribute"]) == cols
        assert np.array_equal(_bits(iv1["iv"].to_numpy()), _bits(iv0["iv"].to_numpy()))
        assert np.array_equal(_bits(ig1["ig"].to_numpy()), _bits(ig0["ig"].to_numpy()))
        # spike / log-normal / +inf columns keep the whole call on the host
        # path; without them the cutoffs reach the kernel from the device
        assert len(seen) == (1 if device_cutoffs else 0)
        for m in seen:
            assert m.shape == (len(host_cuts), 9)
            assert np.array_equal(_bits(m), _bits(np.array(host_cuts, dtype=np.float64)))
        seen.clear()
