"""Placement of the binning family against an fp64 reference.

The float kernels place f32 data against f32 cutoffs nudged one ulp with
nextafterf and promise the verdict of the fp64 comparison
`cut < float64(v)`. Here that promise is checked directly, with cutoffs
that f32 cannot hold (so the adjustment fires) and, for every cutoff, the
cutoff rounded to the column's dtype and both of its neighbours planted in
the data.

Reference, in numpy, never touching the code under test:
label = 1 + count(cuts < float64(v)); NaN data -> NaN (-1 for the int
kernel, whose label is the count itself); counts = bincount of the labels
with nulls in slot 0; label counts put null into slot 0 and bin b into
slot b + 1 clamped to slots - 1, split by a random uint8 label.

Cutoff lists: sorted uniform(-3, 3) of 1, 9, 10 (9 / 16 register
cutoffs), 16, 17 (LDS linear scan; private / shared counters switch at
ncut + 2 <= 17), 32, 33 (binary search) and 40 entries; and a list of
extremes (beyond FLT_MAX, f32 denormals, below the smallest denormal,
2^24 + 1, FLT_MAX + half an ulp) as it is and padded on the right to 17
and 33 entries. The pads rise from 1e300 in equal steps of the exponent
(1e309 is no double, so powers of ten alone do not reach 33 entries)."""

import functools

import numpy as np
import pytest
import torch

from anovos_amd.ops import bucketize as bk
from test_quantile_contract import DEVICES

LENGTHS = [4_099, 65_539]  # one chunk; two chunks with an unaligned boundary
DTYPES = [torch.float32, torch.float64]
NAN = float("nan")
FLT_MAX = float(np.finfo(np.float32).max)

RANDOM_NCUTS = [1, 9, 10, 16, 17, 32, 33, 40]
EXTREMES = [-1e300, -3.5e38, -1e-42, -1e-50, 0.0, 1e-50, 2.0 ** -150, 2.0 ** -149, 1e-42, 0.1, 16777217.0,
            3.4028235677973366e38, 3.5e38, 1e300]


def _padded(total):
    k = total - len(EXTREMES)
    step = 1.0 if k <= 8 else 0.4  # 1e301, 1e302, ... while they fit below DBL_MAX
    return EXTREMES + [10.0 ** (300 + step * (i + 1)) for i in range(k)]


@functools.lru_cache(maxsize=None)
def _lists():
    rng = np.random.default_rng(3001)
    out = {f"u{k}": np.sort(rng.uniform(-3, 3, k)) for k in RANDOM_NCUTS}
    out["ext14"] = np.array(EXTREMES)
    out["ext17"] = np.array(_padded(17))
    out["ext33"] = np.array(_padded(33))
    return out


LISTS = list(_lists.__wrapped__())


def test_cutoff_lists():
    for name, cuts in _lists().items():
        assert cuts.dtype == np.float64 and np.all(np.isfinite(cuts)), name
        assert np.all(np.diff(cuts) > 0), name
        if name.startswith("u"):
            for c in cuts:
                assert float(np.float32(c)) != c, (name, c)  # the f32 adjustment has to decide
    assert [len(_lists()[k]) for k in ("ext14", "ext17", "ext33")] == [14, 17, 33]
    assert _lists()["ext17"][14:].tolist() == [1e301, 1e302, 1e303]


# -------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _column(name, dtype, n):
    """CPU tensor: the planted values first, then random values over the
    cutoffs' span (for the extremes: both signs, magnitudes 1e-48 .. 1e39
    log-uniform, which overflow to +-inf and underflow to 0 in f32), about
    3 % NaN."""
    cuts = _lists()[name]
    npdt = np.float32 if dtype == torch.float32 else np.float64
    rng = np.random.default_rng([3011, LISTS.index(name), DTYPES.index(dtype), n])
    if name.startswith("u"):
        x = rng.uniform(-3.5, 3.5, n)
    else:
        x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-48, 39, n)
    with np.errstate(over="ignore", under="ignore"):
        x = x.astype(npdt)
        x[rng.random(n) < 0.03] = np.nan
        planted = []
        for c in cuts:
            r = npdt(c)
            planted += [r, np.nextafter(r, npdt(np.inf)), np.nextafter(r, npdt(-np.inf))]
        planted += [0.0, -0.0, np.inf, -np.inf, FLT_MAX, -FLT_MAX]
        if npdt is np.float32:
            planted += [1e-45, -1e-45]  # the smallest f32 denormal
        planted = np.array(planted, dtype=npdt)
    assert planted.size < n
    x[: planted.size] = planted
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def _below(name, dtype, n):
    """count(cuts < float64(v)) per element as int64, -1 for NaN."""
    cuts = _lists()[name]
    v = _column(name, dtype, n).to(torch.float64).numpy()
    below = (cuts[None, :] < v[:, None]).sum(axis=1).astype(np.int64)
    below[np.isnan(v)] = -1
    return below


def _ref_labels(name, dtype, n):
    b = _below(name, dtype, n)
    return np.where(b < 0, np.float32(np.nan), (b + 1).astype(np.float32))


def _ref_counts(name, dtype, n, stride):
    return np.bincount(_below(name, dtype, n) + 1, minlength=stride)  # -1 -> slot 0, label b -> slot b


@functools.lru_cache(maxsize=None)
def _label(n):
    rng = np.random.default_rng(3019 + n)
    return torch.from_numpy(rng.choice(np.array([0, 0, 1, 7, 255], dtype=np.uint8), n))


def _ref_label_counts(name, dtype, n, slots):
    b = _below(name, dtype, n)
    slot = np.where(b < 0, 0, np.minimum(b + 2, slots - 1))
    event = _label(n).numpy() != 0
    return np.bincount(slot, minlength=slots), np.bincount(slot[event], minlength=slots)


def test_planted_neighbours_straddle_their_cutoffs():
    """Not a test of the code: the planted neighbours must fall on both
    sides of their cutoff, or the data would not probe the adjustment."""
    for name in LISTS:
        cuts = _lists()[name]
        for dtype in DTYPES:
            v = _column(name, dtype, LENGTHS[0]).to(torch.float64).numpy()[: 3 * len(cuts)].reshape(-1, 3)
            for j, c in enumerate(cuts):
                assert (v[j] > c).any() and (v[j] <= c).any(), (name, dtype, c, v[j])


# ------------------------------------------------------------------ checks
def _assert_labels(got, want, what):
    """Bit-exact: NaN exactly where the reference has NaN, the same bits
    elsewhere (labels are small positive integers in f32)."""
    got = got.cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape, what
    g = got.numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)), what
    ok = ~np.isnan(want)
    bad = np.nonzero(g.view(np.int32)[ok] != want.view(np.int32)[ok])[0]
    assert bad.size == 0, (what, "first mismatches at", np.nonzero(ok)[0][bad[:5]], g[ok][bad[:5]], want[ok][bad[:5]])


def _check_float_family(fns, specs, device, what):
    """specs: (list name, dtype, n) per column, all in ONE call of each
    function. fns: (int labels, float labels, float labels + counts)."""
    int_fn, float_fn, counts_fn = fns
    cols = [_column(*s).to(device) for s in specs]
    cuts = [torch.from_numpy(_lists()[s[0]]) for s in specs]
    stride = max(len(_lists()[s[0]]) for s in specs) + 2
    outs = float_fn(cols, cuts)
    outs_c, counts = counts_fn(cols, cuts)
    ints = int_fn(cols, cuts)
    counts = counts.cpu()
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (len(specs), stride), what
    for i, s in enumerate(specs):
        _assert_labels(outs[i], _ref_labels(*s), (what, "float", s))
        _assert_labels(outs_c[i], _ref_labels(*s), (what, "float+counts", s))
        assert np.array_equal(counts[i].numpy(), _ref_counts(*s, stride)), (what, "counts", s)
        got = ints[i].cpu()
        assert got.dtype == torch.int32, what
        assert np.array_equal(got.numpy().astype(np.int64), _below(*s)), (what, "int", s)


def _fns(device):
    if device == "cpu":  # the torch fallbacks
        return bk.bucketize_columns, bk.bucketize_columns_float, bk.bucketize_columns_float_counts
    from anovos_amd.ops import backend

    ext = backend.require_hip()
    assert ext is not None, "HIP extension must be loadable on the GPU box"
    return ext.bucketize_columns, ext.bucketize_columns_float, ext.bucketize_columns_float_counts


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", LISTS)
@pytest.mark.parametrize("device", DEVICES)
def test_placement_one_list(device, name, dtype):
    """Both lengths in one call, every column against the same list: the
    launch takes the path its cutoff count selects (registers, LDS scan,
    binary search; private or shared counters)."""
    _check_float_family(_fns(device), [(name, dtype, n) for n in LENGTHS], device, name)


@pytest.mark.parametrize("device", DEVICES)
def test_placement_mixed_lists_one_call(device):
    """Every list, both dtypes and both lengths in one call, each column
    with its own list: the launch is sized by the longest list and every
    column must still read its own cutoffs."""
    specs = [(name, dtype, LENGTHS[(i + j) % 2]) for i, name in enumerate(LISTS) for j, dtype in enumerate(DTYPES)]
    _check_float_family(_fns(device), specs, device, "mixed")
    # short lists only, of different lengths: the register path with mixed lists
    short = [(name, torch.float32, n) for name, n in (("u9", LENGTHS[1]), ("u1", LENGTHS[0]), ("ext14", LENGTHS[1]),
                                                       ("u16", LENGTHS[0]), ("u10", LENGTHS[1]))]
    _check_float_family(_fns(device), short, device, "mixed short")


def _check_label_counts(ext, specs, n, what):
    cols = [_column(name, dtype, n).to("cuda") for name, dtype in specs]
    cuts = [torch.from_numpy(_lists()[name]) for name, _ in specs]
    sizes = [len(_lists()[name]) + 3 for name, _ in specs]
    got = ext.bucketize_label_counts(cols, cuts, _label(n).to("cuda"), sizes).cpu().numpy()
    assert got.dtype == np.int64 and got.size == 2 * sum(sizes), what
    pos = 0
    for (name, dtype), s in zip(specs, sizes):
        tot, evt = _ref_label_counts(name, dtype, n, s)
        assert np.array_equal(got[pos:pos + s], tot), (what, "totals", name, dtype)
        assert np.array_equal(got[pos + s:pos + 2 * s], evt), (what, "events", name, dtype)
        pos += 2 * s


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", LISTS)
def test_label_counts_placement(name, n):
    """bucketize_label_counts with sizes = ncut + 3 (every column of a call
    shares the label's length): one list in f32 and f64, then — once per
    length, with the first list — all lists and both dtypes in one call."""
    from anovos_amd.ops import backend

    ext = backend.require_hip()
    assert ext is not None, "HIP extension must be loadable on the GPU box"
    _check_label_counts(ext, [(name, dt) for dt in DTYPES], n, name)
    if name == LISTS[0]:
        _check_label_counts(ext, [(nm, dt) for nm in LISTS for dt in DTYPES], n, "mixed")
        _check_label_counts(ext, [(nm, torch.float32) for nm in ("u9", "u1", "u10")], n, "mixed short")
