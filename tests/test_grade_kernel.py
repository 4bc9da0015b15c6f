"""Tests of the rank-grade kernels (K24, ops/hip/grades.hip).

Every input is built on the CPU from a seeded generator. The reference is
fp64 numpy written here: a value x lies in cell(x) = #{j : c_j < x} =
searchsorted(cutoffs, x, side="left"), NaN is null;

- grade_counts: int64 [ncols, max_ncut + 2], slot 0 nulls, slot 1 + j the
  rows of cell j (bincount), zero beyond a column's own ncut + 2 slots —
  compared exactly;
- grade_apply: table[cell(x)] as f32, null_grade for NaN — compared bit
  for bit.

Shapes follow the binding: rows split into chunks of about 65 536 (one
block per column and chunk), rows up to the first 16-byte line peeled,
16-byte vector loads, a scalar tail; per-thread private counters up to 15
cutoffs per launch, shared LDS atomics from 16; a linear scan up to 32
cutoffs, a binary search from 33."""

import numpy as np
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025, 65536, 65537, 131075]
NCUTS = [0, 1, 15, 16, 32, 33, 1023, 4095]


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _ref_counts(cols, cutoffs):
    stride = max([len(c) + 2 for c in cutoffs] + [2])
    out = np.zeros((len(cols), stride), dtype=np.int64)
    for i, (x, c) in enumerate(zip(cols, cutoffs)):
        xv = x.numpy().astype(np.float64)
        null = np.isnan(xv)
        cell = np.searchsorted(np.asarray(c, dtype=np.float64), xv[~null], side="left")
        out[i, 0] = null.sum()
        out[i, 1:] = np.bincount(cell, minlength=stride - 1)
    return out


def _ref_apply(x, c, table, null_grade):
    xv = x.numpy().astype(np.float64)
    null = np.isnan(xv)
    cell = np.searchsorted(np.asarray(c, dtype=np.float64), np.where(null, 0.0, xv), side="left")
    t = np.asarray(table, dtype=np.float32)
    return np.where(null, np.float32(null_grade), t[cell]).astype(np.float32)


def _table(ncut, g):
    """ncut + 1 distinct-looking f32 entries, none equal to the null grade used."""
    return (torch.rand(ncut + 1, generator=g, dtype=torch.float64) - 0.5).to(torch.float32).numpy()


def _check(ext, cols, cutoffs, tables=None, null_grade=-7.25, g=None):
    """Both ops against the reference; returns (counts, outs) as numpy."""
    g = g or torch.Generator().manual_seed(1)
    cuts = [torch.tensor(np.asarray(c, dtype=np.float64)) for c in cutoffs]
    tables = tables if tables is not None else [_table(len(c), g) for c in cutoffs]
    dcols = [x.to(DEV) for x in cols]
    counts = ext.grade_counts(dcols, cuts)
    assert counts.dtype == torch.int64 and counts.is_cuda
    want = _ref_counts(cols, cutoffs)
    assert tuple(counts.shape) == want.shape
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    outs = ext.grade_apply(dcols, cuts, [torch.tensor(t) for t in tables], null_grade)
    assert len(outs) == len(cols)
    res = []
    for x, c, t, o in zip(cols, cutoffs, tables, outs):
        assert o.dtype == torch.float32 and o.is_cuda and tuple(o.shape) == tuple(x.shape)
        got = o.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), _ref_apply(x, c, t, null_grade).view(np.uint32))
        res.append(got)
    return counts.cpu().numpy(), res


def _cutoffs(ncut, g, lo=-3.0, hi=3.0):
    """ncut strictly ascending fp64 cutoffs inside [lo, hi], most of them not
    representable in f32."""
    if ncut == 0:
        return np.zeros(0)
    base = np.linspace(lo, hi, ncut + 2)[1:-1]
    jitter = (torch.rand(ncut, generator=g, dtype=torch.float64).numpy() - 0.5) * (hi - lo) / (4 * (ncut + 2))
    c = base + jitter
    assert np.all(np.diff(c) > 0)
    return c


def _column(n, g, dtype, cutoffs):
    """Normal values with NaN, and every 7th value (where there are
    cutoffs) set to a cutoff rounded to the dtype, so rows sit on and next
    to cell boundaries."""
    x = torch.randn(n, generator=g, dtype=torch.float64) * 1.5
    if len(cutoffs) and n:
        pick = torch.randint(0, len(cutoffs), (n,), generator=g)
        on = torch.arange(n) % 7 == 3
        x = torch.where(on, torch.tensor(cutoffs)[pick], x)
    x = x.to(dtype)
    if n:
        x[torch.rand(n, generator=g) < 0.05] = float("nan")
    return x


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lengths(ext, dtype):
    """Every length on both sides of the vector width, the block width and
    the chunk size, at a linear-scan grid (private counters) and a
    binary-search grid (shared counters)."""
    g = torch.Generator().manual_seed(11)
    for ncut in (9, 100):
        c = _cutoffs(ncut, g)
        for n in LENGTHS:
            _check(ext, [_column(n, g, dtype, c)], [c], g=g)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cutoff_counts(ext, dtype):
    """Every cutoff count at which the kernel takes another path, each as a
    launch of its own (the launch's largest count picks the counters)."""
    g = torch.Generator().manual_seed(12)
    for ncut in NCUTS:
        c = _cutoffs(ncut, g)
        for n in (1025, 70001):
            _check(ext, [_column(n, g, dtype, c)], [c], g=g)


@requires_gpu
@pytest.mark.gpu
def test_mixed_dtypes_lengths_and_cutoff_counts_in_one_launch(ext):
    """f32 and f64 columns of different lengths and cutoff counts in one
    call: one launch per dtype, results back in the original order, counts
    rows padded with zeros to the call's longest."""
    g = torch.Generator().manual_seed(13)
    ncuts = [33, 0, 1023, 5, 16, 1, 32, 15]
    dtypes = [torch.float32, torch.float64] * 4
    lens = [70001, 5, 1025, 131075, 0, 257, 65537, 1023]
    cuts = [_cutoffs(k, g) for k in ncuts]
    cols = [_column(n, g, d, c) for n, d, c in zip(lens, dtypes, cuts)]
    counts, _ = _check(ext, cols, cuts, g=g)
    assert counts.shape == (8, 1025)
    for i, k in enumerate(ncuts):
        assert counts[i, : k + 2].sum() == lens[i] and not counts[i, k + 2 :].any()
    # launches of short lists only: the private-counter path with columns of
    # differing cutoff counts
    short = [i for i, k in enumerate(ncuts) if k <= 15]
    _check(ext, [cols[i] for i in short], [cuts[i] for i in short], g=g)


@requires_gpu
@pytest.mark.gpu
def test_values_on_cutoffs_and_cutoffs_f32_cannot_hold(ext):
    """Right-closed cells: a value equal to a cutoff stays below it. For an
    f32 column the cutoffs are planted between f32 neighbours, at the
    neighbours themselves and one fp64 ulp to either side of them."""
    f = np.float32
    vals = np.array([1.0, 1.0 + 2.0 ** -23, 3.0, 1e-3, 16777216.0, -2.5, 0.1, 7.0, 1000.5, -1e-3], dtype=f)
    cuts = []
    for v in vals:
        up = np.nextafter(v, f(np.inf))
        v64, up64 = float(v), float(up)
        cuts += [np.nextafter(v64, -np.inf), v64, np.nextafter(v64, np.inf), (v64 + up64) / 2,
                 np.nextafter(up64, -np.inf)]
    cuts = np.unique(np.asarray(cuts, dtype=np.float64))
    assert np.any(cuts.astype(f).astype(np.float64) != cuts) and len(cuts) > 33
    near = np.concatenate([[np.nextafter(v, f(-np.inf)), v, np.nextafter(v, f(np.inf)),
                            np.nextafter(np.nextafter(v, f(np.inf)), f(np.inf))] for v in vals]).astype(f)
    x32 = torch.tensor(np.tile(near, 50))
    x64 = torch.tensor(np.tile(np.concatenate([cuts, near.astype(np.float64)]), 40))
    for ncut in (len(cuts), 12):  # binary search / linear scan
        c = cuts[:ncut]
        counts, outs = _check(ext, [x32, x64], [c, c])
        # spot check of the rule itself, independent of searchsorted
        want0 = sum(int((c < float(v)).sum()) == 0 for v in x32.numpy())
        assert counts[0, 1] == want0


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zeros_denormals_infinities(ext, dtype):
    tiny = 1e-45 if dtype == torch.float32 else 5e-324
    special = [0.0, -0.0, tiny, -tiny, 2 * tiny, float("inf"), -float("inf"), float("nan"), 1.0, -1.0]
    x = torch.tensor(special * 30, dtype=dtype)
    for c in (
        np.array([-1.0, -tiny, 0.0, tiny, 1.0]),
        np.array([-np.inf, 0.0, np.inf]),
        # 5e-46 lies between zero and the smallest f32 denormal
        np.array([-np.inf, -1e300, -tiny, -0.0, tiny if dtype == torch.float64 else 5e-46, 1e300, np.inf]),
        np.concatenate([[-np.inf], np.linspace(-2, 2, 41), [np.inf]]),
    ):
        counts, outs = _check(ext, [x], [c])
    # +-0 share a cell, -inf is below every cutoff, +inf above every finite one
    c = np.array([-1.0, 0.0, 1.0])
    t = np.array([10.0, 20.0, 30.0, 40.0], dtype=np.float32)
    _, outs = _check(ext, [x], [c], tables=[t], null_grade=-1.0)
    assert list(outs[0][:10]) == [20.0, 20.0, 30.0, 20.0, 30.0, 40.0, 10.0, -1.0, 30.0, 10.0]


@requires_gpu
@pytest.mark.gpu
def test_all_nan_and_one_value_columns(ext):
    """An all-NaN column counts into slot 0 only; 100 000 rows of one value
    all bump one counter (private rows and shared atomics)."""
    n = 100_000
    nan = torch.full((n,), float("nan"), dtype=torch.float32)
    one = torch.full((n,), 0.75, dtype=torch.float32)
    one64 = torch.full((n,), 0.75, dtype=torch.float64)
    g = torch.Generator().manual_seed(14)
    for ncut in (3, 40):
        c = _cutoffs(ncut, g, lo=0.0, hi=1.5)
        counts, outs = _check(ext, [nan, one, one64], [c, c, c], g=g)
        assert counts[0, 0] == n and counts[0, 1:].sum() == 0
        cell = int((c < 0.75).sum())
        assert counts[1, 1 + cell] == n and counts[2, 1 + cell] == n
    # a value on its own cutoff
    counts, _ = _check(ext, [one], [np.array([0.5, 0.75, 1.0])])
    assert counts[0, 2] == n


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_offset_views_with_guard_values_and_outs_reuse(ext, dtype):
    """Inputs and outputs are views at every offset inside a 16-byte line,
    with different offsets for input and output; the elements around the
    views must come back untouched, and a reused `outs` slab is fully
    overwritten."""
    g = torch.Generator().manual_seed(15)
    c = _cutoffs(20, g)
    table = _table(20, g)
    tabs = [torch.tensor(table)]
    cuts = [torch.tensor(c)]
    GUARD = 12345.0
    for n in (0, 1, 6, 259, 1030, 65539):
        for ioff in range(4):
            ooff = (ioff * 3 + 1) % 4
            x = _column(n, g, dtype, c)
            buf = torch.full((n + 8,), 9.0e9, dtype=dtype)
            buf[ioff : ioff + n] = x
            dbuf = buf.to(DEV)
            obuf = torch.full((n + 8,), GUARD, dtype=torch.float32, device=DEV)
            view, oview = dbuf[ioff : ioff + n], obuf[ooff : ooff + n]
            res = ext.grade_apply([view], cuts, tabs, 0.5, [oview])
            assert res[0].data_ptr() == oview.data_ptr()
            want = _ref_apply(x, c, table, 0.5)
            host = obuf.cpu().numpy()
            np.testing.assert_array_equal(host[ooff : ooff + n].view(np.uint32), want.view(np.uint32))
            assert np.all(host[:ooff] == GUARD) and np.all(host[ooff + n :] == GUARD)
            np.testing.assert_array_equal(dbuf.cpu().numpy().view(np.uint8), buf.numpy().view(np.uint8))
            # the guard cells around the input would count as rows of the top cell
            np.testing.assert_array_equal(ext.grade_counts([view], cuts).cpu().numpy(), _ref_counts([x], [c]))
            # second use of the same slab with another table and null grade
            table2 = (table * 2 + 1).astype(np.float32)
            ext.grade_apply([view], cuts, [torch.tensor(table2)], -0.5, [oview])
            host = obuf.cpu().numpy()
            np.testing.assert_array_equal(host[ooff : ooff + n].view(np.uint32),
                                          _ref_apply(x, c, table2, -0.5).view(np.uint32))
            assert np.all(host[:ooff] == GUARD) and np.all(host[ooff + n :] == GUARD)


@requires_gpu
@pytest.mark.gpu
def test_counts_repeat_bit_equal_and_limit_matches_python(ext):
    from anovos_amd.ops import rank

    assert ext.GRADE_MAX_CELLS == rank.GRADE_MAX_CELLS == 4096
    g = torch.Generator().manual_seed(16)
    c = _cutoffs(200, g)
    x = _column(131075, g, torch.float32, c).to(DEV)
    a = ext.grade_counts([x], [torch.tensor(c)])
    b = ext.grade_counts([x], [torch.tensor(c)])
    assert torch.equal(a, b)


def test_ops_torch_path_matches_reference():
    """ops.rank.grade_counts / grade_columns on the CPU (the torch path)
    against the numpy reference of this file."""
    from anovos_amd.ops import rank

    g = torch.Generator().manual_seed(17)
    ncuts = [0, 1, 16, 33, 200]
    cuts = [_cutoffs(k, g) for k in ncuts]
    cols = [_column(n, g, d, c) for n, d, c in
            zip([0, 5, 1000, 1001, 3000], [torch.float32, torch.float64] * 3, cuts)]
    np.testing.assert_array_equal(rank.grade_counts(cols, cuts).numpy(), _ref_counts(cols, cuts))
    tables = [_table(k, g) for k in ncuts]
    outs = rank.grade_columns(cols, cuts, tables, null_grade=0.25)
    for x, c, t, o in zip(cols, cuts, tables, outs):
        assert o.dtype == torch.float32
        np.testing.assert_array_equal(o.numpy().view(np.uint32), _ref_apply(x, c, t, 0.25).view(np.uint32))
    slab = [torch.full((x.numel(),), 3.0, dtype=torch.float32) for x in cols]
    res = rank.grade_columns(cols, cuts, tables, null_grade=0.25, outs=slab)
    for o, s, r in zip(outs, slab, res):
        assert r is s and torch.equal(o, s)


def test_refusals_without_a_device():
    """Host tensors and empty lists are refused before any device call."""
    from anovos_amd.ops import backend

    ext = backend.hip_ext()
    if ext is None:
        pytest.skip("HIP extension not built")
    x = torch.zeros(32, dtype=torch.float32)
    c = torch.tensor([0.5], dtype=torch.float64)
    t = torch.zeros(2, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="grade_counts: device columns required"):
        ext.grade_counts([x], [c])
    with pytest.raises(RuntimeError, match="grade_counts: no columns"):
        ext.grade_counts([], [])
    with pytest.raises(RuntimeError, match="grade_apply: device columns required"):
        ext.grade_apply([x], [c], [t], 0.0)
    with pytest.raises(RuntimeError, match="grade_apply: device columns required"):
        ext.grade_apply([x], [c], [t], 0.0, [torch.zeros(32)])
    with pytest.raises(RuntimeError, match="grade_apply: no columns"):
        ext.grade_apply([], [], [], 0.0)
    assert ext.GRADE_MAX_CELLS == 4096


@requires_gpu
@pytest.mark.gpu
def test_refusals(ext):
    n = 64
    x = torch.ones(n, dtype=torch.float32, device=DEV)
    y = torch.ones(n, dtype=torch.float64, device=DEV)
    c = torch.tensor([0.5, 1.5], dtype=torch.float64)
    t = torch.zeros(3, dtype=torch.float32)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    strided = torch.zeros(2 * n, dtype=torch.float32, device=DEV)[::2]
    big = torch.arange(ext.GRADE_MAX_CELLS, dtype=torch.float64)

    def both(cols, cuts, match):
        with pytest.raises(RuntimeError, match=match):
            ext.grade_counts(cols, cuts)
        with pytest.raises(RuntimeError, match=match):
            ext.grade_apply(cols, cuts, [torch.zeros(k.numel() + 1) for k in cuts], 0.0)

    both([x.cpu()], [c], "device columns required")
    both([strided], [c], "must be contiguous")
    both([x.to(torch.int32)], [c], "expected float32/float64")
    both([x.to(torch.float16)], [c], "expected float32/float64")
    both([x, y], [c], "cutoffs has 1 entries, expected 2")
    both([x], [c, c], "cutoffs has 2 entries, expected 1")
    both([x], [big], "at most 4095 fit")
    both([x, y], [c, big], "at most 4095 fit")
    both([x], [torch.tensor([1.0, 1.0], dtype=torch.float64)], "strictly ascending")
    both([x], [torch.tensor([2.0, 1.0], dtype=torch.float64)], "strictly ascending")
    both([x], [torch.tensor([float("nan")], dtype=torch.float64)], "strictly ascending")
    both([x], [torch.tensor([0.0, float("nan")], dtype=torch.float64)], "strictly ascending")
    both([y, x], [c, torch.tensor([0.0, 1.0, float("nan")], dtype=torch.float64)], "strictly ascending")
    # the largest grid is accepted
    assert ext.grade_counts([x], [big[:-1]]).shape == (1, ext.GRADE_MAX_CELLS + 1)

    for bad_tables, match in (
        ([], "tables has 0 entries, expected 1"),
        ([t, t], "tables has 2 entries, expected 1"),
        ([torch.zeros(2)], "table of column 0 has 2 entries, expected 3"),
        ([torch.zeros(4)], "table of column 0 has 4 entries, expected 3"),
    ):
        with pytest.raises(RuntimeError, match=match):
            ext.grade_apply([x], [c], bad_tables, 0.0)
    for bad_out, match in (
        ([], "outs has 0 entries, expected 1"),
        ([out, out], "outs has 2 entries, expected 1"),
        ([out.to(torch.float64)], "outs must be a contiguous"),
        ([out.cpu()], "outs must be a contiguous"),
        ([torch.empty(2 * n, dtype=torch.float32, device=DEV)[::2]], "outs must be a contiguous"),
        ([out[:-1]], "length mismatch"),
        ([torch.empty(n + 1, dtype=torch.float32, device=DEV)], "length mismatch"),
    ):
        with pytest.raises(RuntimeError, match=match):
            ext.grade_apply([x], [c], [t], 0.0, bad_out)
    # f64 input with a preallocated f32 out is the normal case
    res = ext.grade_apply([y], [c], [torch.tensor([1.0, 2.0, 3.0])], 0.0, [out])
    assert torch.equal(res[0].cpu(), torch.full((n,), 2.0))
