"""Tests of the grouped-moments kernel (K23, ops/hip/grouped_moments.hip).

Every input is built on the CPU from a seeded generator. The reference is
a plain fp64 numpy group-by written here: slot v for a code 0 <= v < size,
the null slot `size` for anything else; per slot (n, s1, s2) = (#rows,
sum d, sum d^2) with d = (double)x - shift over the rows whose x is not
NaN; blocks [size + 1][3] concatenated in pair order.

Integer-valued data with |x| <= 1000 and integer shifts make every sum
exact in fp64 in any order (|d| <= 2000, d^2 <= 4e6, fewer than 2^18 rows:
below 2^53), so those tests compare with exact equality. Real-valued data
is held to the any-order summation bound of the issue.

Shapes follow the binding: rows split into chunks of about 65 536 (one
block each per work item), 16-byte vector loads with a scalar head and
tail, GRP_CELLS accumulator cells per work item (one window of slots times
the packed value columns)."""

import math

import numpy as np
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _ref_block(codes, size, x, shift):
    """fp64 [size + 1, 3] of one pair."""
    c = codes.numpy().astype(np.int64)
    slot = np.where((c >= 0) & (c < size), c, size)
    xv = x.numpy().astype(np.float64)
    ok = ~np.isnan(xv)
    d = xv[ok] - float(shift)
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.bincount(slot[ok], minlength=size + 1).astype(np.float64)
        s1 = np.bincount(slot[ok], weights=d, minlength=size + 1)
        s2 = np.bincount(slot[ok], weights=d * d, minlength=size + 1)
    return np.stack([n, s1, s2], axis=1)


def _run(ext, codes, sizes, values, shifts, pair_c, pair_v, dev_codes=None, dev_values=None):
    dev_codes = dev_codes if dev_codes is not None else [c.to(DEV) for c in codes]
    dev_values = dev_values if dev_values is not None else [v.to(DEV) for v in values]
    got = ext.grouped_moments(dev_codes, sizes, dev_values, shifts, pair_c, pair_v)
    assert got.dtype == torch.float64 and got.dim() == 1 and got.is_cuda
    assert got.numel() == sum(3 * (sizes[c] + 1) for c in pair_c)
    return got.cpu().numpy()


def _blocks(flat, sizes, pair_c):
    out, off = [], 0
    for c in pair_c:
        k = 3 * (sizes[c] + 1)
        out.append(flat[off : off + k].reshape(sizes[c] + 1, 3))
        off += k
    return out


def _check_exact(ext, codes, sizes, values, shifts, pair_c, pair_v, **kw):
    """Run the binding and compare block by block, bit for bit (NaN = NaN),
    at the offsets the contract gives."""
    got = _blocks(_run(ext, codes, sizes, values, shifts, pair_c, pair_v, **kw), sizes, pair_c)
    for q, (c, v) in enumerate(zip(pair_c, pair_v)):
        want = _ref_block(codes[c], sizes[c], values[v], shifts[v])
        assert np.array_equal(got[q], want, equal_nan=True), f"pair {q} = (code {c}, value {v})"
    return got


def _codes(n, size, g):
    """Codes in [-1, size]: every valid code, NULL_CODE and `size` itself
    (the first code past the dictionary)."""
    return torch.randint(-1, size + 1, (n,), generator=g).to(torch.int32)


def _ints(n, g, dtype):
    return torch.randint(-1000, 1001, (n,), generator=g).to(dtype)


# 0: no launch; 1, 3: below one vector; 4, 5: one vector (+ tail); 255..257
# around one vector per thread; 1023 / 1025: around one trip of the block;
# 65 535..65 537: around the first length with two chunks; 131 075: three
# chunks (rounded up to a multiple of 4 rows) with a short last one
LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025, 65_535, 65_536, 65_537, 131_075]


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", LENGTHS)
def test_exact_lengths_and_sizes(ext, n, dtype):
    """Only the null slot, one category, one window up to its edge
    (GRP_CELLS - 2 and - 1 categories: GRP_CELLS - 1 and GRP_CELLS slots),
    the first size with two windows (GRP_CELLS categories) and three
    windows (2 * GRP_CELLS + 1); three value columns per code column, one
    of them with a group that is all NaN, one all NaN."""
    G = ext.GRP_CELLS
    g = torch.Generator().manual_seed(2300 + n)
    sizes = [0, 1, G - 2, G - 1, G, 2 * G + 1]
    codes = [_codes(n, s, g) for s in sizes]
    x0 = _ints(n, g, dtype)
    x1 = _ints(n, g, dtype)
    x1[torch.rand(n, generator=g) < 0.1] = float("nan")
    x1[codes[3] == 2] = float("nan")  # a whole group of code column 3
    x2 = torch.full((n,), float("nan"), dtype=dtype)
    values = [x0, x1, x2]
    shifts = [0.0, -7.0, 3.0]
    pair_c = [c for c in range(len(sizes)) for _ in values]
    pair_v = [v for _ in sizes for v in range(len(values))]
    got = _check_exact(ext, codes, sizes, values, shifts, pair_c, pair_v)
    # every non-NaN row lands in exactly one slot of every block
    for q, v in enumerate(pair_v):
        assert got[q][:, 0].sum() == float((~torch.isnan(values[v])).sum())
    if n:
        assert got[3 * 3 + 1][2, 0] == 0.0  # the all-NaN group counts nothing


@requires_gpu
@pytest.mark.gpu
def test_packing_offsets_and_mixed_dtypes(ext):
    """More value columns than one item packs, f32 and f64 interleaved in
    one list, several code columns, pairs in scrambled order, a pair
    listed twice."""
    G = ext.GRP_CELLS
    g = torch.Generator().manual_seed(41)
    n = 70_003  # two chunks
    sizes = [0, 1, 3, G - 1, 3 * G]
    codes = [_codes(n, s, g) for s in sizes]
    values, shifts = [], []
    for j in range(11):
        x = _ints(n, g, torch.float32 if j % 3 else torch.float64)
        x[torch.rand(n, generator=g) < 0.05] = float("nan")
        values.append(x)
        shifts.append(float(j - 5))
    pair_c = [c for c in range(len(sizes)) for _ in values]
    pair_v = [v for _ in sizes for v in range(len(values))]
    perm = torch.randperm(len(pair_c), generator=g).tolist()
    pair_c = [pair_c[i] for i in perm] + [2, 2]
    pair_v = [pair_v[i] for i in perm] + [4, 4]
    got = _check_exact(ext, codes, sizes, values, shifts, pair_c, pair_v)
    assert np.array_equal(got[-1], got[-2])
    # the plan of a launch with 9 value columns of one dtype: a dictionary
    # within one window packs min(8, G // slots) value columns per item,
    # 3 G + 1 slots take four windows per pair
    items, reads, cells = ext.grouped_moments_plan(sizes, [c for c in range(5) for _ in range(9)],
                                                   [v for _ in range(5) for v in range(9)])
    packed = [min(8, G // slots) for slots in (1, 2, 4, G)]
    want_items = sum(-(-9 // p) for p in packed) + 9 * 4
    assert (items, reads) == (want_items, want_items + 4 * 9 + 9 * 4)
    assert cells == G  # the G-slot dictionary fills an item on its own


def _view(base_fill, data, offset, pad=9):
    """data as a view at element `offset` of a larger device buffer whose
    other elements hold base_fill."""
    base = torch.full((data.numel() + offset + pad,), base_fill, dtype=data.dtype)
    base[offset : offset + data.numel()] = data
    v = base.to(DEV)[offset : offset + data.numel()]
    assert v.is_contiguous() and v.storage_offset() == offset
    return v


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_offset_views(ext, dtype):
    """Views into larger buffers at every combination of 16-byte
    misalignment of the codes (0..3 elements) and of the values (0..3 f32
    elements, 0..1 f64 elements), plus value columns of one item at
    different misalignments. Outside the views sit a valid code (0) and a
    huge value, so a read past either end shows up in slot 0 and in the
    sums."""
    g = torch.Generator().manual_seed(59)
    n = 70_003
    sizes = [3, 40]
    per_line = 16 // torch.tensor([], dtype=dtype).element_size()
    codes = [_codes(n, s, g) for s in sizes]
    values = [_ints(n, g, dtype) for _ in range(3)]
    values[1][torch.rand(n, generator=g) < 0.1] = float("nan")
    shifts = [1.0, 0.0, -2.0]
    pair_c = [0, 0, 0, 1, 1]
    pair_v = [0, 1, 2, 0, 2]
    want = [_ref_block(codes[c], sizes[c], values[v], shifts[v]) for c, v in zip(pair_c, pair_v)]
    combos = [(oc, (ov, ov, ov)) for oc in range(4) for ov in range(per_line)]
    combos += [(1, (0, 1, 0)), (0, (1, 1, 0)), (3, (per_line - 1, 0, 1))]
    for oc, ovs in combos:
        dev_codes = [_view(0, c, oc) for c in codes]
        dev_values = [_view(1e30, x, ov) for x, ov in zip(values, ovs)]
        got = _blocks(_run(ext, codes, sizes, values, shifts, pair_c, pair_v,
                           dev_codes=dev_codes, dev_values=dev_values), sizes, pair_c)
        for q in range(len(pair_c)):
            assert np.array_equal(got[q], want[q], equal_nan=True), (oc, ovs, q)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ["plus", "minus", "both"])
def test_infinities(ext, dtype, case):
    """+inf only, -inf only and both in one group: counted, and carried
    through the sums as IEEE says (inf, -inf, NaN for s1; inf for s2)."""
    G = ext.GRP_CELLS
    g = torch.Generator().manual_seed(67)
    n = 70_003
    sizes = [5, 2 * G + 1]
    codes = [_codes(n, s, g) for s in sizes]
    x = _ints(n, g, dtype)
    rows = torch.nonzero(codes[0] == 1).flatten()
    if case in ("plus", "both"):
        x[rows[:3]] = float("inf")
    if case in ("minus", "both"):
        x[rows[-2:]] = float("-inf")
    got = _check_exact(ext, codes, sizes, [x], [4.0], [0, 1], [0, 0])
    b = got[0]
    assert b[1, 0] == float(len(rows)) and b[1, 2] == float("inf")
    assert {"plus": b[1, 1] == float("inf"), "minus": b[1, 1] == float("-inf"), "both": math.isnan(b[1, 1])}[case]
    assert np.isfinite(b[[0, 2, 3, 4, 5]]).all()


def _real_case(dtype, kind, n=131_075):
    G = 16  # sizes around typical windows; the exact value is irrelevant here
    g = torch.Generator().manual_seed(73)
    sizes = [5, 2 * G + 1]
    codes = [_codes(n, s, g) for s in sizes]
    x = torch.randn(n, generator=g, dtype=torch.float64)
    if kind == "offset":
        x = x + 1.0e6  # |mean| >> sigma
    x = x.to(dtype)
    x[torch.rand(n, generator=g) < 0.02] = float("nan")
    shift = float(np.nanmean(x.numpy().astype(np.float64))) if kind == "offset" else 0.0
    return codes, sizes, [x], [shift], [0, 1], [0, 0]


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["normal", "offset"])
def test_real_values_within_summation_bound(ext, dtype, kind):
    """d = (double)x - shift is one IEEE rounding, identical on both sides;
    any summation order of n_g terms stays within (n_g - 1) u sum|t| of the
    exact sum, one more u for a squaring that is fused or not, one for the
    rounding of fsum: |s1 - fsum(d)| <= (n_g + 2) u sum|d| and
    |s2 - fsum(d^2)| <= (n_g + 2) u sum d^2 with u = 2^-53. n is exact."""
    codes, sizes, values, shifts, pair_c, pair_v = _real_case(dtype, kind)
    got = _blocks(_run(ext, codes, sizes, values, shifts, pair_c, pair_v), sizes, pair_c)
    xv = values[0].numpy().astype(np.float64)
    ok = ~np.isnan(xv)
    d = xv - shifts[0]
    for q, c in enumerate(pair_c):
        cc = codes[c].numpy().astype(np.int64)
        slot = np.where((cc >= 0) & (cc < sizes[c]), cc, sizes[c])
        for s in range(sizes[c] + 1):
            dg = d[ok & (slot == s)]
            n_g = dg.size
            assert got[q][s, 0] == float(n_g)
            e1 = abs(got[q][s, 1] - math.fsum(dg))
            e2 = abs(got[q][s, 2] - math.fsum(dg * dg))
            b1 = (n_g + 2) * U * math.fsum(np.abs(dg))
            b2 = (n_g + 2) * U * math.fsum(dg * dg)
            assert e1 <= b1 and e2 <= b2, (q, s, n_g, e1, b1, e2, b2)


@requires_gpu
@pytest.mark.gpu
def test_same_call_gives_same_bits(ext):
    codes, sizes, values, shifts, pair_c, pair_v = _real_case(torch.float32, "normal")
    dc = [c.to(DEV) for c in codes]
    dv = [v.to(DEV) for v in values]
    a = ext.grouped_moments(dc, sizes, dv, shifts, pair_c, pair_v)
    b = ext.grouped_moments(dc, sizes, dv, shifts, pair_c, pair_v)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))  # bit for bit; no NaN in this input
    assert torch.equal(a, b)


def test_refusals_without_a_device():
    """Host tensors and empty lists are refused before any device call."""
    from anovos_amd.ops import backend

    ext = backend.hip_ext()
    if ext is None:
        pytest.skip("HIP extension not built")
    c = torch.zeros(32, dtype=torch.int32)
    x = torch.zeros(32, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="grouped_moments: device columns required"):
        ext.grouped_moments([c], [2], [x], [0.0], [0], [0])
    with pytest.raises(RuntimeError, match="grouped_moments: no columns"):
        ext.grouped_moments([], [], [x], [0.0], [], [])
    assert ext.GRP_CELLS >= 4
    # the plan needs no device either
    with pytest.raises(RuntimeError, match="pair index out of range"):
        ext.grouped_moments_plan([2], [1], [0])
    with pytest.raises(RuntimeError, match="length mismatch"):
        ext.grouped_moments_plan([2], [0, 0], [0])
    assert ext.grouped_moments_plan([2], [], []) == [0, 0, 0]


@requires_gpu
@pytest.mark.gpu
def test_refusals(ext):
    n = 64
    c = torch.zeros(n, dtype=torch.int32, device=DEV)
    x = torch.ones(n, dtype=torch.float32, device=DEV)
    y = torch.ones(n, dtype=torch.float64, device=DEV)
    strided_c = torch.zeros(2 * n, dtype=torch.int32, device=DEV)[::2]
    strided_x = torch.zeros(2 * n, dtype=torch.float32, device=DEV)[::2]
    ok = dict(codes=[c], sizes=[2], values=[x, y], shifts=[0.0, 0.0], pair_c=[0, 0], pair_v=[0, 1])

    def call(**kw):
        a = {**ok, **kw}
        return ext.grouped_moments(a["codes"], a["sizes"], a["values"], a["shifts"], a["pair_c"], a["pair_v"])

    for bad in (
        dict(codes=[c.cpu()]),                       # host tensors
        dict(values=[x.cpu(), y]),
        dict(codes=[strided_c]),                     # strided views
        dict(values=[strided_x, y]),
        dict(codes=[c.to(torch.int64)]),             # wrong dtypes
        dict(values=[x.to(torch.float16), y]),
        dict(values=[c, y]),
        dict(codes=[x]),
        dict(values=[x[: n - 1], y]),                # unequal lengths within a list
        dict(codes=[c, c[: n - 1]], sizes=[2, 2]),
        dict(codes=[c[: n - 1]]),                    # and between the lists
        dict(sizes=[]),                              # short sizes / shifts
        dict(shifts=[0.0]),
        dict(pair_c=[0, 1]),                         # pair indices out of range
        dict(pair_c=[0, -1]),
        dict(pair_v=[0, 2]),
        dict(pair_v=[-1, 0]),
        dict(pair_v=[0]),                            # pair_c / pair_v mismatch
        dict(sizes=[-1]),
    ):
        with pytest.raises(RuntimeError):
            call(**bad)
    # an empty pair list returns an empty tensor
    empty = call(pair_c=[], pair_v=[])
    assert empty.dtype == torch.float64 and empty.numel() == 0
    # a good call still works after the refusals
    got = call().cpu().reshape(2, 3, 3)
    assert got[:, 0].tolist() == [[n, n, n], [n, n, n]]
    assert got[:, 1:].abs().sum() == 0
