"""The row quadratic-form kernel (K26, ops/hip/row_quadform.hip).

`row_quadform_bf16x2(cols, shift, scale, W)` returns f32 [n]:

    z_j = isnan(x_j) ? 0 : (x_j - shift_j) * scale_j       (f32)
    y_i = sum_j W[i][j] z_j                                 i < r
    d2  = sum_i y_i^2

with every operand split into bf16 hi + lo and y accumulated as
wh.zh + wh.zl + wl.zh in fp32 on the matrix cores.

Layout under test: columns padded to 32 (one MFMA k-step), W's rows to 16;
persistent blocks stage 64-row slabs, full slabs on an unguarded
prefetching path (two slabs per trip, a drain for an odd count), the one
partial slab at the end of the frame on a guarded one; W's rows beyond what
LDS holds go in windows, one launch each, that add into the result.
ANOVOS_ROWQUAD_BLOCKS forces the grid, so small inputs reach the
multi-slab paths (1 block: every slab in one loop; 3 blocks: ranges of
differing length).

Exact tests: with small integer data every operand is exact in bf16 (the
lo planes are zero) and, once the sum over i of (|W| @ |z|)_i^2 is below
2^24, every fp32 partial sum is an integer below 2^24 - exact in any order -
so the result must equal the int64 reference bit for bit. The lo-plane
tests use z with exactly 16 significant bits and a W that picks one
column, so y = z_j exactly only if both planes land where they belong.
"""

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
NAN = float("nan")
W_ROW_NNZ = 24  # non-zeros per row of W in the dense exact tests (see _int_case)


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _sparsify(W, nnz, g):
    """keep at most `nnz` entries per row, at random positions"""
    order = torch.rand(W.shape, generator=g).argsort(dim=1).argsort(dim=1)
    return W * (order < nnz)


def _int_case(k, n, r, g, nnz=W_ROW_NNZ):
    """x f32 [k, n]: integers in [-2, 2], 1-30 % NaN per column; integer
    shifts in [-2, 2]; scales in {0.5, 1, 2}; W [r, k] in {-1, 0, 1} with
    at most `nnz` non-zeros per row. |z| <= 8, so a component is at most
    8 * nnz = 192 and the sum of 160 squares at most 5.9e6 < 2^24."""
    x = torch.randint(-2, 3, (k, n), generator=g).float()
    rate = 0.01 + 0.29 * torch.rand(k, 1, generator=g)
    x[torch.rand(k, n, generator=g) < rate] = NAN
    shift = torch.randint(-2, 3, (k,), generator=g).float()
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (k,), generator=g)]
    W = _sparsify(torch.randint(-1, 2, (r, k), generator=g).float(), nnz, g)
    return x, shift, scale, W


def _int_reference(x, shift, scale, W):
    """int64 d2 [n]; asserts the 2^24 condition that makes fp32 exact.
    z is a multiple of 1/2: the reference works on 2z."""
    z2 = torch.where(torch.isnan(x), torch.zeros_like(x), (x - shift[:, None]) * scale[:, None] * 2)
    assert torch.equal(z2, z2.round())
    z2 = z2.long()
    Wl = W.long()
    bound = ((Wl.abs() @ z2.abs()) ** 2).sum(0)  # of 4 d2
    assert int(bound.max()) < 4 * 2 ** 24, "reference outside the exact fp32 range"
    d2x4 = ((Wl @ z2) ** 2).sum(0)
    return d2x4.double() / 4  # d2 is a multiple of 1/4 below 2^24: exact in f32


def _run(ext, x, shift, scale, W):
    xd = x.to(DEV)
    cols = [xd[i] for i in range(xd.shape[0])]
    out = ext.row_quadform_bf16x2(cols, shift.to(DEV), scale.to(DEV), W.to(DEV))
    assert out.dtype == torch.float32 and tuple(out.shape) == (x.shape[1],)
    return out.cpu()


def _assert_exact(got, ref, what):
    diff = (got.double() - ref).abs()
    assert torch.equal(got.double(), ref), (
        f"{what}: {int((diff > 0).sum())} of {ref.numel()} rows differ, max {float(diff.max())}, "
        f"first at row {int((diff > 0).nonzero()[0]) if (diff > 0).any() else -1}")


NS = [1, 15, 16, 17, 63, 64, 65, 129, 516]


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("k", [1, 16, 17, 37, 150, 160])
def test_exact_small_integers(ext, monkeypatch, k, blocks):
    """every n of NS (no slab, one slab, several slabs with and without a
    tail) x r in {1, 16, 17, k}, bit for bit"""
    monkeypatch.setenv("ANOVOS_ROWQUAD_BLOCKS", str(blocks))
    g = torch.Generator().manual_seed(2600 + k)
    for r in sorted({min(r, k) for r in (1, 16, 17, k)}):
        for n in NS:
            x, shift, scale, W = _int_case(k, n, r, g)
            ref = _int_reference(x, shift, scale, W)
            _assert_exact(_run(ext, x, shift, scale, W), ref, f"k={k} r={r} n={n} blocks={blocks}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("k", [37, 150])
def test_exact_lo_planes(ext, k):
    """z = odd integers in [2^8, 2^16): 16 significant bits, so zh and zl
    are both non-zero and zh + zl = z. W has one row with a single +-1 at
    column j: y = z_j exactly, out = f32(z_j * z_j)."""
    g = torch.Generator().manual_seed(2601)
    n = 129
    x = (torch.randint(2 ** 7, 2 ** 15, (k, n), generator=g) * 2 + 1).float()
    assert int(x.min()) >= 2 ** 8 and int(x.max()) < 2 ** 16
    shift, scale = torch.zeros(k), torch.ones(k)
    for j in sorted({0, 7, 8, 15, 16, 31, 32, k - 1}):
        for sign in (1.0, -1.0):
            W = torch.zeros(1, k)
            W[0, j] = sign
            got = _run(ext, x, shift, scale, W)
            want = x[j] * x[j]  # f32 product, rounded once
            assert torch.equal(got, want), (
                f"k={k} j={j} sign={sign}: {int((got != want).sum())} rows differ, "
                f"max {float((got.double() - want.double()).abs().max())}")


@requires_gpu
@pytest.mark.gpu
def test_exact_lo_plane_of_w(ext):
    """the mirror image: W carries the 16-bit value, z = +-1 picks it"""
    g = torch.Generator().manual_seed(2602)
    k, n = 37, 65
    w = (torch.randint(2 ** 7, 2 ** 15, (k,), generator=g) * 2 + 1).float()
    for j in (0, 7, 8, 31, 32, 36):
        x = torch.zeros(k, n)
        x[j] = torch.where(torch.rand(n, generator=g) < 0.5, 1.0, -1.0)
        W = torch.zeros(3, k)
        W[1] = w
        got = _run(ext, x, torch.zeros(k), torch.ones(k), W)
        want = (w[j] * w[j]).expand(n)
        assert torch.equal(got, want), f"j={j}: max {float((got - want).abs().max())}"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [None, 3])
@pytest.mark.parametrize("k", [161, 256])
def test_windowed_path_exact(ext, monkeypatch, k, blocks):
    """k = r beyond one window of W's rows: several launches that add into
    the result. W has at most 4 non-zeros per row: a component is at most
    32, the sum of 256 squares at most 2.6e5 < 2^24."""
    if blocks is not None:
        monkeypatch.setenv("ANOVOS_ROWQUAD_BLOCKS", str(blocks))
    g = torch.Generator().manual_seed(2603 + k)
    for n in (65, 516):
        x, shift, scale, W = _int_case(k, n, k, g, nnz=4)
        ref = _int_reference(x, shift, scale, W)
        _assert_exact(_run(ext, x, shift, scale, W), ref, f"k=r={k} n={n} blocks={blocks}")


@requires_gpu
@pytest.mark.gpu
def test_argument_checks(ext):
    def cols(k, n=8):
        return [torch.zeros(n, device=DEV) for _ in range(k)]

    def vec(k):
        return torch.ones(k, device=DEV)

    with pytest.raises(RuntimeError, match="at most 256"):
        ext.row_quadform_bf16x2(cols(257), vec(257), vec(257), torch.zeros(4, 257, device=DEV))
    with pytest.raises(RuntimeError, match="W has 5 columns, expected 4"):
        ext.row_quadform_bf16x2(cols(4), vec(4), vec(4), torch.zeros(2, 5, device=DEV))
    with pytest.raises(RuntimeError, match="W has 5 rows"):
        ext.row_quadform_bf16x2(cols(4), vec(4), vec(4), torch.zeros(5, 4, device=DEV))
    with pytest.raises(RuntimeError, match="W has 0 rows"):
        ext.row_quadform_bf16x2(cols(4), vec(4), vec(4), torch.zeros(0, 4, device=DEV))
    with pytest.raises(RuntimeError, match="2-D"):
        ext.row_quadform_bf16x2(cols(4), vec(4), vec(4), torch.zeros(4, device=DEV))
    with pytest.raises(RuntimeError, match="2-D floating-point"):
        ext.row_quadform_bf16x2(cols(4), vec(4), vec(4),
                                torch.zeros(2, 4, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="shift has 3 entries, expected 4"):
        ext.row_quadform_bf16x2(cols(4), vec(3), vec(4), torch.zeros(2, 4, device=DEV))
    with pytest.raises(RuntimeError, match="on the columns' device"):
        ext.row_quadform_bf16x2(cols(4), vec(4), vec(4), torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="expected float32"):
        ext.row_quadform_bf16x2([c.double() for c in cols(4)], vec(4), vec(4),
                                torch.zeros(2, 4, device=DEV))
    empty = ext.row_quadform_bf16x2(cols(4, 0), vec(4), vec(4), torch.zeros(2, 4, device=DEV))
    assert empty.dtype == torch.float32 and tuple(empty.shape) == (0,)
    # a float64 W is converted
    out = ext.row_quadform_bf16x2(cols(4), vec(4), vec(4),
                                  torch.ones(2, 4, device=DEV, dtype=torch.float64))
    assert torch.equal(out.cpu(), torch.full((8,), 32.0))


def _bound(z, W32, k, z_err=0.0):
    """(ref, bound) per row, fp64, of the derived bound:
    eps_i = (3 * 2^-18 + 3 * k_pad * 2^-24 + z_err) * sum_j |W_ij| |z_j|
    |got - ref| <= sum_i (2 |y_i| eps_i + eps_i^2) + r * 2^-24 * ref
    eps_i: 2^-18 for each operand's split residual and for the dropped
    lo.lo term, the fp32 summation term over 3 * k_pad products, and z_err
    where `z` is not the kernel's own f32 z but a more exact one."""
    k_pad = (k + 31) // 32 * 32
    z, W = z.double(), W32.double()
    y = W @ z                       # [r, n]
    ref = (y * y).sum(0)
    eps = (3 * 2.0 ** -18 + 3 * k_pad * 2.0 ** -24 + z_err) * (W.abs() @ z.abs())
    bound = (2 * y.abs() * eps + eps * eps).sum(0) + W.shape[0] * 2.0 ** -24 * ref
    return ref, bound


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 32, 150, 256])
def test_derived_bound(ext, monkeypatch, k):
    """real-valued data, z ~ 3 N(0,1), W ~ N(0,1), r = k, 5 % NaN; fp64
    reference on the f32 z formed by the same subtract and multiply. A
    hi-only kernel exceeds this bound by a median factor of 18 at k = 16
    and 8 at k = 32; a CPU simulation of the scheme stays below 0.24."""
    monkeypatch.setenv("ANOVOS_ROWQUAD_BLOCKS", "3")
    g = torch.Generator().manual_seed(2610 + k)
    n = 333
    scale = 0.5 + 2 * torch.rand(k, generator=g)
    shift = 10 * torch.randn(k, generator=g)
    x = 3 * torch.randn(k, n, generator=g) / scale[:, None] + shift[:, None]
    x[torch.rand(k, n, generator=g) < 0.05] = NAN
    W = torch.randn(k, k, generator=g)
    z32 = torch.where(torch.isnan(x), torch.zeros_like(x), (x - shift[:, None]) * scale[:, None])
    ref, bound = _bound(z32, W, k)
    got = _run(ext, x, shift, scale, W).double()
    ratio = (got - ref).abs() / bound
    print(f"row_quadform derived bound k={k}: max |got-ref|/bound = {float(ratio.max()):.4f}, "
          f"median {float(ratio.median()):.4f}")
    assert bool((ratio <= 1).all()), (
        f"k={k}: {int((ratio > 1).sum())} rows beyond the bound, worst ratio {float(ratio.max())}")


@requires_gpu
@pytest.mark.gpu
def test_deterministic_and_null_rows(ext):
    g = torch.Generator().manual_seed(2620)
    k, n = 150, 1000
    x = torch.randn(k, n, generator=g)
    x[torch.rand(k, n, generator=g) < 0.05] = NAN
    x[:, 17] = NAN
    x[:, 999] = NAN
    shift, scale = torch.randn(k, generator=g), 0.5 + torch.rand(k, generator=g)
    W = torch.randn(k, k, generator=g)
    a = _run(ext, x, shift, scale, W)
    b = _run(ext, x, shift, scale, W)
    assert torch.equal(a, b), "the same call returned different bits"
    assert float(a[17]) == 0.0 and float(a[999]) == 0.0, "an all-null row is at the mean: d2 = 0"
    assert bool((a[:17] > 0).all())


@requires_gpu
@pytest.mark.gpu
def test_f64_columns_centred_before_downcast(ext):
    """mahalanobis_d2 on f64 columns, one offset by 1e8 (f32 spacing there
    is 8): centred in f64 first, the result stays within the derived bound
    of the fp64 reference on the same f32 z."""
    import numpy as np

    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.ops.mahalanobis import WhiteningModel, mahalanobis_d2

    g = torch.Generator().manual_seed(2630)
    k, n = 16, 200
    x = torch.randn(k, n, generator=g, dtype=torch.float64) * 3
    mean = torch.zeros(k, dtype=torch.float64)
    mean[3] = 1e8
    mean[5] = -250.0
    x = x + mean[:, None]
    x[torch.rand(k, n, generator=g) < 0.05] = NAN
    sd = 0.5 + 2 * torch.rand(k, generator=g, dtype=torch.float64)
    W = torch.randn(k, k, generator=g, dtype=torch.float64)
    names = [f"c{i}" for i in range(k)]
    # columns 0..7 f64, 8..15 f32 (the f32 ones keep their shift in the kernel)
    colmap = {}
    for i, c in enumerate(names):
        t = x[i] if i < 8 else x[i].float()
        colmap[c] = Column(c, "double" if i < 8 else "float", t.to(DEV))
    frame = AnovosFrame(colmap, DEV)
    model = WhiteningModel(names, mean.numpy(), sd.numpy(), W.numpy(), k)
    got = mahalanobis_d2(frame, names, model)
    assert got.dtype == torch.float32 and got.device.type == "cuda"
    scale32 = (1.0 / sd).float()
    z32 = torch.empty(k, n)
    for i in range(k):
        if i < 8:
            z32[i] = ((x[i] - mean[i]).float() - 0.0) * scale32[i]
        else:
            z32[i] = (x[i].float() - mean[i].float()) * scale32[i]
    z32 = torch.where(torch.isnan(z32), torch.zeros_like(z32), z32)
    ref, bound = _bound(z32, W.float(), k)
    ratio = (got.cpu().double() - ref).abs() / bound
    print(f"mahalanobis_d2 f64 columns: max |got-ref|/bound = {float(ratio.max()):.4f}")
    assert bool((ratio <= 1).all()), f"worst ratio {float(ratio.max())}"
    # and the signal of the offset column survived: against the exact fp64
    # z, which the f32 z misses by three roundings (the cast of x - mean,
    # the scale, the product), 2^-24 relative each
    z64 = torch.where(torch.isnan(x), torch.zeros_like(x), (x - mean[:, None]) / sd[:, None])
    z64[8:] = torch.where(torch.isnan(x[8:]), torch.zeros_like(x[8:]),
                          (x[8:].float().double() - mean[8:, None]) / sd[8:, None])
    ref64, bound64 = _bound(z64, W.float(), k, z_err=3 * 2.0 ** -24)
    ratio64 = (got.cpu().double() - ref64).abs() / bound64
    assert bool((ratio64 <= 1).all()), f"worst ratio against exact z {float(ratio64.max())}"
