"""Edge-shape tests for the HIP kernels outside the bucketize suite.

Every input is built on the CPU from a seeded generator and every result
is compared on the CPU with a reference written here in plain fp64 /
int64 torch or Python integers. Inputs are chosen so the comparisons are
exact (multiples of 0.5 or 1/64, small integers, counts); the one
exception, the bf16 rounding case of the Gram kernel, carries a bound
derived from the arithmetic.

Shapes follow the chunking of the bindings: one chunk up to 65 536
elements, 65 539 gives two chunks of 32 770 (no multiple of 4, so the
second chunk's 16-byte vector loads start 8 bytes off), 300 001 several
chunks plus a tail. Lists also carry a zero-length column and contiguous
views with a storage offset (`buf[1:]`, `buf[3:]`)."""

import numpy as np
import pandas as pd
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
NAN = float("nan")
INF = float("inf")

# 1, 3: below one vector; 2047/2053: around one two-vector trip of 256
# threads; 65 539: first length with two chunks (unaligned boundary);
# 300 001: several chunks plus a tail
LENGTHS = [1, 3, 2047, 2053, 65_539, 300_001]


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _dev(x, offset=0):
    """x on the device; offset > 0 gives a contiguous view that starts
    `offset` elements into its storage."""
    if not offset:
        return x.to(DEV)
    buf = torch.zeros(x.numel() + offset, dtype=x.dtype)
    buf[offset:] = x
    v = buf.to(DEV)[offset:]
    assert v.is_contiguous() and v.storage_offset() == offset
    return v


def _same_bits(got, want, what=""):
    """Bit-exact comparison, NaN positions and signed zeros included."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    iv = {4: torch.int32, 8: torch.int64}[got.element_size()]
    assert torch.equal(got.view(iv), want.view(iv)), what


def _eq_nan(got, want):
    """Exact equality where NaN equals NaN."""
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(
        torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)
    )


# ------------------------------------------------------------ shared data
def _grid_data(n, g, dtype, denom):
    """Multiples of 1/denom with |x| <= 64, about 3 % NaN, exact zeros of
    both signs; exact in f32."""
    x = torch.randint(-64 * denom, 64 * denom + 1, (n,), generator=g).to(torch.float64) / denom
    r = torch.rand(n, generator=g)
    x[r < 0.03] = NAN
    x[(r >= 0.03) & (r < 0.06)] = 0.0
    x[(r >= 0.06) & (r < 0.08)] = -0.0
    return x.to(dtype)


def _column_set(seed, denom):
    """(cpu column, storage offset) pairs: all LENGTHS, f32 and f64
    interleaved, a zero-length column of each dtype, offset views, all-NaN."""
    g = torch.Generator().manual_seed(seed)
    f32, f64 = torch.float32, torch.float64
    spec = [(1, f32, 0), (3, f64, 0), (2047, f32, 0), (2053, f64, 0), (65_539, f32, 0),
            (0, f32, 0), (300_001, f32, 0), (65_539, f64, 0), (2053, f32, 1), (0, f64, 0),
            (65_539, f32, 3), (300_001, f64, 0), (3, f32, 1)]
    cols = [(_grid_data(n, g, dt, denom), off) for n, dt, off in spec]
    cols.append((torch.full((2047,), NAN, dtype=f32), 0))
    cols.append((torch.full((5,), NAN, dtype=f64), 0))
    return cols


@pytest.fixture(scope="module")
def half_cols():
    """Multiples of 0.5: moment sums of (x - shift)^k are exact in fp64."""
    cpu = _column_set(41, 2)
    return [c for c, _ in cpu], [_dev(c, off) for c, off in cpu]


@pytest.fixture(scope="module")
def fine_cols():
    """Multiples of 1/64 for the histogram tests."""
    cpu = _column_set(43, 64)
    return [c for c, _ in cpu], [_dev(c, off) for c, off in cpu]


def _shifts(k, seed=47):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-128, 129, (k,), generator=g).to(torch.float64) * 0.5).tolist()


# --------------------------------------------------------------- moments
def _moments_ref(x, shift):
    v = x.to(torch.float64)
    v = v[~torch.isnan(v)]
    d = v - shift
    n = v.numel()
    d2 = d * d
    return torch.tensor([
        float(n), float(d.sum()), float(d2.sum()), float((d2 * d).sum()), float((d2 * d2).sum()),
        float(v.min()) if n else NAN, float(v.max()) if n else NAN,
        float((v == 0).sum()), float((v != torch.trunc(v)).sum()),
    ], dtype=torch.float64)


def _check_moments(got, cpu_cols, shifts):
    got = got.cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(cpu_cols), 9)
    for i, x in enumerate(cpu_cols):
        want = _moments_ref(x, shifts[i] if shifts else 0.0)
        assert _eq_nan(got[i], want), f"column {i} (n={x.numel()}, {x.dtype}): {got[i].tolist()} vs {want.tolist()}"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("shifted", [False, True])
def test_column_moments_all_slots_exact(ext, half_cols, shifted):
    """|x - shift| <= 128 in steps of 0.5, so d^4 is a multiple of 1/16
    below 2^28 and a sum of 300 001 of them stays below 2^53 in units of
    1/16: all nine slots are exact in fp64 in any order of summation.
    All-NaN and zero-length columns give n = 0, zero sums, NaN min/max."""
    cpu, dev = half_cols
    shifts = _shifts(len(cpu)) if shifted else []
    _check_moments(ext.column_moments(dev, shifts), cpu, shifts)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_column_moments_infinities(ext, dtype):
    x = torch.tensor([INF, -INF, 1.5, 0.0, NAN, 2.0, -0.0], dtype=dtype)
    got = ext.column_moments([_dev(x)], []).cpu()[0]
    assert got[0] == 6 and got[5] == -INF and got[6] == INF and got[7] == 2 and got[8] == 1


# Infinities of ONE sign: min / max accumulators that start at +-DBL_MAX
# never reach +inf / -inf (fmin(DBL_MAX, inf) is DBL_MAX).
_ONE_SIGN_INF = [[INF, INF, NAN], [-INF], [INF, 1.0], [-INF, 1.0], [INF] * 2053]


def _same_or_both_nan(got, want):
    """Strict: NaN where the reference has NaN, equal elsewhere, where inf
    equals only inf of the same sign (_eq_nan's nan_to_num would make inf
    and DBL_MAX compare equal)."""
    return torch.equal(torch.isnan(got), torch.isnan(want)) and bool(((got == want) | torch.isnan(want)).all())


def _check_moments_strict(got, cpu_cols, shifts):
    got = got.cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(cpu_cols), 9)
    for i, x in enumerate(cpu_cols):
        want = _moments_ref(x, shifts[i] if shifts else 0.0)
        assert _same_or_both_nan(got[i], want), f"column {i} (n={x.numel()}, {x.dtype}): {got[i].tolist()} vs {want.tolist()}"


def _one_sign_inf_cols(dtype):
    return [torch.tensor(v, dtype=dtype) for v in _ONE_SIGN_INF]


def test_moments_reference_on_one_signed_infinities():
    """What the fp64 reference says: the extremum is the infinity, the odd
    power sums carry its sign, nothing is NaN."""
    ref = [_moments_ref(x, 0.0) for x in _one_sign_inf_cols(torch.float64)]
    assert [(r[0].item(), r[5].item(), r[6].item()) for r in ref] == [
        (2, INF, INF), (1, -INF, -INF), (2, 1.0, INF), (2, -INF, 1.0), (2053, INF, INF)]
    assert ref[3][1:5].tolist() == [-INF, INF, -INF, INF] and ref[2][1:5].tolist() == [INF] * 4
    assert all(r[7] == 0 and r[8] == 0 for r in ref)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_moments_one_signed_infinities(ext, dtype, shifted):
    """n, min, max, zeros and n_frac equal the reference; the power sums
    are +-inf exactly where the reference's are (no NaN arises: only one
    sign is present). Plain and fused kernel."""
    cpu = _one_sign_inf_cols(dtype)
    dev = [_dev(x) for x in cpu]
    shifts = [0.5, -2.0, 1.0, 0.0, 3.5] if shifted else []
    _check_moments_strict(ext.column_moments(dev, shifts), cpu, shifts)
    _check_moments_strict(ext.moments_hll(dev, 12, shifts)[0], cpu, shifts)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_moments_one_signed_infinities_cpu_path(dtype):
    from anovos_amd.ops import stats

    cpu = _one_sign_inf_cols(dtype)
    for shifts in ([0.0] * 5, [0.5, -2.0, 1.0, 0.0, 3.5]):
        _check_moments_strict(stats.column_moments_local(cpu, shifts), cpu, shifts)


def test_merge_moments_global_keeps_infinite_extrema(monkeypatch):
    """A one-rank world (is_dist patched to true, the all-reduce to the
    identity): the merge returns what it was given. Finite and infinite
    extrema survive; only the row with n = 0 has NaN min / max."""
    from anovos_amd.core import dist
    from anovos_amd.ops import stats

    monkeypatch.setattr(dist, "is_dist", lambda: True)
    monkeypatch.setattr(dist, "all_reduce_", lambda t, op="sum": t)
    cols = [torch.tensor(v, dtype=torch.float64) for v in
            ([-INF, 1.0, 2.0], [INF, 1.0], [NAN, NAN], [-1.5, 4.0, 0.0], [INF, NAN], [-INF])]
    local = torch.stack([_moments_ref(x, 0.0) for x in cols])
    assert local[:, 5].tolist()[:2] == [-INF, 1.0] and local[:, 6].tolist()[:2] == [2.0, INF]
    got = stats.merge_moments_global(local.clone())
    assert _same_or_both_nan(got, local), (got.tolist(), local.tolist())
    assert torch.isnan(got[:, 5:7]).any(dim=1).tolist() == [False, False, True, False, False, False]
    assert got[2, 0] == 0


# ------------------------------------------------------------------- HLL
_M32 = (1 << 32) - 1
_M64 = (1 << 64) - 1


def _fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def _splitmix64(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x


def _hll_ref(x, p):
    """HyperLogLog registers in Python integers over the raw bits of the
    non-NaN values: f32 through fmix32, f64 through splitmix64; idx = top
    p bits, rho = leading zeros of the rest + 1, capped at width - p + 1.
    Registers depend on the SET of bit patterns, so duplicates are
    dropped first."""
    v = x[~torch.isnan(x)]
    if x.dtype == torch.float32:
        width, mix, iv = 32, _fmix32, torch.int32
    else:
        width, mix, iv = 64, _splitmix64, torch.int64
    mask = (1 << width) - 1
    regs = [0] * (1 << p)
    for b in torch.unique(v.contiguous().view(iv)).tolist():
        h = mix(b & mask)
        idx = h >> (width - p)
        rem = (h << p) & mask
        rho = min(width - rem.bit_length() + 1, width - p + 1)
        regs[idx] = max(regs[idx], rho)
    return torch.tensor(regs, dtype=torch.int32)


def _hll_inputs():
    g = torch.Generator().manual_seed(53)
    special32 = torch.tensor([NAN, 0.0, -0.0, INF, -INF, 1e-40, 2.5, 2.5, 2.5, -7.0], dtype=torch.float32)
    special64 = torch.tensor([NAN, 0.0, -0.0, INF, -INF, 5e-320, 2.5, 2.5, 2.5, -7.0], dtype=torch.float64)
    a = torch.cat([special32, torch.randn(4989, generator=g)])
    b = torch.cat([special64, torch.randn(4990, generator=g, dtype=torch.float64) * 1e3])
    c = torch.randint(0, 40, (4093,), generator=g).float()  # heavy repeats
    return [
        (a, 0), (b, 0), (c, 1), (torch.full((77,), NAN), 0), (torch.empty(0), 0),
        (torch.randn(2053, generator=g, dtype=torch.float64), 3), (torch.empty(0, dtype=torch.float64), 0),
        (torch.randn(3, generator=g), 0),
    ]


@pytest.mark.parametrize("p", [4, 12, 14])
def test_hll_reference_matches_cpu_path(p):
    """The Python-integer reference agrees with the project's torch path
    on CPU tensors, so it is trusted before any GPU comparison."""
    from anovos_amd.ops import distinct as distinct_ops

    for x, _ in _hll_inputs():
        got = distinct_ops.hll_registers(x, p).to(torch.int32)
        assert torch.equal(got, _hll_ref(x, p)), (x.dtype, x.numel())


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("p", [4, 12, 14])
def test_hll_registers_single_and_multi(ext, p):
    inputs = _hll_inputs()
    dev = [_dev(x, off) for x, off in inputs]
    multi = ext.hll_registers_multi(dev, p).cpu()
    assert multi.dtype == torch.int32 and tuple(multi.shape) == (len(inputs), 1 << p)
    for i, (x, _) in enumerate(inputs):
        want = _hll_ref(x, p)
        assert torch.equal(multi[i], want), f"multi column {i}"
        assert torch.equal(ext.hll_registers(dev[i], p).cpu(), want), f"single column {i}"


@requires_gpu
@pytest.mark.gpu
def test_hll_multi_second_chunk(ext):
    """hll_registers_multi splits a column only above 2^20 rows: 1 048 579
    rows give two chunks of 524 290; values 500.. occur only in the second."""
    g = torch.Generator().manual_seed(59)
    n = (1 << 20) + 3
    x = torch.randint(0, 500, (n,), generator=g).float()
    x[600_000:] += 500.0
    x[-1] = 7777.0
    x[5::1001] = NAN
    got = ext.hll_registers_multi([_dev(x)], 12).cpu()[0]
    assert torch.equal(got, _hll_ref(x, 12))


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("p", [4, 12, 14])
def test_moments_hll_against_references(ext, half_cols, p):
    """The fused kernel against the fp64 moment reference and the integer
    HLL reference (not merely against the two separate kernels)."""
    cpu, dev = half_cols
    shifts = _shifts(len(cpu), seed=61)
    mom, regs = ext.moments_hll(dev, p, shifts)
    _check_moments(mom, cpu, shifts)
    regs = regs.cpu()
    assert regs.dtype == torch.int32 and tuple(regs.shape) == (len(cpu), 1 << p)
    for i, x in enumerate(cpu):
        assert torch.equal(regs[i], _hll_ref(x, p)), f"column {i}"
    mom0, _ = ext.moments_hll(dev, p)
    _check_moments(mom0, cpu, [])


# ------------------------------------------------------------ histograms
def _hist_ref(x, lo, hi, nbins):
    v = x.to(torch.float64)
    v = v[~torch.isnan(v)]
    out = torch.zeros(nbins, dtype=torch.int64)
    if not hi > lo:
        out[0] = v.numel()
        return out
    if v.numel():
        idx = ((v - lo) * (nbins / (hi - lo))).long().clamp_(0, nbins - 1)
        out += torch.bincount(idx, minlength=nbins)
    return out


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("nbins", [1, 2, 512])
def test_column_histograms_edges(ext, fine_cols, nbins):
    """lo / hi strictly inside the data's [-64, 64], so values clamp into
    both edge bins; hi itself is a data value; the last two columns repeat
    the long f32 and f64 columns with hi == lo and hi < lo."""
    cpu, dev = fine_cols
    cpu = cpu + [cpu[6], cpu[11]]
    dev = dev + [dev[6], dev[11]]
    k = len(cpu)
    lo = torch.tensor([-20.25 - 0.5 * i for i in range(k)], dtype=torch.float64)
    hi = torch.tensor([31.5 + 0.25 * i for i in range(k)], dtype=torch.float64)
    lo[-2], hi[-2] = 3.0, 3.0
    lo[-1], hi[-1] = 5.0, -5.0
    got = ext.column_histograms(dev, lo, hi, nbins).cpu()
    assert got.dtype == torch.int64 and tuple(got.shape) == (k, nbins)
    for i, x in enumerate(cpu):
        want = _hist_ref(x, float(lo[i]), float(hi[i]), nbins)
        assert torch.equal(got[i], want), f"column {i} (n={x.numel()}, {x.dtype})"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_column_histograms_infinities_match_cpu_path(ext, dtype):
    """+-inf clamp into the edge bins: +inf counts in the last bin, -inf
    in the first, on the GPU and in the project's torch path alike."""
    from anovos_amd.ops import histogram as hist_ops

    x = torch.tensor([INF, -INF, -INF, 0.0, 1.0, 9.75, 10.0, 1e300 if dtype == torch.float64 else 1e30,
                      NAN, INF, 4.0], dtype=dtype)
    lo = torch.tensor([0.0], dtype=torch.float64)
    hi = torch.tensor([10.0], dtype=torch.float64)
    cpu = hist_ops.column_histograms([x], lo, hi, 8)
    # bin 0: two -inf, 0.0, 1.0; bin 3: 4.0; bin 7: two +inf, 9.75, 10.0, 1e30
    want = torch.tensor([[4, 0, 0, 1, 0, 0, 0, 5]], dtype=torch.int64)
    assert torch.equal(cpu, want)
    assert torch.equal(ext.column_histograms([_dev(x)], lo, hi, 8).cpu(), cpu)


def _bracket_ref(x, lo, hi, nbins):
    """The torch loop of ops.histogram._refine_pass's CPU branch."""
    out = torch.zeros(nbins, dtype=torch.int64)
    v = x.to(torch.float64)
    v = v[~torch.isnan(v)]
    if hi <= lo:
        return out
    v = v[(v >= lo) & (v < hi)]
    if v.numel():
        idx = ((v - lo) * (nbins / (hi - lo))).long().clamp_(0, nbins - 1)
        out += torch.bincount(idx, minlength=nbins)
    return out


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("nbins", [7, 512])
def test_bracket_histograms_edges(ext, fine_cols, dtype, nbins):
    cpu_all, dev_all = fine_cols
    pick = [i for i, c in enumerate(cpu_all) if c.dtype == dtype and c.numel() >= 2053][:3]
    cpu, dev = [cpu_all[i] for i in pick], [dev_all[i] for i in pick]
    # (column, lo, hi): both bounds are data values (lo counted, hi not);
    # unaligned bounds; an empty bracket; a bracket beyond the data
    brackets = [(0, -10.0, 5.0), (1, -10.0, 5.0), (0, -3.2501, 7.7499), (1, 2.0, 2.0), (0, 9.0, 3.0),
                (1, 100.0, 200.0), (2, -64.0, 64.0), (0, 63.0, 64.0 + 1 / 64)]
    ci = torch.tensor([b[0] for b in brackets], dtype=torch.int64)
    lo = torch.tensor([b[1] for b in brackets], dtype=torch.float64)
    hi = torch.tensor([b[2] for b in brackets], dtype=torch.float64)
    got = ext.bracket_histograms(dev, ci, lo, hi, nbins).cpu()
    assert tuple(got.shape) == (len(brackets), nbins)
    for j, (c, l, h) in enumerate(brackets):
        assert torch.equal(got[j], _bracket_ref(cpu[c], l, h, nbins)), f"bracket {j}"
    assert int(got[0].sum()) == int(((cpu[0].double() >= -10.0) & (cpu[0].double() < 5.0)).sum())
    assert int(got[3].sum()) == 0 and int(got[4].sum()) == 0 and int(got[5].sum()) == 0


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("p1bins", [16, 2048])
def test_bracket_histograms_grouped_edges(ext, fine_cols, dtype, p1bins):
    """Brackets are cells of a pass-1 grid of p1bins over [-64, 64] (cell
    width 8 or 1/16, exact): 16 on the first column with the first and the
    last cell among them, none on the second, one on the third. The last
    column has the other dtype and no bracket, so it is never read."""
    cpu_all, dev_all = fine_cols
    pick = [i for i, c in enumerate(cpu_all) if c.dtype == dtype and c.numel() >= 2053][:3]
    other = next(i for i, c in enumerate(cpu_all) if c.dtype != dtype and c.numel() >= 2053)
    cpu = [cpu_all[i] for i in pick]
    dev = [dev_all[i] for i in pick] + [dev_all[other]]
    w = 128.0 / p1bins
    cells0 = list(range(16)) if p1bins == 16 else [0, 1, 2, 640, 641, 700, 1023, 1024, 1025, 1500, 1501, 1777,
                                                  2000, 2045, 2046, 2047]
    brackets = [(0, b) for b in cells0] + [(2, p1bins // 2)]
    bc = torch.tensor([c for c, _ in brackets], dtype=torch.int64)
    lo = torch.tensor([-64.0 + b * w for _, b in brackets], dtype=torch.float64)
    hi = torch.tensor([-64.0 + (b + 1) * w for _, b in brackets], dtype=torch.float64)
    p1lo = torch.full((len(dev),), -64.0, dtype=torch.float64)
    p1scale = torch.full((len(dev),), p1bins / 128.0, dtype=torch.float64)
    got = ext.bracket_histograms_grouped(dev, bc, lo, hi, p1lo, p1scale, p1bins).cpu()
    assert tuple(got.shape) == (len(brackets), 512)
    for j, (c, _) in enumerate(brackets):
        assert torch.equal(got[j], _bracket_ref(cpu[c], float(lo[j]), float(hi[j]), 512)), f"bracket {j}"
    assert int(got[0].sum()) > 0  # the first cell holds the -64.0 values
    # one bracket alone, on the last referenced column
    one = ext.bracket_histograms_grouped(dev, bc[-1:], lo[-1:], hi[-1:], p1lo, p1scale, p1bins).cpu()
    assert torch.equal(one[0], got[-1])


SUB_CELLS = [0, 8, 15]  # first, a middle and the last cell of the 16-cell grid
SUB_DEPTHS = [1, 2, 3]


def _sub_cell_bracket(cell, depth, top):
    """[lo, hi) of width 8 / 512^depth at the bottom or the top of a cell of
    the 16-cell grid over [-64, 64]; every bound is an exact double."""
    w = 8.0 / 512 ** depth
    start = -64.0 + 8.0 * cell
    lo = start + 8.0 - w if top else start
    return lo, lo + w


@pytest.fixture(scope="module")
def sub_cell_column():
    """One f64 column that holds, for every (cell, depth, bottom/top)
    bracket, one value per sub-bin (lo + j * width / 512; for the depth-3
    bracket at the top of the cell ending at 8k these are 8k - j * 2^-33,
    j = 1..512) and values just outside both bounds, hi itself among them;
    shuffled into 2^16 background values and NaNs, which makes two chunks
    with an unaligned boundary. The smallest step, 2^-35, is far above the
    ulp of 64 (2^-46), so every value is exact."""
    g = torch.Generator().manual_seed(53)
    parts = [_grid_data(65_536, g, torch.float64, 64)]
    for cell in SUB_CELLS:
        for depth in SUB_DEPTHS:
            for top in (False, True):
                lo, hi = _sub_cell_bracket(cell, depth, top)
                sub = (hi - lo) / 512
                assert sub == 2.0 ** (3 - 9 * (depth + 1))
                inside = lo + torch.arange(512, dtype=torch.float64) * sub
                outside = torch.tensor([lo - sub, lo - sub / 4, hi, hi + sub / 4, hi + sub], dtype=torch.float64)
                parts += [inside, outside]
    x = torch.cat(parts)
    x = x[torch.randperm(x.numel(), generator=g)]
    assert x.numel() > 65_536
    return x, _dev(x)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("top", [False, True], ids=["bottom", "top"])
@pytest.mark.parametrize("depth", SUB_DEPTHS)
def test_bracket_histograms_grouped_sub_cell(ext, sub_cell_column, fine_cols, depth, top):
    """Brackets 512^depth times narrower than a pass-1 cell, as the second
    and later refinement passes produce them, at the bottom and at the top
    of the first, a middle and the last cell: one launch, one bracket per
    cell. A bracket at the top of a cell ends on the next cell's start (on
    the end of the grid in the last cell) and must still be found through
    its own cell's LUT entry, however narrow it is."""
    cpu, dev = sub_cell_column
    f32 = next(d for c, d in zip(*fine_cols) if c.dtype == torch.float32 and c.numel() >= 2053)
    bounds = [_sub_cell_bracket(cell, depth, top) for cell in SUB_CELLS]
    bc = torch.zeros(len(bounds), dtype=torch.int64)
    lo = torch.tensor([b[0] for b in bounds], dtype=torch.float64)
    hi = torch.tensor([b[1] for b in bounds], dtype=torch.float64)
    p1lo = torch.full((2,), -64.0, dtype=torch.float64)
    p1scale = torch.full((2,), 16 / 128.0, dtype=torch.float64)
    # the f32 column carries no bracket and is never read
    got = ext.bracket_histograms_grouped([dev, f32], bc, lo, hi, p1lo, p1scale, 16).cpu()
    assert tuple(got.shape) == (len(bounds), 512)
    for j, (l, h) in enumerate(bounds):
        want = _bracket_ref(cpu, l, h, 512)
        assert int(want.min()) >= 1 and int(want.sum()) >= 512  # one planted value per sub-bin
        assert torch.equal(got[j], want), f"cell {SUB_CELLS[j]}: {int(got[j].sum())} counted, {int(want.sum())} expected"


# ----------------------------------------------------------- code counts
def _codes(n, size, g):
    """int32 codes in [0, size) with nulls and out-of-range values mixed in."""
    c = torch.randint(0, max(size, 1), (n,), generator=g).to(torch.int32)
    r = torch.rand(n, generator=g)
    c[r < 0.02] = -1
    c[(r >= 0.02) & (r < 0.03)] = size
    c[(r >= 0.03) & (r < 0.04)] = size + 5
    c[(r >= 0.04) & (r < 0.05)] = -(2 ** 31)
    if n >= 2 and size >= 1:
        c[0], c[-1] = 0, size - 1
    return c


def _code_counts_ref(c, size):
    valid = (c >= 0) & (c < size)
    cnt = torch.bincount(c[valid].long(), minlength=size) if size else torch.zeros(0, dtype=torch.int64)
    return cnt, int(c.numel() - valid.sum())


def _check_code_counts_multi(ext, cols, offs, sizes):
    got = ext.code_counts_multi([_dev(c, o) for c, o in zip(cols, offs)], sizes).cpu()
    assert got.dtype == torch.int64 and got.numel() == sum(s + 1 for s in sizes)
    pos = 0
    for i, (c, s) in enumerate(zip(cols, sizes)):
        cnt, nulls = _code_counts_ref(c, s)
        assert torch.equal(got[pos:pos + s], cnt), f"column {i} (size {s})"
        assert int(got[pos + s]) == nulls, f"column {i} (size {s}) null slot"
        pos += s + 1


@requires_gpu
@pytest.mark.gpu
def test_code_counts_multi_mixed_dictionary_sizes(ext):
    """One launch with a dictionary too large for LDS next to small ones:
    the small columns still stage their counters in LDS, which the
    launcher must size from them (it used to give them none). 16 383 is
    the last size that stages (16 384 slots with the null slot), 16 384
    the first that counts in global memory."""
    g = torch.Generator().manual_seed(67)
    sizes = [3, 20_000, 0, 16_383, 16_384]
    lens = [300_001, 65_539, 2053, 65_539, 65_539]
    cols = [_codes(n, s, g) for n, s in zip(lens, sizes)]
    _check_code_counts_multi(ext, cols, [0, 0, 1, 3, 0], sizes)
    # the same without any staging column, and with staging columns only
    _check_code_counts_multi(ext, [cols[1], cols[4]], [0, 0], [20_000, 16_384])
    _check_code_counts_multi(ext, [cols[0], cols[3]], [0, 0], [3, 16_383])


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_code_counts_multi_lengths(ext, n):
    g = torch.Generator().manual_seed(71 + n)
    sizes = [3, 40, 1]
    cols = [_codes(n, s, g) for s in sizes]
    _check_code_counts_multi(ext, cols, [0, 1, 3], sizes)
    # a zero-length column among them
    _check_code_counts_multi(ext, cols + [torch.empty(0, dtype=torch.int32)], [3, 0, 1, 0], sizes + [7])


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 16_384, 16_385])
def test_code_counts_sizes(ext, size):
    """16 384 is the last size counted in LDS, 16 385 the first counted in
    global memory; out-of-range codes are dropped."""
    g = torch.Generator().manual_seed(73)
    for n, off in [(300_001, 0), (65_539, 1), (3, 0)]:
        c = _codes(n, size, g)
        got = ext.code_counts(_dev(c, off), size).cpu()
        assert torch.equal(got, _code_counts_ref(c, size)[0]), (n, size)


@requires_gpu
@pytest.mark.gpu
def test_cat_value_counts_id_column_next_to_small_dictionary():
    """Frame level: an all-distinct string column (dictionary > 16 383)
    and a 3-value column go through one fused launch."""
    from anovos_amd.core.frame import AnovosFrame
    from anovos_amd.ops import groupby

    rng = np.random.default_rng(79)
    n = 20_000
    ids = np.array([f"id{i:05d}" for i in range(n)], dtype=object)
    small = rng.choice(["x", "y", "z"], n).astype(object)
    ids[rng.choice(n, 90, replace=False)] = None
    small[rng.choice(n, 400, replace=False)] = None
    pdf = pd.DataFrame({"id": ids, "c": small})
    cpu_f = AnovosFrame.from_pandas(pdf, device="cpu")
    gpu_f = cpu_f.to_device("cuda:0")
    assert len(cpu_f.col("id").dictionary) > 16_384  # counted in global memory
    assert len(cpu_f.col("c").dictionary) <= 4  # staged in LDS
    want = groupby.cat_value_counts(cpu_f, ["id", "c"])
    got = groupby.cat_value_counts(gpu_f, ["id", "c"])
    for c in ["id", "c"]:
        assert gpu_f.col(c).dictionary == cpu_f.col(c).dictionary
        assert torch.equal(got[c].cpu(), want[c].cpu()), c
        # per value against pandas (an ingest placeholder entry may count 0)
        by_value = {v: k for v, k in zip(gpu_f.col(c).dictionary, got[c].tolist()) if k}
        assert by_value == pdf[c].value_counts().to_dict(), c
    assert int(got["id"].sum()) == n - 90 and int(got["id"].max()) == 1
    assert gpu_f.col("id").cache["nulls_local"] == 90
    assert gpu_f.col("c").cache["nulls_local"] == 400


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_label_counts_multi_lengths_sizes_labels(ext, n):
    """f32 binned values: NaN -> slot 0, v -> trunc(v) + 1 clamped into
    [0, slots - 1] (negative, beyond the slots, 1e30, +-inf). int32 codes:
    0 .. slots - 2 count in their own slot, everything else in the last.
    Any non-zero label byte is an event."""
    g = torch.Generator().manual_seed(83 + n)
    sizes = [1, 2, 12, 8192]
    fcols, icols = [], []
    for s in sizes:
        x = torch.randint(-3, s + 3, (n,), generator=g).float() + 0.5 * torch.randint(0, 2, (n,), generator=g)
        r = torch.rand(n, generator=g)
        x[r < 0.03] = NAN
        x[(r >= 0.03) & (r < 0.04)] = 1e30
        x[(r >= 0.04) & (r < 0.05)] = -1e30
        x[(r >= 0.05) & (r < 0.06)] = INF
        x[(r >= 0.06) & (r < 0.07)] = -INF
        x[(r >= 0.07) & (r < 0.08)] = -0.5
        fcols.append(x)
        icols.append(_codes(n, s - 1, g))
    cols = [c for pair in zip(fcols, icols) for c in pair]
    offs = [0, 1, 3, 0, 1, 0, 0, 3]
    all_sizes = [s for s in sizes for _ in range(2)]
    dev = [_dev(c, o) for c, o in zip(cols, offs)]
    labels = [
        torch.tensor([0, 1, 7, 255], dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)],
        torch.zeros(n, dtype=torch.uint8),
        torch.ones(n, dtype=torch.uint8),
    ]
    slots_of = []
    for c, s in zip(cols, all_sizes):
        if c.dtype == torch.float32:
            t = torch.where(torch.isnan(c), torch.full_like(c, -1.0), torch.trunc(c)).double() + 1.0
            slots_of.append(t.clamp_(0, s - 1).long())
        else:
            slots_of.append(torch.where((c >= 0) & (c < s - 1), c, torch.full_like(c, s - 1)).long())
    for lab in labels:
        got = ext.label_counts_multi(dev, _dev(lab), all_sizes).cpu()
        assert got.numel() == 2 * sum(all_sizes)
        pos = 0
        for i, (sl, s) in enumerate(zip(slots_of, all_sizes)):
            tot = torch.bincount(sl, minlength=s)
            evt = torch.bincount(sl[lab != 0], minlength=s)
            assert torch.equal(got[pos:pos + s], tot), f"column {i} totals"
            assert torch.equal(got[pos + s:pos + 2 * s], evt), f"column {i} events"
            pos += 2 * s


# -------------------------------------------------------------- row nulls
def _null_matrix(k, n, dtype, g):
    if dtype == torch.int32:
        m = torch.randint(0, 5, (k, n), generator=g).to(torch.int32)
        m[torch.rand(k, n, generator=g) < 0.2] = -1
        return m, m == -1
    m = torch.randn(k, n, generator=g).to(dtype)
    m[torch.rand(k, n, generator=g) < 0.2] = NAN
    return m, torch.isnan(m)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 8191, 8192, 8193, 8196, 16_387])
def test_row_null_counts_shapes(ext, n):
    """Row chunks of 8192 (a chunk length off a multiple of 4 takes the
    LDS fallback), column chunks of 64 (65 and 130 columns take the atomic
    path). Columns are rows of one matrix, so for odd n they start off a
    16-byte boundary. The kernel adds into a non-zero `out`."""
    g = torch.Generator().manual_seed(89 + n)
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    layouts = [[(f32, 1)], [(f32, 64)], [(f32, 65)], [(f32, 130)], [(f64, 65)], [(i32, 65)], [(i32, 64)],
               [(f32, 3), (f64, 2), (i32, 2)]]
    before = (torch.arange(n, dtype=torch.int32) % 7) + 1
    for layout in layouts:
        cols, ref = [], torch.zeros(n, dtype=torch.int32)
        for dtype, k in layout:
            m, nulls = _null_matrix(k, n, dtype, g)
            md = m.to(DEV)
            cols += [md[i] for i in range(k)]
            ref += nulls.sum(0).to(torch.int32)
        # interleave the dtypes of a mixed list
        order = torch.randperm(len(cols), generator=g).tolist()
        out = before.clone().to(DEV)
        ext.row_null_counts_num([cols[i] for i in order], out)
        assert torch.equal(out.cpu(), before + ref), layout


# ------------------------------------------------------------ elementwise
def _value_cols(seed):
    """(cpu column, offset): LENGTHS in f32, three f64, a zero-length and
    two offset views; NaN, +-inf and -0.0 mixed in."""
    g = torch.Generator().manual_seed(seed)
    f32, f64 = torch.float32, torch.float64
    spec = [(n, f32, 0) for n in LENGTHS] + [(3, f64, 0), (65_539, f64, 0), (2053, f64, 1), (0, f32, 0),
                                             (2053, f32, 1), (65_539, f32, 3)]
    # dtypes interleaved in the list
    spec = [spec[i] for i in [0, 6, 1, 2, 7, 3, 9, 4, 8, 5, 10, 11]]
    out = []
    for n, dt, off in spec:
        x = torch.randn(n, generator=g, dtype=torch.float64).to(dt)
        r = torch.rand(n, generator=g)
        x[r < 0.03] = NAN
        x[(r >= 0.03) & (r < 0.04)] = INF
        x[(r >= 0.04) & (r < 0.05)] = -INF
        x[(r >= 0.05) & (r < 0.06)] = -0.0
        out.append((x, off))
    return out


@requires_gpu
@pytest.mark.gpu
def test_scale_columns_bit_exact(ext):
    """The kernel widens x to f64, computes (x - a) * b in f64 with a and b
    as given, and rounds the product to f32 once, for f32 and f64 columns
    alike: a subtraction followed by a multiplication, nothing to
    contract."""
    cols = _value_cols(97)
    a = torch.tensor([0.1 * (i + 1) for i in range(len(cols))], dtype=torch.float64)
    b = torch.tensor([(-1.0) ** i / (3.0 + i) for i in range(len(cols))], dtype=torch.float64)
    outs = ext.scale_columns([_dev(c, o) for c, o in cols], a, b)
    for i, (c, _) in enumerate(cols):
        want = ((c.double() - a[i]) * b[i]).float()
        assert outs[i].dtype == torch.float32
        _same_bits(outs[i], want, f"column {i}")


@requires_gpu
@pytest.mark.gpu
def test_fill_nan_columns_bit_exact(ext):
    """The f64 fill 0.1 is not representable in f32: an f32 column gets it
    rounded to f32. -0.0 and +-inf stay untouched."""
    cols = _value_cols(101)
    fill = torch.tensor([0.1 + i for i in range(len(cols))], dtype=torch.float64)
    outs = ext.fill_nan_columns([_dev(c, o) for c, o in cols], fill)
    for i, (c, _) in enumerate(cols):
        want = torch.where(torch.isnan(c), fill[i].to(c.dtype), c)
        _same_bits(outs[i], want, f"column {i}")
        assert not bool(torch.isnan(outs[i]).any())


def _code_cols(seed, sizes):
    """(codes, offset, size) over LENGTHS, a zero-length column and two
    offset views; sizes cycle through `sizes`."""
    g = torch.Generator().manual_seed(seed)
    spec = [(n, 0) for n in LENGTHS] + [(0, 0), (2053, 1), (65_539, 3)]
    out = []
    for j, (n, off) in enumerate(spec):
        s = sizes[j % len(sizes)]
        c = torch.randint(0, s, (n,), generator=g).to(torch.int32)
        c[torch.rand(n, generator=g) < 0.05] = -1
        if n >= 3:
            c[0], c[1], c[-1] = 0, -1, s - 1
        out.append((c, off, s))
    return out


@requires_gpu
@pytest.mark.gpu
def test_fill_code_columns_lengths(ext):
    cols = _code_cols(103, [4, 70_000])
    fills = [7 + i for i in range(len(cols))]
    outs = ext.fill_code_columns([_dev(c, o) for c, o, _ in cols], fills)
    for i, (c, _, _) in enumerate(cols):
        want = torch.where(c == -1, torch.full_like(c, fills[i]), c)
        assert outs[i].dtype == torch.int32 and torch.equal(outs[i].cpu(), want), f"column {i}"


@requires_gpu
@pytest.mark.gpu
def test_lut_apply_f32_and_i32(ext):
    """LUT sizes 1, 5 and 70 000 side by side in one call (each column
    must read its own slice of the flattened LUTs); code -1 -> NaN / -1;
    codes 0 and size - 1 present; the LUTs themselves hold NaN / -1."""
    cols = _code_cols(107, [1, 5, 70_000])
    g = torch.Generator().manual_seed(109)
    dev = [_dev(c, o) for c, o, _ in cols]
    fl, il = [], []
    for _, _, s in cols:
        f = torch.randn(s, generator=g)
        i = torch.randint(-1, 1000, (s,), generator=g).to(torch.int32)
        if s > 1:
            f[s // 2], i[s // 2] = NAN, -1
            f[0], f[-1] = -0.0, INF
        fl.append(f)
        il.append(i)
    fo = ext.lut_apply_f32(dev, fl)
    io = ext.lut_apply_i32(dev, il)
    for j, (c, _, _) in enumerate(cols):
        idx = c.clamp(min=0).long()
        wf = torch.where(c < 0, torch.full((c.numel(),), NAN), fl[j][idx])
        wi = torch.where(c < 0, torch.full_like(c, -1), il[j][idx])
        assert fo[j].dtype == torch.float32 and io[j].dtype == torch.int32
        _same_bits(fo[j], wf, f"f32 column {j}")
        assert torch.equal(io[j].cpu(), wi), f"i32 column {j}"
    # a LUT that is all NaN / all -1
    one = ext.lut_apply_f32(dev[:1], [torch.tensor([NAN])])[0].cpu()
    assert bool(torch.isnan(one).all())
    assert torch.equal(ext.lut_apply_i32(dev[:1], [torch.tensor([-1], dtype=torch.int32)])[0].cpu(),
                       torch.full_like(cols[0][0], -1))


def _with_neighbours(x, bounds):
    """Plant, near the front of x, each bound rounded to x's dtype and its
    neighbours on both sides."""
    npdt = np.float32 if x.dtype == torch.float32 else np.float64
    vals = []
    for b in bounds:
        r = npdt(b)
        vals += [float(r), float(np.nextafter(r, npdt(np.inf))), float(np.nextafter(r, npdt(-np.inf)))]
    k = min(len(vals), x.numel())
    x[:k] = torch.tensor(vals[:k], dtype=torch.float64).to(x.dtype)
    return x


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_outlier_clamp_columns_bounds(ext, mode):
    """Bounds 0.1 and -0.3 are not representable in f32, so for f32
    columns the kernel's nextafter adjustment decides for the planted
    neighbours; the verdict must be that of comparing x as fp64 with the
    fp64 bound. NaN bound = unbounded side; lo > hi flags values on both
    sides (low wins the replacement); NaN data is never counted or
    replaced. Mode 1 writes the bound rounded to the column's dtype."""
    bounds = [(-0.3, 0.1), (NAN, 0.1), (-0.3, NAN), (0.1, -0.3), (-0.3, 0.1)]
    cols = [(_with_neighbours(c, [-0.3, 0.1]), o) for c, o in _value_cols(113)]
    lo = torch.tensor([bounds[i % len(bounds)][0] for i in range(len(cols))], dtype=torch.float64)
    hi = torch.tensor([bounds[i % len(bounds)][1] for i in range(len(cols))], dtype=torch.float64)
    counts, outs = ext.outlier_clamp_columns([_dev(c, o) for c, o in cols], lo, hi, mode)
    counts = counts.cpu()
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (len(cols), 2)
    assert len(outs) == (len(cols) if mode else 0)
    for i, (c, _) in enumerate(cols):
        xd = c.double()
        l, h = float(lo[i]), float(hi[i])
        low = (xd < l) if l == l else torch.zeros_like(xd, dtype=torch.bool)
        high = (xd > h) if h == h else torch.zeros_like(xd, dtype=torch.bool)
        assert counts[i].tolist() == [int(low.sum()), int(high.sum())], f"column {i} ({c.dtype}, n={c.numel()})"
        if mode:
            lrep = torch.tensor(NAN if mode == 2 else l, dtype=torch.float64).to(c.dtype)
            hrep = torch.tensor(NAN if mode == 2 else h, dtype=torch.float64).to(c.dtype)
            want = torch.where(low, lrep, torch.where(high, hrep, c))
            _same_bits(outs[i], want, f"column {i}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("ncut", [0, 1, 9, 33])
def test_bucketize_columns_int_output(ext, ncut):
    """Multiples of 0.25 against cutoffs that are multiples of 0.25 too
    (values sit on cutoffs), one duplicated cutoff, +-inf, f64 columns."""
    g = torch.Generator().manual_seed(127)
    spec = [(n, torch.float32, 0) for n in LENGTHS] + [(65_539, torch.float64, 0), (0, torch.float32, 0),
                                                       (2053, torch.float64, 1), (65_539, torch.float32, 3)]
    spec = [spec[i] for i in [0, 6, 1, 2, 8, 3, 7, 4, 9, 5]]
    cols = []
    for n, dt, off in spec:
        x = (torch.randint(-20, 21, (n,), generator=g).to(torch.float64) * 0.25).to(dt)
        r = torch.rand(n, generator=g)
        x[r < 0.03] = NAN
        x[(r >= 0.03) & (r < 0.04)] = INF
        x[(r >= 0.04) & (r < 0.05)] = -INF
        cols.append((x, off))
    cuts = torch.arange(ncut, dtype=torch.float64) * 0.25 - 4.0 if ncut else torch.empty(0, dtype=torch.float64)
    if ncut >= 3:
        cuts[2] = cuts[1]
    outs = ext.bucketize_columns([_dev(c, o) for c, o in cols], [cuts.to(DEV) for _ in cols])
    for i, (c, _) in enumerate(cols):
        want = torch.bucketize(c.double(), cuts, right=False).to(torch.int32)
        want = torch.where(torch.isnan(c), torch.full_like(want, -1), want)
        assert outs[i].dtype == torch.int32 and torch.equal(outs[i].cpu(), want), f"column {i}"


# ------------------------------------------------------------------ Gram
def _int_matrix(k, n, g, device="cpu"):
    """Integers in [-2, 2] with about 1 % NaN as f32 [k, n], integer means
    in [-2, 2], and the exact centered Gram (NaN -> 0 after centering)."""
    x = torch.randint(-2, 3, (k, n), generator=g, device=device).float()
    nan = torch.rand(k, n, generator=g, device=device) < 0.01
    means = torch.randint(-2, 3, (k,), generator=g, device=device).float()
    xc = torch.where(nan, torch.zeros_like(x), x - means[:, None])
    x[nan] = NAN
    if device == "cpu":
        ref = (xc.long() @ xc.long().T).double()
    else:
        xd = xc.double()
        ref = xd @ xd.T  # integers below 2^21: exact in fp64
    return x, means, ref


def _check_gram_exact(ext, x, means, ref, what):
    got = ext.centered_gram_bf16([x[i] for i in range(x.shape[0])], means)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    got = got.double()
    assert torch.equal(got, got.T), f"{what}: not symmetric"
    assert torch.equal(got.cpu(), ref.cpu()), f"{what}: max abs diff {float((got.cpu() - ref.cpu()).abs().max())}"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 16, 17, 37, 160, 161, 208, 209, 225])
def test_centered_gram_exact_small_integers(ext, k):
    """Centered values are integers with |v| <= 4: exact in bf16, every
    product exact, every partial sum an integer below 2^21 and so exact
    in fp32 in any order. k <= 160 runs the single-read kernel with 14
    pair accumulators, 161..208 the one with 23, k >= 209 the
    pair-parallel kernel; n covers less than one 32-row step, exactly
    one, and lengths off a multiple of 32 and of 128."""
    g = torch.Generator().manual_seed(131 + k)
    for n in [1, 7, 31, 32, 33, 1027]:
        x, means, ref = _int_matrix(k, n, g)
        _check_gram_exact(ext, x.to(DEV), means.to(DEV), ref, f"k={k} n={n}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "3", "7"])
def test_centered_gram_exact_forced_row_chunks(ext, monkeypatch, chunks):
    monkeypatch.setenv("ANOVOS_GRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(137)
    for k in [37, 161]:
        x, means, ref = _int_matrix(k, 1027, g)
        _check_gram_exact(ext, x.to(DEV), means.to(DEV), ref, f"k={k} chunks={chunks}")


@requires_gpu
@pytest.mark.gpu
def test_centered_gram_exact_pair_parallel_two_row_chunks(ext):
    """k = 209, n = 131 075: the pair-parallel kernel with row_chunks = 2
    (about 110 MB, built on the device). Rows of one matrix with an odd
    row length, so every second column starts off a 16-byte boundary."""
    g = torch.Generator(device=DEV).manual_seed(139)
    x, means, ref = _int_matrix(209, 131_075, g, device=DEV)
    _check_gram_exact(ext, x, means, ref, "k=209 n=131075")


@requires_gpu
@pytest.mark.gpu
def test_centered_gram_bf16_rounding_bound(ext):
    """Real-valued data: the reference rounds (x - mean_f32) to bf16 with
    round-to-nearest-even, as the kernel does, and forms the Gram in
    fp64. What is left is the fp32 summation of n exact products:
    |err_ij| <= n * 2^-23 * sum|a b| <= n * 2^-23 * sqrt(ref_ii ref_jj)
    (Cauchy-Schwarz). Truncation to bf16 instead of round-to-nearest-even
    would bias the diagonal by about 2^-9 relative, far above this."""
    g = torch.Generator().manual_seed(149)
    k, n = 37, 1027
    x = torch.stack([torch.randn(n, generator=g) * (1 + i % 5) + i for i in range(k)])
    x[torch.rand(k, n, generator=g) < 0.01] = NAN
    means = torch.nanmean(x, dim=1)
    xc = torch.nan_to_num(x - means[:, None], nan=0.0).to(torch.bfloat16).double()
    ref = xc @ xc.T
    d = torch.sqrt(torch.diagonal(ref))
    bound = n * 2.0 ** -23 * d[:, None] * d[None, :]
    got = ext.centered_gram_bf16([r for r in x.to(DEV)], means.to(DEV)).cpu().double()
    err = (got - ref).abs()
    print(f"max err / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), f"max err / bound = {float((err / bound).max())}"
    assert torch.equal(got, got.T)


# ------------------------------------------------------------ validation
@requires_gpu
@pytest.mark.gpu
def test_bindings_reject_strided_views(ext):
    """A strided view would be read as if dense: every binding that takes
    data_ptr() refuses it, alone or behind a dense column."""
    f64 = torch.float64
    strided = [torch.arange(64, dtype=torch.float32, device=DEV)[::2], torch.arange(64, dtype=f64, device=DEV)[::2]]
    dense = torch.arange(32, dtype=torch.float32, device=DEV)
    codes = torch.zeros(64, dtype=torch.int32, device=DEV)[::2]
    assert not strided[0].is_contiguous() and not codes.is_contiguous()
    cuts = torch.tensor([1.0, 2.0], dtype=f64)
    b0 = torch.tensor([0], dtype=torch.int64)
    lo1, hi1 = torch.tensor([0.0], dtype=f64), torch.tensor([10.0], dtype=f64)

    def zeros(ts):
        return torch.zeros(len(ts), dtype=f64)

    def tens(ts):
        return torch.full((len(ts),), 10.0, dtype=f64)

    calls = {
        "column_histograms": lambda ts: ext.column_histograms(ts, zeros(ts), tens(ts), 4),
        "bracket_histograms": lambda ts: ext.bracket_histograms(ts, b0, lo1, hi1, 4),
        "bracket_histograms_grouped": lambda ts: ext.bracket_histograms_grouped(
            ts, b0, lo1, hi1, zeros(ts), tens(ts), 16),
        "bucketize_columns": lambda ts: ext.bucketize_columns(ts, [cuts for _ in ts]),
        "bucketize_columns_float": lambda ts: ext.bucketize_columns_float(ts, [cuts for _ in ts]),
        "hll_registers_multi": lambda ts: ext.hll_registers_multi(ts, 4),
        "scale_columns": lambda ts: ext.scale_columns(ts, zeros(ts), tens(ts)),
        "fill_nan_columns": lambda ts: ext.fill_nan_columns(ts, zeros(ts)),
    }
    for name, call in calls.items():
        call([dense])  # the arguments are otherwise valid
        for t in strided:
            with pytest.raises(RuntimeError, match="contiguous"):
                call([t])
        with pytest.raises(RuntimeError, match="contiguous"):
            call([dense, strided[0]])
        with pytest.raises(RuntimeError, match="same device"):
            call([dense, dense.cpu()])
    ext.hll_registers(dense, 4)
    for t in strided:
        with pytest.raises(RuntimeError, match="contiguous"):
            ext.hll_registers(t, 4)
    lut_f, lut_i = torch.zeros(1), torch.zeros(1, dtype=torch.int32)
    dense_codes = torch.zeros(32, dtype=torch.int32, device=DEV)
    ext.lut_apply_f32([dense_codes], [lut_f])
    ext.lut_apply_i32([dense_codes], [lut_i])
    for cols, luts in [([codes], 1), ([dense_codes, codes], 2)]:
        with pytest.raises(RuntimeError, match="contiguous"):
            ext.lut_apply_f32(cols, [lut_f] * luts)
        with pytest.raises(RuntimeError, match="contiguous"):
            ext.lut_apply_i32(cols, [lut_i] * luts)


def _column_list_calls(ext):
    """binding name -> call(ts) for every binding that takes a column list;
    all other arguments are valid for len(ts) columns of 32 rows. The
    bool says whether the binding wants int32 code columns."""
    f64 = torch.float64
    cuts = torch.tensor([1.0, 2.0], dtype=f64)
    b0 = torch.tensor([0], dtype=torch.int64)
    lo1, hi1 = torch.tensor([0.0], dtype=f64), torch.tensor([10.0], dtype=f64)

    def zeros(ts):
        return torch.zeros(len(ts), dtype=f64)

    def tens(ts):
        return torch.full((len(ts),), 10.0, dtype=f64)

    def label(ts):
        return torch.zeros(32, dtype=torch.uint8, device=ts[0].device if ts else "cpu")

    def out(ts):
        return torch.zeros(32, dtype=torch.int32, device=ts[0].device if ts else "cpu")

    floats = {
        "column_moments": lambda ts: ext.column_moments(ts, []),
        "moments_hll": lambda ts: ext.moments_hll(ts, 4),
        "column_histograms": lambda ts: ext.column_histograms(ts, zeros(ts), tens(ts), 4),
        "bracket_histograms": lambda ts: ext.bracket_histograms(ts, b0, lo1, hi1, 4),
        "bracket_histograms_grouped": lambda ts: ext.bracket_histograms_grouped(
            ts, b0, lo1, hi1, zeros(ts), tens(ts), 16),
        "bucketize_columns": lambda ts: ext.bucketize_columns(ts, [cuts for _ in ts]),
        "bucketize_columns_float": lambda ts: ext.bucketize_columns_float(ts, [cuts for _ in ts]),
        "bucketize_columns_float_counts": lambda ts: ext.bucketize_columns_float_counts(ts, [cuts for _ in ts]),
        "bucketize_label_counts": lambda ts: ext.bucketize_label_counts(
            ts, [cuts for _ in ts], label(ts), [4 for _ in ts]),
        "hll_registers_multi": lambda ts: ext.hll_registers_multi(ts, 4),
        "scale_columns": lambda ts: ext.scale_columns(ts, zeros(ts), tens(ts)),
        "fill_nan_columns": lambda ts: ext.fill_nan_columns(ts, zeros(ts)),
        "outlier_clamp_columns": lambda ts: ext.outlier_clamp_columns(ts, zeros(ts), tens(ts), 1),
        "centered_gram_bf16": lambda ts: ext.centered_gram_bf16(ts, torch.zeros(len(ts))),
        "row_null_counts_num": lambda ts: ext.row_null_counts_num(ts, out(ts)),
    }
    codes = {
        "fill_code_columns": lambda ts: ext.fill_code_columns(ts, [7 for _ in ts]),
        "lut_apply_f32": lambda ts: ext.lut_apply_f32(ts, [torch.zeros(3) for _ in ts]),
        "lut_apply_i32": lambda ts: ext.lut_apply_i32(ts, [torch.zeros(3, dtype=torch.int32) for _ in ts]),
        "code_counts_multi": lambda ts: ext.code_counts_multi(ts, [3 for _ in ts]),
        "pair_code_counts": lambda ts: ext.pair_code_counts(ts, [3 for _ in ts], [0], [len(ts) - 1]),
        "label_counts_multi": lambda ts: ext.label_counts_multi(ts, label(ts), [4 for _ in ts]),
    }
    return [(n, c, False) for n, c in floats.items()] + [(n, c, True) for n, c in codes.items()]


def test_bindings_reject_host_and_empty_lists():
    """No binding lets an empty column list or host tensors past its first
    check: the refusal comes before any device call, so this runs without
    a GPU (with one, a missing check would hand host pointers to a kernel)."""
    from anovos_amd.ops import backend

    ext = backend.hip_ext()
    if ext is None:
        pytest.skip("HIP extension not built")
    host_f = [torch.arange(32, dtype=torch.float32), torch.ones(32, dtype=torch.float32)]
    host_c = [torch.zeros(32, dtype=torch.int32), torch.ones(32, dtype=torch.int32)]
    calls = _column_list_calls(ext)
    assert len(calls) == 21
    for name, call, wants_codes in calls:
        with pytest.raises(RuntimeError, match=name + ": no columns"):
            call([])
        for ts in ([host_c[0]], host_c) if wants_codes else ([host_f[0]], host_f):
            with pytest.raises(RuntimeError, match=name + ": device columns required"):
                call(ts)
    # the two bindings that take one column
    with pytest.raises(RuntimeError, match="hll_registers: device columns required"):
        ext.hll_registers(host_f[0], 4)
    with pytest.raises(RuntimeError, match="code_counts: device columns required"):
        ext.code_counts(host_c[0], 3)


@requires_gpu
@pytest.mark.gpu
def test_bindings_reject_short_parameter_arrays(ext):
    """Per-column and per-bracket arrays one entry short, a column index
    past the list, and a host `label` / `out` next to device columns are
    refused; the same call with the argument right succeeds."""
    f64 = torch.float64
    ts = [torch.arange(32, dtype=torch.float32, device=DEV), torch.ones(32, dtype=torch.float32, device=DEV)]
    cs = [torch.zeros(32, dtype=torch.int32, device=DEV), torch.ones(32, dtype=torch.int32, device=DEV)]
    for name, call, wants_codes in _column_list_calls(ext):
        call(cs if wants_codes else ts)  # every call of the table is valid as it stands

    def vec(k, v=0.0):
        return torch.full((k,), v, dtype=f64)

    cuts = torch.tensor([1.0, 2.0], dtype=f64)
    lut_f, lut_i = torch.zeros(3), torch.zeros(3, dtype=torch.int32)
    bidx = torch.tensor([0, 1], dtype=torch.int64)
    label = torch.zeros(32, dtype=torch.uint8, device=DEV)
    out = torch.zeros(32, dtype=torch.int32, device=DEV)
    # name -> call(k): k entries in the array under test; 2 is right
    short = {
        "scale a": lambda k: ext.scale_columns(ts, vec(k), vec(2, 10.0)),
        "scale b": lambda k: ext.scale_columns(ts, vec(2), vec(k, 10.0)),
        "fill_nan fill": lambda k: ext.fill_nan_columns(ts, vec(k)),
        "hist lo": lambda k: ext.column_histograms(ts, vec(k), vec(2, 10.0), 4),
        "hist hi": lambda k: ext.column_histograms(ts, vec(2), vec(k, 10.0), 4),
        "outlier lo": lambda k: ext.outlier_clamp_columns(ts, vec(k), vec(2, 10.0), 1),
        "outlier hi": lambda k: ext.outlier_clamp_columns(ts, vec(2), vec(k, 10.0), 0),
        "bracket lo": lambda k: ext.bracket_histograms(ts, bidx, vec(k), vec(2, 10.0), 4),
        "bracket hi": lambda k: ext.bracket_histograms(ts, bidx, vec(2), vec(k, 10.0), 4),
        "grouped lo": lambda k: ext.bracket_histograms_grouped(ts, bidx, vec(k), vec(2, 10.0), vec(2), vec(2, 1.6), 16),
        "grouped hi": lambda k: ext.bracket_histograms_grouped(ts, bidx, vec(2), vec(k, 10.0), vec(2), vec(2, 1.6), 16),
        "grouped p1lo": lambda k: ext.bracket_histograms_grouped(ts, bidx, vec(2), vec(2, 10.0), vec(k), vec(2, 1.6), 16),
        "grouped p1scale": lambda k: ext.bracket_histograms_grouped(ts, bidx, vec(2), vec(2, 10.0), vec(2), vec(k, 1.6), 16),
        "luts f32": lambda k: ext.lut_apply_f32(cs, [lut_f] * k),
        "luts i32": lambda k: ext.lut_apply_i32(cs, [lut_i] * k),
        "cutoffs int": lambda k: ext.bucketize_columns(ts, [cuts] * k),
        "cutoffs float": lambda k: ext.bucketize_columns_float(ts, [cuts] * k),
        "cutoffs counts": lambda k: ext.bucketize_columns_float_counts(ts, [cuts] * k),
        "cutoffs label": lambda k: ext.bucketize_label_counts(ts, [cuts] * k, label, [4, 4]),
        "sizes bucketize_label": lambda k: ext.bucketize_label_counts(ts, [cuts] * 2, label, [4] * k),
        "sizes label_counts": lambda k: ext.label_counts_multi(cs, label, [4] * k),
        "sizes code_counts": lambda k: ext.code_counts_multi(cs, [3] * k),
        "sizes pair_counts": lambda k: ext.pair_code_counts(cs, [3] * k, [0], [1]),
        "fills": lambda k: ext.fill_code_columns(cs, [7] * k),
        "gram means": lambda k: ext.centered_gram_bf16(ts, torch.zeros(k)),
    }
    for name, call in short.items():
        call(2)
        with pytest.raises(RuntimeError, match="has 1 entries, expected 2"):
            call(1)
    # a bracket that names a column past the list
    ext.bracket_histograms(ts, torch.tensor([1]), vec(1), vec(1, 10.0), 4)
    with pytest.raises(RuntimeError, match="colidx"):
        ext.bracket_histograms(ts, torch.tensor([2]), vec(1), vec(1, 10.0), 4)
    # host label / out next to device columns
    ext.label_counts_multi(cs, label, [4, 4])
    with pytest.raises(RuntimeError, match="label"):
        ext.label_counts_multi(cs, label.cpu(), [4, 4])
    ext.bucketize_label_counts(ts, [cuts] * 2, label, [4, 4])
    with pytest.raises(RuntimeError, match="label"):
        ext.bucketize_label_counts(ts, [cuts] * 2, label.cpu(), [4, 4])
    ext.row_null_counts_num(ts, out)
    with pytest.raises(RuntimeError, match="out"):
        ext.row_null_counts_num(ts, out.cpu())
    assert out.cpu().tolist() == [0] * 32  # no NaN in ts, nothing added
