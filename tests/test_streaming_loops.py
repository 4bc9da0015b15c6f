"""The streaming loops of anovos_kernels.hip at the sizes where their
pipelines can go wrong.

The loops take 16-byte vectors, 256 threads a trip. The deepest pipeline
(bucketize_label_counts: two vectors a trip and the next trip's two in
flight) looks U = 4 vectors ahead; the others look one or two ahead. A
single-chunk column of n = 4 v + r rows has v vectors and an r-row scalar
tail, so v runs over the boundaries of one trip and of U trips and r over
{0, 1, 3}. Chunk starts that are only 4-byte aligned come from 200 003 rows
in 3 columns (4 chunks of 50 001 rows) and from views that start 1 or 3
elements into their storage.

Every input is a view into a larger buffer whose elements before and after
it hold a value the kernel would count or that would change a sum, so a
read outside the view shows in a count, a sum or an extremum. Outputs are
allocated by the bindings with exactly the input's length and are compared
whole and bit for bit. References are plain torch / numpy on the CPU and
integer arithmetic written here."""

import numpy as np
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
NAN = float("nan")
INF = float("inf")

U = 4
VECS = [0, 1, 255, 256, 257, 256 * U - 1, 256 * U, 256 * U + 1, 256 * (U + 1) + 3]
SINGLE = [4 * v + r for v in VECS for r in (0, 1, 3)]  # 0 .. 5135 rows, one chunk each
MULTI_N, MULTI_COLS, MULTI_PER = 200_003, 3, 50_001
PS = [4, 12, 14]
_M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _guarded(x, guard, j=0):
    """x as a contiguous device view that starts 1 or 3 elements into a
    buffer filled with `guard` (5 more guard elements behind it)."""
    pre = (1, 3)[j % 2]
    buf = torch.full((pre + x.numel() + 5,), guard, dtype=x.dtype)
    buf[pre:pre + x.numel()] = x
    v = buf.to(DEV)[pre:pre + x.numel()]
    assert v.is_contiguous() and v.storage_offset() == pre
    return v


def _same_bits(got, want, what=""):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    iv = {4: torch.int32, 8: torch.int64}[got.element_size()]
    assert torch.equal(got.view(iv), want.view(iv)), what


def _values(n, g):
    """Multiples of 0.25 in [-5, 5] with NaN, +-inf and -0.0 mixed in."""
    x = (torch.randint(-20, 21, (n,), generator=g).to(torch.float64) * 0.25).float()
    r = torch.rand(n, generator=g)
    x[r < 0.03] = NAN
    x[(r >= 0.03) & (r < 0.04)] = INF
    x[(r >= 0.04) & (r < 0.05)] = -INF
    x[(r >= 0.05) & (r < 0.06)] = -0.0
    return x


def _codes(n, size, g):
    c = torch.randint(0, size, (n,), generator=g).to(torch.int32)
    c[torch.rand(n, generator=g) < 0.05] = -1
    return c


def _column_sets(make, seed):
    """[(name, [cpu columns])]: every single-chunk length in one list, and
    the multi-chunk shape."""
    g = torch.Generator().manual_seed(seed)
    return [("single", [make(n, g) for n in SINGLE]),
            ("multi", [make(MULTI_N, g) for _ in range(MULTI_COLS)])]


@pytest.fixture(scope="module")
def value_sets():
    return _column_sets(_values, 211)


@pytest.fixture(scope="module")
def code_sets():
    return _column_sets(lambda n, g: _codes(n, 6, g), 223)


# ------------------------------------------------- the rho formula, no GPU
def _clz32(x):
    """Leading zeros of uint32 values held in uint64 (0 -> 32)."""
    return 32 - np.frexp(x.astype(np.float64))[1]


def _rho_capped(h, p):
    rem = (h << np.uint64(p)) & np.uint64(_M32)
    return np.where(rem == 0, 32 - p + 1, np.minimum(_clz32(rem) + 1, 32 - p + 1))


def _rho_guard_bit(h, p):
    rem = (h << np.uint64(p)) & np.uint64(_M32)
    return _clz32(rem | np.uint64(1 << (p - 1))) + 1


@pytest.mark.parametrize("p", PS)
def test_rho_guard_bit_equals_capped_rho(p):
    """rho = clz((h << p) | 1 << (p - 1)) + 1 is the capped rho for every
    h: checked on the low 2^24 values, a 2^24-value stride sample of the
    whole range, and the edge patterns of every register index (remainder
    0, each single remainder bit, all remainder bits)."""
    w = 32 - p
    low = np.arange(1 << 24, dtype=np.uint64)
    strided = (low << np.uint64(8)) | np.uint64(0xA5)
    idx = np.arange(1 << p, dtype=np.uint64) << np.uint64(w)
    edges = [idx, idx | np.uint64((1 << w) - 1)] + [idx | np.uint64(1 << j) for j in range(w)]
    for h in [low, strided, np.concatenate(edges), np.array([0, _M32], dtype=np.uint64)]:
        assert np.array_equal(_rho_guard_bit(h, p), _rho_capped(h, p))
    assert int(_rho_guard_bit(np.array([0], dtype=np.uint64), p)[0]) == w + 1


# ------------------------------------------------------- elementwise kernels
@requires_gpu
@pytest.mark.gpu
def test_scale_and_fill_nan(ext, value_sets):
    """Scaling is (float)(((double)x - a) * b) with a and b as given;
    the fill is rounded to the column's dtype."""
    for name, cols in value_sets:
        k = len(cols)
        dev = [_guarded(c, NAN if j % 3 else 7.0, j) for j, c in enumerate(cols)]
        a = torch.tensor([0.1 * (i + 1) for i in range(k)], dtype=torch.float64)
        b = torch.tensor([(-1.0) ** i / (3.0 + i) for i in range(k)], dtype=torch.float64)
        fill = torch.tensor([0.1 + i for i in range(k)], dtype=torch.float64)
        scaled = ext.scale_columns(dev, a, b)
        filled = ext.fill_nan_columns(dev, fill)
        for i, c in enumerate(cols):
            _same_bits(scaled[i], ((c.double() - a[i]) * b[i]).float(), f"{name} scale {i}")
            _same_bits(filled[i], torch.where(torch.isnan(c), fill[i].float(), c), f"{name} fill {i}")


@requires_gpu
@pytest.mark.gpu
def test_fill_code_and_lut_apply(ext, code_sets):
    g = torch.Generator().manual_seed(227)
    for name, cols in code_sets:
        dev = [_guarded(c, (-1, 5)[j % 2], j) for j, c in enumerate(cols)]
        fills = [7 + i for i in range(len(cols))]
        fl = [torch.randn(6, generator=g) for _ in cols]
        il = [torch.randint(-1, 1000, (6,), generator=g).to(torch.int32) for _ in cols]
        for f in fl:
            f[0], f[3], f[5] = -0.0, NAN, INF
        fo = ext.fill_code_columns(dev, fills)
        lf = ext.lut_apply_f32(dev, fl)
        li = ext.lut_apply_i32(dev, il)
        for i, c in enumerate(cols):
            idx = c.clamp(min=0).long()
            assert torch.equal(fo[i].cpu(), torch.where(c == -1, torch.full_like(c, fills[i]), c)), f"{name} {i}"
            _same_bits(lf[i], torch.where(c < 0, torch.full((c.numel(),), NAN), fl[i][idx]), f"{name} f32 {i}")
            assert torch.equal(li[i].cpu(), torch.where(c < 0, torch.full_like(c, -1), il[i][idx])), f"{name} i32 {i}"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_outlier_clamp(ext, value_sets, mode):
    """Guards of 100 and -100 lie outside the bounds: one read of them and
    a count is off."""
    for name, cols in value_sets:
        k = len(cols)
        dev = [_guarded(c, (100.0, -100.0)[j % 2], j) for j, c in enumerate(cols)]
        lo = torch.tensor([-2.3 + 0.01 * i for i in range(k)], dtype=torch.float64)
        hi = torch.tensor([1.6 - 0.01 * i for i in range(k)], dtype=torch.float64)
        counts, outs = ext.outlier_clamp_columns(dev, lo, hi, mode)
        counts = counts.cpu()
        for i, c in enumerate(cols):
            low, high = c.double() < lo[i], c.double() > hi[i]
            assert counts[i].tolist() == [int(low.sum()), int(high.sum())], f"{name} column {i}"
            if mode:
                lrep = (torch.tensor(NAN) if mode == 2 else lo[i]).float()
                hrep = (torch.tensor(NAN) if mode == 2 else hi[i]).float()
                _same_bits(outs[i], torch.where(low, lrep, torch.where(high, hrep, c)), f"{name} column {i}")


def _bin_labels(c, cuts):
    lab = (torch.bucketize(c.double(), cuts, right=False) + 1).float()
    return torch.where(torch.isnan(c), torch.full_like(lab, NAN), lab)


def _cuts(ncut):
    return torch.arange(ncut, dtype=torch.float64) * (8.0 / ncut) - 4.0


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("ncut", [9, 16, 33])
def test_bucketize_float_with_and_without_counts(ext, value_sets, ncut):
    """9 cutoffs: registers and private counters; 16: registers and shared
    counters; 33: LDS binary search. The guard 4.5 lies in the top bin."""
    cuts = _cuts(ncut)
    for name, cols in value_sets:
        dev = [_guarded(c, (4.5, NAN)[j % 2], j) for j, c in enumerate(cols)]
        outs, counts = ext.bucketize_columns_float_counts(dev, [cuts for _ in cols])
        plain = ext.bucketize_columns_float(dev, [cuts for _ in cols])
        counts = counts.cpu()
        for i, c in enumerate(cols):
            want = _bin_labels(c, cuts)
            _same_bits(outs[i], want, f"{name} counting column {i}")
            _same_bits(plain[i], want, f"{name} plain column {i}")
            slot = torch.nan_to_num(want, nan=0.0).long()
            assert torch.equal(counts[i], torch.bincount(slot, minlength=ncut + 2)), f"{name} counts {i}"


# ------------------------------------------------------------ count kernels
def _label(n, g):
    return torch.tensor([0, 1, 7, 255], dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)]


def _check_label_counts(got, slots, lab, sizes, what):
    pos = 0
    for i, (sl, s) in enumerate(zip(slots, sizes)):
        assert torch.equal(got[pos:pos + s], torch.bincount(sl, minlength=s)), f"{what} column {i} totals"
        assert torch.equal(got[pos + s:pos + 2 * s], torch.bincount(sl[lab != 0], minlength=s)), f"{what} column {i} events"
        pos += 2 * s
    assert pos == got.numel()


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("ncut", [9, 20])
def test_bucketize_label_counts(ext, ncut):
    """Columns of a call share their length, so one call per length; the
    label is a guarded view too (guard 1 = an event). 9 cutoffs take the
    private counters with two vectors a trip, 20 the shared ones."""
    g = torch.Generator().manual_seed(229)
    cuts = _cuts(ncut)
    sizes = [ncut + 3] * 3
    for n in [m for m in SINGLE if m] + [MULTI_N]:
        cols = [_values(n, g) for _ in range(3)]
        lab = _label(n, g)
        dev = [_guarded(c, (4.5, NAN, -9.0)[j], j) for j, c in enumerate(cols)]
        got = ext.bucketize_label_counts(dev, [cuts] * 3, _guarded(lab, 1, 1), sizes).cpu()
        slots = [torch.nan_to_num(_bin_labels(c, cuts) + 1, nan=0.0).long() for c in cols]
        _check_label_counts(got, slots, lab, sizes, f"n={n}")


@requires_gpu
@pytest.mark.gpu
def test_label_counts_multi(ext):
    g = torch.Generator().manual_seed(233)
    sizes = [12, 7, 12]
    for n in [m for m in SINGLE if m] + [MULTI_N]:
        binned = [torch.where(torch.isnan(v), v, torch.trunc(v.abs() * 2)) for v in (_values(n, g), _values(n, g))]
        cols = [binned[0], _codes(n, 6, g), binned[1]]
        lab = _label(n, g)
        dev = [_guarded(c, (3.0, 2, NAN)[j], j) for j, c in enumerate(cols)]
        got = ext.label_counts_multi(dev, _guarded(lab, 1, 0), sizes).cpu()
        slots = []
        for c, s in zip(cols, sizes):
            if c.dtype == torch.float32:
                t = torch.where(torch.isnan(c), torch.full_like(c, -1.0), torch.trunc(c)).double() + 1.0
                slots.append(t.clamp_(0, s - 1).long())
            else:
                slots.append(torch.where((c >= 0) & (c < s - 1), c, torch.full_like(c, s - 1)).long())
        _check_label_counts(got, slots, lab, sizes, f"n={n}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("masks", [False, True])
def test_code_counts_multi(ext, code_sets, masks):
    for name, cols in code_sets:
        dev = [_guarded(c, (0, -1)[j % 2], j) for j, c in enumerate(cols)]
        sizes = [6] * len(cols)
        got = ext.code_counts_multi(dev, sizes, masks) if masks else ext.code_counts_multi(dev, sizes)
        got = (got[0] if masks else got).cpu()
        for i, c in enumerate(cols):
            slot = torch.where((c >= 0) & (c < 6), c, torch.full_like(c, 6)).long()
            assert torch.equal(got[7 * i:7 * i + 7], torch.bincount(slot, minlength=7)), f"{name} column {i}"


@requires_gpu
@pytest.mark.gpu
def test_column_histograms(ext, value_sets):
    """8 bins over [-4, 4]: bin = floor(x + 4) clamped; +-inf land in the
    edge bins, NaN nowhere. The guard 0.5 is an in-range value."""
    for name, cols in value_sets:
        dev = [_guarded(c, 0.5, j) for j, c in enumerate(cols)]
        lo = torch.full((len(cols),), -4.0, dtype=torch.float64)
        got = ext.column_histograms(dev, lo, -lo, 8).cpu()
        for i, c in enumerate(cols):
            v = c[~torch.isnan(c)].double()
            b = torch.clamp(v + 4.0, 0.0, 7.0).long()
            assert torch.equal(got[i], torch.bincount(b, minlength=8)), f"{name} column {i}"


# ----------------------------------------------------- fused moments + HLL
def _fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(_M32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(_M32)
    x ^= x >> np.uint64(16)
    return x


def _unmix32(h):
    """Inverse of fmix32 on Python integers (both multipliers are odd)."""
    h ^= h >> 16
    h = (h * pow(0xC2B2AE35, -1, 1 << 32)) & _M32
    h ^= (h >> 13) ^ (h >> 26)
    h = (h * pow(0x85EBCA6B, -1, 1 << 32)) & _M32
    h ^= h >> 16
    return h


def _planted_values():
    """f32 values whose hash has, for some p in PS, an all-zero remainder
    (rho at its cap) or a remainder with its top bit set (rho = 1). The bit
    patterns come from inverting fmix32 and are checked through fmix32."""
    bits = []
    for p in PS:
        w = 32 - p
        for idx in range(0, 1 << p, max(1, (1 << p) // 16)):
            for h in (idx << w, (idx << w) | (1 << (w - 1)), (idx << w) | 1):
                b = _unmix32(h)
                assert int(_fmix32(np.array([b]))[0]) == h
                if (b & 0x7F800000) != 0x7F800000:  # a finite f32
                    bits.append(b)
    v = torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())
    h = _fmix32(np.array(bits))
    for p in PS:
        rem = (h << np.uint64(p)) & np.uint64(_M32)
        assert (rem == 0).sum() >= 4 and (rem >> np.uint64(31)).sum() >= 4
    return v


def _hll_ref(x, p):
    v = x[~torch.isnan(x)].numpy().view(np.uint32)
    h = _fmix32(v)
    regs = np.zeros(1 << p, dtype=np.int64)
    np.maximum.at(regs, (h >> np.uint64(32 - p)).astype(np.int64), _rho_capped(h, p))
    return torch.from_numpy(regs).to(torch.int32)


def _moments_ref(x, shift):
    v = x.double()
    v = v[~torch.isnan(v)]
    d = v - shift
    n = v.numel()
    d2 = d * d
    return torch.tensor([
        float(n), float(d.sum()), float(d2.sum()), float((d2 * d).sum()), float((d2 * d2).sum()),
        float(v.min()) if n else NAN, float(v.max()) if n else NAN,
        float((v == 0).sum()), float((v != torch.trunc(v)).sum()),
    ], dtype=torch.float64)


def _eq_nan(got, want):
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(
        torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


def _half_values(n, g):
    """Multiples of 0.5 with |x| <= 64 (all nine slots are exact in fp64 in
    any order), NaN, zeros of both signs."""
    x = (torch.randint(-128, 129, (n,), generator=g).to(torch.float64) * 0.5).float()
    r = torch.rand(n, generator=g)
    x[r < 0.03] = NAN
    x[(r >= 0.03) & (r < 0.06)] = 0.0
    x[(r >= 0.06) & (r < 0.08)] = -0.0
    return x


@pytest.fixture(scope="module")
def half_sets():
    return _column_sets(_half_values, 239), _planted_values()


def _mask_words(nulls, nchunks):
    """(words, written) of the null lane masks of a bool row vector: chunk
    of `per` rows from s, vector i = offset // 4, group i >> 6, four words a
    group, bit i & 63 of word c = row s + 4 i + c; tail rows set bits 0..2
    of word 0 of the next group."""
    n = nulls.size
    per = -(-n // nchunks)
    wpc = 4 * ((((per // 4) + 63) // 64) + 1)
    r = np.arange(n, dtype=np.int64)
    chunk = r // per
    s = chunk * per
    nv = (np.minimum(n, s + per) - s) // 4
    j = r - s
    vec = j < 4 * nv
    word = np.where(vec, chunk * wpc + 4 * ((j // 4) >> 6) + (j & 3), chunk * wpc + 4 * ((nv + 63) >> 6))
    bit = np.where(vec, (j // 4) & 63, j - 4 * nv).astype(np.uint64)
    words = np.zeros(nchunks * wpc, dtype=np.uint64)
    np.add.at(words, word[nulls], np.uint64(1) << bit[nulls])
    written = np.zeros(nchunks * wpc, dtype=bool)
    written[word] = True
    return words, written


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("shifted", [False, True])
def test_moments_hll_slots_exact_masks_on_and_off(ext, half_sets, shifted):
    """Half-integer data: |x - shift| <= 128 in steps of 0.5, so every
    power sum is exact in fp64 whatever the order. With masks the moments
    and registers are the same bits, and the masks are the columns' nulls.
    The guard 1e30 would show in max, in every sum and in the registers."""
    sets, _ = half_sets
    for name, cols in sets:
        k = len(cols)
        dev = [_guarded(c, 1e30, j) for j, c in enumerate(cols)]
        g = torch.Generator().manual_seed(241)
        shifts = (torch.randint(-128, 129, (k,), generator=g).double() * 0.5).tolist() if shifted else []
        mom, regs = ext.moments_hll(dev, 12, shifts)
        mom_m, regs_m, masks, parts = ext.moments_hll(dev, 12, shifts, True)
        assert torch.equal(mom.view(torch.int64), mom_m.view(torch.int64)) and torch.equal(regs, regs_m)
        mom = mom.cpu()
        nchunks = 1 if name == "single" else -(-MULTI_N // MULTI_PER)
        for i, c in enumerate(cols):
            want = _moments_ref(c, shifts[i] if shifted else 0.0)
            assert _eq_nan(mom[i], want), f"{name} column {i} (n={c.numel()}): {mom[i].tolist()} vs {want.tolist()}"
            if c.numel():
                assert tuple(parts[i]) == (c.numel(), nchunks, -(-c.numel() // nchunks))
                words, written = _mask_words(torch.isnan(c).numpy(), nchunks)
                got = masks[i].cpu().numpy().view(np.uint64)
                assert got.shape == words.shape and np.array_equal(got[written], words[written]), f"{name} mask {i}"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("p", PS)
def test_moments_hll_registers_against_integer_reference(ext, half_sets, p):
    """Registers against fmix32 + capped rho in integers; values whose
    remainder is all zero (rho at the cap) and whose remainder has its top
    bit set (rho = 1) are planted at the head and, reversed, at the end of
    every column long enough, so some sit in the scalar tail."""
    sets, planted = half_sets
    for name, cols in sets:
        cols = [c.clone() for c in cols]
        for c in cols:
            m = min(planted.numel(), c.numel() // 2)
            if m:
                c[:m] = planted[:m]
                c[c.numel() - m:] = planted[:m].flip(0)
        dev = [_guarded(c, 1e30, j) for j, c in enumerate(cols)]
        regs = ext.moments_hll(dev, p)[1].cpu()
        assert regs.dtype == torch.int32 and tuple(regs.shape) == (len(cols), 1 << p)
        for i, c in enumerate(cols):
            assert torch.equal(regs[i], _hll_ref(c, p)), f"{name} column {i} (n={c.numel()})"
        if name == "multi":
            assert int(regs.max()) == 32 - p + 1  # a planted all-zero remainder reached its cap


@requires_gpu
@pytest.mark.gpu
def test_moments_hll_real_values_bound_and_repeatable(ext):
    """One real-valued column against fp64: a term t_i = d_i^k carries at
    most 3 roundings (d, d^2, the product inside the fma), and summing n of
    them in any order adds at most (n - 1) u sum|t_i| to first order, so
    |error| <= (n + 3) u sum|t_i| (1 + small) with u = 2^-53; the fp64
    reference sum itself is allowed the same. Two calls return equal bits."""
    g = torch.Generator().manual_seed(251)
    n = MULTI_N
    x = (torch.randn(n, generator=g, dtype=torch.float64) * 3.0 + 10.0).float()
    x[torch.rand(n, generator=g) < 0.01] = NAN
    dev = [_guarded(x, 1e30, 0), _guarded(x, 1e30, 1), _guarded(x, 1e30, 0)]
    shift = 9.75
    mom, regs = ext.moments_hll(dev, 12, [shift] * 3)
    mom2, regs2 = ext.moments_hll(dev, 12, [shift] * 3)
    assert torch.equal(mom.view(torch.int64), mom2.view(torch.int64)) and torch.equal(regs, regs2)
    mom = mom.cpu()
    assert torch.equal(mom[0].view(torch.int64), mom[1].view(torch.int64))  # the view's offset changes nothing
    v = x[~torch.isnan(x)].double()
    d = v - shift
    u = 2.0 ** -53
    for k in (1, 2, 3, 4):
        t = d ** k
        bound = 2.0 * (n + 3) * u * float(t.abs().sum()) * 1.001
        err = abs(float(mom[0, k]) - float(t.sum()))
        print(f"s{k}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    assert mom[0, 0] == v.numel() and mom[0, 5] == v.min() and mom[0, 6] == v.max()
    assert mom[0, 7] == (v == 0).sum() and mom[0, 8] == (v != torch.trunc(v)).sum()
