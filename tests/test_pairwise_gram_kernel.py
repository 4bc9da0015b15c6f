"""The pairwise-complete Gram kernel (K25, ops/hip/pairwise_gram.hip).

`pairwise_gram_bf16(cols, means)` returns fp64 [4, k, k] = (N, P, S, Q)
with m = !isnan(x) and z = m ? x - mean : 0:

    N[i][j] = sum m_i m_j      P[i][j] = sum z_i z_j
    S[i][j] = sum z_i m_j      Q[i][j] = sum z_i^2 m_j

Layout under test: 16-column tiles in groups of 4 (64 columns), one work
item per pair of groups, one block per (item, row chunk) staging 64-row
macro-slabs; full macro-slabs take an unguarded prefetching path, the one
partial macro-slab at the end a guarded one; padding columns are zeroed
once. The shapes are the smallest that reach each path and hand-over.

Data as in tests/test_gram_staging.py: integers in [-2, 2], integer means
in [-2, 2], 1-30 % NaN. So |z| <= 4, z^2 <= 16, m in {0, 1}: every operand
is exact in bf16 and every sum is an integer far below 2^24, the fp32
accumulators are exact in any order and all four matrices are compared
with `torch.equal` against int64 matmuls. S and Q are compared entry by
entry on both triangles, which catches a mirrored tile where a transposed
product belongs.
"""

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _reference(x, means):
    """int64 (N, P, S, Q) of f32 [k, n] `x` with NaN nulls."""
    m = ~torch.isnan(x)
    z = torch.where(m, x - means[:, None], torch.zeros_like(x)).long()
    m = m.long()
    return torch.stack([m @ m.T, z @ z.T, z @ m.T, (z * z) @ m.T])


def _int_matrix(k, n, g):
    """f32 [k, n] of integers in [-2, 2], a NaN rate of 1-30 % drawn per
    column, integer means in [-2, 2]."""
    x = torch.randint(-2, 3, (k, n), generator=g).float()
    rate = 0.01 + 0.29 * torch.rand(k, 1, generator=g)
    x[torch.rand(k, n, generator=g) < rate] = NAN
    means = torch.randint(-2, 3, (k,), generator=g).float()
    return x, means


def _check_exact(ext, cols, means, ref, what):
    got = ext.pairwise_gram_bf16(cols, means.to(DEV))
    k = len(cols)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, k, k)
    got = got.cpu()
    assert torch.equal(got[0], got[0].T), f"{what}: N not symmetric"
    assert torch.equal(got[1], got[1].T), f"{what}: P not symmetric"
    for p, name in enumerate("NPSQ"):
        diff = (got[p] - ref[p].double()).abs()
        assert torch.equal(got[p], ref[p].double()), (
            f"{what}: {name} differs in {int((diff > 0).sum())} entries, max {float(diff.max())}")


def _rows(x):
    xd = x.to(DEV)
    return [xd[i] for i in range(xd.shape[0])]


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 516])
def test_round_boundary_lengths_one_block(ext, monkeypatch, n):
    """One block per item (ANOVOS_PAIRGRAM_CHUNKS=1) runs 0 to 8 full
    rounds and then a tail of 0 to 63 rows: the prefetch is not primed at
    all, or primed, used and drained, with and without a tail behind it."""
    monkeypatch.setenv("ANOVOS_PAIRGRAM_CHUNKS", "1")
    g = torch.Generator().manual_seed(2503 + n)
    for k in [37, 150]:
        x, means = _int_matrix(k, n, g)
        _check_exact(ext, _rows(x), means, _reference(x, means), f"k={k} n={n}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["2", "3", "5", "9"])
@pytest.mark.parametrize("n", [771, 1027])
def test_several_blocks_some_without_rounds(ext, monkeypatch, n, chunks):
    """13 and 17 macro-slabs over 2..9 blocks per item: blocks own one or
    several macro-slabs, the last non-empty block owns the partial
    macro-slab behind full ones (chunks 2, 3) or alone, with no round at
    all (chunks 5, 9), and trailing blocks own nothing (n = 771, chunks
    9)."""
    monkeypatch.setenv("ANOVOS_PAIRGRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(2521 + n + int(chunks))
    for k in [65, 150]:
        x, means = _int_matrix(k, n, g)
        _check_exact(ext, _rows(x), means, _reference(x, means), f"k={k} n={n} chunks={chunks}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 15, 16, 17, 37, 63, 64, 65, 129, 150])
def test_column_counts(ext, k):
    """A single tile, padding columns inside a tile, one full group, one
    column past a group (a second group of one tile: items (0,0), (0,1),
    (1,1)), three groups, the workload's width; at the default grid.
    n = 193 gives three full macro-slabs and one row."""
    g = torch.Generator().manual_seed(2531 + k)
    x, means = _int_matrix(k, 193, g)
    _check_exact(ext, _rows(x), means, _reference(x, means), f"k={k}")


@requires_gpu
@pytest.mark.gpu
def test_more_items_than_one_launch_holds(ext, monkeypatch):
    """k = 321 makes 6 groups and 21 items; a forced split of 200 row
    chunks leaves room for only a few items per launch, so the host loop
    over items runs several launches into one output."""
    monkeypatch.setenv("ANOVOS_PAIRGRAM_CHUNKS", "200")
    g = torch.Generator().manual_seed(2539)
    x, means = _int_matrix(321, 64 * 200 + 5, g)
    _check_exact(ext, _rows(x), means, _reference(x, means), "k=321")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "3"])
def test_special_columns(ext, monkeypatch, chunks):
    """An all-NaN column (its rows and columns are zero in all four
    matrices), a column with no NaN, and two columns whose present rows
    are disjoint (N[i][j] = 0 while S and Q against other columns are
    not), placed in different tiles and groups."""
    monkeypatch.setenv("ANOVOS_PAIRGRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(2543)
    k, n = 70, 333
    x, means = _int_matrix(k, n, g)
    x[3] = NAN
    x[66] = torch.randint(-2, 3, (n,), generator=g).float()
    half = torch.arange(n) % 2 == 0
    x[5] = torch.where(half, torch.randint(-2, 3, (n,), generator=g).float(), torch.tensor(NAN))
    x[69] = torch.where(half, torch.tensor(NAN), torch.randint(-2, 3, (n,), generator=g).float())
    ref = _reference(x, means)
    assert int(ref[0][5, 69]) == 0 and int(ref[0][3].sum()) == 0 and int(ref[0][66, 66]) == n
    _check_exact(ext, _rows(x), means, ref, f"chunks={chunks}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "2"])
@pytest.mark.parametrize("n", [65, 129])
def test_unaligned_bases_and_guard_values(ext, monkeypatch, n, chunks):
    """Columns are views 1, 2 and 3 elements off a 16-byte boundary into
    one flat tensor whose gaps hold 1e30 and -7: a load that runs past a
    column's end or starts before it picks up a present value (a NaN
    guard would only count as a null), and a tail that does not clear
    the rows past n leaves the previous round's values in LDS; either
    changes N, S or Q. The guards lie inside the allocation, so nothing
    is read out of bounds."""
    monkeypatch.setenv("ANOVOS_PAIRGRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(2549 + n)
    for k in [37, 150]:
        x, means = _int_matrix(k, n, g)
        starts, pos = [], 8
        for i in range(k):
            pos = (pos + 3) // 4 * 4 + 1 + i % 3  # offset 1, 2, 3 mod 4
            starts.append(pos)
            pos += n + 5  # at least 5 guards behind every column
        flat = torch.full((pos + 8,), 1e30)
        flat[1::2] = -7.0
        for i, s in enumerate(starts):
            flat[s:s + n] = x[i]
        fd = flat.to(DEV)
        cols = [fd[s:s + n] for s in starts]
        assert all(c.is_contiguous() and c.storage_offset() % 4 == 1 + i % 3
                   for i, c in enumerate(cols))
        _check_exact(ext, cols, means, _reference(x, means), f"k={k} n={n} chunks={chunks}")


@requires_gpu
@pytest.mark.gpu
def test_counts_past_fp32(ext, monkeypatch):
    """Two null-free columns of 2^24 + 40 zeros. One block per item would
    count 2^24 + 40 rows in an fp32 accumulator, which stops at 2^24; the
    binding raises the forced split of 1 so that no block owns 2^24 rows,
    and the fp64 second stage adds the blocks exactly."""
    monkeypatch.setenv("ANOVOS_PAIRGRAM_CHUNKS", "1")
    n = (1 << 24) + 40
    cols = [torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(2)]
    got = ext.pairwise_gram_bf16(cols, torch.zeros(2, device=DEV)).cpu()
    assert torch.equal(got[0], torch.full((2, 2), float(n), dtype=torch.float64))
    assert torch.equal(got[1:], torch.zeros(3, 2, 2, dtype=torch.float64))


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [None, "3"])
def test_real_values_repeat_bit_for_bit_and_stay_in_bound(ext, monkeypatch, chunks):
    """Real-valued data, k = 150, n = 1027. Two calls return the same bits
    (fixed block split, fixed order in the fp64 stage, no atomics). The
    values are held to the bound of tests/test_gram_staging.py: the
    reference forms the kernel's bf16 operands (zb = bf16(x - mean),
    bf16(zb * zb), m) and multiplies them in fp64, so what is left is the
    fp32 summation of n exact products, |err| <= n 2^-23 sum |a b| <=
    n 2^-23 sqrt(sum a^2 sum b^2) (Cauchy-Schwarz)."""
    if chunks is not None:
        monkeypatch.setenv("ANOVOS_PAIRGRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(2551)
    k, n = 150, 1027
    x = torch.stack([torch.randn(n, generator=g) * (1 + i % 5) + i for i in range(k)])
    x[torch.rand(k, n, generator=g) < 0.01 + 0.002 * torch.arange(k)[:, None]] = NAN
    means = torch.nanmean(x, dim=1)
    cols = _rows(x)
    a = ext.pairwise_gram_bf16(cols, means.to(DEV))
    b = ext.pairwise_gram_bf16(cols, means.to(DEV))
    assert torch.equal(a, b)
    a = a.cpu()
    m = ~torch.isnan(x)
    zb = torch.where(m, x - means[:, None], torch.zeros_like(x)).to(torch.bfloat16).float()
    qb = (zb * zb).to(torch.bfloat16).double()
    zb, m = zb.double(), m.double()
    ref = torch.stack([m @ m.T, zb @ zb.T, zb @ m.T, qb @ m.T])
    nz, nq, nm = (torch.sqrt((t * t).sum(1)) for t in (zb, qb, m))
    eps = n * 2.0 ** -23
    bound = torch.stack([0 * nm[:, None] * nm[None, :], eps * nz[:, None] * nz[None, :],
                         eps * nz[:, None] * nm[None, :], eps * nq[:, None] * nm[None, :]])
    err = (a - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    print(f"chunks={chunks}: max err / bound = {float(ratio[1:].max()):.4f}")
    assert torch.equal(a[0], ref[0]), "counts must be exact"
    assert bool((err <= bound).all()), f"max err / bound = {float(ratio.max())}"


def test_refusals_without_a_device():
    """An empty list and host tensors are refused before any device call,
    so this runs without a GPU."""
    from anovos_amd.ops import backend

    ext = backend.hip_ext()
    if ext is None:
        pytest.skip("HIP extension not built")
    assert hasattr(ext, "pairwise_gram_bf16")
    with pytest.raises(RuntimeError, match="pairwise_gram_bf16: no columns"):
        ext.pairwise_gram_bf16([], torch.zeros(0))
    host = [torch.arange(32, dtype=torch.float32), torch.ones(32, dtype=torch.float32)]
    for ts in ([host[0]], host):
        with pytest.raises(RuntimeError, match="pairwise_gram_bf16: device columns required"):
            ext.pairwise_gram_bf16(ts, torch.zeros(len(ts)))


@requires_gpu
@pytest.mark.gpu
def test_refusals_on_the_device(ext):
    """Strided views, f64 columns, unequal lengths, and a `means` of the
    wrong length or on the host are refused; the same call with the
    argument right succeeds."""
    ts = [torch.arange(32, dtype=torch.float32, device=DEV), torch.ones(32, dtype=torch.float32, device=DEV)]
    means = torch.zeros(2, device=DEV)
    assert tuple(ext.pairwise_gram_bf16(ts, means).shape) == (4, 2, 2)
    wide = torch.zeros(32, 2, device=DEV)
    with pytest.raises(RuntimeError, match="pairwise_gram_bf16: columns must be contiguous"):
        ext.pairwise_gram_bf16([wide[:, 0], wide[:, 1]], means)
    with pytest.raises(RuntimeError, match="pairwise_gram_bf16: expected float32 columns"):
        ext.pairwise_gram_bf16([ts[0], ts[1].double()], means)
    with pytest.raises(RuntimeError, match="pairwise_gram_bf16: all columns must have equal length"):
        ext.pairwise_gram_bf16([ts[0], ts[1][:31]], means)
    with pytest.raises(RuntimeError, match="pairwise_gram_bf16: means has 3 entries, expected 2"):
        ext.pairwise_gram_bf16(ts, torch.zeros(3, device=DEV))
    with pytest.raises(RuntimeError, match="pairwise_gram_bf16: means must be on the columns' device"):
        ext.pairwise_gram_bf16(ts, torch.zeros(2))
