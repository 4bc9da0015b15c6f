"""Staging structure of the single-read Gram kernel (K8).

The kernel stages 128-row macro-slabs of all columns through LDS. Full
macro-slabs take an unguarded path whose loads for round s+1 are issued
before the MFMA phase of round s (k <= 160) or in batches at staging
time (161 <= k <= 208); the one partial macro-slab at the end of the
column takes a guarded path; padding columns are zeroed once. The
shapes here are the smallest that reach every one of those paths and
every hand-over between them.

Data as in the edge suite: integers in [-2, 2], integer means, about
1 % NaN. Centered values are integers with |v| <= 4, exact in bf16;
every product and every partial sum is an integer far below 2^24, so
the fp32 result is exact in any summation order and is compared with
`torch.equal` against the int64 product. The one real-valued case
carries the bound derived in its docstring.
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


def _int_matrix(k, n, g):
    """f32 [k, n] of integers in [-2, 2] with about 1 % NaN, integer means
    in [-2, 2], and the exact centered Gram (NaN -> 0 after centering)."""
    x = torch.randint(-2, 3, (k, n), generator=g).float()
    nan = torch.rand(k, n, generator=g) < 0.01
    means = torch.randint(-2, 3, (k,), generator=g).float()
    xc = torch.where(nan, torch.zeros_like(x), x - means[:, None])
    x[nan] = NAN
    ref = (xc.long() @ xc.long().T).double()
    return x, means, ref


def _check_exact(ext, cols, means, ref, what):
    got = ext.centered_gram_bf16(cols, means.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    got = got.double().cpu()
    assert torch.equal(got, got.T), f"{what}: not symmetric"
    assert torch.equal(got, ref), f"{what}: max abs diff {float((got - ref).abs().max())}"


def _rows(x):
    xd = x.to(DEV)
    return [xd[i] for i in range(xd.shape[0])]


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", [127, 128, 129, 255, 256, 257, 383, 385, 516])
def test_round_boundary_lengths_one_block(ext, monkeypatch, n):
    """One block (ANOVOS_GRAM_CHUNKS=1) runs 0 to 4 full rounds and then
    a tail of 0, 1, 4 (n = 516) or 127 rows: the prefetch is not primed
    at all, or primed, used and drained, with and without a tail behind
    it."""
    monkeypatch.setenv("ANOVOS_GRAM_CHUNKS", "1")
    g = torch.Generator().manual_seed(1009 + n)
    for k in [37, 150]:
        x, means, ref = _int_matrix(k, n, g)
        _check_exact(ext, _rows(x), means, ref, f"k={k} n={n}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["2", "3", "5", "9"])
@pytest.mark.parametrize("n", [1027, 128 * 6 + 3])
def test_several_blocks_some_without_rounds(ext, monkeypatch, n, chunks):
    """9 and 7 macro-slabs over 2..9 blocks: blocks own 0, 1 and >= 2
    macro-slabs, a block may own the partial macro-slab alone (n = 1027,
    chunks 5 and 9), and trailing blocks may own nothing (n = 771,
    chunks 5 and 9). k = 161 runs the batched instance."""
    monkeypatch.setenv("ANOVOS_GRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(1013 + n + int(chunks))
    for k in [150, 161]:
        x, means, ref = _int_matrix(k, n, g)
        _check_exact(ext, _rows(x), means, ref, f"k={k} n={n} chunks={chunks}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 15, 17, 145, 150, 160, 161, 200, 208])
def test_padding_columns(ext, k):
    """k one below, on and one above multiples of 8 and of 16, in both
    the prefetching (k <= 160) and the batched (k <= 208) instances, at
    the default grid: n = 257 gives two full macro-slabs and one row."""
    g = torch.Generator().manual_seed(1019 + k)
    x, means, ref = _int_matrix(k, 257, g)
    _check_exact(ext, _rows(x), means, ref, f"k={k}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "2"])
@pytest.mark.parametrize("n", [129, 257])
def test_unaligned_bases_and_guard_values(ext, monkeypatch, n, chunks):
    """Columns are views 1, 2 and 3 elements off a 16-byte boundary into
    one flat tensor whose gaps, between the columns and after the last,
    hold 1e30 and NaN. A full-slab load that runs past a column's end
    would pick up 1e30 (NaN alone would be zeroed and go unseen), and a
    tail that does not zero the rows past n leaves the previous round's
    values in LDS; either changes the result. The sentinels lie inside
    the allocation, so nothing is read out of bounds."""
    monkeypatch.setenv("ANOVOS_GRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(1021 + n)
    for k in [37, 150]:
        x, means, ref = _int_matrix(k, n, g)
        starts, pos = [], 0
        for i in range(k):
            pos = (pos + 3) // 4 * 4 + 1 + i % 3  # offset 1, 2, 3 mod 4
            starts.append(pos)
            pos += n + 5  # at least 5 sentinels behind every column
        flat = torch.full((pos + 8,), 1e30)
        flat[1::2] = NAN
        for i, s in enumerate(starts):
            flat[s:s + n] = x[i]
        fd = flat.to(DEV)
        cols = [fd[s:s + n] for s in starts]
        assert all(c.is_contiguous() and c.storage_offset() % 4 == 1 + i % 3
                   for i, c in enumerate(cols))
        _check_exact(ext, cols, means, ref, f"k={k} n={n} chunks={chunks}")


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "3"])
@pytest.mark.parametrize("k", [37, 150])
def test_real_values_within_fp32_summation_bound(ext, monkeypatch, k, chunks):
    """Real-valued data at n = 1027. The order in which one
    v_mfma_f32_16x16x32_bf16 adds its 32 products is not specified, so
    the kernel's sum is not emulated bit for bit on the host; the
    assertion is the derived bound instead. The reference rounds
    (x - mean_f32) to bf16 with round-to-nearest-even, as the kernel
    does, and forms the Gram in fp64; what is left is the fp32
    summation of n exact products:
    |err_ij| <= n * 2^-23 * sum|a b| <= n * 2^-23 * sqrt(ref_ii ref_jj)
    (Cauchy-Schwarz). Bit-identity with the previous kernel at equal
    row_chunks is checked on the benchmark's dumped outputs
    (profiles/gram_staging_ab.md)."""
    monkeypatch.setenv("ANOVOS_GRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(1031 + k)
    n = 1027
    x = torch.stack([torch.randn(n, generator=g) * (1 + i % 5) + i for i in range(k)])
    x[torch.rand(k, n, generator=g) < 0.01] = NAN
    means = torch.nanmean(x, dim=1)
    xc = torch.nan_to_num(x - means[:, None], nan=0.0).to(torch.bfloat16).double()
    ref = xc @ xc.T
    d = torch.sqrt(torch.diagonal(ref))
    bound = n * 2.0 ** -23 * d[:, None] * d[None, :]
    got = ext.centered_gram_bf16(_rows(x), means.to(DEV)).cpu().double()
    err = (got - ref).abs()
    print(f"k={k} chunks={chunks}: max err / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), f"max err / bound = {float((err / bound).max())}"
    assert torch.equal(got, got.T)
