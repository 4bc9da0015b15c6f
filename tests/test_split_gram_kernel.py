"""The split-bf16 Gram kernel (K28, ops/hip/split_gram.hip) against int64 and
fp64 torch on the CPU; F = SPLITGRAM_FLUSH_ROWS."""

import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

DEV = "cuda"
NAN = float("nan")
F = 64  # SPLITGRAM_FLUSH_ROWS; the ext fixture holds the extension to it
GAMMA = 3 * 2.0 ** -18 + (3 * F + 4) * 2.0 ** -24


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend, corr

    e = backend.require_hip()
    assert e.SPLITGRAM_FLUSH_ROWS == F == corr.SPLITGRAM_FLUSH_ROWS and corr.SPLITGRAM_GAMMA == GAMMA
    return e


def _int_matrix(k, n, g):
    # as tests/test_pairwise_gram_kernel.py: exact in bf16, every lo plane zero
    x = torch.randint(-2, 3, (k, n), generator=g).float()
    rate = 0.01 + 0.29 * torch.rand(k, 1, generator=g)
    x[torch.rand(k, n, generator=g) < rate] = NAN
    return x, torch.randint(-2, 3, (k,), generator=g).double()


def _int_gram(x, means):
    z = torch.where(torch.isnan(x), torch.zeros_like(x), x - means[:, None].float()).long()
    return (z @ z.T).double()


def _rows(x):
    xd = x.to(DEV)
    return [xd[i] for i in range(xd.shape[0])]


def _check_exact(ext, cols, means, ref, what):
    got = ext.centered_gram_bf16x2(cols, means.to(DEV))
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape)
    got = got.cpu()
    assert torch.equal(got, got.T), f"{what}: not symmetric"
    assert torch.equal(got, ref), f"{what}: max difference {float((got - ref).abs().max())}"


@pytest.mark.parametrize("chunks", ["1", "3", "5"])
@pytest.mark.parametrize("n", sorted({1, 31, 32, 33, 63, 64, 65, 129, F - 1, F, F + 1, 2 * F + 65}))
def test_lengths_and_row_splits(ext, monkeypatch, n, chunks):
    """Over 3 and 5 blocks some own no macro-slab or only the partial one."""
    monkeypatch.setenv("ANOVOS_SPLITGRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(2801 + n)
    for k in [37, 150]:
        x, means = _int_matrix(k, n, g)
        _check_exact(ext, _rows(x), means, _int_gram(x, means), f"k={k} n={n} chunks={chunks}")


@pytest.mark.parametrize("k", [1, 15, 16, 17, 63, 64, 65, 129, 150, 200])
def test_column_counts(ext, k):
    g = torch.Generator().manual_seed(2803 + k)
    x, means = _int_matrix(k, 193, g)
    _check_exact(ext, _rows(x), means, _int_gram(x, means), f"k={k}")


def test_offset_views_with_guard_values(ext, monkeypatch):
    """Columns 1, 2, 3 elements off a 16-byte boundary; the gaps hold 1e30 and -7."""
    monkeypatch.setenv("ANOVOS_SPLITGRAM_CHUNKS", "2")
    g = torch.Generator().manual_seed(2819)
    k, n = 70, 129
    x, means = _int_matrix(k, n, g)
    starts, pos = [], 8
    for i in range(k):
        pos = (pos + 3) // 4 * 4 + 1 + i % 3
        starts.append(pos)
        pos += n + 5
    flat = torch.full((pos + 8,), 1e30)
    flat[1::2] = -7.0
    for i, s in enumerate(starts):
        flat[s:s + n] = x[i]
    fd = flat.to(DEV)
    _check_exact(ext, [fd[s:s + n] for s in starts], means, _int_gram(x, means), "offset views")


@pytest.mark.parametrize("chunks", ["1", "3"])
def test_lo_planes(ext, monkeypatch, chunks):
    """Even columns ("wide"): odd integers below 2^16, hi and lo both exact.
    Odd columns ("pick"): at most 64 entries of +-1 over all slabs. A
    wide-pick sum is exact (below 2^22) and needs hi and lo of the wide side,
    as A operand in [i][j] and as B in [j][i]. Wide-wide: the bound only."""
    monkeypatch.setenv("ANOVOS_SPLITGRAM_CHUNKS", chunks)
    g = torch.Generator().manual_seed(2833)
    k, n = 150, 4 * F + 65
    x = (2 * torch.randint(-2 ** 15, 2 ** 15, (k, n), generator=g) + 1).float()
    pick = torch.zeros(k, n)
    for i in range(1, k, 2):
        at = torch.randperm(n, generator=g)[:64 - i % 7]
        pick[i, at] = torch.randint(0, 2, (at.numel(),), generator=g).float() * 2 - 1
    wide = torch.arange(k) % 2 == 0
    x = torch.where(wide[:, None], x, pick)
    got = ext.centered_gram_bf16x2(_rows(x), torch.zeros(k, dtype=torch.float64, device=DEV)).cpu()
    ref = (x.long() @ x.long().T).double()
    ww = wide[:, None] & wide[None, :]
    assert torch.equal(got[~ww], ref[~ww]), int((got != ref)[~ww].sum())
    assert bool(((got - ref).abs() <= GAMMA * (x.double().abs() @ x.double().abs().T))[ww].all())


@pytest.mark.parametrize("k", [16, 64, 150])
def test_real_values_within_the_bound(ext, k):
    """Correlated f32 columns, means up to 1e4 sigma, 2 % NaN, against the
    fp64 Gram about the fp64 mean; a hi-only product is outside the bound."""
    g = torch.Generator().manual_seed(2843 + k)
    n = 20000
    base = torch.randn(5, n, generator=g, dtype=torch.float64)
    x = torch.randn(k, 5, generator=g, dtype=torch.float64) @ base + 0.5 * torch.randn(k, n, generator=g, dtype=torch.float64)
    sigma = 10.0 ** torch.linspace(-2, 2, k, dtype=torch.float64)
    x = ((x + torch.linspace(0, 1e4, k, dtype=torch.float64)[:, None]) * sigma[:, None]).float()
    x[torch.rand(k, n, generator=g) < 0.02] = NAN
    means = torch.nanmean(x.double(), dim=1)
    z = torch.nan_to_num(x.double() - means[:, None], nan=0.0)
    ref, bound = z @ z.T, GAMMA * (z.abs() @ z.abs().T)
    cols = _rows(x)
    got = ext.centered_gram_bf16x2(cols, means.to(DEV))
    assert torch.equal(got, ext.centered_gram_bf16x2(cols, means.to(DEV)))
    got = got.cpu()
    assert torch.equal(got, got.T)
    ratio = float(((got - ref).abs() / bound).max())
    zh = z.float().bfloat16().double()
    hi_only = float(((zh @ zh.T - ref).abs() / bound).max())
    print(f"k={k}: max err / bound = {ratio:.4f}, hi-only {hi_only:.1f}")
    assert ratio <= 1.0
    assert hi_only > 1.0


def test_empty_and_refusals(ext):
    ts = [torch.arange(32, dtype=torch.float32, device=DEV), torch.ones(32, dtype=torch.float32, device=DEV)]
    means = torch.zeros(2, dtype=torch.float64, device=DEV)
    empty = ext.centered_gram_bf16x2([t[:0] for t in ts], means)
    assert torch.equal(empty.cpu(), torch.zeros(2, 2, dtype=torch.float64))
    for cols, mu, why in [([ts[0], ts[1].double()], means, "expected float32 columns"),
                          ([ts[0], ts[1][:31]], means, "all columns must have equal length"),
                          (ts, means[:1], "means has 1 entries, expected 2"),
                          (ts, means.cpu(), "means must be on the columns' device"),
                          ([t.cpu() for t in ts], means.cpu(), "device columns required")]:
        with pytest.raises(RuntimeError, match="centered_gram_bf16x2: " + why):
            ext.centered_gram_bf16x2(cols, mu)
