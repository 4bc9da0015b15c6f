"""The regression-imputation kernel K31 (ops/hip/chain_impute.hip, whose header
states the operation) against ops.chain.chain_replay_fp64, the fp64 numpy
replay of the same recurrence. ANOVOS_CHAIN_BLOCKS forces the grid, so small
inputs reach several slabs per block and blocks that own only the partial
slab, or nothing. Outputs are views buf[j, 3 : 3 + n] of a sentinel-filled
buffer: everything but the null entries of served columns must keep its bits.

Derived bound, largest |got - ref| / bound seen: see docs/KERNELS.md, K31."""

import numpy as np
import pytest
import torch

from anovos_amd.ops.chain import chain_error_bound, chain_model, chain_replay_fp64

pytestmark = [pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"), pytest.mark.gpu]

DEV = "cuda"
INF = float("inf")


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    return backend.require_hip()


def _run(ext, X, center, order, C, beta, lo, hi, given=None):
    """[m, n + 5] sentinel buffer after the call (outs[j] = buf[j, 3 : 3 + n], None where
    given[j] is False) and what it must hold: the replay at the null entries of columns
    that are in `order` and given, the sentinel pattern elsewhere."""
    n, m = X.shape
    given = np.ones(m, dtype=bool) if given is None else given
    f = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).float().to(DEV)
    xd = torch.as_tensor(X.T.copy()).to(DEV)
    want = np.arange(m * (n + 5), dtype=np.float32).reshape(m, n + 5) % 977 - 5000
    buf = torch.as_tensor(want.copy()).to(DEV)
    ext.chain_impute_bf16x2([xd[j] for j in range(m)], torch.as_tensor(np.asarray(center, dtype=np.float64)),
                            torch.as_tensor(np.asarray(order, dtype=np.int32)), f(C), f(beta), f(lo), f(hi),
                            [buf[j, 3:3 + n] if given[j] else None for j in range(m)])
    ref = chain_replay_fp64(X, center, order, C, beta, lo, hi)
    served = np.zeros(m, dtype=bool)
    served[np.asarray(order)] = True
    fill = (np.isnan(X) & (served & given)[None, :]).T
    want[:, 3:3 + n][fill] = ref.T[fill].astype(np.float32)
    return buf.cpu().numpy(), want


# (n, m, R, m_s, blocks, drop): every KS, partial and several slabs, blocks without work,
# m_s < m, outs with None entries (drop)
SHAPES = [(1, 2, 1, 2, 1, 0), (15, 2, 3, 1, 1, 0), (16, 8, 3, 8, 1, 0), (17, 8, 10, 5, 3, 1), (63, 31, 3, 31, 1, 0),
          (64, 31, 1, 17, 3, 0), (65, 32, 3, 32, 1, 1), (129, 32, 10, 16, 3, 0), (516, 32, 3, 32, 3, 0),
          (64, 33, 3, 33, 1, 0), (65, 33, 10, 20, 3, 1), (129, 64, 3, 64, 1, 0), (516, 64, 3, 49, 3, 0),
          (17, 64, 10, 64, 3, 0), (63, 96, 3, 96, 1, 0), (129, 96, 3, 65, 3, 1), (65, 128, 3, 128, 3, 0),
          (516, 128, 1, 100, 3, 0), (1, 150, 3, 150, 1, 0), (16, 150, 10, 150, 1, 0), (64, 150, 3, 150, 3, 0),
          (65, 150, 3, 129, 3, 1), (129, 150, 3, 150, 1, 0), (516, 150, 3, 150, 3, 0), (15, 160, 3, 160, 1, 0),
          (63, 160, 1, 160, 3, 1), (129, 160, 3, 145, 3, 0), (516, 160, 10, 160, 3, 0), (516, 8, 10, 8, 1, 0),
          (200, 20, 32, 20, 3, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_exact_small_integers(ext, monkeypatch, shape):
    """z0 integers in [-3, 3] with integer centres, C in {-1, 0, 1} with <= 3 non-zeros a
    step, integer beta, clip [-8, 8]: every intermediate is an integer of magnitude <= 27,
    exact in bf16 products and f32 sums. 20 % nulls, an all-null row, a null-free row, an
    all-null column; a shuffled visiting order."""
    n, m, R, m_s, blocks, drop = shape
    monkeypatch.setenv("ANOVOS_CHAIN_BLOCKS", str(blocks))
    rng = np.random.default_rng(3100 + sum(shape))
    center = rng.integers(-2, 3, m).astype(np.float64)
    X = (rng.integers(-3, 4, (n, m)) + center).astype(np.float32)
    X[rng.random((n, m)) < 0.2] = np.nan
    X[:, m // 2] = np.nan
    X[n // 2] = np.nan
    if n > 1:
        X[n // 3] = (rng.integers(-3, 4, m) + center).astype(np.float32)
    order = rng.permutation(m)[:m_s]
    C = np.zeros((R, m_s, m))
    for r in range(R):
        for p in range(m_s):
            others = np.setdiff1d(np.arange(m), order[p])
            C[r, p, rng.choice(others, min(3, m - 1), replace=False)] = rng.integers(-1, 2, min(3, m - 1))
    beta = rng.integers(-3, 4, (R, m_s))
    given = np.ones(m, dtype=bool)
    given[order[::4]] = not drop
    got, want = _run(ext, X, center, order, C, beta, np.full(m, -8.0), np.full(m, 8.0), given)
    assert np.array_equal(got, want), f"{int((got != want).sum())} elements differ"


@pytest.mark.parametrize("plane", ["z", "C"])
@pytest.mark.parametrize("m", [33, 150])
def test_exact_lo_planes(ext, monkeypatch, plane, m):
    """Row i has its one null at column i % m; step p reads only column (p + 1) % m, so
    every column position is a source. Odd 16-bit integers, which one bf16 would miss, as
    z0 against C = +-1, or as C (scaled by 2^-8) against z0 = +-1: both products are exact."""
    monkeypatch.setenv("ANOVOS_CHAIN_BLOCKS", "3")
    rng = np.random.default_rng(3101 + m)
    n = 2 * m + 3
    odd = lambda *s: (rng.integers(2 ** 7, 2 ** 15, s) * 2 + 1) * rng.choice([-1.0, 1.0], s)
    X = (odd(n, m) if plane == "z" else rng.choice([-1.0, 1.0], (n, m))).astype(np.float32)
    X[np.arange(n), np.arange(n) % m] = np.nan
    C = np.zeros((1, m, m))
    C[0, np.arange(m), (np.arange(m) + 1) % m] = rng.choice([-1.0, 1.0], m) if plane == "z" else odd(m) / 256
    got, want = _run(ext, X, np.zeros(m), np.arange(m), C, np.zeros((1, m)), np.full(m, -INF), np.full(m, INF))
    assert np.array_equal(got, want)


def test_clip_and_chain_order(ext):
    """Two columns, centre 0, R = 2, every step beta = 1; column 0 <- 1 + 2 z1 unclipped,
    column 1 <- clip(1 + z0, -5, 4). A row with both null, visiting (0, 1):
      round 0: z0 = 1 + 2 * 0 = 1, z1 = 1 + 1 = 2;  round 1: z0 = 1 + 2 * 2 = 5, z1 = min(1 + 5, 4) = 4
    (6 without the clip). Visiting (1, 0):
      round 0: z1 = 1 + 0 = 1, z0 = 1 + 2 = 3;      round 1: z1 = min(1 + 3, 4) = 4, z0 = 1 + 8 = 9.
    Row (null, 3): z0 = 1 + 2 * 3 = 7. Row (10, null): z1 = min(11, 4) = 4."""
    X = np.array([[np.nan, np.nan], [np.nan, 3.0], [10.0, np.nan]], dtype=np.float32)
    lo, hi = np.array([-INF, -5.0]), np.array([INF, 4.0])
    c0, c1 = [0.0, 2.0], [1.0, 0.0]
    for order, steps, both in [([0, 1], [c0, c1], (5.0, 4.0)), ([1, 0], [c1, c0], (9.0, 4.0))]:
        got, want = _run(ext, X, np.zeros(2), order, np.array([steps, steps]), np.ones((2, 2)), lo, hi)
        assert np.array_equal(got, want)
        assert (got[0, 3], got[1, 3]) == both and got[0, 4] == 7.0 and got[1, 5] == 4.0


@pytest.mark.parametrize("m,max_iter", [(8, 10), (32, 4), (150, 2)])
def test_derived_bound(ext, monkeypatch, m, max_iter):
    """A model fitted by sklearn on correlated columns with means up to 1e4 sigma, 10 %
    nulls. Reference: the replay on the kernel's own f32 z0 and f32 parameters. Bound:
    ops.chain.chain_error_bound, the recurrence run on errors, and one more rounding
    for z_j + centre."""
    from sklearn.experimental import enable_iterative_imputer  # noqa: F401
    from sklearn.impute import IterativeImputer
    from sklearn.linear_model import LinearRegression

    monkeypatch.setenv("ANOVOS_CHAIN_BLOCKS", "3")
    rng = np.random.default_rng(3110 + m)
    n, u = 2000, 2.0 ** -24
    sd = 0.5 + 2 * rng.random(m)
    mean = 10 * rng.standard_normal(m)
    mean[::5] *= 1000
    X = ((rng.standard_normal((n, 4)) @ rng.standard_normal((4, m)) + 0.3 * rng.standard_normal((n, m))) * sd + mean)
    X = X.astype(np.float32)
    X[rng.random((n, m)) < 0.1] = np.nan
    model = IterativeImputer(LinearRegression(), max_iter=max_iter, tol=0)  # plain least squares: the fit stays quick
    cm = chain_model(model.fit(X.astype(np.float64)), m)
    assert cm is not None
    s, order = cm[0], cm[1]
    C, beta, lo, hi = (a.astype(np.float32).astype(np.float64) for a in cm[2:])
    mh = s.astype(np.float32)
    z0 = (X - mh) - (s - mh).astype(np.float32)  # f32, as the kernel forms it; NaN kept
    got, want = _run(ext, X, s, order, C, beta, lo, hi)
    again, _ = _run(ext, X, s, order, C, beta, lo, hi)
    assert np.array_equal(got, again), "the same call returned different bits"
    miss = np.isnan(X)
    z, e = chain_error_bound(z0, order, C, beta, lo, hi, (m + 31) // 32 * 32)
    ref = z + mh.astype(np.float64)
    bound = e + u * (np.abs(ref) + e)
    ratio = (np.abs(got[:, 3:3 + n].T.astype(np.float64) - ref) / bound)[miss]
    print(f"chain_impute derived bound m={m}: max |got-ref|/bound = {ratio.max():.4f}")
    assert (ratio <= 1).all(), f"m={m}: {int((ratio > 1).sum())} entries beyond the bound, worst {ratio.max()}"
    assert np.array_equal(got[:, :3], want[:, :3]) and np.array_equal(got[:, 3 + n:], want[:, 3 + n:])


def test_argument_checks(ext):
    def call(m=4, m_s=4, R=2, n=8, order=None, n_lo=None, n_beta=None, n_outs=None, out_dtype=torch.float32,
             strided=False):
        cols = [torch.zeros(2 * n, device=DEV)[::2] if strided else torch.zeros(n, device=DEV) for _ in range(m)]
        order = torch.arange(m_s, dtype=torch.int32) if order is None else torch.tensor(order, dtype=torch.int32)
        z = lambda *s: torch.zeros(*s, device=DEV)
        outs = [torch.zeros(n, device=DEV, dtype=out_dtype) for _ in range(m if n_outs is None else n_outs)]
        ext.chain_impute_bf16x2(cols, torch.zeros(m, dtype=torch.float64), order, z(R, m_s, m),
                                z((R * m_s) if n_beta is None else n_beta), z(m if n_lo is None else n_lo), z(m), outs)
        return outs

    for match, kw in [
        ("expected 2 .. 160", dict(m=1, m_s=1)),
        ("expected 2 .. 160", dict(m=161, m_s=4)),
        ("rounds, expected 1 .. 32", dict(R=33)),
        ("steps per round", dict(m_s=5)),
        ("order entry 4 outside", dict(order=[0, 1, 2, 4])),
        ("order entry -1 outside", dict(order=[0, 1, 2, -1])),
        ("twice", dict(order=[0, 1, 2, 1])),
        ("lo has 3 entries, expected 4", dict(n_lo=3)),
        ("beta has 7 entries, expected 8", dict(n_beta=7)),
        ("outs has 3 entries, expected 4", dict(n_outs=3)),
        ("outs must be a contiguous Float", dict(out_dtype=torch.float64)),
        ("must be contiguous", dict(strided=True)),
    ]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    assert all(bool((t == 0).all()) for t in call(n=0) + call())  # empty frame; null-free columns
