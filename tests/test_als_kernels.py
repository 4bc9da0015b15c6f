"""The two halves of K32 (ops/hip/als_sweep.hip; ops/als.py states the method)
against int64 sums where every product and sum is exact, and against fp64 with
the bounds derived in ops/als.py where it is not. ANOVOS_ALS_BLOCKS and
ANOVOS_ALS_CHUNKS force the grids, so small inputs reach several slabs per
block and blocks that own only the partial slab, or nothing.

Largest ratios to the bounds seen: see docs/KERNELS.md, K32."""

import numpy as np
import pytest
import torch

from anovos_amd.ops.als import (ALS_GAMMA_A, ALS_GAMMA_G, ALS_GAMMA_H, ALS_GAMMA_RHS, als_kr, als_tri,
                                unpack_normal)

pytestmark = [pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"), pytest.mark.gpu]

DEV = "cuda"
ids = lambda s: "-".join(map(str, s))


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    return backend.require_hip()


def _cols(X, guard=None):
    """One device tensor per column; with `guard`, views [4 : 4 + n] of buffers filled with it."""
    if guard is None:
        return [torch.as_tensor(np.ascontiguousarray(X[:, j])).to(DEV) for j in range(X.shape[1])]
    out = []
    for j in range(X.shape[1]):
        buf = torch.full((X.shape[0] + 8,), guard, dtype=torch.float32, device=DEV)
        buf[4:4 + X.shape[0]] = torch.as_tensor(X[:, j])
        out.append(buf[4:4 + X.shape[0]])
    return out


def _integer_frame(rng, n, m, zmax=3):
    """(X f32, Z int64, M int64, shift): integer z and shift, 20 % NaN, an all-NaN row, a
    NaN-free row, an all-NaN column."""
    shift = rng.integers(-2, 3, m)
    Z = rng.integers(-zmax, zmax + 1, (n, m))
    null = rng.random((n, m)) < 0.2
    null[:, m // 2] = True
    null[n // 2] = True
    if n > 1:
        null[n // 3] = False
    X = (Z + shift).astype(np.float32)
    X[null] = np.nan
    return X, np.where(null, 0, Z), (~null).astype(np.int64), shift.astype(np.float64)


def _packed_int(M, Z, W, kr):
    """int64 [.., T + kr]: sum m w_a w_b over the packed lower triangle, then sum z w; W [m, k]."""
    Wp = np.zeros((W.shape[0], kr), dtype=np.int64)
    Wp[:, :W.shape[1]] = W
    a, b = np.tril_indices(kr)
    return np.concatenate([M @ (Wp[:, a] * Wp[:, b]), Z @ Wp], axis=1)


def _row(ext, X, shift, V, reg=0.5, cols=None, **kw):
    m = X.shape[1]
    return ext.als_row_solve_bf16x2(cols or _cols(X), torch.as_tensor(shift), torch.ones(m, dtype=torch.float64),
                                    torch.ones(m, dtype=torch.float64),
                                    torch.as_tensor(np.asarray(V, dtype=np.float32)).to(DEV), reg, **kw)


# (n, m, rank, blocks)
ROW_SHAPES = [(1, 2, 1, 1), (15, 2, 1, 1), (16, 31, 4, 1), (17, 32, 5, 3), (63, 33, 10, 1), (64, 150, 13, 3),
              (65, 160, 16, 1), (129, 31, 16, 3), (516, 33, 5, 3), (516, 150, 10, 1), (129, 160, 13, 3),
              (64, 32, 4, 1), (516, 160, 16, 3)]


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ids)
def test_row_normal_exact(ext, monkeypatch, shape):
    """V and z integers in [-3, 3], integer shift, scale 1: the normal equations are integers
    below 2^24, exact in bf16 products and f32 sums."""
    n, m, rank, blocks = shape
    monkeypatch.setenv("ANOVOS_ALS_BLOCKS", str(blocks))
    rng = np.random.default_rng(3200 + sum(shape))
    X, Z, M, shift = _integer_frame(rng, n, m)
    V = rng.integers(-3, 4, (m, rank))
    _, N = _row(ext, X, shift, V, want_u=False, normal=True)
    want = torch.as_tensor(_packed_int(M, Z, V, als_kr(rank)))
    assert torch.equal(N.cpu().to(torch.int64), want)


@pytest.mark.parametrize("m", [33, 150])
@pytest.mark.parametrize("plane", ["vv", "z"])
def test_row_normal_lo_planes(ext, monkeypatch, plane, m):
    """vv: V odd and up to 255, so v v needs 16 bits. z: row i observes only column i % m, an
    odd 16-bit z against V = +-1 (rank 1), so every column position is hit. One bf16 misses both."""
    monkeypatch.setenv("ANOVOS_ALS_BLOCKS", "3")
    rng = np.random.default_rng(3201 + m)
    n = 2 * m + 3
    if plane == "vv":
        X, Z, M, shift = _integer_frame(rng, n, m, zmax=1)
        V = (rng.integers(0, 128, (m, 5)) * 2 + 1) * rng.choice([-1, 1], (m, 5))
    else:
        Z = np.zeros((n, m), dtype=np.int64)
        M = np.zeros((n, m), dtype=np.int64)
        at = (np.arange(n), np.arange(n) % m)
        Z[at] = (rng.integers(2 ** 7, 2 ** 15, n) * 2 + 1) * rng.choice([-1, 1], n)
        M[at] = 1
        X = np.where(M == 1, Z, np.nan).astype(np.float32)
        V, shift = rng.choice([-1, 1], (m, 1)), np.zeros(m)
    _, N = _row(ext, X, shift, V, want_u=False, normal=True)
    assert torch.equal(N.cpu().to(torch.int64), torch.as_tensor(_packed_int(M, Z, V, als_kr(V.shape[1]))))


@pytest.mark.parametrize("m,rank", [(8, 4), (32, 10), (150, 16)])
def test_row_solve_bound(ext, m, rank):
    """Real values, V from eigh of a random correlation matrix, n = 2000: u against the fp64
    solution u* of the same A and b, within
      2 |A^-1| ((gamma_A |sum m |v v||_F + k (3 k + 1) 2^-24 |A|) |u*| + gamma_b |sum |z| |v||),
    the normal equations' bounds, the backward error of the Cholesky solve, and a factor 2
    for the second-order terms."""
    rng = np.random.default_rng(3210 + m)
    n, reg = 2000, 0.01
    B = rng.normal(size=(4 * m, m))
    V = np.linalg.eigh(np.corrcoef(B.T))[1][:, -rank:].astype(np.float32).astype(np.float64)
    X = rng.normal(size=(n, m)).astype(np.float32)
    X[rng.random((n, m)) < 0.2] = np.nan
    X[n // 2] = np.nan
    U, _ = _row(ext, X, np.zeros(m), V, reg=reg)
    U = U.cpu().numpy().astype(np.float64).T[:, :rank]
    M = (~np.isnan(X)).astype(np.float64)
    Z = np.nan_to_num(X.astype(np.float64))
    A = np.einsum("rj,ja,jb->rab", M, V, V) + (reg * np.maximum(M.sum(1), 1))[:, None, None] * np.eye(rank)
    ustar = np.linalg.solve(A, (Z @ V)[:, :, None])[:, :, 0]
    ev = np.linalg.eigvalsh(A)
    m_pad = (m + 31) // 32 * 32
    absA = np.linalg.norm(np.einsum("rj,ja,jb->rab", M, np.abs(V), np.abs(V)), axis=(1, 2))
    bound = 2 / ev[:, 0] * ((ALS_GAMMA_A(m_pad) * absA + rank * (3 * rank + 1) * 2.0 ** -24 * ev[:, -1])
                            * np.linalg.norm(ustar, axis=1)
                            + ALS_GAMMA_RHS(m_pad) * np.linalg.norm(np.abs(Z) @ np.abs(V), axis=1))
    err = np.linalg.norm(U - ustar, axis=1)
    print(f"m={m} rank={rank}: largest |u - u*| / bound = {(err[bound > 0] / bound[bound > 0]).max():.3f}")
    assert (err <= bound).all()


def test_row_solve_by_hand(ext):
    """V = (1, 2), reg 0.5. (3, 1): A = 5 + 0.5 * 2, b = 5. (3, null): A = 1 + 0.5, b = 3.
    (null, null): u = 0. (null, 4): A = 4 + 0.5, b = 8."""
    X = np.array([[3, 1], [3, np.nan], [np.nan, np.nan], [np.nan, 4]], dtype=np.float32)
    U, _ = _row(ext, X, np.zeros(2), [[1.0], [2.0]])
    assert U.shape == (4, 4) and torch.equal(U[1:].cpu(), torch.zeros(3, 4))
    np.testing.assert_allclose(U[0].cpu().numpy(), [5 / 6, 2, 0, 16 / 9], rtol=3e-7)


def test_row_outputs(ext, monkeypatch):
    """outs[j] = buf[j, 3 : 3 + n] of a sentinel buffer, some None: only null entries change, to
    fmaf(u . v_j, sd_j, mu_j) of the returned U within 1 ulp (mu is 1100, |u . v| sd stays below 40,
    so the f32 dot's error is far below half an ulp of the result); all-null rows get mu_j."""
    monkeypatch.setenv("ANOVOS_ALS_BLOCKS", "3")
    rng = np.random.default_rng(3220)
    n, m, rank = 333, 37, 6
    mu = 1100.0 + rng.integers(0, 50, m).astype(np.float64)
    sd = 2.0 ** rng.integers(-1, 2, m).astype(np.float64)
    X = (mu + sd * rng.normal(size=(n, m))).astype(np.float32)
    X[rng.random((n, m)) < 0.2] = np.nan
    X[7] = np.nan
    V = (rng.normal(size=(m, rank)) / np.sqrt(rank)).astype(np.float32)
    given = rng.random(m) < 0.8
    want = (np.arange(m * (n + 5), dtype=np.float32).reshape(m, n + 5) % 977 - 5000)
    run = []
    for _ in range(2):
        buf = torch.as_tensor(want.copy()).to(DEV)
        U, _ = ext.als_row_solve_bf16x2(_cols(X), torch.as_tensor(mu), torch.as_tensor(1 / sd), torch.as_tensor(sd),
                                        torch.as_tensor(V).to(DEV), 0.01,
                                        outs=[buf[j, 3:3 + n] if given[j] else None for j in range(m)])
        run.append((buf.cpu().numpy(), U.cpu().numpy()))
    assert np.array_equal(run[0][0], run[1][0]) and np.array_equal(run[0][1], run[1][1])
    got, U = run[0]
    fill = (np.isnan(X) & given[None, :]).T
    assert np.array_equal(got[:, 3:3 + n][~fill], want[:, 3:3 + n][~fill])
    assert np.array_equal(got[:, :3], want[:, :3]) and np.array_equal(got[:, 3 + n:], want[:, 3 + n:])
    pred = ((U[:rank].astype(np.float64).T @ V.astype(np.float64).T) * sd + mu).T
    assert np.abs(pred - mu[:, None]).max() < 40
    assert (np.abs(got[:, 3:3 + n][fill] - pred[fill]) <= np.spacing(np.float32(1024.0))).all()
    assert np.array_equal(got[:, 3 + 7][given], mu.astype(np.float32)[given])


def test_row_edges_and_refusals(ext):
    X = np.zeros((0, 3), dtype=np.float32)
    U, N = _row(ext, X, np.zeros(3), np.ones((3, 2)), normal=True)
    assert U.shape == (4, 0) and N.shape == (0, 14)
    X = np.ones((8, 3), dtype=np.float32)
    with pytest.raises(RuntimeError, match="rank"):
        _row(ext, np.ones((8, 20), dtype=np.float32), np.zeros(20), np.ones((20, 17)))
    with pytest.raises(RuntimeError, match="ALS_MAX_COLS"):
        _row(ext, np.ones((8, 161), dtype=np.float32), np.zeros(161), np.ones((161, 2)))
    for reg in (0.0, -1.0):
        with pytest.raises(RuntimeError, match="reg"):
            _row(ext, X, np.zeros(3), np.ones((3, 2)), reg=reg)
    with pytest.raises(RuntimeError, match="contiguous"):
        _row(ext, X, np.zeros(3), np.ones((3, 2)), cols=[torch.ones(16, device=DEV)[::2] for _ in range(3)])


def _col(ext, X, shift, Uk, kr, guard=1e30):
    """The column half on U [n, k] held as the view [:, 4 : 4 + n] of a guard-filled [kr, .] buffer."""
    n, m = X.shape
    big = torch.full((kr, (n + 3) // 4 * 4 + 8), guard, dtype=torch.float32, device=DEV)
    big[:, 4:4 + n] = 0
    big[:Uk.shape[1], 4:4 + n] = torch.as_tensor(np.asarray(Uk, dtype=np.float32).T)
    return ext.als_col_normal_bf16x2(_cols(X, guard=float("nan")), torch.as_tensor(shift),
                                     torch.ones(m, dtype=torch.float64), big[:, 4:4 + n]).cpu()


# (n, m, rank, chunks)
COL_SHAPES = [(1, 1, 1, 1), (31, 16, 1, 1), (32, 17, 10, 3), (33, 64, 16, 1), (63, 65, 10, 5), (64, 150, 16, 3),
              (65, 160, 1, 1), (129, 16, 16, 5), (193, 65, 10, 3), (193, 160, 16, 5), (129, 150, 10, 1)]


@pytest.mark.parametrize("shape", COL_SHAPES, ids=ids)
def test_col_normal_exact(ext, monkeypatch, shape):
    """U and z integers in [-3, 3]; frame columns and U are offset views between guard values."""
    n, m, rank, chunks = shape
    monkeypatch.setenv("ANOVOS_ALS_CHUNKS", str(chunks))
    rng = np.random.default_rng(3230 + sum(shape))
    X, Z, M, shift = _integer_frame(rng, n, m)
    U = rng.integers(-3, 4, (n, rank))
    got = _col(ext, X, shift, U, als_kr(rank))
    assert torch.equal(got, torch.as_tensor(_packed_int(M.T, Z.T, U, als_kr(rank))).double())


@pytest.mark.parametrize("plane", ["uu", "z"])
def test_col_normal_lo_planes(ext, monkeypatch, plane):
    """uu: U odd and up to 255. z: odd 16-bit z against U = +-1, over five macro-slabs."""
    monkeypatch.setenv("ANOVOS_ALS_CHUNKS", "3")
    rng = np.random.default_rng(3231)
    n, m = 300, 33
    X, Z, M, shift = _integer_frame(rng, n, m, zmax=1)
    if plane == "uu":
        U = (rng.integers(0, 128, (n, 5)) * 2 + 1) * rng.choice([-1, 1], (n, 5))
    else:
        Z = np.where(M == 1, (rng.integers(2 ** 7, 2 ** 15, (n, m)) * 2 + 1) * rng.choice([-1, 1], (n, m)), 0)
        X = np.where(M == 1, Z + shift, np.nan).astype(np.float32)
        U = rng.choice([-1, 1], (n, 1))
    # 64 rows of 2^16 stay below 2^24 in the fp32 chain; the fp64 sums are exact
    got = _col(ext, X, shift, U, als_kr(U.shape[1]))
    assert torch.equal(got, torch.as_tensor(_packed_int(M.T, Z.T, U, als_kr(U.shape[1]))).double())


@pytest.mark.parametrize("m", [16, 150])
def test_col_normal_bound(ext, m):
    """Real values, n = 20 000, rank 10: every entry within gamma_H sum m |u_a u_b| and
    gamma_g sum |z| |u| of the fp64 sums."""
    rng = np.random.default_rng(3240 + m)
    n, rank, kr = 20_000, 10, 12
    X = rng.normal(size=(n, m)).astype(np.float32)
    X[rng.random((n, m)) < 0.2] = np.nan
    U = rng.normal(size=(n, rank)).astype(np.float32).astype(np.float64)
    H, g = unpack_normal(_col(ext, X, np.zeros(m), U, kr).numpy(), kr)
    M, Z = (~np.isnan(X)).astype(np.float64), np.nan_to_num(X.astype(np.float64))
    UU = (U[:, :, None] * U[:, None, :]).reshape(n, -1)
    eH = np.abs(H[:, :rank, :rank].reshape(m, -1) - M.T @ UU) / (ALS_GAMMA_H * (M.T @ np.abs(UU)))
    eg = np.abs(g[:, :rank] - Z.T @ U) / (ALS_GAMMA_G * (np.abs(Z).T @ np.abs(U)))
    print(f"m={m}: largest ratio to the bound: H {eH.max():.3f}, g {eg.max():.3f}")
    assert eH.max() <= 1 and eg.max() <= 1
    assert not H[:, rank:].any() and not g[:, rank:].any() and als_tri(kr) == 78
