"""The KNN imputation kernel (K29, ops/hip/knn_impute.hip):
`knn_impute_bf16x2(cols, rows, center, donors, target, k)` -> (est, idx, d2).

Exact tests: integers in [-3, 3] and integer centres make every plane exact in
bf16 and sq, ov exact in fp32, so the result equals the int64 reference bit for
bit, ties included; ANOVOS_KNN_BLOCKS forces the grid. The filter pass is read
back through the optional candidate output and held to gamma S m / ov: largest
error 0.15 of it on 16-bit values (any one lo plane dropped: 28 to 57 times the
bound in a CPU simulation), 0.36 / 0.19 / 0.03 at m = 8 / 32 / 128 on real
values, where 0 of 500 tasks fell outside the filter's precondition (reference
alone; at most 1 % may).
"""

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")]

DEV = "cuda"
NAN = float("nan")
INF = float("inf")


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    e = backend.require_hip()
    assert e is not None, "HIP extension must be loadable on the GPU box"
    return e


def _reference(X, F, target, k):
    """(est, idx, d2) of task rows X [r, m] against F [s, m] (integer-valued):
    sq, ov in int64, d2 by the same f32 multiply and divide, a stable sort"""
    r, m = X.shape
    mx, mf = ~torch.isnan(X), ~torch.isnan(F)
    Xi, Fi = torch.nan_to_num(X).long(), torch.nan_to_num(F).long()
    both = mx[:, None, :] & mf[None, :, :]
    diff = Xi[:, None, :] - Fi[None, :, :]
    sq = (diff * diff * both).sum(-1)
    ov = both.sum(-1)
    d2 = (torch.tensor(float(m)) * sq.float()) / ov.float()
    d2 = torch.where((ov > 0) & mf[None, :, target], d2, torch.full_like(d2, INF))
    d2 = torch.cat([d2, torch.full((r, k), INF)], dim=1)  # fewer than k donors
    dk, order = torch.sort(d2, dim=1, stable=True)
    dk, order = dk[:, :k], order[:, :k]
    found = torch.isfinite(dk)
    idx = torch.where(found, order, torch.full_like(order, -1)).int()
    vals = torch.where(found, torch.nan_to_num(F)[:, target][order.clamp(max=F.shape[0] - 1)], torch.zeros(()))
    total = torch.zeros(r)
    for t in range(k):  # f32, in neighbour order
        total = total + vals[:, t]
    est = total / found.sum(1).float()  # 0 / 0 = NaN without a donor
    return est, idx, dk


def _int_case(r, s, m, k, g):
    """n = r + 5 rows, integers in [-3, 3], 5-30 % NaN per column; r task rows"""
    n = r + 5
    x = torch.randint(-3, 4, (m, n), generator=g).float()
    x[torch.rand(m, n, generator=g) < 0.05 + 0.25 * torch.rand(m, 1, generator=g)] = NAN
    F = torch.randint(-3, 4, (s, m), generator=g).float()
    F[torch.rand(s, m, generator=g) < 0.05 + 0.25 * torch.rand(1, m, generator=g)] = NAN
    target = int(torch.randint(0, m, (1,), generator=g))
    rows = torch.randperm(n, generator=g)[:r]
    x[target, rows] = NAN
    center = torch.randint(-3, 4, (m,), generator=g).double()
    return x, rows, center, F, target


def _run(ext, x, rows, center, F, target, k, candidates=False):
    xd = x.to(DEV)
    cols = [xd[i] for i in range(xd.shape[0])]
    out = ext.knn_impute_bf16x2(cols, rows.to(DEV), center, F.to(DEV), target, k, candidates)
    est, idx, d2 = out[:3]
    assert est.dtype == torch.float32 and idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert tuple(idx.shape) == tuple(d2.shape) == (rows.numel(), k)
    return [t.cpu() for t in out]


def _assert_equal(got, ref):
    for name, a, b in zip(("est", "idx", "d2"), got, ref):
        same = torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) if a.is_floating_point() else torch.equal(a, b)
        assert same, f"{name}: {int((a != b).sum())} entries differ"


_R = [1, 15, 16, 17, 63, 64, 65, 129]
_S = [1, -1, 0, 15, 16, 17, 31, 32, 33, 97]  # -1, 0: k - 1, k; 32 donors = one ring stage
_M = [1, 8, 31, 32, 33, 64, 128]
_K = [1, 5, 8]
_CASES = [(_R[i % 8], _S[i % 10], _M[i % 7], _K[i % 3]) for i in range(30)]
_CASES += [(65, 97, 96, 5), (17, 97, 128, 8)]  # KS = 3, and KS = 4 over several ring stages


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("r,s,m,k", _CASES)
def test_exact_shapes(ext, monkeypatch, r, s, m, k, blocks):
    monkeypatch.setenv("ANOVOS_KNN_BLOCKS", str(blocks))
    s = max(1, k + s) if s <= 0 else s
    g = torch.Generator().manual_seed(1000 * r + 10 * s + m + k)
    x, rows, center, F, target = _int_case(r, s, m, k, g)
    _assert_equal(_run(ext, x, rows, center, F, target, k), _reference(x[:, rows].T, F, target, k))


@pytest.mark.parametrize("plant", ["duplicates", "nearest_lacks_target", "no_overlap", "no_donors", "fewer_than_k"])
def test_exact_planted(ext, plant):
    k, m = 5, 8
    g = torch.Generator().manual_seed(7)
    x, rows, center, F, target = _int_case(40, 50, m, k, g)
    if plant == "duplicates":  # the tie rule: equal donors enter by index
        F[10:20] = F[3]
        F[40] = F[3]
    elif plant == "nearest_lacks_target":  # each row's own values, target column null
        F[: rows.numel()] = x[:, rows].T
    elif plant == "no_overlap":
        x[:, rows[::3]] = NAN
    else:
        F[(0 if plant == "no_donors" else 3):, target] = NAN
    got, ref = _run(ext, x, rows, center, F, target, k), _reference(x[:, rows].T, F, target, k)
    if plant == "no_donors":
        assert torch.isnan(ref[0]).all() and (ref[1] == -1).all() and torch.isinf(ref[2]).all()
    _assert_equal(got, ref)


def _tables(X, F, center, target):
    """fp64 d2 [r, s] (inf for a non-donor) and S m / ov, S = sum_overlap (|zx| + |zf|)^2"""
    m = X.shape[1]
    zx, zf = X.astype(np.float64) - center, F.astype(np.float64) - center
    mx, mf = ~np.isnan(zx), ~np.isnan(zf)
    zx, zf = np.nan_to_num(zx), np.nan_to_num(zf)
    ov = mx.astype(np.float64) @ mf.T
    sq = (zx * zx) @ mf.T + mx @ (zf * zf).T - 2 * zx @ zf.T
    S = (zx * zx) @ mf.T + mx @ (zf * zf).T + 2 * np.abs(zx) @ np.abs(zf).T
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.where((ov > 0) & mf[:, target], m * sq / ov, np.inf)
        return d2, np.where(np.isfinite(d2), m * S / ov, 0.0)


def _filter_fraction(cand_idx, cand_d2, d2, Sd, m):
    """every candidate's filter d2 within gamma S m / ov (+ 2 ulp: multiply, divide) of fp64"""
    from anovos_amd.ops.knn import KNN_FILTER_GAMMA

    gamma = KNN_FILTER_GAMMA((m + 31) // 32 * 32)
    ci, cd = cand_idx.numpy().astype(np.int64), cand_d2.numpy().astype(np.float64)
    have = ci >= 0
    assert have.any() and np.isinf(cd[~have]).all()
    at = np.where(have, ci, 0)
    err = np.abs(np.where(have, cd, 0.0) - np.where(have, np.take_along_axis(d2, at, axis=1), 0.0))
    scale = np.where(have, np.take_along_axis(Sd, at, axis=1), 1.0)
    frac = float((err / (gamma * scale)).max())
    print(f"filter error / bound: {frac:.3f} (m = {m})")
    assert (err <= (gamma + 2.0 ** -23) * scale).all(), frac
    return frac


@pytest.mark.parametrize("swap", [False, True])
def test_lo_planes(ext, swap):
    """16-bit odd centred values on one side (swap: the donors), the other +-1
    away in one column; all 64 donors fit the lists, so every filter d2 is read"""
    k, m, r, target = 5, 4, 8, 2
    g = torch.Generator().manual_seed(11 + swap)
    center = torch.tensor([1000.0, -250.0, 0.0, 77.0], dtype=torch.float64)
    base = (torch.randint(-(2 ** 15), 2 ** 15, (r, m), generator=g) * 2 + 1).float()  # 16-bit odd
    moved = base.repeat_interleave(1 if swap else 8, dim=0)
    col = torch.randint(0, m - 1, (moved.shape[0],), generator=g)
    sign = torch.randint(0, 2, col.shape, generator=g).float() * 2 - 1
    moved[torch.arange(moved.shape[0]), col + (col >= target)] += sign
    X, F = (moved, base.repeat_interleave(8, dim=0)) if swap else (base, moved)
    F = F + center.float()
    F[:, target] = torch.randint(-3, 4, (F.shape[0],), generator=g).float()
    x = (X + center.float()).T.contiguous()
    x[target] = NAN
    got = _run(ext, x, torch.arange(r), center, F, target, k, candidates=True)
    ref = _reference(x.T - center.float(), F - center.float(), target, k)
    assert torch.equal(ref[2], torch.full((r, k), 4.0 / 3.0))  # sq = 1 over three columns
    _assert_equal(got[:3], ref)
    assert (got[3] >= 0).sum() == r * 64
    _filter_fraction(got[3], got[4], *_tables(x.T.numpy(), F.numpy(), center.numpy(), target), m)


@pytest.mark.parametrize("m,seed", [(8, 1), (32, 2), (128, 3)])
def test_real_values(ext, m, seed, s=2000, r=500, k=5):
    """f32 data, means up to 1e4 sigma. Departure from "the returned set is
    correct": the f32 re-rank may swap donors closer than its resolution, so the
    set's fp64 distances are held to the true k smallest plus twice its bound."""
    from anovos_amd.ops.knn import KNN_FILTER_GAMMA

    rng = np.random.default_rng(seed)
    sd = rng.uniform(0.5, 2.0, m)
    mean = rng.uniform(-1e4, 1e4, m) * sd
    F = (mean + sd * rng.standard_normal((s, m))).astype(np.float32)
    X = (mean + sd * rng.standard_normal((r, m))).astype(np.float32)
    F[rng.random((s, m)) < 0.05] = np.nan
    X[rng.random((r, m)) < 0.05] = np.nan
    target = m // 2
    X[:, target] = np.nan
    center = np.nanmean(F.astype(np.float64), axis=0)
    d64all, Sd = _tables(X, F, center, target)
    ds = np.sort(d64all, axis=1)
    met = ds[:, k + 7] - ds[:, k - 1] > 2 * KNN_FILTER_GAMMA((m + 31) // 32 * 32) * Sd.max(1)
    assert met.mean() >= 0.99  # from the reference alone, before anything runs
    x = torch.from_numpy(np.ascontiguousarray(X.T))
    est, idx, d2, cand_idx, cand_d2 = _run(ext, x, torch.arange(r), torch.from_numpy(center),
                                           torch.from_numpy(F), target, k, candidates=True)
    _filter_fraction(cand_idx, cand_d2, d64all, Sd, m)
    idx = idx.numpy().astype(np.int64)
    assert (idx >= 0).all() and all(len(set(row)) == k for row in idx)
    u = 2.0 ** -24
    # direct form: 7u (|zx| + |zf|)^2 per square, (m - 1) u on the sum, 2u multiply and divide
    direct = (m + 8) * u * np.take_along_axis(Sd, idx, axis=1)
    d64 = np.take_along_axis(d64all, idx, axis=1)
    assert (np.abs(d2.numpy().astype(np.float64) - d64) <= direct).all()
    vals = F[:, target].astype(np.float64)[idx]
    assert (np.abs(est.numpy() - vals.mean(1)) <= k * u * np.abs(vals).sum(1) / k).all()  # k - 1 adds, a divide
    assert (np.sort(d64, axis=1)[met] <= ds[met, :k] + 2 * direct.max(1, keepdims=True)[met]).all()


def test_repeats_empty_rows_and_refusals(ext):
    g = torch.Generator().manual_seed(5)
    x, rows, center, F, target = _int_case(200, 300, 20, 5, g)
    xd, Fd, rd = x.to(DEV), F.to(DEV), rows.to(DEV)
    cols = [xd[i] for i in range(20)]
    first = ext.knn_impute_bf16x2(cols, rd, center, Fd, target, 5)
    for _ in range(3):
        for a, b in zip(first, ext.knn_impute_bf16x2(cols, rd, center, Fd, target, 5)):
            assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))
    est, idx, d2 = ext.knn_impute_bf16x2(cols, rd[:0], center, Fd, target, 5)
    assert est.numel() == 0 and tuple(idx.shape) == tuple(d2.shape) == (0, 5)
    for match, args in [
        ("KNN_MAX_COLS", ([xd[0]] * 129, rd, torch.zeros(129, dtype=torch.float64), torch.zeros(4, 129, device=DEV), 0, 5)),
        ("KNN_MAX_K", (cols, rd, center, Fd, target, 9)),
        ("device columns required", ([t.cpu() for t in cols], rd, center, Fd, target, 5)),
        ("contiguous", ([xd[:, ::2][i] for i in range(20)], rd, center, Fd, target, 5)),
    ]:
        with pytest.raises(RuntimeError, match=match):
            ext.knn_impute_bf16x2(*args)
