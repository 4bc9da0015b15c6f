"""grouped_moments and numerical_categorical_association over two gloo
ranks against the single-process result. The row counts merge exactly;
the shift of the sums is a global mean whose last bits may differ between
world sizes, so mean, M2 and the matrices are held to 1e-9 relative, not
to bit equality.

Case "disjoint": column `g` has rank-disjoint categories, so its
per-rank dictionaries differ in size and order until
align_dictionaries heals them. Case "empty": rank 1 holds no rows and
must still take part in every collective."""

import json
import multiprocessing as mp
import os
import socket

import numpy as np
import pandas as pd
import pytest

REL_TOL = 1e-9


@pytest.fixture(autouse=True)
def _gloo_backend(monkeypatch):
    """The spawned workers inherit this; without it a machine with one
    visible GPU picks RCCL and refuses two ranks on the same device."""
    monkeypatch.setenv("ANOVOS_AMD_DIST_BACKEND", "gloo")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


N = 1200
CATS = ["g", "w"]
NUMS = ["x", "z"]
METHODS = ("correlation_ratio", "eta_squared", "anova_f")


def _make_pdf():
    rng = np.random.default_rng(101)
    half = N // 2
    # first half (rank 0): g in {a, b, c}; second half (rank 1): g in {x, y}
    g = np.concatenate([rng.choice(["a", "b", "c"], half), rng.choice(["x", "y"], N - half)]).astype(object)
    w = rng.choice(["u", "v", "w"], N).astype(object)
    w[rng.choice(N, 40, replace=False)] = None
    x = rng.normal(0, 1, N) + (g == "a") * 1.2 + (w == "v") * 0.3
    x[rng.choice(N, 25, replace=False)] = np.nan
    z = 50.0 + rng.normal(0, 2, N) - (g == "y") * 1.5
    return pd.DataFrame({"g": g, "w": w, "x": x, "z": z})


def _shard(pdf, case, rank):
    if case == "disjoint":
        half = len(pdf) // 2
        return pdf.iloc[rank * half : (rank + 1) * half]
    return pdf if rank == 0 else pdf.iloc[0:0]  # "empty": rank 1 holds nothing


def _compute(ctx, idf):
    from anovos_amd.data_analyzer import association_evaluator as ae
    from anovos_amd.ops.grouped import grouped_moments

    mom = grouped_moments(idf, CATS, NUMS)
    # NaN (slots without a row) travels as None through JSON
    res = {"moments": {c + "|" + v: np.where(np.isnan(t), None, t.astype(object)).tolist() for (c, v), t in mom.items()},
           "dicts": {c: list(idf.col(c).dictionary) for c in CATS}}
    for method in METHODS:
        m = ae.numerical_categorical_association(ctx, idf, method_type=method)
        res[method] = {"columns": list(m.columns), "attribute": list(m["attribute"]),
                       "values": m[NUMS].to_numpy(dtype=np.float64).tolist()}
    return res


def _worker(rank, port, case, out_path):
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": "2",
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as td

    from anovos_amd.core import dist
    from anovos_amd.core.frame import AnovosFrame
    from anovos_amd.shared.context import init_context

    dist.init_from_env(timeout_s=120)
    ctx = init_context("cpu")
    shard = _shard(_make_pdf(), case, rank).reset_index(drop=True)
    idf = AnovosFrame.from_pandas(shard, device="cpu")
    res = _compute(ctx, idf)
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    td.barrier()
    td.destroy_process_group()


@pytest.fixture(scope="module")
def single():
    """The single-process result, computed once for both cases."""
    from anovos_amd.core.frame import AnovosFrame
    from anovos_amd.shared.context import AnovosContext

    return json.loads(json.dumps(_compute(AnovosContext("cpu"), AnovosFrame.from_pandas(_make_pdf(), device="cpu"))))


def _array(rows):
    return np.array([[np.nan if v is None else v for v in r] for r in rows], dtype=np.float64)


@pytest.mark.parametrize("case", ["disjoint", "empty"])
def test_two_ranks_match_single_process(tmp_path, single, case):
    port = _free_port()
    out = str(tmp_path / "res.json")
    mp_ctx = mp.get_context("spawn")
    procs = [mp_ctx.Process(target=_worker, args=(r, port, case, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0, f"worker failed: exit {p.exitcode}"
    with open(out) as f:
        res = json.load(f)
    assert res["dicts"] == single["dicts"]
    assert res["dicts"]["g"] == ["a", "b", "c", "x", "y"]
    assert set(res["moments"]) == {c + "|" + v for c in CATS for v in NUMS}
    for key, rows in res["moments"].items():
        got, want = _array(rows), _array(single["moments"][key])
        np.testing.assert_array_equal(got[:, 0], want[:, 0])  # n: exact
        np.testing.assert_allclose(got[:, 1:], want[:, 1:], rtol=REL_TOL, atol=0, equal_nan=True)
    pdf = _make_pdf()
    assert _array(res["moments"]["g|x"])[:, 0].sum() == pdf["x"].notna().sum()
    assert _array(res["moments"]["w|z"])[-1, 0] == 40  # the null slot
    for method in METHODS:
        assert res[method]["columns"] == single[method]["columns"] == ["attribute"] + NUMS
        assert res[method]["attribute"] == single[method]["attribute"] == CATS
        got = np.array(res[method]["values"], dtype=np.float64)
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, np.array(single[method]["values"], dtype=np.float64), rtol=REL_TOL, atol=0)
