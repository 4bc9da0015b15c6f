"""correlation_matrix(null_policy="pairwise") and
pairwise_observation_counts over two gloo ranks equal the single-process
result: the four sums (N, P, S, Q) are plain sums over rows about the
global column means, merged with one fp64 all-reduce, so only the order
of the additions differs (matrix to 1e-12, NaNs in the same places, counts
exactly).

Case "halves": the frame is sorted by one column, so the shards hold
disjoint value ranges. Case "empty": rank 1 holds no rows and must still
take part in every collective."""

import json
import multiprocessing as mp
import os
import socket

import numpy as np
import pandas as pd
import pytest


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


N = 3000
COLS = ["cont", "skew32", "ints", "nulls", "sparse", "allnull", "lowhalf"]


def _make_pdf():
    rng = np.random.default_rng(79)
    z = rng.normal(size=N)
    nulls = z + rng.normal(size=N)
    nulls[rng.random(N) < 0.3] = np.nan
    sparse = -z + rng.normal(size=N)
    sparse[rng.random(N) < 0.9] = np.nan
    skew = np.exp(z + rng.normal(size=N)).astype(np.float32)
    skew[rng.random(N) < 0.1] = np.nan
    # sorted by z: the two halves hold disjoint value ranges of `cont`,
    # and `lowhalf` has all its values on rank 0
    order = np.argsort(z)
    pdf = pd.DataFrame({
        "cont": z,
        "skew32": skew,
        "ints": rng.integers(0, 9, N).astype(np.float64),
        "nulls": nulls,
        "sparse": sparse,
        "allnull": np.full(N, np.nan),
        "lowhalf": np.where(z < np.median(z), z + rng.normal(size=N), np.nan),
    })
    return pdf.iloc[order].reset_index(drop=True)


def _shard(pdf, case, rank):
    if case == "halves":
        half = len(pdf) // 2
        return pdf.iloc[rank * half : (rank + 1) * half]
    return pdf if rank == 0 else pdf.iloc[0:0]  # "empty": rank 1 holds nothing


def _compute(ctx, idf):
    from anovos_amd.data_analyzer import association_evaluator as ae

    res = {}
    for name, m in (
        ("corr", ae.correlation_matrix(ctx, idf, null_policy="pairwise")),
        ("corr_min_periods", ae.correlation_matrix(ctx, idf, null_policy="pairwise", min_periods=400)),
        ("counts", ae.pairwise_observation_counts(ctx, idf)),
    ):
        vals = m[list(m["attribute"])].to_numpy(dtype=np.float64)
        res[name] = {"columns": list(m.columns), "attribute": list(m["attribute"]),
                     "values": [[None if v != v else v for v in row] for row in vals.tolist()]}
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


def _values(entry):
    return np.array([[np.nan if v is None else v for v in row] for row in entry["values"]], dtype=np.float64)


@pytest.mark.parametrize("case", ["halves", "empty"])
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
    for name in ("corr", "corr_min_periods", "counts"):
        assert res[name]["columns"] == single[name]["columns"] == ["attribute"] + sorted(COLS)
        assert res[name]["attribute"] == single[name]["attribute"]
    for name in ("corr", "corr_min_periods"):
        got, want = _values(res[name]), _values(single[name])
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max() <= 1e-12
    np.testing.assert_array_equal(_values(res["counts"]), _values(single["counts"]))
    # the single-process result is the pairwise one, and the rows are there
    pdf = _make_pdf()
    srt = sorted(COLS)
    want = _values(single["corr"])
    ref = pdf[srt].astype(np.float64).corr(min_periods=2).to_numpy()
    np.testing.assert_array_equal(np.isnan(want), np.isnan(ref))
    assert np.abs(want[~np.isnan(ref)] - ref[~np.isnan(ref)]).max() <= 1e-8
    present = pdf[srt].notna().to_numpy().astype(np.int64)
    np.testing.assert_array_equal(_values(single["counts"]), present.T @ present)
    assert np.isnan(_values(single["corr_min_periods"])).sum() > np.isnan(want).sum()
    i, j = srt.index("cont"), srt.index("nulls")
    assert want[i, j] > 0.5
