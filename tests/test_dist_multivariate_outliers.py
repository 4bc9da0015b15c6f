"""multivariate_outlier_detection over two gloo ranks equals the
single-process result: the model comes from globally reduced moments and
one all-reduced fp64 covariance matrix, so every rank fits the same W (to
the order of the additions), the distances are per row, and the counts are
merged with one batched all-reduce that every rank takes part in.

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


N = 4000
COLS = ["a", "b", "c", "d", "lin", "const"]


def _make_pdf():
    rng = np.random.default_rng(83)
    f = rng.normal(size=(N, 2))
    X = f @ rng.normal(size=(2, 4)) + 0.3 * rng.normal(size=(N, 4))
    X = X * np.array([0.5, 5.0, 50.0, 2.0]) + np.array([100.0, -3.0, 0.0, 40.0])
    pdf = pd.DataFrame(X, columns=["a", "b", "c", "d"])
    # ten rows that are ordinary in every coordinate and break the structure
    sd = X.std(0)
    pdf.iloc[:10, :4] = X.mean(0) + sd * rng.uniform(-1.5, 1.5, (10, 4))
    pdf["lin"] = pdf["a"] - 2.0 * pdf["d"]
    pdf["const"] = 1.5
    pdf.loc[rng.random(N) < 0.05, "b"] = np.nan
    return pdf.sort_values("c").reset_index(drop=True)


def _shard(pdf, case, rank):
    if case == "halves":
        half = len(pdf) // 2
        return pdf.iloc[rank * half : (rank + 1) * half]
    return pdf if rank == 0 else pdf.iloc[0:0]  # "empty": rank 1 holds nothing


def _compute(ctx, idf):
    import warnings

    from anovos_amd.data_analyzer import quality_checker as qc

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the constant column is reported
        odf, stats = qc.multivariate_outlier_detection(ctx, idf, confidence=0.99, append_distance=True)
        cut, _ = qc.multivariate_outlier_detection(ctx, idf, confidence=0.99, treatment=True)
    thr = float(stats.loc[stats["metric"] == "threshold", "value"].iloc[0])
    d2 = odf.col("mahalanobis_d2").data.double()
    return {"stats": {m: v for m, v in zip(stats["metric"], stats["value"])},
            "d2": d2.tolist(), "flags": (d2 > thr).long().tolist(), "kept": cut.local_rows()}


def _worker(rank, port, case, out_dir):
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
    with open(os.path.join(out_dir, f"res{rank}.json"), "w") as f:
        json.dump(res, f)
    td.barrier()
    td.destroy_process_group()


@pytest.fixture(scope="module")
def single():
    """The single-process result, computed once for both cases."""
    from anovos_amd.core.frame import AnovosFrame
    from anovos_amd.shared.context import AnovosContext

    return _compute(AnovosContext("cpu"), AnovosFrame.from_pandas(_make_pdf(), device="cpu"))


@pytest.mark.parametrize("case", ["halves", "empty"])
def test_two_ranks_match_single_process(tmp_path, single, case):
    port = _free_port()
    mp_ctx = mp.get_context("spawn")
    procs = [mp_ctx.Process(target=_worker, args=(r, port, case, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0, f"worker failed: exit {p.exitcode}"
    res = []
    for r in range(2):
        with open(tmp_path / f"res{r}.json") as f:
            res.append(json.load(f))
    want = single["stats"]
    assert want["rank"] == 4.0 and want["attributes_count"] == 5.0
    assert want["excluded_constant_attributes"] == "const"
    assert want["outlier_rows"] >= 10
    for r in range(2):  # every rank reports the global figures
        got = res[r]["stats"]
        assert list(got) == list(want)
        for m in ("rows_count", "attributes_count", "rank", "threshold", "outlier_rows", "outlier_pct",
                  "excluded_constant_attributes"):
            assert got[m] == want[m], (r, m)
        assert got["max_distance"] == pytest.approx(want["max_distance"], rel=1e-6)
    # rows in shard order are the frame's rows in order
    d2 = np.array(res[0]["d2"] + res[1]["d2"])
    flags = np.array(res[0]["flags"] + res[1]["flags"])
    ref = np.array(single["d2"])
    assert d2.shape == ref.shape
    assert np.abs(d2 - ref).max() <= 1e-5 * ref.max()  # f32 results of models equal to ~1e-15
    assert np.array_equal(flags, np.array(single["flags"]))
    assert res[0]["kept"] + res[1]["kept"] == single["kept"] == N - int(want["outlier_rows"])
    if case == "empty":
        assert res[1]["d2"] == [] and res[1]["kept"] == 0
