"""correlation_matrix(method="spearman") over two gloo ranks equals the
single-process result to 1e-12: the grid comes from global quantiles, the
cell counts merge with one int64 all-reduce, and the fp64 Grams of the
ranks' slabs add up (only their summation order differs).

Case "halves": each rank holds half the rows. Case "empty": rank 1 holds
no rows and must still take part in every collective."""

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
COLS = ["cont", "skew32", "ties", "ints", "nulls", "allnull"]


def _make_pdf():
    rng = np.random.default_rng(77)
    z = rng.normal(size=N)
    nulls = z + rng.normal(size=N)
    nulls[rng.random(N) < 0.1] = np.nan
    # sorted by z: the two halves hold disjoint value ranges of `cont`
    order = np.argsort(z)
    pdf = pd.DataFrame({
        "cont": z,
        "skew32": np.exp(z + rng.normal(size=N)).astype(np.float32),
        "ties": np.where(rng.random(N) < 0.2, 0.5, (z + rng.normal(size=N)).round(1)),
        "ints": rng.integers(0, 9, N).astype(np.float64),
        "nulls": nulls,
        "allnull": np.full(N, np.nan),
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
    for cells in (1024, 64):
        m = ae.correlation_matrix(ctx, idf, method="spearman", rank_cells=cells)
        res[str(cells)] = {"columns": list(m.columns), "attribute": list(m["attribute"]),
                           "values": m[list(m["attribute"])].to_numpy(dtype=np.float64).tolist()}
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
    for cells in ("1024", "64"):
        assert res[cells]["columns"] == single[cells]["columns"] == ["attribute"] + sorted(COLS)
        assert res[cells]["attribute"] == single[cells]["attribute"]
        got = np.array(res[cells]["values"], dtype=np.float64)
        want = np.array(single[cells]["values"], dtype=np.float64)
        assert not np.isnan(got).any()
        assert np.abs(got - want).max() <= 1e-12
    # the rows are there: a rank-disjoint column still correlates
    want = np.array(single["1024"]["values"])
    i, j = sorted(COLS).index("cont"), sorted(COLS).index("nulls")
    assert want[i, j] > 0.5
