"""imputation_matrixFactorization(precision="bf16x2") (ops/als.py, kernel K32)
against als_fit_fp64, the fp64 numpy fit from the same V0; the default
precision untouched; two gloo ranks against one process."""

import multiprocessing as mp
import os
import socket

import numpy as np
import pandas as pd
import pytest
import torch

from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.ops import als
from anovos_amd.shared.context import AnovosContext

COLS = list("abcdefgh")
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


def _make(n, seed=91, wide=False):
    """(frame with 10 % nulls, truth): rank 3 plus noise over 8 columns; with `wide`, column a is
    f32 and 1e8 off zero, column b the only f64 one."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 3)) @ rng.normal(size=(3, 8)) + 0.2 * rng.normal(size=(n, 8))
    X = X * np.array([1e3, 5.0, 50.0, 2.0, 1.0, 0.1, 3.0, 7.0]) + np.array([1e8 if wide else 10.0, -3, 0, 40, 1, 0, 5, -9])
    pdf = pd.DataFrame(X, columns=COLS).astype(np.float32 if wide else np.float64)
    if wide:
        pdf["b"] = X[:, 1]
    truth = pdf.to_numpy(dtype=np.float64)
    return pdf.mask(rng.random((n, 8)) < 0.1), truth


def _impute(idf, device, **kw):
    from anovos_amd.data_transformer.transformers import imputation_matrixFactorization as mf

    odf = mf(AnovosContext(device), idf, list_of_cols=COLS, rank=3, max_iter=5, **kw)
    return np.column_stack([odf.col(c).data.double().cpu().numpy() for c in COLS])


def _reference(idf):
    mu, sd, _ = als.column_scales(idf, COLS)
    X = np.column_stack([idf.col(c).data.double().cpu().numpy() for c in COLS])
    return als.als_fit_fp64(X, mu, sd, als.als_v0(idf, COLS, sd, 3), 5, 0.01)[0], sd


def test_cpu_matches_fp64_definition():
    idf = AnovosFrame.from_pandas(_make(3000)[0], device="cpu")
    ref, sd = _reference(idf)
    assert np.abs((_impute(idf, "cpu", precision="bf16x2") - ref) / sd).max() <= 1e-9


def test_default_is_untouched_and_unknown_precision_raises():
    idf = AnovosFrame.from_pandas(_make(500)[0], device="cpu")
    torch.manual_seed(0)
    first = _impute(idf, "cpu")
    torch.manual_seed(0)
    assert np.array_equal(first, _impute(idf, "cpu", precision="fp32"))
    with pytest.raises(TypeError):
        _impute(idf, "cpu", precision="fp64")


def _worker(rank, port, out_dir):
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": "2",
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as td

    from anovos_amd.core import dist

    dist.init_from_env(timeout_s=120)
    pdf = _make(3000)[0]
    shard = pdf if rank == 0 else pdf.iloc[0:0]  # rank 1 holds nothing and joins every collective
    got = _impute(AnovosFrame.from_pandas(shard.reset_index(drop=True), device="cpu"), "cpu", precision="bf16x2")
    np.save(os.path.join(out_dir, f"res{rank}.npy"), got)
    td.barrier()
    td.destroy_process_group()


def test_two_gloo_ranks_match_single_process(tmp_path, monkeypatch):
    monkeypatch.setenv("ANOVOS_AMD_DIST_BACKEND", "gloo")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [mp.get_context("spawn").Process(target=_worker, args=(r, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0, f"worker failed: exit {p.exitcode}"
    idf = AnovosFrame.from_pandas(_make(3000)[0], device="cpu")
    single = _impute(idf, "cpu", precision="bf16x2")
    got = np.load(tmp_path / "res0.npy")
    assert np.load(tmp_path / "res1.npy").shape == (0, 8)
    assert np.abs((got - single) / als.column_scales(idf, COLS)[1]).max() <= 1e-9


# largest |K32 - fp64| in sd units measured on MI355X on this data, and the asserted 4 x it
E2E_MEASURED = 2.029e-3
E2E_TOL = 4 * E2E_MEASURED


@pytest.mark.gpu
@needs_gpu
def test_gpu_end_to_end():
    """20 000 x 8, true rank 3 plus noise, column a f32 and 1e8 off zero, column b f64, 10 %
    nulls, rank 3: imputed entries against als_fit_fp64 from the same V0, in sd units.
    Measured on MI355X: 2.029e-3 sd, all of it the f32 spacing (8) of the column at 1e8, whose
    sd is about 2000; the other columns stay below 1e-4 (8.9e-5). Asserted at 4 x that, which must stay
    below a tenth of the reference's own held-out RMSE (0.337 sd)."""
    pdf, truth = _make(20_000, wide=True)
    idf = AnovosFrame.from_pandas(pdf, device="cuda")
    ref, sd = _reference(idf)
    got = _impute(idf, "cuda", precision="bf16x2")
    null = pdf.isna().to_numpy()
    dev = np.abs((got - ref) / sd)[null].max()
    rmse = np.sqrt((((ref - truth) / sd)[null] ** 2).mean())
    print(f"largest deviation {dev:.3e} sd, held-out RMSE of the reference {rmse:.3e} sd")
    assert np.array_equal(got[~null], ref[~null])
    print(f"other columns: {np.abs((got - ref) / sd)[:, 1:][null[:, 1:]].max():.3e} sd")
    assert E2E_TOL < 0.1 * rmse
    assert dev <= E2E_TOL


@pytest.mark.gpu
@needs_gpu
def test_gpu_memory():
    """2^21 rows x 20 columns, rank 10 (KR = 12): beyond the frame and the output clones the fit
    peaks at no more than U (KR * 4 * n bytes) plus 32 MiB."""
    n, m = 1 << 21, 20
    g = torch.Generator(device="cuda").manual_seed(5)
    cols = [f"c{j}" for j in range(m)]
    data = {}
    for c in cols:
        x = torch.randn(n, device="cuda", generator=g)
        x[torch.rand(n, device="cuda", generator=g) < 0.1] = float("nan")
        data[c] = Column(c, "float", x)
    idf = AnovosFrame(data, device="cuda")
    clones = {c: idf.col(c).data.clone() for c in cols}
    als.column_scales(idf, cols)  # the cached moments are not part of the fit
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    als.als_impute(idf, cols, 10, 2, 0.01, clones)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak beyond frame and clones: {extra / 2 ** 20:.1f} MiB")
    assert extra <= 12 * 4 * n + (32 << 20)
    assert not any(bool(torch.isnan(t).any()) for t in clones.values())
