"""Time the projection kernel (K27) against the library path of PCA's apply.

Workload shape: 150 float32 columns (the numeric block of the flagship
benchmark) at 32M rows with 5 % NaN per column, generated as in
tools/bench_pairwise_corr.py; mean, sd and the components W [r, 150]
(eigenvectors of the correlation matrix) are fitted on a 1M-row sample.

  (a) K27 project_columns_bf16x2 into r preallocated columns, r in --ranks;
      bytes = the frame once plus the r columns it writes.
  (b) the library path - what PCA_latentFeatures did before the kernel:
      the standardization pass (scale_columns, one new f32 column per input
      column), X = stack(nan_to_num(column)) as f32 [n, k], X @ W through
      torch.matmul (rocBLAS). Same bytes figure, so the TB/s column says how
      far from one read and one write of the data each path is.
  (c) PCA_latentFeatures(output_mode="replace") end to end with saved models
      (standardization and components), wall clock around a synchronised
      call, and the peak of torch.cuda.max_memory_allocated beyond what was
      allocated before the call - next to the same figure of (b).
  (d) accuracy: the largest |kernel - library| and, on the first 200 000
      rows, both against the fp64 product, relative to the largest score.

Kernels are timed with device events around each repetition after warm-up;
the median is reported with the extremes.

    python tools/bench_project.py --rows 32000000
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_pairwise_corr import make_values, timed, wall  # noqa: E402

NCOLS = 150


def library_scores(values, mean, inv_sd, W_kr):
    from anovos_amd.ops import elementwise

    scaled = elementwise.scale_columns(values, mean, inv_sd)
    X = torch.stack([torch.nan_to_num(t, nan=0.0) for t in scaled], dim=1)
    return X @ W_kr


def peak_beyond(fn):
    """(result, bytes): the peak of allocated device memory during fn beyond
    what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = fn()
    torch.cuda.synchronize()
    return res, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32_000_000)
    ap.add_argument("--ranks", type=int, nargs="*", default=[8, 32, 150])
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_project needs a GPU: a CPU timing says nothing about the kernel")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.data_transformer import transformers_advanced as TA
    from anovos_amd.ops import backend
    from anovos_amd.shared.context import AnovosContext

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    rows = args.rows
    results = []
    print(f"columns={NCOLS} float32, rows={rows}, null rate {args.null_rate}")
    print(f"{'r':>4} {'variant':<58} {'median ms':>10} {'min':>9} {'max':>9} {'GB':>7} {'TB/s':>6}")

    def report(r, name, t, nbytes, extra=None):
        med, lo, hi = t
        tbs = nbytes / (med * 1e-3) / 1e12
        print(f"{r:>4} {name:<58} {med:>10.2f} {lo:>9.2f} {hi:>9.2f} {nbytes / 1e9:>7.1f} {tbs:>6.2f}", flush=True)
        results.append({"r": r, "variant": name, "median_ms": med, "min_ms": lo, "max_ms": hi,
                        "bytes": nbytes, "tb_per_s": tbs, **(extra or {})})

    values = make_values(rows, NCOLS, args.null_rate, g, dev)
    names = [f"c{j:03d}" for j in range(NCOLS)]
    idf = AnovosFrame({n: Column(n, "float", t) for n, t in zip(names, values)}, device=dev)
    m = min(rows, 1_000_000)
    sample = AnovosFrame({n: Column(n, "float", t[:m]) for n, t in zip(names, values)}, device=dev)
    ctx = AnovosContext("cuda:0")
    model_dir = tempfile.mkdtemp(prefix="bench_project_")
    zcfg = {"pre_existing_model": False, "model_path": model_dir}
    TA.PCA_latentFeatures(ctx, sample, explained_variance_cutoff=1.0, model_path=model_dir,
                          standardization_configs=zcfg)
    zm = pd.read_parquet(os.path.join(model_dir, "z_standardization", "part-00000.parquet")).set_index("feature")
    comp_path = os.path.join(model_dir, "PCA_latentFeatures", "components.parquet")
    comp = pd.read_parquet(comp_path)
    mean = [float(zm.loc[n, "mean"]) for n in names]
    inv_sd = [1.0 / float(zm.loc[n, "stddev"]) for n in names]
    shift = torch.tensor(mean, dtype=torch.float64).to(torch.float32).to(dev)
    scale = torch.tensor(inv_sd, dtype=torch.float64).to(torch.float32).to(dev)
    W_all = torch.tensor(np.ascontiguousarray(comp.values.T), dtype=torch.float32, device=dev)  # [150, k]
    frame_bytes = NCOLS * rows * 4
    zcfg = {"pre_existing_model": True, "model_path": model_dir}

    for r in args.ranks:
        W = W_all[:r].contiguous()
        W_kr = W.T.contiguous()
        nbytes = frame_bytes + r * rows * 4
        outs = [torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(r)]
        a = timed(lambda: ext.project_columns_bf16x2(values, shift, scale, W, outs), args.warmup, args.reps)
        report(r, "K27 project_columns_bf16x2, direct 64-byte-run stores", a, nbytes)

        (Y, lib_peak) = peak_beyond(lambda: library_scores(values, mean, inv_sd, W_kr))
        top = float(Y.abs().max())
        dev_kl = max(float((outs[c] - Y[:, c]).abs().max()) for c in range(r)) / top
        s = min(rows, 200_000)
        Z = torch.stack([v[:s].double() for v in values], dim=1)
        Z = (Z - torch.tensor(mean, device=dev)) * torch.tensor(inv_sd, device=dev)
        Z = torch.where(torch.isnan(Z), torch.zeros_like(Z), Z)
        ref = Z @ W_kr.double()
        err_k = float((torch.stack([o[:s] for o in outs], dim=1).double() - ref).abs().max()) / float(ref.abs().max())
        err_l = float((Y[:s].double() - ref).abs().max()) / float(ref.abs().max())
        del Y, Z, ref
        lib = timed(lambda: library_scores(values, mean, inv_sd, W_kr), 1, max(2, args.reps // 3))
        report(r, "library path (scale_columns, stack, torch.matmul)", lib, nbytes,
               {"peak_bytes_beyond_frame": lib_peak})
        del outs
        torch.cuda.empty_cache()

        comp.iloc[:, :r].to_parquet(comp_path)
        call = lambda: TA.PCA_latentFeatures(ctx, idf, pre_existing_model=True, model_path=model_dir,  # noqa: E731
                                             standardization_configs=zcfg, output_mode="replace")
        _, pca_peak = peak_beyond(call)
        e2e = wall(call, max(2, args.reps // 3))
        report(r, "PCA_latentFeatures(replace), saved models, wall clock", e2e, nbytes,
               {"peak_bytes_beyond_frame": pca_peak})
        print(f"{r:>4} library path {lib[0] / a[0]:.2f} x the kernel's time; peak memory beyond the frame: "
              f"PCA_latentFeatures {pca_peak / 1e9:.2f} GB (r columns = {r * rows * 4 / 1e9:.2f} GB), library path "
              f"{lib_peak / 1e9:.2f} GB; largest |kernel - library| {dev_kl:.2e} of the largest score ({top:.1f}); "
              f"against fp64 on {s} rows: kernel {err_k:.2e}, library {err_l:.2e}", flush=True)
        results.append({"r": r, "variant": "agreement", "library_over_kernel": lib[0] / a[0],
                        "pca_peak_bytes_beyond_frame": pca_peak, "library_peak_bytes_beyond_frame": lib_peak,
                        "max_rel_kernel_library": dev_kl, "max_rel_kernel_fp64": err_k,
                        "max_rel_library_fp64": err_l})
        torch.cuda.empty_cache()

    print(json.dumps({"bench": "project", "columns": NCOLS, "rows": rows, "null_rate": args.null_rate,
                      "results": results}))


if __name__ == "__main__":
    main()
