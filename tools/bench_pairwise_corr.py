"""Time the pairwise-complete Gram kernel (K25) and pairwise_sums built on it.

Workload shape: 150 float32 columns (the numeric block of the flagship
benchmark) at 32M rows with 5 % NaN per column; every third column is
normal about a non-zero mean, every third log-normal, the rest rounded to
one decimal.

  (a) K25 pairwise_gram_bf16: the four matrices (N, P, S, Q) from one
      launch pair; bytes = the columns once (its HBM read multiple is
      ceil(k / 64) = 3 at this width, mostly served by the caches because
      the items that share a column group run side by side), also at the
      forced row splits of --chunks
  (b) K8 centered_gram_bf16 on the same data: one plane instead of three,
      one product per tile pair instead of six, every column read once -
      the lower bound
  (c) pairwise_sums through the library path of the same change
      (use_bf16=False): Z, Z*Z and M planes per row slab and four f32
      rocBLAS matmuls - the baseline - and through the kernel path, both
      with a wall clock around a synchronised call (they end with a copy
      to the host)
  (d) the largest difference between the two paths' correlation matrices

Kernels are timed with device events around each repetition after warm-up;
the median is reported.

    python tools/bench_pairwise_corr.py --rows 32000000
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NCOLS = 150


def make_values(rows: int, ncols: int, null_rate: float, g, dev):
    cols = []
    for j in range(ncols):
        x = torch.randn(rows, generator=g, device=dev, dtype=torch.float32)
        if j % 3 == 1:
            x = torch.exp(x * 0.8)
        elif j % 3 == 2:
            x = torch.round(x * 10.0 * (1.0 + j % 5)) / 10.0
        else:
            x = x * (1.0 + j % 7) + float(j % 11)
        x[torch.rand(rows, generator=g, device=dev) < null_rate] = float("nan")
        cols.append(x)
    return cols


def timed(fn, warmup: int, reps: int):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def wall(fn, reps: int):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[32_000_000])
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--chunks", type=int, nargs="*", default=[],
                    help="forced row splits (ANOVOS_PAIRGRAM_CHUNKS) to time next to the default")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_pairwise_corr needs a GPU: a CPU timing says nothing about the kernels")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.ops import backend, corr, stats

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    results = []
    head = f"{'rows':>10} {'variant':<52} {'median ms':>10} {'min':>9} {'max':>9} {'GB':>7} {'TB/s':>6}"
    print(f"columns={NCOLS} float32, null rate {args.null_rate}")
    print(head)

    def report(rows, name, t, nbytes, extra=None):
        med, lo, hi = t
        tbs = nbytes / (med * 1e-3) / 1e12 if nbytes else float("nan")
        print(f"{rows:>10} {name:<52} {med:>10.2f} {lo:>9.2f} {hi:>9.2f} {nbytes / 1e9:>7.1f} {tbs:>6.2f}", flush=True)
        results.append({"rows": rows, "variant": name, "median_ms": med, "min_ms": lo, "max_ms": hi,
                        "bytes": nbytes, "tb_per_s": tbs, **(extra or {})})

    for rows in args.rows:
        values = make_values(rows, NCOLS, args.null_rate, g, dev)
        names = [f"c{j:03d}" for j in range(NCOLS)]
        idf = AnovosFrame({n: Column(n, "float", t) for n, t in zip(names, values)}, device=dev)
        col_bytes = NCOLS * rows * 4
        moments = stats.frame_moments(idf, names)
        means = torch.tensor([moments[n].mean for n in names], dtype=torch.float32, device=dev)

        os.environ.pop("ANOVOS_PAIRGRAM_CHUNKS", None)
        a = timed(lambda: ext.pairwise_gram_bf16(values, means), args.warmup, args.reps)
        report(rows, "K25 pairwise_gram_bf16 (N, P, S, Q), default grid", a, col_bytes)
        for ch in args.chunks:
            os.environ["ANOVOS_PAIRGRAM_CHUNKS"] = str(ch)
            t = timed(lambda: ext.pairwise_gram_bf16(values, means), args.warmup, args.reps)
            report(rows, f"K25 pairwise_gram_bf16, {ch} row chunks per item", t, col_bytes, {"chunks": ch})
        os.environ.pop("ANOVOS_PAIRGRAM_CHUNKS", None)

        b = timed(lambda: ext.centered_gram_bf16(values, means), args.warmup, args.reps)
        report(rows, "K8 centered_gram_bf16 (one plane, NaN -> mean)", b, col_bytes)

        kern = wall(lambda: corr.pairwise_sums(idf, names, moments=moments), args.reps)
        report(rows, "pairwise_sums, kernel path", kern, col_bytes)
        lib = wall(lambda: corr.pairwise_sums(idf, names, moments=moments, use_bf16=False), max(2, args.reps // 2))
        slabs = -(-rows // max(1, min(corr.PAIR_SLAB_BYTES // (3 * NCOLS * 4), corr.PAIR_SLAB_MAX_ROWS)))
        report(rows, f"pairwise_sums, library path (4 f32 matmuls, {slabs} slabs)", lib, col_bytes, {"slabs": slabs})

        r_k = corr.pairwise_pearson_matrix(idf, names, moments=moments)
        r_l = corr.pairwise_pearson_matrix(idf, names, moments=moments, use_bf16=False)
        dev_r = float(np.nanmax(np.abs(r_k - r_l)))
        n_k = corr.pairwise_sums(idf, names, moments=moments)[0]
        n_l = corr.pairwise_sums(idf, names, moments=moments, use_bf16=False)[0]
        print(f"{rows:>10} K25 {a[0] / b[0]:.2f} x K8's time; library path {lib[0] / kern[0]:.1f} x the kernel path; "
              f"largest |r_kernel - r_library| {dev_r:.2e}; NaN entries {int(np.isnan(r_k).sum())} / "
              f"{int(np.isnan(r_l).sum())}; counts equal: {bool(np.array_equal(n_k, n_l))}", flush=True)
        results.append({"rows": rows, "variant": "agreement", "max_abs_r_diff": dev_r,
                        "counts_equal": bool(np.array_equal(n_k, n_l))})
        del values, idf
        torch.cuda.empty_cache()

    print(json.dumps({"bench": "pairwise_corr", "columns": NCOLS, "null_rate": args.null_rate, "results": results}))


if __name__ == "__main__":
    main()
