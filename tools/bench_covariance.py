"""Time the split-bf16 Gram kernel (K28) and covariance_matrix built on it.

Workload shape: 150 float32 columns (the numeric block of the flagship
benchmark) at 32M rows with 5 % NaN per column, the data of
tools/bench_pairwise_corr.py.

  (a) K28 centered_gram_bf16x2 at SPLITGRAM_FLUSH_ROWS and at the flush
      settings of --flush-rows, alternating within every repetition; bytes =
      the columns once (the HBM read multiple is ceil(k / 64) = 3)
  (b) K8 centered_gram_bf16 and K25 pairwise_gram_bf16 on the same data
  (c) covariance_matrix(precision="bf16x2") and ("fp64"): wall clock around
      a synchronised call, and torch.cuda.max_memory_allocated beyond the
      frame; the fp64 path stacks an fp64 copy of the frame, so --fp64-rows
      gives the rows it runs on (the first rows of the same columns)
  (d) accuracy against an fp64 Gram of the first 200 000 rows: the largest
      |G - G64| / (gamma sum |z_i| |z_j|) of K28, and the largest error of
      K28 and K8 relative to sqrt(G_ii G_jj); the largest eigenvalue error of
      the correlation matrix against k gamma

Kernels are timed with device events around each repetition after warm-up;
the median is reported.

    python tools/bench_covariance.py --rows 32000000
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

from tools.bench_pairwise_corr import NCOLS, make_values  # noqa: E402

ACC_ROWS = 200_000


def timed_alternating(fns, warmup: int, reps: int):
    """Median, min, max ms of every fn; one repetition runs each fn once, in
    order, so drift of the machine falls on all of them alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms[i].append(t0.elapsed_time(t1))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def wall_and_peak(fn, reps: int):
    """(median, min, max) wall ms of a synchronised call and the peak of
    allocated device memory beyond what was allocated before it."""
    ms, peak = [], 0
    for _ in range(reps):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
        peak = max(peak, torch.cuda.max_memory_allocated() - before)
    return (statistics.median(ms), min(ms), max(ms)), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32_000_000)
    ap.add_argument("--fp64-rows", type=int, default=None,
                    help="rows of the fp64 path's run (default: --rows)")
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--flush-rows", type=int, nargs="*", default=[1024],
                    help="flush settings (ANOVOS_SPLITGRAM_FLUSH_ROWS) to time against the built-in one")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_covariance needs a GPU: a CPU timing says nothing about the kernels")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.ops import backend, corr, stats

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    rows = args.rows
    results = []
    print(f"columns={NCOLS} float32, null rate {args.null_rate}")
    print(f"{'rows':>10} {'variant':<58} {'median ms':>10} {'min':>9} {'max':>9} {'TB/s':>6} {'peak GB':>8}")

    def report(nrows, name, t, peak=None):
        med, lo, hi = t
        tbs = NCOLS * nrows * 4 / (med * 1e-3) / 1e12
        pk = f"{peak / 1e9:>8.3f}" if peak is not None else f"{'':>8}"
        print(f"{nrows:>10} {name:<58} {med:>10.2f} {lo:>9.2f} {hi:>9.2f} {tbs:>6.2f} {pk}", flush=True)
        results.append({"rows": nrows, "variant": name, "median_ms": med, "min_ms": lo, "max_ms": hi,
                        "tb_per_s": tbs, "peak_bytes": peak})

    values = make_values(rows, NCOLS, args.null_rate, g, dev)
    names = [f"c{j:03d}" for j in range(NCOLS)]
    idf = AnovosFrame({n: Column(n, "float", t) for n, t in zip(names, values)}, device=dev)
    moments = stats.frame_moments(idf, names)
    mean64 = torch.tensor([moments[n].mean for n in names], dtype=torch.float64, device=dev)
    mean32 = mean64.to(torch.float32)

    def k28(flush):
        def run():
            if flush is None:
                os.environ.pop("ANOVOS_SPLITGRAM_FLUSH_ROWS", None)
            else:
                os.environ["ANOVOS_SPLITGRAM_FLUSH_ROWS"] = str(flush)
            return ext.centered_gram_bf16x2(values, mean64)
        return run

    flushes = [None] + list(args.flush_rows)
    labels = [f"K28 centered_gram_bf16x2, flush every {f or ext.SPLITGRAM_FLUSH_ROWS} rows" for f in flushes]
    fns = [k28(f) for f in flushes] + [lambda: ext.pairwise_gram_bf16(values, mean32),
                                       lambda: ext.centered_gram_bf16(values, mean32)]
    labels += ["K25 pairwise_gram_bf16 (three planes, six products)", "K8 centered_gram_bf16 (one plane, fp32 out)"]
    for name, t in zip(labels, timed_alternating(fns, args.warmup, args.reps)):
        report(rows, name, t)
    os.environ.pop("ANOVOS_SPLITGRAM_FLUSH_ROWS", None)

    t, peak = wall_and_peak(lambda: corr.covariance_matrix(idf, names, moments=moments, precision="bf16x2"), args.reps)
    report(rows, 'covariance_matrix(precision="bf16x2")', t, peak)
    frows = args.fp64_rows or rows
    sub = AnovosFrame({n: Column(n, "float", v[:frows]) for n, v in zip(names, values)}, device=dev)
    t, peak = wall_and_peak(lambda: corr.covariance_matrix(sub, names, moments=moments, precision="fp64"), 3)
    report(frows, 'covariance_matrix(precision="fp64")', t, peak)
    del sub

    # accuracy on the first ACC_ROWS rows, about the fp64 mean of those rows
    head = [v[:ACC_ROWS] for v in values]
    X = torch.stack(head).to(torch.float64)
    m = torch.nanmean(X, dim=1)
    Z = torch.nan_to_num(X - m[:, None], nan=0.0)
    G64 = Z @ Z.T
    A = Z.abs() @ Z.abs().T
    d = torch.sqrt(torch.diag(G64))
    G28 = ext.centered_gram_bf16x2(head, m)
    G8 = ext.centered_gram_bf16(head, m.to(torch.float32)).to(torch.float64)
    C64, C28 = (G64 / torch.outer(d, d)).cpu().numpy(), (G28 / torch.outer(d, d)).cpu().numpy()
    acc = {
        "rows": ACC_ROWS, "variant": "accuracy", "gamma": corr.SPLITGRAM_GAMMA,
        "k28_max_err_over_bound": float(((G28 - G64).abs() / (corr.SPLITGRAM_GAMMA * A)).max()),
        "k28_max_rel_err": float(((G28 - G64).abs() / torch.outer(d, d)).max()),
        "k8_max_rel_err": float(((G8 - G64).abs() / torch.outer(d, d)).max()),
        "k28_max_eigenvalue_err": float(np.abs(np.linalg.eigvalsh(C28) - np.linalg.eigvalsh(C64)).max()),
        "eigenvalue_floor_k_gamma": NCOLS * corr.SPLITGRAM_GAMMA,
    }
    print(" ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in acc.items()), flush=True)
    results.append(acc)
    print(json.dumps({"bench": "covariance", "columns": NCOLS, "null_rate": args.null_rate, "results": results}))


if __name__ == "__main__":
    main()
