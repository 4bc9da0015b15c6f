"""Time the rank-grade kernels (K24) and spearman_matrix built on them.

Workload shape: 150 float32 columns (the numeric block of the flagship
benchmark) at 4M and 32M rows, 1024 cells. Every third column is normal,
every third log-normal, the rest rounded to one decimal (heavy ties);
about 1 % NaN.

  (a) grade_counts: the read-only counting pass, bytes = the columns read
  (b) grade_apply: the transform pass into a preallocated slab, bytes =
      columns read + f32 slab written
  (c) bucketize_columns_float_counts at the same cutoffs: the nearest
      existing kernel (K6 with counts), reads the columns and writes a
      binned f32 copy, bytes = read + written
  (d) spearman_matrix, cold (quantile sketch, counting pass, tables,
      transform + Gram) and with the grade cache warm (transform + Gram),
      the warm call also at SLAB_BYTES of 1, 4 and 16 GiB
  (e) the sort-based route on --sort-cols columns: torch.sort, mid-ranks
      from run lengths, scatter back, centred f32 Gram; reported per column
  (f) the LDS-atomic path against a contended column: 150 columns of 40
      distinct values (39 cutoffs + their predecessors, shared counters that
      all rows of a value hit), of 2 distinct values (private counters) and
      the smooth columns of (a)

Kernels are timed with device events around each repetition after warm-up;
the median is reported. spearman_matrix is timed with a wall clock around
a synchronised call (it ends with a copy to the host). The counts of (a)
are compared for equality with those of (c).

    python tools/bench_spearman.py --rows 4000000 32000000
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


def make_values(rows: int, ncols: int, g, dev):
    cols = []
    for j in range(ncols):
        x = torch.randn(rows, generator=g, device=dev, dtype=torch.float32)
        if j % 3 == 1:
            x = torch.exp(x * 0.8)
        elif j % 3 == 2:
            x = torch.round(x * 10.0 * (1.0 + j % 5)) / 10.0
        else:
            x = x * (1.0 + j % 7) + float(j % 11)
        x[torch.rand(rows, generator=g, device=dev) < 0.01] = float("nan")
        cols.append(x)
    return cols


def make_discrete(rows: int, ncols: int, distinct: int, g, dev):
    return [torch.randint(0, distinct, (rows,), generator=g, device=dev).to(torch.float32) * 0.37 + 0.1
            for _ in range(ncols)]


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


def sort_route(cols):
    """Spearman by sorting: per column torch.sort, mid-ranks from the run
    lengths of the sorted values, scattered back; NaN takes the mean rank;
    then the centred f32 Gram."""
    ranks = []
    for x in cols:
        ok = ~torch.isnan(x)
        m = int(ok.sum())
        xs, idx = torch.sort(x)  # NaN sorts last
        _, inv, cnt = torch.unique_consecutive(xs[:m], return_inverse=True, return_counts=True)
        before = torch.cumsum(cnt, 0) - cnt
        mid = before.to(torch.float64) + (cnt.to(torch.float64) + 1.0) / 2.0
        r = torch.zeros(x.numel(), dtype=torch.float32, device=x.device)
        r[idx[:m]] = ((mid[inv] - (m + 1) / 2.0) / max(m, 1)).to(torch.float32)
        ranks.append(r)
    X = torch.stack(ranks)
    return X @ X.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[4_000_000, 32_000_000])
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--sort-cols", type=int, default=16)
    ap.add_argument("--slab-gib", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_spearman needs a GPU: a CPU timing says nothing about the kernels")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.ops import backend, rank

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    results = []
    all_ok = True
    head = f"{'rows':>10} {'variant':<44} {'median ms':>10} {'min':>9} {'max':>9} {'GB moved':>9} {'TB/s':>6}"
    print(f"columns={NCOLS} float32, cells={args.cells}, GRADE_MAX_CELLS={ext.GRADE_MAX_CELLS}")
    print(head)

    def report(rows, name, t, nbytes, extra=None):
        med, lo, hi = t
        tbs = nbytes / (med * 1e-3) / 1e12 if nbytes else float("nan")
        print(f"{rows:>10} {name:<44} {med:>10.2f} {lo:>9.2f} {hi:>9.2f} {nbytes / 1e9:>9.1f} {tbs:>6.2f}", flush=True)
        results.append({"rows": rows, "variant": name, "median_ms": med, "min_ms": lo, "max_ms": hi,
                        "bytes": nbytes, "tb_per_s": tbs, **(extra or {})})

    for rows in args.rows:
        values = make_values(rows, NCOLS, g, dev)
        names = [f"c{j:03d}" for j in range(NCOLS)]
        idf = AnovosFrame({n: Column(n, "float", t) for n, t in zip(names, values)}, device=dev)
        col_bytes = NCOLS * rows * 4

        t = time.perf_counter()
        grids = rank.rank_grid(idf, names, args.cells)
        torch.cuda.synchronize()
        grid_ms = (time.perf_counter() - t) * 1e3
        ncut = [len(c) for c in grids]
        print(f"{rows:>10} rank_grid (moments + quantile sketch, cold): {grid_ms:.0f} ms; cutoffs per column "
              f"min {min(ncut)} / median {int(statistics.median(ncut))} / max {max(ncut)}", flush=True)
        cuts = [torch.from_numpy(c) for c in grids]

        counts = ext.grade_counts(values, cuts)
        a = timed(lambda: ext.grade_counts(values, cuts), args.warmup, args.reps)
        report(rows, "K24 grade_counts (read)", a, col_bytes)

        m = counts[:, 1:].sum(dim=1).cpu().numpy()
        tables = [torch.from_numpy(rank.grade_tables(counts[i, 1 : ncut[i] + 2].cpu().numpy(), int(m[i])).astype(np.float32))
                  for i in range(NCOLS)]
        slab = torch.empty(NCOLS, rows, dtype=torch.float32, device=dev)
        outs = [slab[i] for i in range(NCOLS)]
        b = timed(lambda: ext.grade_apply(values, cuts, tables, 0.0, outs), args.warmup, args.reps)
        report(rows, "K24 grade_apply (read + write)", b, 2 * col_bytes)
        del slab, outs

        _, bcounts = ext.bucketize_columns_float_counts(values, cuts)
        same = bool(torch.equal(bcounts, counts))
        all_ok = all_ok and same
        c = timed(lambda: ext.bucketize_columns_float_counts(values, cuts), args.warmup, args.reps)
        report(rows, "K6 bucketize_columns_float_counts (r + w)", c, 2 * col_bytes, {"counts_agree": same})
        print(f"{rows:>10} per element: grade_counts {a[0] * 1e6 / (NCOLS * rows):.4f} ns, bucketize with counts "
              f"{c[0] * 1e6 / (NCOLS * rows):.4f} ns, grade_apply {b[0] * 1e6 / (NCOLS * rows):.4f} ns; "
              f"counts agree: {same}", flush=True)
        del bcounts
        torch.cuda.empty_cache()

        # ---- the whole matrix
        idf.clear_stats_cache()
        cold = wall(lambda: rank.spearman_matrix(idf, names, cells=args.cells), 1)
        report(rows, "spearman_matrix cold, bf16 Gram", cold, 0)
        warm = wall(lambda: rank.spearman_matrix(idf, names, cells=args.cells), args.reps)
        report(rows, f"spearman_matrix warm, SLAB_BYTES {rank.SLAB_BYTES >> 30} GiB", warm, 3 * col_bytes)
        ref = rank.spearman_matrix(idf, names, cells=args.cells)
        default_slab = rank.SLAB_BYTES
        for gib in args.slab_gib:
            rank.SLAB_BYTES = gib << 30
            slabs = -(-rows // max(4, (rank.SLAB_BYTES // (4 * NCOLS)) & ~3))
            w = wall(lambda: rank.spearman_matrix(idf, names, cells=args.cells), args.reps)
            dev_ = float(np.abs(rank.spearman_matrix(idf, names, cells=args.cells) - ref).max())
            report(rows, f"spearman_matrix warm, {gib} GiB slabs ({slabs})", w, 3 * col_bytes,
                   {"slabs": slabs, "max_abs_diff_to_default": dev_})
        rank.SLAB_BYTES = default_slab
        f32 = wall(lambda: rank.spearman_matrix(idf, names, cells=args.cells, use_bf16=False), args.reps)
        report(rows, "spearman_matrix warm, f32 Gram", f32, 3 * col_bytes)

        # ---- sorting instead
        k = min(args.sort_cols, NCOLS)
        if k:
            s = timed(lambda: sort_route(values[:k]), 1, max(2, args.reps // 2))
            report(rows, f"torch.sort route, {k} columns", s, 0, {"columns": k})
            sub = [names.index(n) for n in names[:k]]
            got = sort_route(values[:k]).to(torch.float64).cpu().numpy()
            d = np.sqrt(np.clip(np.diag(got), 1e-300, None))
            dev_sort = float(np.abs(np.clip(got / np.outer(d, d), -1, 1) - ref[np.ix_(sub, sub)])[~np.eye(k, dtype=bool)].max())
            print(f"{rows:>10} sort route {s[0] / k:.2f} ms per column, {s[0] / k * NCOLS:.0f} ms extrapolated to {NCOLS}; "
                  f"spearman_matrix warm {warm[0]:.1f} ms, cold {cold[0]:.0f} ms; largest |rho_grid - rho_sort| "
                  f"over the {k} columns {dev_sort:.2e}", flush=True)
        del values, idf
        torch.cuda.empty_cache()

        # ---- counter contention
        for distinct, label in ((40, "40 distinct values (shared LDS atomics)"),
                                (2, "2 distinct values (private counters)")):
            disc = make_discrete(rows, NCOLS, distinct, g, dev)
            vals = np.unique(disc[0].cpu().numpy().astype(np.float64))
            grid = rank._grid_from_quantiles(np.repeat(vals, 2), torch.float32, args.cells)
            dcuts = [torch.from_numpy(grid)] * NCOLS
            cnt = ext.grade_counts(disc, dcuts)
            occupied = int((cnt[0, 1:] > 0).sum())
            all_ok = all_ok and occupied == len(vals)
            e = timed(lambda: ext.grade_counts(disc, dcuts), args.warmup, args.reps)
            report(rows, f"K24 grade_counts, {label}", e, col_bytes,
                   {"cutoffs": len(grid), "occupied_cells": occupied, "smooth_median_ms": a[0]})
            print(f"{rows:>10} {distinct} distinct values, {len(grid)} cutoffs: {e[0] / a[0]:.2f} x the smooth columns' time",
                  flush=True)
            del disc, cnt
            torch.cuda.empty_cache()

    print(json.dumps({"bench": "spearman", "cells": args.cells, "columns": NCOLS, "results": results}))
    if not all_ok:
        sys.exit("grade_counts disagrees with the binning kernel's counts, or a distinct value lost its cell")


if __name__ == "__main__":
    main()
