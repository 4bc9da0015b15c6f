"""Time the grouped-moments kernel (K23) against the torch path it stands
beside (ops.grouped.grouped_sums_torch: bincount + two fp64 index_add_).

Workload shape: the categorical block of bench.make_synthetic_frame —
N_CAT int32 code columns with CAT_CARD categories and about 1 % nulls —
against N_NUM_CONT + N_NUM_INT float32 value columns with about 1 % NaN,
all N_CAT * N_NUM pairs.

  (a) grouped_moments: one launch; value columns that share a code column
      are packed into a work item when the dictionary fits one window of
      GRP_CELLS slots, a larger dictionary takes one item per window
  (b) torch path: per pair, slot mapping, NaN filter, bincount, two
      index_add_ over fp64

The torch path takes seconds per pair at this shape (fp64 index_add_ into
41 addresses), hours over all pairs, so it is timed on an evenly spaced
subset of the pairs (--baseline-pairs) and the kernel is timed on the same
subset next to it; the kernel is timed on all pairs as well. The sweep
times 1 code column x 2 value columns over dictionary sizes from
GRP_CELLS upwards: its crossover sets ops.grouped.KERNEL_MAX_SLOTS.

Both are timed with device events around each repetition after warm-up;
the median is reported. Bytes: (a) reads one column stream per work item
for the codes plus one per packed value column (from
grouped_moments_plan); for (b) the figure is the two columns each pair has
to read at the least — its int64 / fp64 intermediates are extra traffic on
top. TB/s is those bytes over the median time. At every timed shape the
row counts of (a) and (b) are compared for equality and the sums at 1e-9
relative to sum |d| and sum d^2 (the orders of summation differ).

    python tools/bench_grouped_moments.py --rows 4000000 32000000
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import CAT_CARD, N_CAT, N_NUM_CONT, N_NUM_INT  # noqa: E402

N_NUM = N_NUM_CONT + N_NUM_INT


def make_codes(rows: int, ncols: int, card: int, g, dev):
    cols = []
    for _ in range(ncols):
        codes = torch.randint(0, card, (rows,), generator=g, device=dev).to(torch.int32)
        codes[torch.rand(rows, generator=g, device=dev) < 0.01] = -1
        cols.append(codes)
    return cols


def make_values(rows: int, ncols: int, g, dev):
    cols = []
    for j in range(ncols):
        x = torch.randn(rows, generator=g, device=dev, dtype=torch.float32) * (1.0 + j % 7) + float(j % 11)
        x[torch.rand(rows, generator=g, device=dev) < 0.01] = float("nan")
        cols.append(x)
    return cols


def baseline(grouped_sums_torch, codes, sizes, values, shifts, pair_c, pair_v):
    return torch.cat([grouped_sums_torch(codes[c], sizes[c], values[v], shifts[v]).reshape(-1)
                      for c, v in zip(pair_c, pair_v)])


def agree(got: torch.Tensor, want: torch.Tensor, values, shifts, pair_v, sizes, pair_c) -> bool:
    """n equal; s1 / s2 within 1e-9 of the pair's sum |d| / sum d^2."""
    ok, off = True, 0
    for c, v in zip(pair_c, pair_v):
        k = sizes[c] + 1
        g = got[off : off + 3 * k].reshape(k, 3)
        w = want[off : off + 3 * k].reshape(k, 3)
        off += 3 * k
        d = torch.nan_to_num(values[v].to(torch.float64) - shifts[v], nan=0.0)
        good = (bool(torch.equal(g[:, 0], w[:, 0])),
                bool(((g[:, 1] - w[:, 1]).abs() <= 1e-9 * d.abs().sum()).all()),
                bool(((g[:, 2] - w[:, 2]).abs() <= 1e-9 * (d * d).sum()).all()))
        if ok and not all(good):
            print(f"pair (code {c}, value {v}) differs: n / s1 / s2 agree = {good}", file=sys.stderr)
        ok = ok and all(good)
    return ok


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[4_000_000, 32_000_000])
    ap.add_argument("--baseline-pairs", type=int, default=2)
    ap.add_argument("--sweep-rows", type=int, default=4_000_000)
    ap.add_argument("--sweep-slots", type=int, nargs="*", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--baseline-warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_grouped_moments needs a GPU: a CPU timing says nothing about the kernel")
    from anovos_amd.ops import backend
    from anovos_amd.ops.grouped import grouped_sums_torch

    ext = backend.require_hip()
    G = ext.GRP_CELLS
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    results = []
    all_ok = True
    head = f"{'rows':>10} {'shape':<26} {'variant':<22} {'median ms':>10} {'min':>9} {'max':>9} {'GB read':>9} {'TB/s':>6}"

    def report(rows, shape, name, t, nbytes, extra):
        med, lo, hi = t
        tbs = nbytes / (med * 1e-3) / 1e12
        print(f"{rows:>10} {shape:<26} {name:<22} {med:>10.2f} {lo:>9.2f} {hi:>9.2f} {nbytes / 1e9:>9.1f} {tbs:>6.2f}",
              flush=True)
        results.append({"rows": rows, "shape": shape, "variant": name, "median_ms": med, "min_ms": lo,
                        "max_ms": hi, "bytes_read": nbytes, "tb_per_s": tbs, **extra})

    # ---- the workload's shape
    sizes = [CAT_CARD] * N_CAT
    pair_c = [c for c in range(N_CAT) for _ in range(N_NUM)]
    pair_v = [v for _ in range(N_CAT) for v in range(N_NUM)]
    items, col_reads, cells = ext.grouped_moments_plan(sizes, pair_c, pair_v)
    step = max(1, len(pair_c) // max(1, args.baseline_pairs))
    sub = list(range(0, len(pair_c), step))[: args.baseline_pairs]
    sub_c, sub_v = [pair_c[q] for q in sub], [pair_v[q] for q in sub]
    _, sub_reads, _ = ext.grouped_moments_plan(sizes, sub_c, sub_v)
    print(f"GRP_CELLS={G} code_columns={N_CAT} categories={CAT_CARD} value_columns={N_NUM} pairs={len(pair_c)} "
          f"work_items={items} column_streams={col_reads} (two per pair would be {2 * len(pair_c)}) cells={cells}; "
          f"baseline subset: {len(sub)} pairs, {sub_reads} kernel column streams")
    print(head)
    for rows in args.rows:
        codes = make_codes(rows, N_CAT, CAT_CARD, g, dev)
        values = make_values(rows, N_NUM, g, dev)
        shifts = [float(torch.nanmean(x.to(torch.float64))) for x in values]
        got = ext.grouped_moments(codes, sizes, values, shifts, sub_c, sub_v)
        want = baseline(grouped_sums_torch, codes, sizes, values, shifts, sub_c, sub_v)
        same = agree(got, want, values, shifts, sub_v, sizes, sub_c)
        # the launch over all pairs splits the rows into other chunks than
        # the launch over the subset: the same blocks up to summation order
        full = ext.grouped_moments(codes, sizes, values, shifts, pair_c, pair_v)
        k = 3 * (CAT_CARD + 1)
        same = same and agree(torch.cat([full[q * k : (q + 1) * k] for q in sub]), want, values, shifts, sub_v, sizes, sub_c)
        all_ok = all_ok and same
        del got, want, full
        shape = f"{N_CAT}x{N_NUM} cols, {CAT_CARD + 1} slots"
        a = timed(lambda: ext.grouped_moments(codes, sizes, values, shifts, pair_c, pair_v), args.warmup, args.reps)
        report(rows, shape, f"K23 all {len(pair_c)} pairs", a, col_reads * rows * 4, {"pairs": len(pair_c), "agree": same})
        a_sub = timed(lambda: ext.grouped_moments(codes, sizes, values, shifts, sub_c, sub_v), args.warmup, args.reps)
        report(rows, shape, f"K23 {len(sub)} pairs", a_sub, sub_reads * rows * 4, {"pairs": len(sub), "agree": same})
        b = timed(lambda: baseline(grouped_sums_torch, codes, sizes, values, shifts, sub_c, sub_v),
                  args.baseline_warmup, args.baseline_reps)
        report(rows, shape, f"torch {len(sub)} pairs", b, 2 * len(sub) * rows * 4, {"pairs": len(sub), "agree": same})
        print(f"{rows:>10} per pair: K23 all pairs {a[0] / len(pair_c):.3f} ms, K23 subset {a_sub[0] / len(sub):.3f} ms, "
              f"torch {b[0] / len(sub):.3f} ms; speed-up on the subset {b[0] / a_sub[0]:.1f}x, "
              f"all pairs against torch per pair {b[0] / len(sub) / (a[0] / len(pair_c)):.1f}x; results agree: {same}",
              flush=True)
        del codes, values
        torch.cuda.empty_cache()

    # ---- sweep over dictionary sizes: 1 code column x 8 value columns
    slots_list = args.sweep_slots
    if slots_list is None:
        # from one window upwards: below, the torch path only gets slower
        # (its index_add_ contends for fewer addresses)
        slots_list = [G, 2 * G + 1, 8 * G, 32 * G, 128 * G, 512 * G, 2048 * G]
    rows = args.sweep_rows
    sweep = []
    if slots_list and rows:
        nv = 2
        values = make_values(rows, nv, g, dev)
        shifts = [float(torch.nanmean(x.to(torch.float64))) for x in values]
        for slots in slots_list:
            size = slots - 1
            codes = make_codes(rows, 1, max(size, 1), g, dev) if size else [torch.full((rows,), -1, dtype=torch.int32, device=dev)]
            pc, pv = [0] * nv, list(range(nv))
            _, reads, _ = ext.grouped_moments_plan([size], pc, pv)
            got = ext.grouped_moments(codes, [size], values, shifts, pc, pv)
            want = baseline(grouped_sums_torch, codes, [size], values, shifts, pc, pv)
            same = agree(got, want, values, shifts, pv, [size], pc)
            all_ok = all_ok and same
            del got, want
            shape = f"1x{nv} cols, {slots} slots"
            a = timed(lambda: ext.grouped_moments(codes, [size], values, shifts, pc, pv), args.warmup, args.reps)
            report(rows, shape, "K23", a, reads * rows * 4, {"slots": slots, "agree": same})
            b = timed(lambda: baseline(grouped_sums_torch, codes, [size], values, shifts, pc, pv),
                      args.baseline_warmup, args.baseline_reps)
            report(rows, shape, "torch", b, 2 * nv * rows * 4, {"slots": slots, "agree": same})
            sweep.append((slots, a[0], b[0]))
            print(f"{rows:>10} {slots} slots: torch / K23 = {b[0] / a[0]:.2f}; results agree: {same}", flush=True)
        wins = [s for s, ka, tb in sweep if ka < tb]
        loses = [s for s, ka, tb in sweep if ka >= tb]
        print(f"sweep: the kernel is faster at slots {wins}, slower at {loses}")
    print(json.dumps({"bench": "grouped_moments", "GRP_CELLS": G, "results": results}))
    if not all_ok:
        sys.exit("results of the kernel and of the torch path differ")


if __name__ == "__main__":
    main()
