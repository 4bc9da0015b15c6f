"""Time the pair-count kernel (K22) against the route it replaces.

Shape: the categorical block of bench.make_synthetic_frame — N_CAT int32
code columns with CAT_CARD categories and about 1 % nulls — and all
N_CAT * (N_CAT - 1) / 2 column pairs.

  (a) pair_code_counts: one launch, anchor + partner packing, LDS tables
  (b) baseline: per pair, torch.bincount over the fused int64 key
      slot_i * (size_j + 1) + slot_j

Both are timed with device events around each repetition after warm-up;
the median is reported. Bytes: (a) reads one column stream per work item
for the anchor plus one per partner (from pair_code_counts_plan); for (b)
the figure is the two int32 columns each pair has to read at the least —
its int64 intermediates are extra traffic on top. TB/s is those bytes
over the median time, to set beside the streaming ceiling of 5.2-5.4 TB/s
(profiles/bwbench_streaming_variants.log). The tables of (a) and (b) are
compared for equality at every timed size.

    python tools/bench_pair_counts.py --rows 4000000 32000000
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import CAT_CARD, N_CAT  # noqa: E402


def make_columns(rows: int, seed: int, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cols = []
    for _ in range(N_CAT):
        codes = torch.randint(0, CAT_CARD, (rows,), generator=g, device=dev).to(torch.int32)
        codes[torch.rand(rows, generator=g, device=dev) < 0.01] = -1
        cols.append(codes)
    return cols


def baseline_tables(cols, sizes, pair_i, pair_j):
    parts = []
    for i, j in zip(pair_i, pair_j):
        si, sj = sizes[i], sizes[j]
        a = cols[i].to(torch.int64)
        b = cols[j].to(torch.int64)
        a = torch.where((a >= 0) & (a < si), a, torch.full_like(a, si))
        b = torch.where((b >= 0) & (b < sj), b, torch.full_like(b, sj))
        parts.append(torch.bincount(a * (sj + 1) + b, minlength=(si + 1) * (sj + 1)))
    return torch.cat(parts)


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
    ap.add_argument("--rows", type=int, nargs="+", default=[4_000_000, 32_000_000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--baseline-warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_pair_counts needs a GPU: a CPU timing says nothing about the kernel")
    from anovos_amd.ops import backend

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    sizes = [CAT_CARD] * N_CAT
    pair_i = [i for i in range(N_CAT) for _ in range(i + 1, N_CAT)]
    pair_j = [j for i in range(N_CAT) for j in range(i + 1, N_CAT)]
    items, col_reads, lds = ext.pair_code_counts_plan(sizes, pair_i, pair_j)
    print(f"columns={N_CAT} categories={CAT_CARD} pairs={len(pair_i)} work_items={items} "
          f"column_streams={col_reads} (one block per pair would be {2 * len(pair_i)}) lds_counters={lds}")
    print(f"{'rows':>10} {'variant':<24} {'median ms':>10} {'min':>9} {'max':>9} {'GB read':>9} {'TB/s':>6}")
    results = []
    for rows in args.rows:
        cols = make_columns(rows, args.seed, dev)
        got = ext.pair_code_counts(cols, sizes, pair_i, pair_j)
        want = baseline_tables(cols, sizes, pair_i, pair_j)
        same = bool(torch.equal(got, want))
        del got, want
        a = timed(lambda: ext.pair_code_counts(cols, sizes, pair_i, pair_j), args.warmup, args.reps)
        b = timed(lambda: baseline_tables(cols, sizes, pair_i, pair_j), args.baseline_warmup, args.baseline_reps)
        for name, (med, lo, hi), nbytes in (
            ("pair_code_counts (K22)", a, col_reads * rows * 4),
            ("bincount per pair", b, 2 * len(pair_i) * rows * 4),
        ):
            tbs = nbytes / (med * 1e-3) / 1e12
            print(f"{rows:>10} {name:<24} {med:>10.2f} {lo:>9.2f} {hi:>9.2f} {nbytes / 1e9:>9.1f} {tbs:>6.2f}")
            results.append({"rows": rows, "variant": name, "median_ms": med, "min_ms": lo, "max_ms": hi,
                            "bytes_read": nbytes, "tb_per_s": tbs, "tables_equal": same})
        print(f"{rows:>10} speed-up {b[0] / a[0]:.1f}x, tables equal: {same}")
        del cols
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "pair_counts", "results": results}))
    if not all(r["tables_equal"] for r in results):
        sys.exit("tables of the kernel and of the baseline differ")


if __name__ == "__main__":
    main()
