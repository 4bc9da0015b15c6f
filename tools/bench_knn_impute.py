"""Time the KNN imputation kernel (K29) against the fp64 torch apply.

Workload shape: --cols float32 columns (generated as in
tools/bench_pairwise_corr.py) at --rows rows with 5 % NaN per column; a
KNNImputer(n_neighbors=5) is fitted once on the first --donors rows and
pickled, and both paths apply that one model.

  (a) imputation_sklearn(apply_precision="bf16x2", pre_existing_model=True):
      wall clock around a synchronised call, and the peak of allocated
      device memory beyond what was allocated before it.
  (b) the same call with apply_precision="fp64" (four fp64 GEMMs per
      16 384-row batch, a top-k per column), on the first --fp64-rows rows
      only when that is set - it is reported per task either way.
  (c) the kernel calls alone: one knn_impute_bf16x2 per column over that
      column's null rows, device events around the m calls.
  (d) agreement: the share of imputed entries where the two paths differ by
      more than rtol 2e-4 / atol 2e-3 (near-ties pick another neighbour).

    python tools/bench_knn_impute.py --rows 32000000 --cols 20
"""

from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_pairwise_corr import make_values, timed, wall  # noqa: E402
from tools.bench_project import peak_beyond  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32_000_000)
    ap.add_argument("--cols", type=int, nargs="*", default=[20, 64])
    ap.add_argument("--donors", type=int, default=10_000)
    ap.add_argument("--fp64-rows", type=int, default=0, help="rows the fp64 path is timed on (0: all)")
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_knn_impute needs a GPU: a CPU timing says nothing about the kernel")
    from sklearn.impute import KNNImputer

    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.data_transformer import transformers_advanced as TA
    from anovos_amd.ops import backend
    from anovos_amd.shared.context import AnovosContext

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    ctx = AnovosContext("cuda:0")
    results = []
    for m in args.cols:
        g = torch.Generator(device=dev)
        g.manual_seed(args.seed)
        values = make_values(args.rows, m, args.null_rate, g, dev)
        names = [f"c{j:03d}" for j in range(m)]
        idf = AnovosFrame({n: Column(n, "float", t) for n, t in zip(names, values)}, device=dev)
        sample = torch.stack([t[: args.donors] for t in values], dim=1).cpu().numpy().astype(np.float64)
        model = KNNImputer(n_neighbors=5).fit(sample)
        mp = tempfile.mkdtemp(prefix="bench_knn_")
        with open(os.path.join(mp, "imputation_sklearn.pkl"), "wb") as f:
            pickle.dump(model, f)
        tasks = int(sum(int(torch.isnan(t).sum()) for t in values))
        print(f"columns={m} float32, rows={args.rows}, null rate {args.null_rate}, donors={sample.shape[0]}, "
              f"tasks={tasks}", flush=True)

        def apply(frame, precision):
            return TA.imputation_sklearn(ctx, frame, names, method_type="KNN", apply_precision=precision,
                                         pre_existing_model=True, model_path=mp)

        out_k, peak_k = peak_beyond(lambda: apply(idf, "bf16x2"))
        e2e_k = wall(lambda: apply(idf, "bf16x2"), args.reps)

        center = torch.from_numpy(np.nanmean(sample, axis=0))
        donors_t = torch.from_numpy(sample).to(torch.float32).to(dev)
        rows = [torch.isnan(t).nonzero(as_tuple=True)[0] for t in values]
        kern = timed(lambda: [ext.knn_impute_bf16x2(values, rows[j], center, donors_t, j, 5) for j in range(m)],
                     1, args.reps)

        n64 = args.fp64_rows or args.rows
        sub = idf if n64 >= args.rows else AnovosFrame(
            {n: Column(n, "float", t[:n64]) for n, t in zip(names, values)}, device=dev)
        tasks64 = int(sum(int(torch.isnan(t[:n64]).sum()) for t in values))
        out_f, peak_f = peak_beyond(lambda: apply(sub, "fp64"))
        e2e_f = wall(lambda: apply(sub, "fp64"), 1)

        differ = total = 0
        for n, t in zip(names, values):
            nul = torch.isnan(t[:n64])
            a, b = out_k.col(n).data[:n64][nul].double(), out_f.col(n).data[nul].double()
            differ += int((~torch.isclose(a, b, rtol=2e-4, atol=2e-3)).sum())
            total += int(nul.sum())
        row = {"cols": m, "rows": args.rows, "tasks": tasks, "donors": int(sample.shape[0]),
               "bf16x2_wall_ms": e2e_k, "bf16x2_peak_bytes": peak_k, "kernel_calls_ms": kern,
               "kernel_ns_per_task": kern[0] * 1e6 / tasks,
               "fp64_rows": n64, "fp64_tasks": tasks64, "fp64_wall_ms": e2e_f, "fp64_peak_bytes": peak_f,
               "fp64_ns_per_task": e2e_f[0] * 1e6 / tasks64, "bf16x2_wall_ns_per_task": e2e_k[0] * 1e6 / tasks,
               "differing_entries": differ, "compared_entries": total}
        print(f"  bf16x2 end to end {e2e_k[0]:.1f} ms ({e2e_k[1]:.1f} - {e2e_k[2]:.1f}), "
              f"{row['bf16x2_wall_ns_per_task']:.1f} ns/task, peak beyond the frame {peak_k / 1e9:.2f} GB")
        print(f"  kernel calls alone {kern[0]:.1f} ms ({kern[1]:.1f} - {kern[2]:.1f}), {row['kernel_ns_per_task']:.1f} ns/task")
        print(f"  fp64 torch on {n64} rows {e2e_f[0]:.1f} ms, {row['fp64_ns_per_task']:.1f} ns/task, "
              f"peak beyond the frame {peak_f / 1e9:.2f} GB")
        print(f"  per task fp64 / bf16x2 = {row['fp64_ns_per_task'] / row['bf16x2_wall_ns_per_task']:.1f} x; "
              f"{differ} of {total} imputed entries differ beyond rtol 2e-4 / atol 2e-3", flush=True)
        results.append(row)
        del values, idf, sub, out_k, out_f, rows
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "knn_impute", "results": results}))


if __name__ == "__main__":
    main()
