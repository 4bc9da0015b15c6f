"""Time the regression-imputation apply kernel (K31) against the fp64 path.

Workload shape: --cols float32 columns (generated as in
tools/bench_pairwise_corr.py) at --rows rows with 5 % NaN per column; an
IterativeImputer(max_iter=10, tol=0: all ten rounds) is fitted once on the
first --fit-rows rows and saved, and both paths apply that model.

  (a) imputation_sklearn(method_type="regression", apply_precision="bf16x2",
      pre_existing_model=True): wall clock around a synchronised call, and the
      peak of allocated device memory beyond what was allocated before it
      (the output clones included).
  (b) the same call with the default apply_precision (rows with a null
      stacked in fp64, one gather and GEMV per step), on the first
      --fp64-rows rows only when that is set.
  (c) the kernel call alone (coefficient image + apply), device events.
  (d) agreement: the largest |bf16x2 - fp64| over the compared rows.

    python tools/bench_chain_impute.py --rows 32000000 --cols 150 64 20 --fp64-rows 2000000
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
    ap.add_argument("--cols", type=int, nargs="*", default=[150, 64, 20])
    ap.add_argument("--fit-rows", type=int, default=10_000)
    ap.add_argument("--fp64-rows", type=int, default=0, help="rows the fp64 path is timed on (0: all)")
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_chain_impute needs a GPU: a CPU timing says nothing about the kernel")
    from sklearn.experimental import enable_iterative_imputer  # noqa: F401
    from sklearn.impute import IterativeImputer
    from sklearn.linear_model import LinearRegression

    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.data_transformer import transformers_advanced as TA
    from anovos_amd.ops import backend, chain
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

        def frame(n):
            return AnovosFrame({c: Column(c, "float", t[:n]) for c, t in zip(names, values)}, device=dev)

        idf = frame(args.rows)
        sample = np.column_stack([t[: args.fit_rows].cpu().numpy().astype(np.float64) for t in values])
        # least squares keeps the fit of 10 x m estimators short; the apply does not depend on the estimator
        model = IterativeImputer(LinearRegression(), max_iter=10, tol=0, random_state=args.seed).fit(sample)
        mp = tempfile.mkdtemp(prefix="bench_chain_")
        with open(os.path.join(mp, "imputation_sklearn.pkl"), "wb") as f:
            pickle.dump(model, f)
        nulls = int(sum(int(torch.isnan(t).sum()) for t in values))
        print(f"columns={m} float32, rows={args.rows}, null rate {args.null_rate}, {model.n_iter_} rounds, "
              f"{nulls} null entries", flush=True)

        def apply(fr, **kw):
            return TA.imputation_sklearn(ctx, fr, names, method_type="regression", pre_existing_model=True,
                                         model_path=mp, **kw)

        out_k, peak_k = peak_beyond(lambda: apply(idf, apply_precision="bf16x2"))
        e2e_k = wall(lambda: apply(idf, apply_precision="bf16x2"), args.reps)

        s, order, C, beta, lo, hi = chain.chain_model(model, m)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dev)
        kargs = (torch.from_numpy(s), torch.from_numpy(order.astype(np.int32)), f32(C), f32(beta), f32(lo), f32(hi))
        outs = [out_k.col(c).data for c in names]
        kern = timed(lambda: ext.chain_impute_bf16x2(values, *kargs, outs), 2, args.reps)

        n64 = args.fp64_rows or args.rows
        sub = idf if n64 >= args.rows else frame(n64)
        out_f, peak_f = peak_beyond(lambda: apply(sub))
        e2e_f = wall(lambda: apply(sub), 1)
        diff = max(float((out_k.col(c).data[:n64] - out_f.col(c).data).abs().max()) for c in names)
        row = {"cols": m, "rows": args.rows, "rounds": int(model.n_iter_), "nulls": nulls, "bf16x2_wall_ms": e2e_k,
               "bf16x2_peak_bytes": peak_k, "kernel_ms": kern, "kernel_ns_per_null": kern[0] * 1e6 / max(nulls, 1),
               "frame_tb_per_s": args.rows * m * 4 / kern[0] / 1e9, "fp64_rows": n64, "fp64_wall_ms": e2e_f,
               "fp64_peak_bytes": peak_f, "max_abs_diff": diff}
        print(f"  bf16x2 end to end {e2e_k[0]:.1f} ms ({e2e_k[1]:.1f} - {e2e_k[2]:.1f}), "
              f"peak beyond the frame {peak_k / 1e9:.2f} GB (output clones {args.rows * m * 4 / 1e9:.2f} GB)")
        print(f"  kernel call alone {kern[0]:.2f} ms ({kern[1]:.2f} - {kern[2]:.2f}), "
              f"{row['kernel_ns_per_null']:.3f} ns per imputed entry, {row['frame_tb_per_s']:.2f} TB/s of the frame")
        print(f"  fp64 path on {n64} rows {e2e_f[0]:.1f} ms, peak beyond the frame {peak_f / 1e9:.2f} GB")
        print(f"  per row fp64 / bf16x2 = {e2e_f[0] / n64 / (e2e_k[0] / args.rows):.1f} x; "
              f"largest |bf16x2 - fp64| = {diff:.3g}", flush=True)
        results.append(row)
        del values, idf, sub, out_k, out_f, outs
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "chain_impute", "results": results}))


if __name__ == "__main__":
    main()
