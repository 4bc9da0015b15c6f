"""Time matrix-factorization imputation on the ALS kernels (K32) against the
default torch path.

Workload shape: --cols float32 columns (generated as in
tools/bench_pairwise_corr.py) at --rows rows with 5 % NaN per column, rank
--rank, reg 0.01.

  (a) imputation_matrixFactorization(precision="bf16x2") with max_iter =
      --iters and with max_iter = 0 (V0 and the final row pass only): wall
      clock around a synchronised call; a sweep costs (t_iters - t_0) / iters.
      Peak of allocated device memory beyond what was allocated before the
      call (the output clones included).
  (b) the same with the default precision (stacked [n, m] copies, batched
      solves, m passes over U) on the first --fp32-rows rows, with max_iter =
      --fp32-iters and 0.
  (c) the two kernels alone, device events: the row half writing U, the
      column half reading it, the row half writing the predictions.
  (d) the floor of a sweep: two reads of the frame, U written once and read
      once per 64-column group, at --tbps TB/s.

    python tools/bench_als.py --rows 32000000 --cols 20 64 150 --fp32-rows 2000000
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_pairwise_corr import make_values, timed, wall  # noqa: E402
from tools.bench_project import peak_beyond  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32_000_000)
    ap.add_argument("--cols", type=int, nargs="*", default=[20, 64, 150])
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--fp32-rows", type=int, default=2_000_000)
    ap.add_argument("--fp32-iters", type=int, default=2)
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tbps", type=float, default=5.3, help="measured read ceiling of the device")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_als needs a GPU: a CPU timing says nothing about the kernels")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.data_transformer import transformers_advanced as TA
    from anovos_amd.ops import als, backend
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
        k, kr = min(args.rank, m), als.als_kr(min(args.rank, m))
        print(f"columns={m} float32, rows={args.rows}, null rate {args.null_rate}, rank {k} (KR {kr})", flush=True)

        def fit(fr, iters, **kw):
            return TA.imputation_matrixFactorization(ctx, fr, names, rank=args.rank, max_iter=iters, **kw)

        fit(idf, 0, precision="bf16x2")  # moments cached, kernels loaded
        _, peak_k = peak_beyond(lambda: fit(idf, 1, precision="bf16x2"))
        t_i = wall(lambda: fit(idf, args.iters, precision="bf16x2"), args.reps)
        t_0 = wall(lambda: fit(idf, 0, precision="bf16x2"), args.reps)
        sweep = (t_i[0] - t_0[0]) / args.iters

        mu, sd, _ = als.column_scales(idf, names)
        V = torch.from_numpy(als.als_v0(idf, names, sd, k).astype(np.float32)).to(dev)
        kargs = (values, torch.from_numpy(mu), torch.from_numpy(1.0 / sd), torch.from_numpy(sd), V, 0.01)
        U, _ = ext.als_row_solve_bf16x2(*kargs)
        outs = [t.clone() for t in values]
        row_u = timed(lambda: ext.als_row_solve_bf16x2(*kargs), 1, args.reps)
        col = timed(lambda: ext.als_col_normal_bf16x2(*kargs[:3], U), 1, args.reps)
        row_p = timed(lambda: ext.als_row_solve_bf16x2(*kargs, outs=outs, want_u=False), 1, args.reps)
        del outs, U
        frame_b, u_b = args.rows * m * 4, args.rows * kr * 4
        floor = (2 * frame_b + (1 + (m + 63) // 64) * u_b) / (args.tbps * 1e9)

        n32 = min(args.fp32_rows or args.rows, args.rows)
        sub = frame(n32)
        fit(sub, 0)
        _, peak_f = peak_beyond(lambda: fit(sub, 1))
        f_i = wall(lambda: fit(sub, args.fp32_iters), 1)
        f_0 = wall(lambda: fit(sub, 0), 1)
        sweep_f = (f_i[0] - f_0[0]) / args.fp32_iters
        row = {"cols": m, "rows": args.rows, "rank": k, "kr": kr, "bf16x2_wall_ms": t_i, "bf16x2_wall0_ms": t_0,
               "bf16x2_sweep_ms": sweep, "bf16x2_peak_bytes": peak_k, "row_u_ms": row_u, "col_ms": col,
               "row_pred_ms": row_p, "floor_ms": floor, "fp32_rows": n32, "fp32_sweep_ms": sweep_f,
               "fp32_peak_bytes": peak_f}
        print(f"  bf16x2 {args.iters} sweeps {t_i[0]:.1f} ms ({t_i[1]:.1f} - {t_i[2]:.1f}), 0 sweeps {t_0[0]:.1f} ms: "
              f"{sweep:.1f} ms per sweep; peak beyond the frame {peak_k / 1e9:.2f} GB "
              f"(output clones {frame_b / 1e9:.2f} GB, U {u_b / 1e9:.2f} GB)")
        print(f"  kernels alone: row half -> U {row_u[0]:.2f} ms, column half {col[0]:.2f} ms, "
              f"row half -> predictions {row_p[0]:.2f} ms; floor of a sweep {floor:.2f} ms: "
              f"{(row_u[0] + col[0]) / floor:.1f} x the floor")
        print(f"  fp32 path on {n32} rows: {sweep_f:.1f} ms per sweep, peak beyond the frame {peak_f / 1e9:.2f} GB; "
              f"per row and sweep fp32 / bf16x2 = {sweep_f / n32 / (sweep / args.rows):.1f} x", flush=True)
        results.append(row)
        del values, idf, sub
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "als", "results": results}))


if __name__ == "__main__":
    main()
