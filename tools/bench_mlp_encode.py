"""Time the fused MLP encode kernel (K30) against the library encode.

Workload shape: --cols float32 columns (generated as in
tools/bench_pairwise_corr.py) at --rows rows with 5 % NaN per column,
reduction_params = 0.5; the autoencoder and its standardization are fitted
once on the first --fit-rows rows and saved, and both paths apply that model.

  (a) autoencoder_latentFeatures(apply_precision="bf16x2",
      pre_existing_model=True): wall clock around a synchronised call, and the
      peak of allocated device memory beyond what was allocated before it.
  (b) the same call with apply_precision="fp32" (z_standardization, a stacked
      f32 copy of the frame, three library GEMMs per 65 536 rows), on the
      first --fp32-rows rows only when that is set.
  (c) the kernel call alone (weight image + encode), device events.
  (d) agreement: the largest |bf16x2 - fp32| over the compared rows.

    python tools/bench_mlp_encode.py --rows 32000000 --cols 150 64 20
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_pairwise_corr import make_values, timed, wall  # noqa: E402
from tools.bench_project import peak_beyond  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32_000_000)
    ap.add_argument("--cols", type=int, nargs="*", default=[150, 64, 20])
    ap.add_argument("--fit-rows", type=int, default=100_000)
    ap.add_argument("--fp32-rows", type=int, default=0, help="rows the fp32 path is timed on (0: all)")
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_mlp_encode needs a GPU: a CPU timing says nothing about the kernel")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.data_transformer import transformers as T
    from anovos_amd.data_transformer import transformers_advanced as TA
    from anovos_amd.ops import backend
    from anovos_amd.shared.context import AnovosContext

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    ctx = AnovosContext("cuda:0")
    results = []
    for d in args.cols:
        g = torch.Generator(device=dev)
        g.manual_seed(args.seed)
        values = make_values(args.rows, d, args.null_rate, g, dev)
        names = [f"c{j:03d}" for j in range(d)]

        def frame(n):
            return AnovosFrame({c: Column(c, "float", t[:n]) for c, t in zip(names, values)}, device=dev)

        idf = frame(args.rows)
        mp = tempfile.mkdtemp(prefix="bench_mlp_")
        torch.manual_seed(args.seed)
        TA.autoencoder_latentFeatures(ctx, frame(args.fit_rows), epochs=1, sample_size=20_000, model_path=mp,
                                      standardization_configs={"pre_existing_model": False, "model_path": mp})
        b = max(1, int(0.5 * d))
        print(f"columns={d} float32, rows={args.rows}, null rate {args.null_rate}, "
              f"encoder {d} -> {2 * d} -> {max(d // 2, b)} -> {b}", flush=True)

        def apply(fr, precision):
            return TA.autoencoder_latentFeatures(ctx, fr, pre_existing_model=True, model_path=mp,
                                                 apply_precision=precision,
                                                 standardization_configs={"pre_existing_model": True, "model_path": mp})

        out_k, peak_k = peak_beyond(lambda: apply(idf, "bf16x2"))
        e2e_k = wall(lambda: apply(idf, "bf16x2"), args.reps)

        state = torch.load(os.path.join(mp, "autoencoder_latentFeatures.pt"), map_location=dev)
        params = [state[f"encoder.{i}.{k}"].contiguous() for i in (0, 2, 4) for k in ("weight", "bias")]
        zs = T._load_model(mp, "z_standardization").set_index("feature").loc[names]
        shift = torch.tensor(zs["mean"].to_numpy(), dtype=torch.float32, device=dev)
        scale = torch.tensor(1.0 / zs["stddev"].to_numpy(), dtype=torch.float32, device=dev)
        outs = [out_k.col(f"latent_{j}").data for j in range(b)]
        kern = timed(lambda: ext.mlp_encode_bf16x2(values, shift, scale, *params, outs), 2, args.reps)

        n32 = args.fp32_rows or args.rows
        sub = idf if n32 >= args.rows else frame(n32)
        out_f, peak_f = peak_beyond(lambda: apply(sub, "fp32"))
        e2e_f = wall(lambda: apply(sub, "fp32"), 2)
        diff = max(float((out_k.col(f"latent_{j}").data[:n32] - out_f.col(f"latent_{j}").data).abs().max())
                   for j in range(b))
        row = {"cols": d, "rows": args.rows, "latents": b, "bf16x2_wall_ms": e2e_k, "bf16x2_peak_bytes": peak_k,
               "kernel_ms": kern, "kernel_ns_per_row": kern[0] * 1e6 / args.rows, "fp32_rows": n32,
               "fp32_wall_ms": e2e_f, "fp32_peak_bytes": peak_f, "max_abs_diff": diff}
        print(f"  bf16x2 end to end {e2e_k[0]:.1f} ms ({e2e_k[1]:.1f} - {e2e_k[2]:.1f}), "
              f"peak beyond the frame {peak_k / 1e9:.2f} GB")
        print(f"  kernel call alone {kern[0]:.2f} ms ({kern[1]:.2f} - {kern[2]:.2f}), {row['kernel_ns_per_row']:.3f} ns/row")
        print(f"  fp32 library path on {n32} rows {e2e_f[0]:.1f} ms ({e2e_f[1]:.1f} - {e2e_f[2]:.1f}), "
              f"peak beyond the frame {peak_f / 1e9:.2f} GB")
        print(f"  per row fp32 / bf16x2 = {e2e_f[0] / n32 / (e2e_k[0] / args.rows):.1f} x; "
              f"largest |bf16x2 - fp32| = {diff:.3g}", flush=True)
        results.append(row)
        del values, idf, sub, out_k, out_f, outs
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "mlp_encode", "results": results}))


if __name__ == "__main__":
    main()
