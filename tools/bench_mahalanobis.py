"""Time the row quadratic-form kernel (K26) against the library path.

Workload shape: 150 float32 columns (the numeric block of the flagship
benchmark) at 32M rows with 5 % NaN per column, generated as in
tools/bench_pairwise_corr.py; the whitening model (mean, sd, W [r, 150]) is
fitted on a 1M-row sample by ops/mahalanobis.fit_whitening.

  (a) K26 row_quadform_bf16x2: d2 of every row from one launch (split
      bf16, three MFMA products, W resident in LDS); bytes = the frame
      once, plus the 4 bytes per row it writes. Also at the forced grids of
      --blocks (ANOVOS_ROWQUAD_BLOCKS).
  (b) the library path - what one would write without the kernel, and the
      baseline: per row slab Z = where(isnan(x), 0, (x - shift) * scale)
      as an f32 [k, rows] block, Y = W @ Z through torch.matmul (rocBLAS),
      d2 = (Y * Y).sum(0).
  (c) mahalanobis_d2 end to end on the kernel path (uploads of shift,
      scale and W included), with a wall clock around a synchronised call.
  (d) accuracy: the largest |kernel - library| and, on the first 200 000
      rows, both against the fp64 form, relative to the largest distance.

Kernels are timed with device events around each repetition after warm-up;
the median is reported.

    python tools/bench_mahalanobis.py --rows 32000000
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_pairwise_corr import make_values, timed, wall  # noqa: E402

NCOLS = 150
LIB_SLAB_BYTES = 1 << 30  # the Z and Y blocks of one slab of the library path


def library_d2(values, shift, scale, W, out):
    k, r = len(values), W.shape[0]
    n = values[0].shape[0]
    rows = max(1, LIB_SLAB_BYTES // (4 * (k + r)))
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        Z = torch.empty(k, r1 - r0, dtype=torch.float32, device=W.device)
        for j, t in enumerate(values):
            v = t[r0:r1]
            Z[j] = torch.where(torch.isnan(v), torch.zeros_like(v), (v - shift[j]) * scale[j])
        Y = W @ Z
        out[r0:r1] = (Y * Y).sum(0)
        del Z, Y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[32_000_000])
    ap.add_argument("--null-rate", type=float, default=0.05)
    ap.add_argument("--blocks", type=int, nargs="*", default=[],
                    help="forced grids (ANOVOS_ROWQUAD_BLOCKS) to time next to the default")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_mahalanobis needs a GPU: a CPU timing says nothing about the kernel")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.ops import backend
    from anovos_amd.ops import mahalanobis as maha

    ext = backend.require_hip()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    results = []
    print(f"columns={NCOLS} float32, null rate {args.null_rate}")
    print(f"{'rows':>10} {'variant':<56} {'median ms':>10} {'min':>9} {'max':>9} {'GB':>7} {'TB/s':>6}")

    def report(rows, name, t, nbytes, extra=None):
        med, lo, hi = t
        tbs = nbytes / (med * 1e-3) / 1e12
        print(f"{rows:>10} {name:<56} {med:>10.2f} {lo:>9.2f} {hi:>9.2f} {nbytes / 1e9:>7.1f} {tbs:>6.2f}", flush=True)
        results.append({"rows": rows, "variant": name, "median_ms": med, "min_ms": lo, "max_ms": hi,
                        "bytes": nbytes, "tb_per_s": tbs, **(extra or {})})

    for rows in args.rows:
        values = make_values(rows, NCOLS, args.null_rate, g, dev)
        names = [f"c{j:03d}" for j in range(NCOLS)]
        idf = AnovosFrame({n: Column(n, "float", t) for n, t in zip(names, values)}, device=dev)
        frame_bytes = NCOLS * rows * 4
        m = min(rows, 1_000_000)
        sample = AnovosFrame({n: Column(n, "float", t[:m]) for n, t in zip(names, values)}, device=dev)
        model = maha.fit_whitening(sample, names)
        shift = torch.tensor(model.mean, dtype=torch.float64).to(torch.float32).to(dev)
        scale = torch.tensor(1.0 / model.sd, dtype=torch.float64).to(torch.float32).to(dev)
        W = torch.tensor(model.W, dtype=torch.float64).to(torch.float32).to(dev)
        print(f"{rows:>10} model: k = {len(model.columns)}, rank = {model.rank}", flush=True)

        os.environ.pop("ANOVOS_ROWQUAD_BLOCKS", None)
        a = timed(lambda: ext.row_quadform_bf16x2(values, shift, scale, W), args.warmup, args.reps)
        report(rows, "K26 row_quadform_bf16x2, default grid", a, frame_bytes)
        for b in args.blocks:
            os.environ["ANOVOS_ROWQUAD_BLOCKS"] = str(b)
            t = timed(lambda: ext.row_quadform_bf16x2(values, shift, scale, W), args.warmup, args.reps)
            report(rows, f"K26 row_quadform_bf16x2, {b} blocks", t, frame_bytes, {"blocks": b})
        os.environ.pop("ANOVOS_ROWQUAD_BLOCKS", None)

        out_lib = torch.empty(rows, dtype=torch.float32, device=dev)
        lib = timed(lambda: library_d2(values, shift, scale, W, out_lib), 1, max(2, args.reps // 2))
        slabs = -(-rows // max(1, LIB_SLAB_BYTES // (4 * (NCOLS + model.rank))))
        report(rows, f"library path (f32 W @ Z by torch.matmul, {slabs} slabs)", lib, frame_bytes, {"slabs": slabs})

        e2e = wall(lambda: maha.mahalanobis_d2(idf, names, model), args.reps)
        report(rows, "mahalanobis_d2, kernel path, wall clock", e2e, frame_bytes)

        d_k = ext.row_quadform_bf16x2(values, shift, scale, W)
        top = float(d_k.max())
        dev_kl = float((d_k - out_lib).abs().max()) / top
        s = min(rows, 200_000)
        Z = torch.stack([v[:s].double() for v in values], dim=1)
        Z = (Z - torch.tensor(model.mean, device=dev)) / torch.tensor(model.sd, device=dev)
        Z = torch.where(torch.isnan(Z), torch.zeros_like(Z), Z)
        Y = Z @ torch.tensor(model.W, device=dev).T
        ref = (Y * Y).sum(1)
        top_s = float(ref.max())
        err_k = float((d_k[:s].double() - ref).abs().max()) / top_s
        err_l = float((out_lib[:s].double() - ref).abs().max()) / top_s
        print(f"{rows:>10} library path {lib[0] / a[0]:.2f} x the kernel's time; largest |kernel - library| "
              f"{dev_kl:.2e} of the largest d2 ({top:.1f}); against fp64 on {s} rows: kernel {err_k:.2e}, "
              f"library {err_l:.2e}", flush=True)
        results.append({"rows": rows, "variant": "agreement", "library_over_kernel": lib[0] / a[0],
                        "max_rel_kernel_library": dev_kl, "max_rel_kernel_fp64": err_k,
                        "max_rel_library_fp64": err_l})
        del values, idf, sample, out_lib, d_k, Z, Y, ref
        torch.cuda.empty_cache()

    print(json.dumps({"bench": "mahalanobis", "columns": NCOLS, "null_rate": args.null_rate, "results": results}))


if __name__ == "__main__":
    main()
