#!/usr/bin/env python3
"""Flagship benchmark: rows/sec (whole node) for the full analyzer + drift +
transform pipeline on synthetic tabular data (BASELINE.json metric).

One process per GPU (torch.distributed over RCCL); rank r holds a
row-shard of the synthetic 200-column frame resident in HBM. A "step" is
one full pipeline pass over the resident frame:

  analyzer   : measures_of_counts, centralTendency (discrete cols),
               cardinality (HLL), dispersion, percentiles, shape,
               nullRows detection, biasedness, outlier detection
  association: correlation_matrix (bf16 MFMA Gram over ALL 150 numeric
               cols), IV + IG over all 200 attributes (fused K9
               label-histogram kernel; equal-frequency binning inside)
  drift      : attribute_binning (source model) + PSI/JSD/HD/KS vs the
               warmup snapshot histograms — ALL numeric columns
  transform  : attribute_binning, z_standardization, imputation_MMM,
               cat_to_num label encoding (all 50 cats), outlier_categories
               (all 50 cats)

Nothing is strided or capped: every section runs over its full column
set, and per-transform checksums are whole-column
device reductions (not 8-element probes).

Data: synthetic, random-init, generated on-device before timing (no
network). Weak scaling: per-GPU rows fixed as N grows; value = aggregate
rows/sec over all ranks = N * rows_per_gpu / max_rank(step_time).

A plain run sets up, warms up, times --steps steps and prints one JSON
result line. --full then also measures the per-section breakdown, in
steps of its own so its sync points stay out of the headline figure.
--dump-outputs DIR writes what the last timed step returned to its
caller as DIR/<name>.npy (see OutputCapture); inputs are seeded, so two
builds can be compared output for output.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

N_NUM_CONT = 100  # continuous fp32 columns
N_NUM_INT = 50  # integer-valued fp32 columns (ages/counts-like)
N_CAT = 50  # categorical dictionary columns
CAT_CARD = 40


def make_synthetic_frame(rows: int, device, seed: int):
    """200-column synthetic tabular frame (numeric + categorical), nulls
    included, generated directly on-device (a 125M-row/GPU shard — the
    1Bx200-at-8-GPU config — is 100 GB and generates in seconds in HBM;
    staging through host RAM would take minutes)."""
    from anovos_amd.core.frame import AnovosFrame, Column

    dev = torch.device(device)
    on_gpu = dev.type == "cuda"
    g = torch.Generator(device=dev if on_gpu else "cpu")
    g.manual_seed(seed)

    def rand(*a, **k):
        return torch.rand(*a, generator=g, device=dev if on_gpu else "cpu", **k)

    def randn(*a, **k):
        return torch.randn(*a, generator=g, device=dev if on_gpu else "cpu", **k)

    def randint(lo, hi, shape, **k):
        return torch.randint(lo, hi, shape, generator=g, device=dev if on_gpu else "cpu", **k)

    cols = {}
    # continuous columns: varied scale/shape, ~1% nulls
    base = randn(rows)
    for i in range(N_NUM_CONT):
        x = (base * (1 + 0.1 * i)).clone() if i % 7 == 0 else randn(rows)
        x = x * (1.0 + i % 5) + (i % 11)
        nulls = rand(rows) < 0.01
        x[nulls] = float("nan")
        cols[f"num_{i}"] = Column(f"num_{i}", "float", x.to(dev))
    del base
    for i in range(N_NUM_INT):
        x = randint(0, 80 + i, (rows,)).to(torch.float32)
        nulls = rand(rows) < 0.01
        x[nulls] = float("nan")
        cols[f"int_{i}"] = Column(f"int_{i}", "int", x.to(dev))
    for i in range(N_CAT):
        codes = randint(0, CAT_CARD, (rows,)).to(torch.int32)
        nulls = rand(rows) < 0.01
        codes[nulls] = -1
        dictionary = [f"cat{i}_v{j}" for j in range(CAT_CARD)]
        cols[f"cat_{i}"] = Column(f"cat_{i}", "string", codes.to(dev), dictionary)
    # label column for supervised paths
    lab = (rand(rows) < 0.25).to(torch.int32)
    cols["label"] = Column("label", "string", lab.to(dev), ["no", "yes"])
    return AnovosFrame(cols, dev)


import contextlib


@contextlib.contextmanager
def _timed(name, sections, ctx):
    """Per-section wall timer for --sections / --full (sync-bracketed so the
    numbers are attributable; adds sync points, so only for profiling)."""
    if sections is None:
        yield
        return
    ctx.synchronize()
    t0 = time.perf_counter()
    yield
    ctx.synchronize()
    sections[name] = sections.get(name, 0.0) + (time.perf_counter() - t0) * 1000


DUMP_SAMPLE_ROWS = 4096  # rows of each output frame kept by --dump-outputs


class OutputCapture:
    """Collects what one pipeline step returned to its caller, for
    --dump-outputs. Stats tables are kept whole; output frames (tens of
    GB at the default shard) are sampled at a fixed, seeded set of rows.
    Files hold finite numbers only; nulls are marked in a file alongside.
    Inside the step only device gathers are queued (no sync); everything
    is converted and written by save(), after the timer has stopped."""

    def __init__(self, rows: int, device, seed: int = 20240517):
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        n = min(rows, DUMP_SAMPLE_ROWS)
        self.idx = torch.randint(0, rows, (n,), generator=g).sort().values.to(device)
        self.items = {}

    def add(self, name, obj, cols=None):
        if cols is not None:  # AnovosFrame: sampled rows of the given columns
            obj = torch.stack([obj.col(c).data[self.idx].to(torch.float32) for c in cols], dim=1)
        self.items[name] = obj

    @staticmethod
    def _to_array(obj):
        import pandas as pd

        if isinstance(obj, torch.Tensor):
            return obj.cpu().numpy()
        if isinstance(obj, pd.DataFrame):
            # rows in attribute order; non-numeric cells (mode labels, ...) become NaN
            if "attribute" in obj.columns:
                obj = obj.sort_values("attribute", kind="stable").drop(columns=["attribute"])
            return obj.apply(pd.to_numeric, errors="coerce").to_numpy(dtype=np.float64)
        return np.asarray(obj, dtype=np.float64)

    def save(self, out_dir):
        """Every file holds finite numbers only. Nulls (NaN) and infinities
        are part of the results, so an array that has any is written with
        those cells zeroed, next to <name>_nonfinite.npy that marks them:
        0 finite, 1 NaN (null or non-numeric cell), 2 +inf, 3 -inf."""
        os.makedirs(out_dir, exist_ok=True)
        for name, obj in self.items.items():
            a = self._to_array(obj)
            if not np.isfinite(a).all():
                marks = np.isnan(a) * 1.0 + np.isposinf(a) * 2.0 + np.isneginf(a) * 3.0
                np.save(os.path.join(out_dir, name + "_nonfinite.npy"), marks.astype(np.float32))
                a = np.where(marks > 0, 0, a).astype(a.dtype)
            np.save(os.path.join(out_dir, name + ".npy"), a)


def pipeline_step(ctx, idf, source_hist, model_dir, sections=None, capture=None):
    """One full analyzer + drift + transform pass. Returns a checksum to
    defeat dead-code elimination. With `capture` (an OutputCapture) the
    step's results are also recorded there."""
    import pandas as pd

    from anovos_amd.data_analyzer import association_evaluator as ae
    from anovos_amd.data_analyzer import quality_checker as qc
    from anovos_amd.data_analyzer import stats_generator as sg
    from anovos_amd.data_transformer import transformers as T
    from anovos_amd.drift_stability import drift_detector as dd
    from anovos_amd.ops import histogram as hist_ops
    from anovos_amd.ops import stats as stats_ops
    from anovos_amd.shared.utils import attributeType_segregation

    def keep(name, obj, cols=None):
        if capture is not None:
            capture.add(name, obj, cols)

    idf.clear_stats_cache()  # every timed step recomputes all statistics
    num_cols, cat_cols, _ = attributeType_segregation(idf)
    num_cols = [c for c in num_cols]
    int_cols = [c for c in idf.columns if c.startswith("int_")]
    chk = 0.0

    # ---- analyzer ----
    # cardinality first: its fused K1/K2+K4 kernel computes moments AND
    # HLL registers in ONE frame read; everything below hits the moment
    # cache (the engine's stats-reuse contract)
    with _timed("cardinality_moments", sections, ctx):
        card = sg.measures_of_cardinality(ctx, idf, num_cols + cat_cols, use_approx_unique_count=True)  # K4 HLL
        chk += float(pd.to_numeric(card["unique_values"], errors="coerce").fillna(0).sum())
        moments = stats_ops.frame_moments(idf, num_cols)  # cached by the fused pass
        keep("cardinality", card)
    with _timed("quantiles", sections, ctx):
        quant = hist_ops.approx_quantiles(
            idf, num_cols, [0.01, 0.05, 0.10, 0.25, 0.50, 0.75, 0.90, 0.95, 0.99], moments=moments
        )  # K3
        keep("quantiles", [quant[c] for c in num_cols])
    with _timed("counts", sections, ctx):
        counts = sg.measures_of_counts(ctx, idf)
        keep("counts", counts)
        chk += float(counts["missing_count"].sum())
    with _timed("central_tendency", sections, ctx):
        ct = sg.measures_of_centralTendency(ctx, idf, int_cols + cat_cols)  # discrete modes (K5)
        keep("central_tendency", ct)
        chk += float(pd.to_numeric(ct["mode_rows"], errors="coerce").fillna(0).sum())
    with _timed("shape", sections, ctx):
        shape = sg.measures_of_shape(ctx, idf)
        keep("shape", shape)
        chk += float(pd.to_numeric(shape["skewness"], errors="coerce").fillna(0).abs().sum())
    with _timed("null_rows", sections, ctx):
        _, nullrows = qc.nullRows_detection(ctx, idf, treatment=False)  # K10 row scan
        keep("null_rows", nullrows)
        chk += float(nullrows["row_count"].sum())
    with _timed("biasedness", sections, ctx):
        _, biased = qc.biasedness_detection(ctx, idf, int_cols + cat_cols, treatment=False, treatment_threshold=0.9)
        keep("biasedness", biased)
    with _timed("outlier_detection", sections, ctx):
        odf_out, outliers = qc.outlier_detection(
            ctx, idf, num_cols, detection_side="both", treatment=True, treatment_method="value_replacement"
        )
        keep("outlier_detection", outliers)
        keep("outlier_treated", odf_out, num_cols)
        chk += float(odf_out.col(num_cols[0]).data.float().nansum().item())
        del odf_out  # free treated copies promptly (125M-row shards: ~75 GB each)

    # ---- association (the MFMA Gram + IV/IG are
    # part of the "full analyzer" headline) ----
    with _timed("correlation", sections, ctx):
        corr = ae.correlation_matrix(ctx, idf, num_cols)  # K8 bf16 MFMA Gram
        keep("correlation", corr)
        chk += float(np.nansum(corr[sorted(num_cols)].to_numpy()))
    with _timed("iv_ig", sections, ctx):
        iv = ae.IV_calculation(ctx, idf, label_col="label", event_label="yes")  # K9
        ig = ae.IG_calculation(ctx, idf, label_col="label", event_label="yes")
        keep("iv", iv)
        keep("ig", ig)
        chk += float(iv["iv"].sum()) + float(ig["ig"].sum())

    # ---- drift (PSI/JSD/HD/KS vs warmup snapshot) ----
    with _timed("binning", sections, ctx):
        binned = T.attribute_binning(ctx, idf, num_cols, bin_size=10, output_mode="append")  # K6
        keep("binned", binned, [c + "_binned" for c in num_cols])
    with _timed("drift", sections, ctx):
        drift_vals = 0.0
        import numpy as _np

        drift_cols = num_cols  # ALL numeric columns (no stride)
        q_freqs = dd.batched_bin_frequencies(binned, [c + "_binned" for c in drift_cols], idf.count(), max_bin=10)
        # vectorize PSI/JSD/HD/KS over the whole (col x bin) matrix at once
        key_union = sorted({k for c in drift_cols for k in source_hist.get(c, {})}
                           | {k for c in drift_cols for k in q_freqs[c + "_binned"][0]}, key=dd._key_order)
        kpos = {k: j for j, k in enumerate(key_union)}
        K = len(key_union)
        P = _np.full((len(drift_cols), K), 0.0001)
        Q = _np.full((len(drift_cols), K), 0.0001)
        for i, c in enumerate(drift_cols):
            for k, v in source_hist.get(c, {}).items():
                P[i, kpos[k]] = max(v, 0.0001)
            qk, qv = q_freqs[c + "_binned"]
            for k, v in zip(qk, qv):
                Q[i, kpos[k]] = max(v, 0.0001)
        M = (P + Q) / 2
        keep("drift_source_freqs", P)
        keep("drift_target_freqs", Q)
        drift_vals += float(_np.sum((P - Q) * _np.log(P / Q)))  # PSI
        drift_vals += float((_np.sum(P * _np.log(P / M)) + _np.sum(Q * _np.log(Q / M))) / 2)  # JSD
        drift_vals += float(_np.sum(_np.sqrt(_np.sum((_np.sqrt(P) - _np.sqrt(Q)) ** 2, axis=1) / 2)))  # HD
        drift_vals += float(_np.sum(_np.max(_np.abs(_np.cumsum(P, axis=1) - _np.cumsum(Q, axis=1)), axis=1)))  # KS
        chk += drift_vals

    # ---- transform ----
    # The transforms need NO stats from the device (fills/cutoffs/LUTs
    # all come from the cached analyzer results), so their checksums
    # accumulate ON-DEVICE and ONE sync closes the step: the host builds
    # frame N+1's launch while the GPU still streams frame N's kernels.
    # `del` stays prompt — freeing is stream-ordered, no sync needed.
    del binned
    chk_dev = torch.zeros((), dtype=torch.float32, device=idf.device)
    with _timed("z_standardization", sections, ctx):
        t1 = T.z_standardization(ctx, idf, num_cols[:N_NUM_CONT])  # K11
        keep("z_standardization", t1, num_cols[:N_NUM_CONT])
        chk_dev += t1.col(num_cols[0]).data.float().nansum()  # whole column
        del t1
    with _timed("imputation_median", sections, ctx):
        t2 = T.imputation_MMM(ctx, idf, method_type="median")
        keep("imputation_median", t2, num_cols + cat_cols)
        chk_dev += t2.col(num_cols[1]).data.float().nansum()
        del t2
    with _timed("cat_label_encoding", sections, ctx):
        t3 = T.cat_to_num_unsupervised(ctx, idf, cat_cols, method_type="label_encoding")  # K12, all 50
        if (cat_cols[0] + "_index") in t3.columns:
            chk_dev += t3.col(cat_cols[0] + "_index").data.float().nansum()
            keep("cat_label_encoding", t3, [c + "_index" for c in cat_cols])
        else:
            chk_dev += t3.col(cat_cols[0]).data.float().nansum()  # nulls are NaN after encoding
            keep("cat_label_encoding", t3, cat_cols)
        del t3
    with _timed("outlier_categories", sections, ctx):
        t4 = T.outlier_categories(ctx, idf, cat_cols, max_category=20)  # all 50
        keep("outlier_categories", t4, cat_cols)
        chk_dev += t4.col(cat_cols[0]).data.float().sum()
        del t4
    chk += float(chk_dev.item())  # the step's ONE transform-phase sync
    return chk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sections", action="store_true",
                    help="print per-section ms (adds sync points; profiling only)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure, also measure the per-section breakdown "
                         "in a pass of its own (same number of steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy "
                         "(stats tables whole, output frames at a fixed seeded row sample)")
    ap.add_argument("--rows", type=int, default=0,
                    help="rows per GPU (default 125M on GPU = the 1Bx200-at-8-GPU shard, 200k on CPU)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    from anovos_amd.core import dist
    from anovos_amd.shared.context import init_context

    ctx = init_context()
    rank = ctx.rank
    world = max(ctx.world_size, 1)
    on_gpu = ctx.device.type == "cuda"
    # GPU default: 125M rows/GPU x 201 cols — at --gpus 8 this IS the
    # BASELINE.json 1Bx200 config (100 GB resident/GPU; bigger shards
    # also amortize host orchestration, see profiles/)
    rows = args.rows or (125_000_000 if on_gpu else 200_000)

    idf = make_synthetic_frame(rows, ctx.device, seed=1234 + rank)

    import tempfile

    from anovos_amd.data_transformer import transformers as T
    from anovos_amd.drift_stability import drift_detector as dd
    from anovos_amd.shared.utils import attributeType_segregation

    model_dir = tempfile.mkdtemp(prefix="anovos_bench_")
    num_cols = attributeType_segregation(idf)[0]

    # warmup builds the drift source snapshot (per-bin frequencies)
    binned = T.attribute_binning(ctx, idf, num_cols, bin_size=10, output_mode="append")
    total = idf.count()
    freqs = dd.batched_bin_frequencies(binned, [c + "_binned" for c in num_cols], total, max_bin=10)
    source_hist = {c: dict(zip(*freqs[c + "_binned"])) for c in num_cols}
    del binned  # 75 GB at the 125M-row shard — must not stay resident

    capture = OutputCapture(rows, ctx.device) if args.dump_outputs and rank == 0 else None

    for _ in range(args.warmup):
        pipeline_step(ctx, idf, source_hist, model_dir)

    dist.barrier()
    ctx.synchronize()
    t0 = time.perf_counter()
    sections = {} if args.sections else None
    for i in range(args.steps):
        pipeline_step(ctx, idf, source_hist, model_dir, sections=sections,
                      capture=capture if i == args.steps - 1 else None)
    dist.barrier()
    ctx.synchronize()
    t1 = time.perf_counter()
    if capture is not None:
        capture.save(args.dump_outputs)

    elapsed = t1 - t0
    # MAX over ranks (slowest rank defines the job)
    elapsed = dist.all_reduce_scalar(elapsed, "max")
    ms_per_step = elapsed / args.steps * 1000.0
    total_rows = rows * world
    value = total_rows / (elapsed / args.steps)

    if args.full and sections is None:
        # per-section breakdown in steps of its own: the sync points it
        # adds must not touch the headline figure above
        sections = {}
        for _ in range(args.steps):
            pipeline_step(ctx, idf, source_hist, model_dir, sections=sections)
    if rank == 0 and sections is not None:
        per = {k: round(v / args.steps, 2) for k, v in sections.items()}
        per["SECTION_SUM"] = round(sum(per.values()), 2)
        print(json.dumps({"sections_ms_per_step": per}))
    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": "rows/sec (whole node) full analyzer+drift+transform",
                    "value": value,
                    "unit": "rows/sec",
                    "n_gpus": world,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": ms_per_step,
                    "higher_is_better": True,
                    "scaling": "weak",
                    "vs_baseline": None,
                    "dtype": "fp32 data + fp64 accumulators",
                    "data": "synthetic",
                    "config": {
                        "model": "anovos-full-pipeline",
                        "rows_per_gpu": rows,
                        "n_cols": 201,
                        "global_batch": total_rows,
                        "seq_len": None,
                        "parallelism": f"dp{world}",
                    },
                }
            )
        )


if __name__ == "__main__":
    main()
