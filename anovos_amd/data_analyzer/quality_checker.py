"""Data-quality checks + treatments — parity with reference
data_analyzer/quality_checker.py (1,711 LoC).

Each function returns ``(treated_df, stats_df)`` like the reference. The
MI355X-native twists:

- duplicate_detection: 64-bit row-hash distinct (K5) instead of a
  groupBy-all-cols shuffle (reference quality_checker.py:122),
- nullRows_detection: fused row-scan kernel over all columns (K10)
  instead of a per-row python UDF (:248-258),
- invalidEntries_detection: the regex battery runs over each column's
  DICTIONARY (small) and flags rows via one LUT gather (:1504-1609
  semantics at dictionary cost),
- outlier_detection: thresholds from the fused quantile/moments kernels
  on a sample, treatment as fused elementwise clamps (:843-906).
"""

from __future__ import annotations

import re
import warnings
from typing import Dict, List

import numpy as np
import pandas as pd
import torch

from anovos_amd.core import dist
from anovos_amd.core.dtypes import NULL_CODE
from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.data_analyzer.stats_generator import (
    measures_of_cardinality,
    missingCount_computation,
    mode_computation,
    uniqueCount_computation,
)
from anovos_amd.data_transformer.transformers import _load_model, _save_model, imputation_MMM
from anovos_amd.ops import histogram as hist_ops
from anovos_amd.ops import rowops
from anovos_amd.ops import stats as stats_ops
from anovos_amd.shared.utils import attributeType_segregation, get_dtype, normalize_columns
from anovos_amd.shared.tracing import traced


def _parse_bool(v, name="treatment"):
    if str(v).lower() == "true":
        return True
    if str(v).lower() == "false":
        return False
    raise TypeError(f"Non-Boolean input for {name}")


@traced
def duplicate_detection(ctx, idf, list_of_cols="all", drop_cols=[], treatment=False, print_impact=False):
    """Reference quality_checker.py:49-150. treatment=True returns the
    deduplicated frame."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    cols = normalize_columns(idf, list_of_cols, drop_cols)
    if len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    treatment = _parse_bool(treatment)

    from anovos_amd.ops import dedup as dedup_ops
    from anovos_amd.ops.groupby import row_hash

    h = row_hash(idf.select(cols), cols)
    idf_count = idf.count()
    # keep first local occurrence of each hash, then resolve cross-rank
    # winners with the hash-exchange protocol (ops/dedup.py — a row
    # present only on a non-owner rank must still survive)
    uniq, first_idx = dedup_ops.unique_first(h)
    keep_idx = first_idx[dedup_ops.global_keep_mask(uniq)]
    odf_tmp = idf.filter_rows(keep_idx)
    odf_tmp_count = odf_tmp.count()
    odf = odf_tmp if treatment else idf
    odf_print = pd.DataFrame(
        [
            ["rows_count", float(idf_count)],
            ["unique_rows_count", float(odf_tmp_count)],
            ["duplicate_rows", float(idf_count - odf_tmp_count)],
            ["duplicate_pct", round((idf_count - odf_tmp_count) / idf_count, 4)],
        ],
        columns=["metric", "value"],
    )
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print


def _unique_first(h: torch.Tensor):
    uniq, inv = torch.unique(h, return_inverse=True)
    first = torch.full((uniq.numel(),), h.numel(), dtype=torch.long, device=h.device)
    first.scatter_reduce_(0, inv, torch.arange(h.numel(), device=h.device), reduce="amin")
    return uniq, first


@traced
def nullRows_detection(ctx, idf, list_of_cols="all", drop_cols=[], treatment=False, treatment_threshold=0.8, print_impact=False):
    """Reference quality_checker.py:152-283. Returns (odf, odf_print) with
    odf_print schema [null_cols_count, row_count, row_pct, flagged/treated]."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    cols = normalize_columns(idf, list_of_cols, drop_cols)
    if len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    treatment = _parse_bool(treatment)
    treatment_threshold = float(treatment_threshold)
    if treatment_threshold < 0 or treatment_threshold > 1:
        raise TypeError("Invalid input for Treatment Threshold Value")

    counts = rowops.row_null_counts(idf, cols)  # [local_rows] int32

    def flag(t):
        # one rule for the rows (treatment) and for the histogram buckets
        if treatment_threshold == 1:
            return t == len(cols)
        return t > (len(cols) * treatment_threshold)

    total = idf.count()
    # null-count histogram: LDS-staged code_counts on GPU (a torch
    # scatter_add here costs ~1.8 s of fp64 atomic contention on 10M rows —
    # measured; bincount/code_counts is ~1000x cheaper). `flagged` is a
    # function of the count alone, so the buckets are split by it on the
    # host and no per-row key is built.
    size = len(cols) + 1
    from anovos_amd.ops import backend as _backend

    if counts.is_cuda and _backend.use_hip(counts):
        hist = _backend.hip_ext().code_counts(counts.contiguous(), size).to(torch.float64)
    else:
        hist = torch.bincount(counts.to(torch.long), minlength=size).to(torch.float64)
    dist.all_reduce_(hist, "sum")
    hist_l = hist.cpu().numpy().tolist()
    bucket_flag = flag(torch.arange(size, dtype=torch.int32)).tolist()
    rows = []
    for nc in range(size):
        c = hist_l[nc]
        if c > 0:
            rows.append([nc, int(c), round(c / total, 4), int(bucket_flag[nc])])
    odf_print = pd.DataFrame(rows, columns=["null_cols_count", "row_count", "row_pct", "flagged"])

    if treatment:
        odf = idf.filter_rows(~flag(counts))
        odf_print = odf_print.rename(columns={"flagged": "treated"})
    else:
        odf = idf
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print


@traced
def nullColumns_detection(
    ctx,
    idf,
    list_of_cols="missing",
    drop_cols=[],
    treatment=False,
    treatment_method="row_removal",
    treatment_configs={},
    stats_missing={},
    stats_unique={},
    stats_mode={},
    print_impact=False,
):
    """Reference quality_checker.py:286-548. Treatments: row_removal /
    column_removal / MMM / KNN / regression / MF / auto."""
    if stats_missing == {}:
        odf_print = missingCount_computation(ctx, idf)
    else:
        from anovos_amd.data_ingest.data_ingest import read_dataset

        odf_print = read_dataset(ctx, **stats_missing, sharded=False).to_pandas()[["attribute", "missing_count", "missing_pct"]]
    missing_cols = odf_print[odf_print["missing_count"] > 0]["attribute"].tolist()

    num_cols, cat_cols, _ = attributeType_segregation(idf)
    if list_of_cols == "all":
        list_of_cols = num_cols + cat_cols
    if list_of_cols == "missing":
        list_of_cols = missing_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|") if x.strip()]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    list_of_cols = [e for e in dict.fromkeys(list_of_cols) if e not in drop_cols]
    if len(list_of_cols) == 0:
        warnings.warn("No Null Detection - No column(s) to analyze")
        return idf, pd.DataFrame(columns=["attribute", "missing_count", "missing_pct"])
    if any(x not in idf.columns for x in list_of_cols):
        raise TypeError("Invalid input for Column(s)")
    treatment = _parse_bool(treatment)
    if treatment_method not in ("MMM", "row_removal", "column_removal", "KNN", "regression", "MF", "auto"):
        raise TypeError("Invalid input for method_type")
    treatment_configs = dict(treatment_configs)
    treatment_threshold = treatment_configs.pop("treatment_threshold", None)
    if treatment_threshold:
        treatment_threshold = float(treatment_threshold)
    elif treatment_method == "column_removal":
        raise TypeError("Invalid input for column removal threshold")

    odf_print = odf_print[odf_print["attribute"].isin(list_of_cols)]
    odf = idf
    if treatment:
        if treatment_threshold:
            threshold_cols = odf_print[odf_print["missing_pct"] > treatment_threshold]["attribute"].tolist()
        if treatment_method == "column_removal":
            odf = idf.drop(threshold_cols)
        elif treatment_method == "row_removal":
            remove_cols = odf_print[odf_print["missing_pct"] == 1.0]["attribute"].tolist()
            cols_ = [e for e in list_of_cols if e not in remove_cols]
            if treatment_threshold:
                cols_ = [e for e in threshold_cols if e not in remove_cols]
            counts = rowops.row_null_counts(idf, cols_) if cols_ else torch.zeros(idf.local_rows(), dtype=torch.int32, device=idf.device)
            odf = idf.filter_rows(counts == 0)
        elif treatment_method == "MMM":
            if stats_unique == {}:
                uc = uniqueCount_computation(ctx, idf, list_of_cols)
            else:
                from anovos_amd.data_ingest.data_ingest import read_dataset

                uc = read_dataset(ctx, **stats_unique, sharded=False).to_pandas()
            remove_cols = uc[uc["unique_values"] < 2]["attribute"].tolist()
            cols_ = [e for e in list_of_cols if e not in remove_cols]
            if treatment_threshold:
                cols_ = [e for e in threshold_cols if e not in remove_cols]
            odf = imputation_MMM(ctx, idf, cols_, **treatment_configs, stats_missing=stats_missing, stats_mode=stats_mode, print_impact=print_impact)
        else:  # KNN / regression / MF / auto
            from anovos_amd.data_transformer.transformers_advanced import (
                auto_imputation,
                imputation_matrixFactorization,
                imputation_sklearn,
            )

            cols_ = threshold_cols if treatment_threshold else list_of_cols
            cols_ = [e for e in cols_ if e in num_cols]
            func_mapping = {
                "KNN": imputation_sklearn,
                "regression": imputation_sklearn,
                "MF": imputation_matrixFactorization,
                "auto": auto_imputation,
            }
            if treatment_method == "KNN":
                treatment_configs.setdefault("method_type", "KNN")
            if treatment_method == "regression":
                treatment_configs.setdefault("method_type", "regression")
            odf = func_mapping[treatment_method](ctx, idf, cols_, **treatment_configs, stats_missing=stats_missing, print_impact=print_impact)
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print.reset_index(drop=True)


@traced
def outlier_detection(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    detection_side="upper",
    detection_configs={
        "pctile_lower": 0.05,
        "pctile_upper": 0.95,
        "stdev_lower": 3.0,
        "stdev_upper": 3.0,
        "IQR_lower": 1.5,
        "IQR_upper": 1.5,
        "min_validation": 2,
    },
    treatment=True,
    treatment_method="value_replacement",
    pre_existing_model=False,
    model_path="NA",
    sample_size=1000000,
    output_mode="replace",
    print_impact=False,
):
    """Reference quality_checker.py:550-1045. Vote-based bounds from
    pctile/stdev/IQR detectors; treatment value/null/row."""
    import copy

    column_order = idf.columns
    num_cols = attributeType_segregation(idf)[0]
    treatment = _parse_bool(treatment)
    pre_existing_model = _parse_bool(pre_existing_model, "pre_existing_model")
    _empty_stats = pd.DataFrame(columns=["attribute", "lower_outliers", "upper_outliers", "excluded_due_to_skewness"])
    if not treatment and not print_impact:
        if (not pre_existing_model and model_path == "NA") or pre_existing_model:
            warnings.warn("The original idf will be the only output. Set print_impact=True to perform detection without treatment")
            return idf, _empty_stats
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if not list_of_cols:
        warnings.warn("No Outlier Check - No numerical column to analyze")
        return idf, _empty_stats
    if any(x not in num_cols for x in list_of_cols):
        raise TypeError("Invalid input for Column(s)")
    if detection_side not in ("upper", "lower", "both"):
        raise TypeError("Invalid input for detection_side")
    if treatment_method not in ("null_replacement", "row_removal", "value_replacement"):
        raise TypeError("Invalid input for treatment_method")
    if output_mode not in ("replace", "append"):
        raise TypeError("Invalid input for output_mode")
    detection_configs = dict(detection_configs)
    for arg in ["pctile_lower", "pctile_upper"]:
        if arg in detection_configs and (detection_configs[arg] < 0 or detection_configs[arg] > 1):
            raise TypeError("Invalid input for " + arg)

    skewed_cols: List[str] = []
    if pre_existing_model:
        dfm = _load_model(model_path, "outlier_numcols")
        params = []
        kept = []
        for c in list_of_cols:
            row = dfm[dfm["attribute"] == c]
            if not len(row):
                continue
            p = list(row.iloc[0]["parameters"])
            if "skewed_attribute" in [str(x) for x in p]:
                skewed_cols.append(c)
                continue
            params.append([None if x is None or (isinstance(x, float) and x != x) else float(x) for x in p])
            kept.append(c)
        list_of_cols = kept
    else:
        sides = {"lower": ["_lower"], "upper": ["_upper"], "both": ["_lower", "_upper"]}[detection_side]
        methodologies = sorted({k.rsplit("_", 1)[0] for k in detection_configs if k.rsplit("_", 1)[0] in ("pctile", "stdev", "IQR")})
        num_methodologies = len([m for m in methodologies if any(m + s in detection_configs for s in sides)])
        if "min_validation" in detection_configs:
            if detection_configs["min_validation"] > max(num_methodologies, 1):
                raise TypeError(
                    "Invalid input for min_validation of detection_configs. It cannot be larger than the total number of methodologies on any side that detection will be applied over."
                )
        else:
            detection_configs["min_validation"] = num_methodologies

        idf_count = idf.count()
        # stats-reuse: when the analyzer already computed the needed
        # full-frame quantiles/moments (workflow runs stats first), use
        # them directly — more accurate than the reference's 1M-row
        # sample AND free (no sampling pass, no fresh quantile sketch)
        _need_q = set()
        if "pctile" in methodologies:
            _need_q.update([detection_configs.get("pctile_lower", 0.05), detection_configs.get("pctile_upper", 0.95)])
        if "IQR" in methodologies:
            _need_q.update([0.25, 0.75])
        _cached_full = all(
            ("q", p) in idf.col(c).cache for c in list_of_cols for p in _need_q
        ) and ("stdev" not in methodologies or all("moments" in idf.col(c).cache for c in list_of_cols))
        if dist.is_dist():
            # the branch chooses between different collective sequences —
            # take it only when EVERY rank has the cache (all-reduce min)
            _cached_full = bool(dist.all_reduce_scalar(1.0 if _cached_full else 0.0, "min"))
        if _cached_full:
            idf_sample = idf
        elif idf_count > sample_size:
            from anovos_amd.data_ingest.data_sampling import data_sample

            idf_sample = data_sample(idf.select(list_of_cols), fraction=sample_size / idf_count, method_type="random", seed_value=11)
        else:
            idf_sample = idf.select(list_of_cols)

        empty_params = [[None, None] for _ in list_of_cols]
        pcts = [detection_configs.get("pctile_lower", 0.05), detection_configs.get("pctile_upper", 0.95)]
        qres = hist_ops.approx_quantiles(idf_sample, list_of_cols, pcts, rel_err=0.01)
        pctile_params = [qres[c] for c in list_of_cols]
        for c, p in zip(list(list_of_cols), list(pctile_params)):
            if p[0] == p[1]:
                skewed_cols.append(c)
        if skewed_cols:
            warnings.warn("Columns excluded from outlier detection due to highly skewed distribution: " + ",".join(skewed_cols))
            keep_idx = [i for i, c in enumerate(list_of_cols) if c not in skewed_cols]
            list_of_cols = [list_of_cols[i] for i in keep_idx]
            pctile_params = [pctile_params[i] for i in keep_idx]
            empty_params = [[None, None] for _ in list_of_cols]
        if "pctile" not in methodologies:
            pctile_params = copy.deepcopy(empty_params)
        if "stdev" in methodologies:
            moments = stats_ops.frame_moments(idf_sample, list_of_cols)
            stdev_params = [
                [
                    moments[c].mean - detection_configs.get("stdev_lower", 0.0) * moments[c].stddev,
                    moments[c].mean + detection_configs.get("stdev_upper", 0.0) * moments[c].stddev,
                ]
                for c in list_of_cols
            ]
        else:
            stdev_params = copy.deepcopy(empty_params)
        if "IQR" in methodologies:
            qres2 = hist_ops.approx_quantiles(idf_sample, list_of_cols, [0.25, 0.75], rel_err=0.01)
            IQR_params = [
                [
                    qres2[c][0] - detection_configs.get("IQR_lower", 0.0) * (qres2[c][1] - qres2[c][0]),
                    qres2[c][1] + detection_configs.get("IQR_upper", 0.0) * (qres2[c][1] - qres2[c][0]),
                ]
                for c in list_of_cols
            ]
        else:
            IQR_params = copy.deepcopy(empty_params)

        n = detection_configs["min_validation"]
        params = []
        for x, y, z in zip(pctile_params, stdev_params, IQR_params):
            lowers = sorted([v for v in [x[0], y[0], z[0]] if v is not None], reverse=True)
            uppers = sorted([v for v in [x[1], y[1], z[1]] if v is not None])
            lower = lowers[n - 1] if lowers else None
            upper = uppers[n - 1] if uppers else None
            if detection_side == "lower":
                params.append([lower, None])
            elif detection_side == "upper":
                params.append([None, upper])
            else:
                params.append([lower, upper])
        if model_path != "NA":
            skewed_param = {"lower": ["skewed_attribute", None], "upper": [None, "skewed_attribute"], "both": ["skewed_attribute", "skewed_attribute"]}[detection_side]
            dfm = pd.DataFrame(
                {
                    "attribute": list_of_cols + skewed_cols,
                    "parameters": [[None if v is None else str(v) for v in p] for p in params] + [skewed_param] * len(skewed_cols),
                }
            )
            _save_model(dfm, model_path, "outlier_numcols")
            if not treatment and not print_impact:
                return idf, _empty_stats

    odf = idf
    rows_print = []
    flags: Dict[str, torch.Tensor] = {}

    from anovos_amd.ops import backend as _backend

    first = idf.col(list_of_cols[0]).data if list_of_cols else None
    fused_ok = (
        first is not None
        and first.is_cuda
        and _backend.use_hip(first)
        and treatment_method in ("value_replacement", "null_replacement")
    )
    if fused_ok:
        # one fused HIP launch for ALL columns: counts + clamp/null-out
        # (K10/K11) — replaces ~10 aten launches per column
        ext = _backend.hip_ext()
        lo_t, hi_t = [], []
        for (lo, hi) in params:
            use_lo = detection_side in ("lower", "both") and lo is not None
            use_hi = detection_side in ("upper", "both") and hi is not None
            lo_t.append(float(lo) if use_lo else float("nan"))
            hi_t.append(float(hi) if use_hi else float("nan"))
        mode = 0 if not treatment else (1 if treatment_method == "value_replacement" else 2)
        tensors = [idf.col(c).data.contiguous() for c in list_of_cols]
        # bounds travel as float64: the kernel gives the verdict of the
        # double comparison, which a bound rounded to float32 would move
        counts, outs = ext.outlier_clamp_columns(
            tensors, torch.tensor(lo_t, dtype=torch.float64), torch.tensor(hi_t, dtype=torch.float64), mode
        )
        counts = dist.all_reduce_(counts.to(torch.float64), "sum").cpu().to(torch.int64)
        for i, c in enumerate(list_of_cols):
            rows_print.append([c, int(counts[i, 0]), int(counts[i, 1]), 0])
            if mode:
                odf = odf.with_column(c + "_outliered", Column(c + "_outliered", idf.col(c).dtype, outs[i]))
        if mode:
            from anovos_amd.data_transformer.transformers import _finish_output

            odf = _finish_output(idf, odf, list_of_cols, "_outliered", output_mode)
        if not treatment:
            odf = idf
        odf_print = pd.DataFrame(rows_print + [[c, 0, 0, 1] for c in skewed_cols], columns=["attribute", "lower_outliers", "upper_outliers", "excluded_due_to_skewness"])
        if print_impact:
            print(odf_print.to_string(index=False))
        return odf, odf_print

    local_lo_hi = []  # batched cross-rank count merge: ONE collective below
    for c, (lo, hi) in zip(list_of_cols, params):
        x = idf.col(c).data
        flag = torch.zeros_like(x, dtype=torch.int8)
        # the verdict is that of the double comparison, as in the fused
        # kernel: a float32 column against a Python scalar would compare
        # in float32, with the bound rounded (NaN compares false)
        xd = x.to(torch.float64)
        if detection_side in ("lower", "both") and lo is not None:
            flag = torch.where(xd < float(lo), torch.full_like(flag, -1), flag)
        if detection_side in ("upper", "both") and hi is not None:
            flag = torch.where(xd > float(hi), torch.ones_like(flag), flag)
        flags[c] = flag
        local_lo_hi.extend([int((flag == -1).sum()), int((flag == 1).sum())])
        if treatment and treatment_method in ("value_replacement", "null_replacement"):
            if treatment_method == "value_replacement":
                lo_v = float(lo) if lo is not None else float("nan")
                hi_v = float(hi) if hi is not None else float("nan")
            else:
                lo_v = hi_v = float("nan")
            # the bound rounded to the column's dtype, as the kernel writes it
            # (full_like refuses a double beyond the float32 range)
            lo_r, hi_r = (torch.tensor(v, dtype=torch.float64, device=x.device).to(x.dtype) for v in (lo_v, hi_v))
            y = torch.where(flags[c] == 1, hi_r, x)
            y = torch.where(flags[c] == -1, lo_r, y)
            odf = odf.with_column(c + "_outliered", Column(c + "_outliered", idf.col(c).dtype, y))
            if output_mode == "replace":
                odf = odf.drop([c]).rename({c + "_outliered": c})
    merged = dist.all_reduce_scalars(local_lo_hi) if local_lo_hi else []
    for i, c in enumerate(list_of_cols):
        rows_print.append([c, int(merged[2 * i]), int(merged[2 * i + 1]), 0])
    if treatment and treatment_method == "row_removal":
        keep = torch.ones(idf.local_rows(), dtype=torch.bool, device=idf.device)
        for c in list_of_cols:
            keep &= flags[c] == 0
        odf = odf.filter_rows(keep)
    if treatment and output_mode == "replace":
        odf = odf.select([c for c in column_order if c in odf.columns])
    if not treatment:
        odf = idf
    odf_print = pd.DataFrame(rows_print + [[c, 0, 0, 1] for c in skewed_cols], columns=["attribute", "lower_outliers", "upper_outliers", "excluded_due_to_skewness"])
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print


@traced
def multivariate_outlier_detection(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    confidence=0.999,
    threshold=None,
    rank_tol=1e-6,
    treatment=False,
    append_distance=False,
    distance_col="mahalanobis_d2",
    pre_existing_model=False,
    model_path="NA",
    sample_size=1000000,
    print_impact=False,
):
    """Beyond the reference (whose outlier_detection is univariate): rows
    whose combination of values is improbable although every coordinate
    may be ordinary. The squared Mahalanobis distance of every row,
    d2 = (x - mu)^T Sigma^+ (x - mu) over the numerical columns
    (ops/mahalanobis.py; on the GPU the MFMA kernel K26), is compared in
    double against `threshold`, by default the chi-square quantile
    chi2.ppf(confidence, rank). The model (mu, sd, whitening matrix) is
    fitted on a sample of `sample_size` rows when the frame is larger; the
    distance is always taken on the full frame. A null counts as the
    column mean. treatment=True removes the flagged rows;
    append_distance=True appends d2 as the f32 column `distance_col`."""
    from anovos_amd.ops import mahalanobis as maha_ops

    num_cols = attributeType_segregation(idf)[0]
    treatment = _parse_bool(treatment)
    append_distance = _parse_bool(append_distance, "append_distance")
    pre_existing_model = _parse_bool(pre_existing_model, "pre_existing_model")
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if any(x not in num_cols for x in list_of_cols):
        raise TypeError("Invalid input for Column(s)")
    if isinstance(confidence, bool) or not isinstance(confidence, (int, float)) or not 0 < confidence < 1:
        raise TypeError("Invalid input for confidence: a value between 0 and 1 (exclusive)")
    if threshold is not None and (
        isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not threshold > 0
    ):
        raise TypeError("Invalid input for threshold: a positive number")
    if isinstance(rank_tol, bool) or not isinstance(rank_tol, (int, float)) or not 0 <= rank_tol < 1:
        raise TypeError("Invalid input for rank_tol: a value in [0, 1)")
    if append_distance and distance_col in idf.columns:
        raise TypeError(f"Invalid input for distance_col: column '{distance_col}' already exists")

    if pre_existing_model:
        dfm = _load_model(model_path, "outlier_multivariate")
        missing = [c for c in dfm["attribute"] if c not in idf.columns]
        if missing:
            raise TypeError(f"Invalid input for Column(s): model attributes not in the frame: {missing}")
        used = dfm[dfm["sd"] > 0]
        excluded = [str(c) for c in dfm[~(dfm["sd"] > 0)]["attribute"]]
        W = np.array([list(w) for w in used["W"]], dtype=np.float64).T  # [r, k]
        model = maha_ops.WhiteningModel(
            [str(c) for c in used["attribute"]],
            used["mean"].to_numpy(dtype=np.float64),
            used["sd"].to_numpy(dtype=np.float64),
            np.ascontiguousarray(W),
            int(dfm["rank"].iloc[0]),
            excluded,
        )
        if any(c not in num_cols for c in model.columns):
            raise TypeError("Invalid input for Column(s)")
        model_threshold = float(dfm["threshold"].iloc[0])
    else:
        if len(list_of_cols) < 2:
            raise TypeError("Invalid input for Column(s): at least 2 numerical columns are needed")
        if len(list_of_cols) > maha_ops.ROWQUAD_MAX_COLS:
            raise TypeError(
                f"Invalid input for Column(s): at most {maha_ops.ROWQUAD_MAX_COLS} numerical columns (ROWQUAD_MAX_COLS)"
            )
        idf_count = idf.count()
        if idf_count > sample_size:
            from anovos_amd.data_ingest.data_sampling import data_sample

            idf_sample = data_sample(idf.select(list_of_cols), fraction=sample_size / idf_count, method_type="random", seed_value=11)
        else:
            idf_sample = idf.select(list_of_cols)
        model = maha_ops.fit_whitening(idf_sample, list_of_cols, rank_tol=rank_tol)
        model_threshold = None
    if len(model.columns) < 2 or model.rank < 1:
        raise TypeError("Invalid input for Column(s): fewer than 2 numerical columns with a non-zero variance")
    if len(model.columns) > maha_ops.ROWQUAD_MAX_COLS:
        raise TypeError(f"Invalid input for Column(s): at most {maha_ops.ROWQUAD_MAX_COLS} numerical columns (ROWQUAD_MAX_COLS)")
    if model.excluded:
        warnings.warn("Columns excluded from multivariate outlier detection (constant): " + ",".join(model.excluded))

    if threshold is not None:
        cut = float(threshold)
    elif model_threshold is not None:
        cut = model_threshold
    else:
        from scipy.stats import chi2

        cut = float(chi2.ppf(confidence, model.rank))
    if model_path != "NA" and not pre_existing_model:
        k_all = len(model.columns) + len(model.excluded)
        dfm = pd.DataFrame(
            {
                "attribute": model.columns + model.excluded,
                "mean": list(model.mean) + [float("nan")] * len(model.excluded),
                "sd": list(model.sd) + [0.0] * len(model.excluded),
                # column j of W, the r weights of attribute j
                "W": [model.W[:, j].tolist() for j in range(len(model.columns))] + [[] for _ in model.excluded],
                "rank": [model.rank] * k_all,
                "threshold": [cut] * k_all,
            }
        )
        _save_model(dfm, model_path, "outlier_multivariate")

    d2 = maha_ops.mahalanobis_d2(idf, model.columns, model)
    # the verdict is that of the double comparison, as K10's
    flag = d2.to(torch.float64) > cut
    # one batched collective on every rank, empty shards included: the
    # count is summed, the maximum travels in a slot per rank
    world, me = dist.world_size(), dist.rank()
    local = [float(flag.sum())] + [0.0] * world
    local[1 + me] = float(d2.max()) if d2.numel() else 0.0
    merged = dist.all_reduce_scalars(local)
    outlier_rows = int(round(merged[0]))
    max_distance = max(merged[1:])
    rows_count = idf.count()

    odf = idf
    if append_distance:
        odf = odf.with_column(distance_col, Column(distance_col, "float", d2))
    if treatment:
        odf = odf.filter_rows(~flag)
    odf_print = pd.DataFrame(
        [
            ["rows_count", float(rows_count)],
            ["attributes_count", float(len(model.columns))],
            ["rank", float(model.rank)],
            ["threshold", cut],
            ["outlier_rows", float(outlier_rows)],
            ["outlier_pct", round(outlier_rows / rows_count, 4) if rows_count else 0.0],
            ["max_distance", float(max_distance)],
            ["excluded_constant_attributes", ",".join(model.excluded)],
        ],
        columns=["metric", "value"],
    )
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print


@traced
def IDness_detection(ctx, idf, list_of_cols="all", drop_cols=[], treatment=False, treatment_threshold=0.8, stats_unique={}, print_impact=False):
    """Reference quality_checker.py:1048-1183."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|")]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    list_of_cols = [e for e in dict.fromkeys(list_of_cols) if e not in drop_cols]
    dtype_map = dict(idf.dtypes)
    list_of_cols = [c for c in list_of_cols if dtype_map.get(c) in ("string", "int", "bigint", "long")]
    if any(x not in idf.columns for x in list_of_cols):
        raise TypeError("Invalid input for Column(s)")
    if len(list_of_cols) == 0:
        warnings.warn("No IDness Check - No discrete column(s) to analyze")
        return idf, pd.DataFrame(columns=["attribute", "unique_values", "IDness", "flagged"])
    treatment_threshold = float(treatment_threshold)
    if treatment_threshold < 0 or treatment_threshold > 1:
        raise TypeError("Invalid input for Treatment Threshold Value")
    treatment = _parse_bool(treatment)
    if stats_unique == {}:
        odf_print = measures_of_cardinality(ctx, idf, list_of_cols)
    else:
        from anovos_amd.data_ingest.data_ingest import read_dataset

        odf_print = read_dataset(ctx, **stats_unique, sharded=False).to_pandas()
        odf_print = odf_print[odf_print["attribute"].isin(list_of_cols)]
    odf_print = odf_print.copy()
    odf_print["flagged"] = (odf_print["IDness"] >= treatment_threshold).astype(int)
    if treatment:
        remove_cols = odf_print[odf_print["flagged"] == 1]["attribute"].tolist()
        odf = idf.drop(remove_cols)
        odf_print = odf_print.rename(columns={"flagged": "treated"})
    else:
        odf = idf
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print.reset_index(drop=True)


@traced
def biasedness_detection(ctx, idf, list_of_cols="all", drop_cols=[], treatment=False, treatment_threshold=0.8, stats_mode={}, print_impact=False):
    """Reference quality_checker.py:1185-1340: flag columns whose mode
    covers >= threshold of non-null rows."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|")]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    list_of_cols = [e for e in dict.fromkeys(list_of_cols) if e not in drop_cols]
    dtype_map = dict(idf.dtypes)
    list_of_cols = [c for c in list_of_cols if dtype_map.get(c) in ("string", "int", "bigint", "long")]
    if any(x not in idf.columns for x in list_of_cols):
        raise TypeError("Invalid input for Column(s)")
    if len(list_of_cols) == 0:
        warnings.warn("No biasedness Check - No discrete column(s) to analyze")
        return idf, pd.DataFrame(columns=["attribute", "mode", "mode_rows", "mode_pct", "flagged"])
    if treatment_threshold < 0 or treatment_threshold > 1:
        raise TypeError("Invalid input for Treatment Threshold Value")
    treatment = _parse_bool(treatment)
    if stats_mode == {}:
        nulls, total = stats_ops.null_counts(idf, list_of_cols)
        dfm = mode_computation(ctx, idf, list_of_cols)
        dfm["mode_pct"] = [
            round(r["mode_rows"] / (total - nulls[r["attribute"]]), 4) if (total - nulls[r["attribute"]]) else None
            for _, r in dfm.iterrows()
        ]
        odf_print = dfm[["attribute", "mode", "mode_rows", "mode_pct"]]
    else:
        from anovos_amd.data_ingest.data_ingest import read_dataset

        odf_print = read_dataset(ctx, **stats_mode, sharded=False).to_pandas()[["attribute", "mode", "mode_rows", "mode_pct"]]
        odf_print = odf_print[odf_print["attribute"].isin(list_of_cols)]
    odf_print = odf_print.copy()
    odf_print["flagged"] = [(1 if (p is None or p != p or p >= treatment_threshold) else 0) for p in odf_print["mode_pct"]]
    if treatment:
        remove_cols = odf_print[odf_print["flagged"] == 1]["attribute"].tolist()
        odf = idf.drop(remove_cols)
        odf_print = odf_print.rename(columns={"flagged": "treated"})
    else:
        odf = idf
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print.reset_index(drop=True)


NULL_VOCAB = ["", " ", "nan", "null", "na", "inf", "n/a", "not defined", "none", "undefined", "blank", "unknown"]
SPECIAL_CHARS_VOCAB = ["&", "$", ";", ":", ".", ",", "*", "#", "@", "_", "?", "%", "!", "^", "(", ")", "-", "/", "'"]


def _detect_invalid_value(e, detection_type, invalid_entries, valid_entries, partial_match) -> int:
    """The reference's per-value detect() (quality_checker.py:1540-1602)."""
    if e is None:
        return -1  # null passthrough
    if detection_type in ("auto", "both"):
        s = str(e).lower().strip()
        if s in NULL_VOCAB or s in SPECIAL_CHARS_VOCAB:
            return 1
        if re.search(r"\b([a-zA-Z0-9])\1\1+\b", s):
            return 1
        l = len(s)
        if l >= 3:
            if all(ord(s[i]) - ord(s[i - 1]) == 1 for i in range(1, l)):
                return 1
    if detection_type in ("manual", "both"):
        s = str(e).lower().strip()
        for regex in invalid_entries:
            p = re.compile(regex)
            if (partial_match and re.search(p, s)) or ((not partial_match) and p.fullmatch(s)):
                return 1
        if valid_entries:
            matched = any(
                (partial_match and re.search(re.compile(rx), s)) or ((not partial_match) and re.compile(rx).fullmatch(s))
                for rx in valid_entries
            )
            if not matched:
                return 1
    return 0


@traced
def invalidEntries_detection(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    detection_type="auto",
    invalid_entries=[],
    valid_entries=[],
    partial_match=False,
    treatment=False,
    treatment_method="null_replacement",
    treatment_configs={},
    stats_missing={},
    stats_unique={},
    stats_mode={},
    output_mode="replace",
    print_impact=False,
):
    """Reference quality_checker.py:1342-1711. The regex battery runs over
    each categorical column's dictionary (and numeric uniques), never the
    rows; flags materialize via a LUT gather."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|")]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    list_of_cols = [e for e in dict.fromkeys(list_of_cols) if e not in drop_cols]
    if any(x not in idf.columns for x in list_of_cols) or len(list_of_cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    if output_mode not in ("replace", "append"):
        raise TypeError("Invalid input for output_mode")
    treatment = _parse_bool(treatment)
    if treatment_method not in ("MMM", "null_replacement", "column_removal"):
        raise TypeError("Invalid input for method_type")
    treatment_configs = dict(treatment_configs)
    treatment_threshold = treatment_configs.pop("treatment_threshold", None)
    if treatment_threshold:
        treatment_threshold = float(treatment_threshold)
    elif treatment_method == "column_removal":
        raise TypeError("Invalid input for column removal threshold")

    total = idf.count()
    invalid_masks: Dict[str, torch.Tensor] = {}
    rows_print = []
    for c in list_of_cols:
        col = idf.col(c)
        if col.kind == "categorical":
            values = list(col.dictionary or [])
            verdict = [
                _detect_invalid_value(v, detection_type, invalid_entries, valid_entries, partial_match) for v in values
            ]
            lut = torch.tensor([1 if v == 1 else 0 for v in verdict] + [0], dtype=torch.int8, device=col.data.device)
            codes = col.data.to(torch.long)
            codes = torch.where(codes == NULL_CODE, torch.full_like(codes, len(values)), codes)
            mask = lut[codes].bool()
            bad_values = [str(values[i]) for i, v in enumerate(verdict) if v == 1]
        else:
            from anovos_amd.ops.groupby import numeric_value_counts

            vals, _cnts = numeric_value_counts(idf, c)
            vv = vals.cpu().numpy()
            strs = [_fmt_like_spark(v) for v in vv]
            verdict = [
                _detect_invalid_value(s, detection_type, invalid_entries, valid_entries, partial_match) for s in strs
            ]
            bad = torch.tensor([v for v, ver in zip(vv.tolist(), verdict) if ver == 1], dtype=col.data.dtype, device=col.data.device)
            bad_values = [_fmt_like_spark(v) for v, ver in zip(vv.tolist(), verdict) if ver == 1]
            if bad.numel():
                mask = torch.isin(col.data, bad)
            else:
                mask = torch.zeros_like(col.data, dtype=torch.bool)
        invalid_masks[c] = mask
        inv_count = int(dist.all_reduce_scalar(int(mask.sum())))
        rows_print.append([c, "|".join(sorted(set(bad_values))), inv_count, round(inv_count / total, 4) if total else None])
    odf_print = pd.DataFrame(rows_print, columns=["attribute", "invalid_entries", "invalid_count", "invalid_pct"])

    odf = idf
    if treatment:
        if treatment_threshold:
            threshold_cols = odf_print[odf_print["invalid_pct"] > treatment_threshold]["attribute"].tolist()
        if treatment_method in ("null_replacement", "MMM"):
            targets = list_of_cols if not treatment_threshold else threshold_cols
            for c in targets:
                col = odf.col(c)
                from anovos_amd.data_ingest.data_ingest import _null_where

                data = _null_where(col, invalid_masks[c])
                name = c if output_mode == "replace" else c + "_invalid"
                odf = odf.with_column(name, Column(name, col.dtype, data, col.dictionary))
        if treatment_method == "column_removal":
            odf = idf.drop(threshold_cols)
        if treatment_method == "MMM":
            uc = uniqueCount_computation(ctx, odf, [c for c in list_of_cols if c in odf.columns])
            remove_cols = uc[uc["unique_values"] < 2]["attribute"].tolist()
            cols_ = [e for e in list_of_cols if e not in remove_cols and e in odf.columns]
            if treatment_threshold:
                cols_ = [e for e in threshold_cols if e not in remove_cols and e in odf.columns]
            if output_mode == "append":
                cols_ = [e + "_invalid" for e in cols_ if (e + "_invalid") in odf.columns]
            odf = imputation_MMM(ctx, odf, cols_, **treatment_configs, stats_missing={}, stats_mode={}, print_impact=print_impact)
    if print_impact:
        print(odf_print.to_string(index=False))
    return odf, odf_print


def _fmt_like_spark(v) -> str:
    """Spark stringifies numeric col values like '111.0' for doubles."""
    f = float(v)
    if f == int(f) and abs(f) < 1e15:
        return f"{int(f)}.0"
    return repr(f)
