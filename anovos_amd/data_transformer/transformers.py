"""Data transformers — parity with reference
data_transformer/transformers.py (3,772 LoC).

Signatures, defaults, output postfixes and model save/load layouts mirror
the reference; compute is columnar-tensor native:

- binning cutoffs via the fused min/max (equal_range) or histogram
  quantile sketch (equal_frequency) kernels; the bin-apply is the
  branchless bucketize kernel (ops/bucketize.py, K6),
- scalers are fused elementwise axpy kernels (K11),
- encodings are dictionary LUT gathers (K12),
- imputation fills via torch.where on the null masks,
- outlier_categories ranks dictionary counts (K5 + K21).

Model artifacts are small pandas tables written to the reference's
relative paths (e.g. ``<model_path>/attribute_binning`` parquet with
[attribute, parameters] — reference transformers.py:241-246).
"""

from __future__ import annotations

import math
import os
import warnings
from typing import Dict, Optional

import numpy as np
import pandas as pd
import torch

from anovos_amd.core import dist
from anovos_amd.core.dtypes import NULL_CODE
from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.ops import bucketize as bucketize_ops
from anovos_amd.ops import encode as encode_ops
from anovos_amd.ops import groupby as groupby_ops
from anovos_amd.ops import histogram as hist_ops
from anovos_amd.ops import stats as stats_ops
from anovos_amd.shared.utils import attributeType_segregation, normalize_columns
from anovos_amd.shared.tracing import traced


# ---------------- model persistence helpers ----------------
def _save_model(pdf: pd.DataFrame, model_path: str, name: str, fmt: str = "parquet"):
    if dist.rank() == 0:
        path = os.path.join(model_path, name)
        os.makedirs(path, exist_ok=True)
        if fmt == "parquet":
            pdf.to_parquet(os.path.join(path, "part-00000.parquet"))
        else:
            pdf.to_csv(os.path.join(path, "part-00000.csv"), index=False)
    dist.barrier()


def _load_model(model_path: str, name: str, fmt: str = "parquet") -> pd.DataFrame:
    import glob

    path = os.path.join(model_path, name)
    if fmt == "parquet":
        parts = sorted(glob.glob(os.path.join(path, "*.parquet"))) or [path]
        return pd.concat([pd.read_parquet(p) for p in parts], ignore_index=True)
    parts = sorted(glob.glob(os.path.join(path, "*.csv"))) or [path]
    return pd.concat([pd.read_csv(p) for p in parts], ignore_index=True)


def _finish_output(idf: AnovosFrame, odf: AnovosFrame, list_of_cols, postfix: str, output_mode: str) -> AnovosFrame:
    """replace: new '<col><postfix>' columns take the original names.
    Single pass over the column dict (a per-column drop/rename/select
    loop is quadratic in frame width — 60 ms at 150x350 columns)."""
    if output_mode != "replace" or not postfix:
        return odf
    replaced = {c for c in list_of_cols if (c + postfix) in odf.columns}
    out = {}
    for name in odf.columns:
        if name in replaced:
            src = odf.col(name + postfix)
            newc = src.clone()
            newc.name = name
            if ("bincounts",) in src.cache:  # same tensor, so the counts still hold
                newc.cache[("bincounts",)] = src.cache[("bincounts",)]
            out[name] = newc
        elif name.endswith(postfix) and name[: -len(postfix)] in replaced:
            continue  # consumed above
        else:
            out[name] = odf.col(name)
    return AnovosFrame(out, odf.device)


# ---------------- binning ----------------
@traced
def compute_bin_cutoffs(ctx, idf, list_of_cols, method_type, bin_size):
    """Bin cutoffs exactly as attribute_binning computes them (reference
    transformers.py:210-232): equal_frequency = j/bin_size quantiles
    (rel_err 0.01, same float chain as the GK rank ceil), equal_range =
    min + j*(max-min)/bin_size with all-null columns warned and dropped.
    Returns (kept_cols, cutoff lists). Shared with the fused
    bucketize+label-count IV/IG path (no binned materialization)."""
    if method_type == "equal_frequency":
        pctile_width = 1 / bin_size
        probs = [j * pctile_width for j in range(1, bin_size)]
        q = hist_ops.approx_quantiles(idf, list_of_cols, probs, rel_err=0.01)
        return list_of_cols, [q[c] for c in list_of_cols]
    moments = stats_ops.frame_moments(idf, list_of_cols)
    bin_cutoffs = []
    dropped = []
    for c in list_of_cols:
        m = moments[c]
        if m.max != m.max:  # all-null column
            dropped.append(c)
            continue
        w = (m.max - m.min) / bin_size
        bin_cutoffs.append([m.min + j * w for j in range(1, bin_size)])
    if dropped:
        warnings.warn("Columns contains too much null values. Dropping " + ", ".join(dropped))
        list_of_cols = [c for c in list_of_cols if c not in dropped]
    return list_of_cols, bin_cutoffs


def _device_bin_cutoffs(idf, list_of_cols, method_type, bin_size):
    """compute_bin_cutoffs for a consumer on the device: the equal-frequency
    cutoffs of `list_of_cols` as an fp64 [ncols, bin_size - 1] device tensor,
    bit for bit what compute_bin_cutoffs returns, without a sync. None when
    the method is another one or a column is not served from cached device
    histograms (ops/histogram.device_quantile_matrix); the caller then
    takes compute_bin_cutoffs."""
    if method_type != "equal_frequency":
        return None
    pctile_width = 1 / bin_size
    probs = [j * pctile_width for j in range(1, bin_size)]
    return hist_ops.device_quantile_matrix(idf, list_of_cols, probs, rel_err=0.01)


def attribute_binning(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    method_type="equal_range",
    bin_size=10,
    bin_dtype="numerical",
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    print_impact=False,
):
    """Equal-range / equal-frequency binning — reference transformers.py:87-292.
    Bin labels are 1..bin_size (numerical) or range strings (categorical)."""
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if any(x not in num_cols for x in list_of_cols):
        raise TypeError("Invalid input for Column(s)")
    if len(list_of_cols) == 0:
        warnings.warn("No Binning Performed - No numerical column(s) to transform")
        return idf
    if method_type not in ("equal_frequency", "equal_range"):
        raise TypeError("Invalid input for method_type")
    if bin_size < 2:
        raise TypeError("Invalid input for bin_size")
    if output_mode not in ("replace", "append"):
        raise TypeError("Invalid input for output_mode")

    if pre_existing_model:
        dfm = _load_model(model_path, "attribute_binning")
        cut_map = {a: list(p) for a, p in zip(dfm["attribute"], dfm["parameters"])}
        bin_cutoffs = [cut_map[c] for c in list_of_cols]
    else:
        list_of_cols, bin_cutoffs = compute_bin_cutoffs(ctx, idf, list_of_cols, method_type, bin_size)
        if model_path != "NA":
            dfm = pd.DataFrame({"attribute": list_of_cols, "parameters": bin_cutoffs})
            _save_model(dfm, model_path, "attribute_binning")

    tensors = [idf.col(c).data for c in list_of_cols]
    cuts = [torch.tensor(bc, dtype=torch.float64) for bc in bin_cutoffs]
    odf = idf
    if bin_dtype == "numerical":
        # fused bin+1/NaN; the same pass counts every bin, and each binned
        # column carries its (device, rank-local) count row so the drift
        # frequency pass need not re-read the binned frame
        vals_all, bin_counts = bucketize_ops.bucketize_columns_float_counts(tensors, cuts)
        for i, (c, vals) in enumerate(zip(list_of_cols, vals_all)):
            newc = Column(c + "_binned", "int", vals)
            newc.cache[("bincounts",)] = bin_counts[i, : len(bin_cutoffs[i]) + 2]
            odf = odf.with_column(c + "_binned", newc)
        bins = []
    else:
        bins = bucketize_ops.bucketize_columns(tensors, cuts)  # 0..len(cuts), -1 null
    for c, b, bc in zip(list_of_cols, bins, bin_cutoffs):
        labels = []
        for i in range(len(bc) + 1):
            if i == 0:
                labels.append("<= " + str(round(bc[0], 4)))
            elif i == len(bc):
                labels.append("> " + str(round(bc[-1], 4)))
            else:
                labels.append(str(round(bc[i - 1], 4)) + "-" + str(round(bc[i], 4)))
        codes = b.to(torch.int32)
        odf = odf.with_column(c + "_binned", Column(c + "_binned", "string", codes, labels))
    odf = _finish_output(idf, odf, list_of_cols, "_binned", output_mode)
    if print_impact:
        from anovos_amd.data_analyzer.stats_generator import uniqueCount_computation

        out_cols = list_of_cols if output_mode == "replace" else [c + "_binned" for c in list_of_cols]
        print(uniqueCount_computation(ctx, odf, out_cols).to_string(index=False))
    return odf


def monotonic_binning(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    label_col="label",
    event_label=1,
    bin_method="equal_range",
    bin_size=10,
    bin_dtype="numerical",
    output_mode="replace",
):
    """Supervised binning: try n=20..3 bins until spearman corr(bin, event
    rate) = ±1, else fall back to bin_size — reference transformers.py:294-425."""
    from scipy import stats as scipy_stats

    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    list_of_cols = [c for c in list_of_cols if c != label_col]
    attribute_binning_ = attribute_binning
    odf = idf
    label = _event_indicator(idf, label_col, event_label)
    for col in list_of_cols:
        chosen = None
        for n_ in range(20, 2, -1):
            tmp = attribute_binning_(ctx, idf.select([col]), [col], [], bin_method, n_, "numerical", False, "NA", "replace")
            b = tmp.col(col).data
            valid = ~torch.isnan(b)
            if not bool(valid.any()):
                continue
            bins_v = b[valid].cpu().numpy()
            ev_v = label[valid.cpu()].cpu().numpy()
            dfb = pd.DataFrame({"b": bins_v, "e": ev_v}).groupby("b")["e"].mean()
            if len(dfb) < 2:
                continue
            r, _ = scipy_stats.spearmanr(dfb.index.to_numpy(), dfb.to_numpy())
            if abs(r) == 1.0:
                chosen = n_
                break
        n_final = chosen if chosen else bin_size
        one = attribute_binning_(ctx, idf, [col], [], bin_method, n_final, bin_dtype, False, "NA", output_mode)
        newname = col if output_mode == "replace" else col + "_binned"
        odf = odf.with_column(newname, one.col(newname))
    return odf


def _event_indicator(idf, label_col: str, event_label) -> torch.Tensor:
    c = idf.col(label_col)
    if c.kind == "categorical":
        try:
            code = (c.dictionary or []).index(str(event_label))
        except ValueError:
            code = -2
        return (c.data == code).to(torch.float32)
    return (c.data == float(event_label)).to(torch.float32)


# ---------------- encoding ----------------
def cat_to_num_transformer(ctx, idf, list_of_cols, drop_cols, method_type, encoding, label_col, event_label):
    """Dispatch supervised/unsupervised encoding for corr-matrix prep —
    reference transformers.py:428-504."""
    if method_type == "supervised":
        return cat_to_num_supervised(ctx, idf, list_of_cols, drop_cols, label_col, event_label)
    return cat_to_num_unsupervised(ctx, idf, list_of_cols, drop_cols, method_type=encoding)


@traced
def cat_to_num_unsupervised(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    method_type="label_encoding",
    index_order="frequencyDesc",
    cardinality_threshold=50,
    pre_existing_model=False,
    model_path="NA",
    stats_unique={},
    output_mode="replace",
    print_impact=False,
):
    """Label encoding (StringIndexer order) or one-hot — reference
    transformers.py:506-773. Columns with cardinality > threshold are
    skipped with a warning."""
    cat_cols = attributeType_segregation(idf)[1]
    if list_of_cols == "all":
        list_of_cols = cat_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=cat_cols)
    if len(list_of_cols) == 0:
        warnings.warn("No Encoding Computation - No categorical column(s) to transform")
        return idf
    # reference accepts 1 = label encoding, 0 = one-hot (transformers.py:506)
    if method_type == 1:
        method_type = "label_encoding"
    elif method_type == 0:
        method_type = "onehot_encoding"
    if method_type not in ("label_encoding", "onehot_encoding"):
        raise TypeError("Invalid input for method_type")

    if pre_existing_model:
        dfm = _load_model(model_path, "cat_to_num_unsupervised", fmt="csv")
        maps = {}
        for c in list_of_cols:
            sub = dfm[dfm["attribute"] == c]
            maps[c] = dict(zip(sub["category"].astype(str), sub["index"].astype(int)))
    else:
        counts = groupby_ops.cat_value_counts(idf, list_of_cols)
        skipped = []
        maps = {}
        for c in list_of_cols:
            card = int((counts[c] > 0).sum())
            if card > cardinality_threshold:
                skipped.append(c)
                continue
            maps[c] = encode_ops.index_map_from_counts(idf.col(c).dictionary or [], counts[c], index_order)
        if skipped:
            warnings.warn(
                f"Columns dropped from encoding due to cardinality > {cardinality_threshold}: " + ", ".join(skipped)
            )
        list_of_cols = [c for c in list_of_cols if c in maps]
        if model_path != "NA":
            rows = []
            for c, m in maps.items():
                for k, v in m.items():
                    rows.append([c, k, v])
            _save_model(pd.DataFrame(rows, columns=["attribute", "category", "index"]), model_path, "cat_to_num_unsupervised", fmt="csv")

    odf = idf
    if method_type == "label_encoding":
        vals_all = encode_ops.apply_index_maps_batch(
            [idf.col(c) for c in list_of_cols], [maps[c] for c in list_of_cols]
        )
        for c, vals in zip(list_of_cols, vals_all):
            odf = odf.with_column(c + "_index", Column(c + "_index", "int", vals))
        odf = _finish_output(idf, odf, list_of_cols, "_index", output_mode)
    else:
        for c in list_of_cols:
            vals = encode_ops.apply_index_map(idf.col(c), maps[c])
            ncat = len(maps[c])
            for j in range(ncat):
                onehot = (vals == j).to(torch.float32)
                onehot = torch.where(torch.isnan(vals), torch.full_like(onehot, float("nan")), onehot)
                odf = odf.with_column(f"{c}_{j}", Column(f"{c}_{j}", "int", onehot))
        if output_mode == "replace":
            odf = odf.drop(list_of_cols)
    if print_impact:
        print(odf.columns)
    return odf


@traced
def cat_to_num_supervised(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    label_col="label",
    event_label=1,
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    persist=True,
    persist_option=None,
    print_impact=False,
):
    """Target-rate encoding — reference transformers.py:776-963: each
    category becomes round(P(label==event | category), 4)."""
    cat_cols = attributeType_segregation(idf)[1]
    if list_of_cols == "all":
        list_of_cols = [c for c in cat_cols if c != label_col]
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=cat_cols)
    list_of_cols = [c for c in list_of_cols if c != label_col]
    if len(list_of_cols) == 0:
        warnings.warn("No Encoding Computation - No categorical column(s) to transform")
        return idf

    odf = idf
    if pre_existing_model:
        rate_maps = {}
        for c in list_of_cols:
            dfm = _load_model(model_path, f"cat_to_num_supervised/{c}", fmt="csv")
            rate_maps[c] = dict(zip(dfm[c].astype(str), dfm[c + "_encoded"].astype(float)))
    else:
        label = _event_indicator(idf, label_col, event_label)
        rate_maps = {}
        for c in list_of_cols:
            col = idf.col(c)
            size = len(col.dictionary or [])
            codes = col.data.to(torch.long)
            valid = codes != NULL_CODE
            ev = torch.zeros(size, dtype=torch.float64, device=codes.device)
            tot = torch.zeros(size, dtype=torch.float64, device=codes.device)
            ev.scatter_add_(0, codes[valid], label[valid].to(torch.float64))
            tot.scatter_add_(0, codes[valid], torch.ones_like(label[valid], dtype=torch.float64))
            dist.all_reduce_(ev, "sum")
            dist.all_reduce_(tot, "sum")
            rate = torch.where(tot > 0, ev / tot, torch.zeros_like(tot))
            rate_maps[c] = {s: round(float(rate[i]), 4) for i, s in enumerate(col.dictionary or [])}
            if model_path != "NA":
                dfm = pd.DataFrame({c: list(rate_maps[c].keys()), c + "_encoded": list(rate_maps[c].values())})
                _save_model(dfm, model_path, f"cat_to_num_supervised/{c}", fmt="csv")
    for c in list_of_cols:
        col = idf.col(c)
        lut = torch.tensor(
            [rate_maps[c].get(s, float("nan")) for s in (col.dictionary or [])] + [float("nan")],
            dtype=torch.float32,
            device=col.data.device,
        )
        codes = col.data.to(torch.long)
        codes = torch.where(codes == NULL_CODE, torch.full_like(codes, lut.numel() - 1), codes)
        odf = odf.with_column(c + "_encoded", Column(c + "_encoded", "double", lut[codes]))
    odf = _finish_output(idf, odf, list_of_cols, "_encoded", output_mode)
    if print_impact:
        print(odf.columns)
    return odf


# ---------------- scaling ----------------
@traced
def z_standardization(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    print_impact=False,
):
    """(x-mean)/stddev — reference transformers.py:965-1100. Columns with
    stddev ~ 0 are excluded with a warning."""
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if len(list_of_cols) == 0:
        warnings.warn("No Standardization Performed - No numerical column(s) to transform")
        return idf

    if pre_existing_model:
        dfm = _load_model(model_path, "z_standardization")
        params = dict(zip(dfm["feature"], zip(dfm["mean"], dfm["stddev"])))
    else:
        moments = stats_ops.frame_moments(idf, list_of_cols)
        params = {c: (moments[c].mean, moments[c].stddev) for c in list_of_cols}
        if model_path != "NA":
            dfm = pd.DataFrame(
                {"feature": list_of_cols, "mean": [params[c][0] for c in list_of_cols], "stddev": [params[c][1] for c in list_of_cols]}
            )
            _save_model(dfm, model_path, "z_standardization")
    excluded = [c for c in list_of_cols if c not in params or not (params[c][1] == params[c][1]) or round(params[c][1], 5) == 0.0]
    if excluded:
        warnings.warn(
            "The following column(s) are excluded from standardization because the standard deviation is zero:" + str(excluded)
        )
    odf = idf
    applied = [c for c in list_of_cols if c not in excluded]
    if applied:
        from anovos_amd.ops import elementwise

        scaled = elementwise.scale_columns(
            [idf.col(c).data for c in applied],
            [params[c][0] for c in applied],
            [1.0 / params[c][1] for c in applied],
        )
        for c, data in zip(applied, scaled):
            odf = odf.with_column(c + "_scaled", Column(c + "_scaled", "double", data))
    odf = _finish_output(idf, odf, applied, "_scaled", output_mode)
    if print_impact:
        print(odf.columns)
    return odf


@traced
def IQR_standardization(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    print_impact=False,
):
    """(x - median)/(p75 - p25) — reference transformers.py:1102-1231."""
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if len(list_of_cols) == 0:
        warnings.warn("No Standardization Performed - No numerical column(s) to transform")
        return idf
    if pre_existing_model:
        dfm = _load_model(model_path, "IQR_standardization")
        params = dict(zip(dfm["feature"], zip(dfm["p25"], dfm["p50"], dfm["p75"])))
    else:
        q = hist_ops.approx_quantiles(idf, list_of_cols, [0.25, 0.5, 0.75])
        params = {c: (q[c][0], q[c][1], q[c][2]) for c in list_of_cols}
        if model_path != "NA":
            dfm = pd.DataFrame(
                {
                    "feature": list_of_cols,
                    "p25": [params[c][0] for c in list_of_cols],
                    "p50": [params[c][1] for c in list_of_cols],
                    "p75": [params[c][2] for c in list_of_cols],
                }
            )
            _save_model(dfm, model_path, "IQR_standardization")
    # a column without values has NaN quartiles: excluded like a constant one
    iqr = {c: params[c][2] - params[c][0] for c in list_of_cols}
    excluded = [c for c in list_of_cols if not (iqr[c] == iqr[c]) or round(iqr[c], 5) == 0.0]
    if excluded:
        warnings.warn("The following column(s) are excluded from standardization because IQR is zero:" + str(excluded))
    odf = idf
    applied = [c for c in list_of_cols if c not in excluded]
    if applied:
        from anovos_amd.ops import elementwise

        scaled = elementwise.scale_columns(
            [idf.col(c).data for c in applied],
            [params[c][1] for c in applied],
            [1.0 / (params[c][2] - params[c][0]) for c in applied],
        )
        for c, data in zip(applied, scaled):
            odf = odf.with_column(c + "_scaled", Column(c + "_scaled", "double", data))
    odf = _finish_output(idf, odf, applied, "_scaled", output_mode)
    if print_impact:
        print(odf.columns)
    return odf


@traced
def normalization(
    idf,
    list_of_cols="all",
    drop_cols=[],
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    print_impact=False,
):
    """Min-max scaling to [0,1] — reference transformers.py:1233-1367
    (MLlib MinMaxScaler semantics)."""
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if len(list_of_cols) == 0:
        warnings.warn("No Normalization Performed - No numerical column(s) to transform")
        return idf
    if pre_existing_model:
        dfm = _load_model(model_path, "normalization")
        params = dict(zip(dfm["feature"], zip(dfm["min"], dfm["max"])))
    else:
        moments = stats_ops.frame_moments(idf, list_of_cols)
        params = {c: (moments[c].min, moments[c].max) for c in list_of_cols}
        if model_path != "NA":
            dfm = pd.DataFrame(
                {"feature": list_of_cols, "min": [params[c][0] for c in list_of_cols], "max": [params[c][1] for c in list_of_cols]}
            )
            _save_model(dfm, model_path, "normalization")
    excluded = [c for c in list_of_cols if not (params[c][0] == params[c][0]) or params[c][1] == params[c][0]]
    if excluded:
        warnings.warn("The following column(s) are excluded from normalization (constant or empty):" + str(excluded))
    odf = idf
    applied = [c for c in list_of_cols if c not in excluded]
    if applied:
        from anovos_amd.ops import elementwise

        scaled = elementwise.scale_columns(
            [idf.col(c).data for c in applied],
            [params[c][0] for c in applied],
            [1.0 / (params[c][1] - params[c][0]) for c in applied],
        )
        for c, data in zip(applied, scaled):
            odf = odf.with_column(c + "_scaled", Column(c + "_scaled", "double", data))
    odf = _finish_output(idf, odf, applied, "_scaled", output_mode)
    if print_impact:
        print(odf.columns)
    return odf


# ---------------- imputation ----------------
@traced
def imputation_MMM(
    ctx,
    idf,
    list_of_cols="missing",
    drop_cols=[],
    method_type="median",
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    stats_missing={},
    stats_mode={},
    print_impact=False,
):
    """Mean/Median/Mode imputation — reference transformers.py:1369-1674.
    Numeric columns filled with mean or median; categorical (and numeric
    when method_type='mode') with mode. 'missing' sentinel = all columns
    with any null."""
    if method_type not in ("mean", "median", "mode"):
        raise TypeError("Invalid input for method_type")
    if output_mode not in ("replace", "append"):
        raise TypeError("Invalid input for output_mode")
    num_all, cat_all, _ = attributeType_segregation(idf)
    candidates = num_all + cat_all
    if stats_missing:
        from anovos_amd.data_ingest.data_ingest import read_dataset as _rd

        miss_df = _rd(ctx, **stats_missing, sharded=False).to_pandas()
        missing = dict(zip(miss_df["attribute"], miss_df["missing_count"]))
    else:
        missing, _ = stats_ops.null_counts(idf, candidates)
    if list_of_cols == "missing":
        list_of_cols = [c for c in candidates if missing.get(c, 0) > 0]
    elif list_of_cols == "all":
        list_of_cols = candidates
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|") if x.strip()]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    list_of_cols = [c for c in list_of_cols if c not in set(drop_cols)]
    if any(x not in candidates for x in list_of_cols):
        raise TypeError("Invalid input for Column(s)")
    if len(list_of_cols) == 0:
        return idf

    num_cols = [c for c in list_of_cols if c in num_all]
    cat_cols = [c for c in list_of_cols if c in cat_all]

    fill_num: Dict[str, float] = {}
    fill_cat: Dict[str, Optional[str]] = {}
    if pre_existing_model:
        if num_cols:
            dfm = _load_model(model_path, "imputation_MMM/num_imputer-model")
            fill_num = dict(zip(dfm["attribute"], dfm["value"]))
        if cat_cols:
            dfc = _load_model(model_path, "imputation_MMM/cat_imputer", fmt="csv")
            fill_cat = dict(zip(dfc["attribute"], dfc["mode"]))
    else:
        if method_type == "mode":
            mode_cols = num_cols + cat_cols
        else:
            mode_cols = cat_cols
        if mode_cols:
            if stats_mode:
                from anovos_amd.data_ingest.data_ingest import read_dataset as _rd

                mdf = _rd(ctx, **stats_mode, sharded=False).to_pandas()
                pre = dict(zip(mdf["attribute"], mdf["mode"]))
            else:
                pre = {}
            # batch: one fused code-count launch for all categorical mode
            # columns and one dense-histogram launch for numeric ones —
            # the per-column mode() loop cost a host sync per column
            need = [c for c in mode_cols if c not in pre or pre[c] is None]
            cat_need = [c for c in need if c in cat_all]
            num_need = [c for c in need if c not in cat_all]
            if cat_need:
                groupby_ops.cat_value_counts(idf, cat_need)  # warms per-col cache
            num_modes = groupby_ops.discrete_modes(idf, num_need) if num_need else {}
            for c in mode_cols:
                if c in pre and pre[c] is not None:
                    mv = pre[c]
                elif c in num_modes:
                    mv = num_modes[c][0]
                else:
                    mv, _cnt = groupby_ops.mode(idf, c)
                if c in cat_all:
                    fill_cat[c] = None if mv is None else str(mv)
                else:
                    fill_num[c] = float("nan") if mv is None else float(mv)
        if method_type in ("mean", "median") and num_cols:
            if method_type == "mean":
                moments = stats_ops.frame_moments(idf, num_cols)
                for c in num_cols:
                    fill_num[c] = moments[c].mean
            else:
                q = hist_ops.approx_quantiles(idf, num_cols, [0.5])
                for c in num_cols:
                    fill_num[c] = q[c][0]
        if model_path != "NA":
            if num_cols:
                _save_model(
                    pd.DataFrame({"attribute": num_cols, "value": [fill_num[c] for c in num_cols]}),
                    model_path,
                    "imputation_MMM/num_imputer-model",
                )
            if cat_cols:
                _save_model(
                    pd.DataFrame({"attribute": cat_cols, "mode": [fill_cat.get(c) for c in cat_cols]}),
                    model_path,
                    "imputation_MMM/cat_imputer",
                    fmt="csv",
                )

    odf = idf
    fillable = [c for c in num_cols if fill_num.get(c) is not None and fill_num[c] == fill_num[c]]
    if fillable:
        from anovos_amd.ops import elementwise

        filled = elementwise.fill_nan_columns(
            [idf.col(c).data for c in fillable], [float(fill_num[c]) for c in fillable]
        )
        for c, data in zip(fillable, filled):
            odf = odf.with_column(c + "_imputed", Column(c + "_imputed", idf.col(c).dtype, data))
    for c in num_cols:
        if c in fillable:
            continue
        col = idf.col(c)
        odf = odf.with_column(c + "_imputed", Column(c + "_imputed", col.dtype, col.data.clone()))
    # categorical mode fill: one fused launch for every column (K11)
    cat_fill_cols, cat_fill_codes, cat_dicts = [], [], {}
    for c in cat_cols:
        v = fill_cat.get(c)
        col = idf.col(c)
        if v is None:
            odf = odf.with_column(
                c + "_imputed", Column(c + "_imputed", "string", col.data.clone(), list(col.dictionary or []))
            )
            continue
        d = list(col.dictionary or [])
        if v in d:
            code = d.index(v)
        else:
            d.append(v)
            code = len(d) - 1
        cat_fill_cols.append(c)
        cat_fill_codes.append(code)
        cat_dicts[c] = d
    if cat_fill_cols:
        from anovos_amd.ops import elementwise

        filled_codes = elementwise.fill_code_columns(
            [idf.col(c).data for c in cat_fill_cols], cat_fill_codes
        )
        for c, data in zip(cat_fill_cols, filled_codes):
            odf = odf.with_column(c + "_imputed", Column(c + "_imputed", "string", data, cat_dicts[c]))
    odf = _finish_output(idf, odf, num_cols + cat_cols, "_imputed", output_mode)
    if print_impact:
        from anovos_amd.data_analyzer.stats_generator import missingCount_computation

        print("Before:")
        print(missingCount_computation(ctx, idf, list_of_cols).to_string(index=False))
        print("After:")
        out_cols = list_of_cols if output_mode == "replace" else [c + "_imputed" for c in list_of_cols]
        print(missingCount_computation(ctx, odf, out_cols).to_string(index=False))
    return odf


# ---------------- elementwise transforms ----------------
def _torch_fns(N):
    return {
        "ln": torch.log,
        "log10": torch.log10,
        "log2": torch.log2,
        "exp": torch.exp,
        "powOf2": lambda x: torch.pow(torch.tensor(2.0, device=x.device), x),
        "powOf10": lambda x: torch.pow(torch.tensor(10.0, device=x.device), x),
        "powOfN": lambda x: torch.pow(torch.tensor(float(N), device=x.device), x),
        "sqrt": torch.sqrt,
        "cbrt": lambda x: torch.sign(x) * torch.pow(torch.abs(x), 1.0 / 3.0),
        "sq": lambda x: x * x,
        "cb": lambda x: x * x * x,
        "toPowerN": lambda x: torch.pow(x, float(N)),
        "sin": torch.sin,
        "cos": torch.cos,
        "tan": torch.tan,
        "asin": torch.asin,
        "acos": torch.acos,
        "atan": torch.atan,
        "radians": torch.deg2rad,
        "remainderDivByN": lambda x: torch.remainder(x, float(N)),
        "factorial": lambda x: torch.exp(torch.lgamma(x + 1.0)).round(),
        "mul_inv": lambda x: 1.0 / x,
        "floor": torch.floor,
        "ceil": torch.ceil,
        "roundN": lambda x: torch.round(x * (10.0**N)) / (10.0**N),
    }


@traced
def feature_transformation(
    idf,
    list_of_cols="all",
    drop_cols=[],
    method_type="sqrt",
    N=None,
    output_mode="replace",
    print_impact=False,
):
    """26 elementwise math transforms — reference transformers.py:3171-3325."""
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    fns = _torch_fns(N)
    if method_type not in fns:
        raise TypeError("Invalid input for method_type")
    odf = idf
    for c in list_of_cols:
        if output_mode == "replace":
            name = c
        elif method_type in ("powOfN", "toPowerN", "remainderDivByN", "roundN"):
            name = c + "_" + method_type[:-1] + str(N)
        else:
            name = c + "_" + method_type
        data = fns[method_type](idf.col(c).data.to(torch.float32))
        odf = odf.with_column(name, Column(name, "double", data))
    if print_impact:
        print(odf.columns)
    return odf


@traced
def boxcox_transformation(
    idf,
    list_of_cols="all",
    drop_cols=[],
    boxcox_lambda=None,
    output_mode="replace",
    print_impact=False,
):
    """Box-Cox with λ selected from the reference's grid by best KS fit to
    a normal — reference transformers.py:3327-3487."""
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    grid = [1, -1, 0.5, -0.5, 2, -2, 0.25, -0.25, 3, -3, 4, -4, 5, -5, 0]
    if boxcox_lambda is not None:
        if isinstance(boxcox_lambda, (list, tuple)):
            lambdas = {c: l for c, l in zip(list_of_cols, boxcox_lambda)}
        else:
            lambdas = {c: boxcox_lambda for c in list_of_cols}
    else:
        lambdas = {}
        for c in list_of_cols:
            t = idf.col(c).data
            x = t[~torch.isnan(t)]
            if x.numel() > 100000:
                idx = torch.randperm(x.numel(), device=x.device)[:100000]
                x = x[idx]
            best, best_ks = 1, float("inf")
            for lam in grid:
                y = _boxcox_apply(x, lam)
                y = y[torch.isfinite(y)]
                if y.numel() < 10:
                    continue
                ks = _ks_vs_normal(y)
                if ks < best_ks:
                    best_ks, best = ks, lam
            lambdas[c] = best
    odf = idf
    applied = []
    for c in list_of_cols:
        lam = lambdas[c]
        if lam == 1:
            continue
        applied.append(c)
        data = _boxcox_apply(idf.col(c).data.to(torch.float32), lam)
        odf = odf.with_column(c + "_bxcx_" + str(lam), Column(c + "_bxcx_" + str(lam), "double", data))
    if output_mode == "replace":
        for c in applied:
            lam = lambdas[c]
            odf = odf.drop([c]).rename({c + "_bxcx_" + str(lam): c})
    if print_impact:
        print(lambdas)
    return odf


def _boxcox_apply(x: torch.Tensor, lam) -> torch.Tensor:
    if lam == 0:
        return torch.log(x)
    return torch.pow(x, float(lam))


def _ks_vs_normal(y: torch.Tensor) -> float:
    y = y.to(torch.float64)
    mu = y.mean()
    sd = y.std()
    if not torch.isfinite(sd) or float(sd) == 0:
        return float("inf")
    z, _ = torch.sort((y - mu) / sd)
    n = z.numel()
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    emp_hi = torch.arange(1, n + 1, dtype=torch.float64, device=y.device) / n
    emp_lo = torch.arange(0, n, dtype=torch.float64, device=y.device) / n
    return float(torch.maximum((cdf - emp_lo).abs(), (emp_hi - cdf).abs()).max())


# ---------------- categorical outliers ----------------
@traced
def outlier_categories(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    coverage=1.0,
    max_category=50,
    pre_existing_model=False,
    model_path="NA",
    output_mode="replace",
    print_impact=False,
):
    """Keep top categories within coverage (max max_category-1), replace
    the rest with 'others' — reference transformers.py:3489-3672."""
    cat_cols = attributeType_segregation(idf)[1]
    if list_of_cols == "all":
        list_of_cols = cat_cols
    list_of_cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=cat_cols)
    if len(list_of_cols) == 0:
        warnings.warn("No Outlier Categories Computation - No categorical column(s) to transform")
        return idf
    if (coverage <= 0) | (coverage > 1):
        raise TypeError("Invalid input for coverage")
    if max_category < 2:
        raise TypeError("Invalid input for max_category")

    if pre_existing_model:
        dfm = _load_model(model_path, "outlier_categories", fmt="csv")
        keep = {c: set(dfm[dfm["attribute"] == c]["parameters"].astype(str)) for c in list_of_cols}
    else:
        counts = groupby_ops.cat_value_counts(idf, list_of_cols)
        keep = {}
        for c in list_of_cols:
            cnt = counts[c]
            d = idf.col(c).dictionary or []
            order = torch.argsort(cnt, descending=True, stable=True)
            total = float(cnt.sum())
            kept = []
            acc = 0.0
            for i in order.tolist():
                if len(kept) >= max_category - 1:
                    break
                if total > 0 and acc >= coverage * total:
                    break
                if cnt[i] == 0:
                    break
                kept.append(d[i])
                acc += float(cnt[i])
            keep[c] = set(kept)
        if model_path != "NA":
            rows = [[c, v] for c in list_of_cols for v in sorted(keep[c])]
            _save_model(pd.DataFrame(rows, columns=["attribute", "parameters"]), model_path, "outlier_categories", fmt="csv")

    odf = idf
    luts, dicts = [], []
    for c in list_of_cols:
        col = idf.col(c)
        d = list(col.dictionary or [])
        if "others" in d:
            others_code = d.index("others")
            newd = d
        else:
            newd = d + ["others"]
            others_code = len(d)
        luts.append(torch.tensor([i if s in keep[c] else others_code for i, s in enumerate(d)] or [0], dtype=torch.int32))
        dicts.append(newd)
    remapped = encode_ops.remap_codes_batch([idf.col(c) for c in list_of_cols], luts)
    for c, codes, newd in zip(list_of_cols, remapped, dicts):
        odf = odf.with_column(c + "_outliered", Column(c + "_outliered", "string", codes, newd))
    odf = _finish_output(idf, odf, list_of_cols, "_outliered", output_mode)
    if print_impact:
        print(odf.columns)
    return odf


# ---------------- SQL-ish expressions ----------------
def expression_parser(idf, list_of_expr, postfix="", print_impact=False):
    """Evaluate arithmetic expressions as new features f<i><postfix> —
    reference transformers.py:3674-3772 (F.expr). Supports +,-,*,/,
    comparison, and/or/not, parentheses, and the math functions of
    feature_transformation over column names."""
    if isinstance(list_of_expr, str):
        list_of_expr = [x.strip() for x in list_of_expr.split("|")]
    odf = idf
    for i, expr in enumerate(list_of_expr):
        data = _eval_expr(idf, expr)
        name = f"f{i}{postfix}"
        odf = odf.with_column(name, Column(name, "double", data))
    if print_impact:
        print(odf.columns)
    return odf


_EXPR_FNS = {
    "log": torch.log,
    "ln": torch.log,
    "log10": torch.log10,
    "log2": torch.log2,
    "exp": torch.exp,
    "sqrt": torch.sqrt,
    "abs": torch.abs,
    "sin": torch.sin,
    "cos": torch.cos,
    "tan": torch.tan,
    "floor": torch.floor,
    "ceil": torch.ceil,
    "pow": torch.pow,
    "power": torch.pow,
    "round": torch.round,
    "greatest": torch.maximum,
    "least": torch.minimum,
}


def _eval_expr(idf: AnovosFrame, expr: str) -> torch.Tensor:
    """Evaluate a SQL-flavored expression over frame columns via a
    restricted python eval (AND/OR/NOT normalized; no builtins)."""
    import re

    s = expr
    s = re.sub(r"\bAND\b", " & ", s, flags=re.I)
    s = re.sub(r"\bOR\b", " | ", s, flags=re.I)
    s = re.sub(r"\bNOT\b", " ~ ", s, flags=re.I)
    s = re.sub(r"(?<![<>!=])=(?!=)", "==", s)
    ns = {}
    for name in idf.columns:
        col = idf.col(name)
        if col.kind == "numerical":
            ns[name] = col.data.to(torch.float32)
    ns.update(_EXPR_FNS)
    out = eval(s, {"__builtins__": {}}, ns)  # noqa: S307 - config-authored expressions
    if not torch.is_tensor(out):
        out = torch.full((idf.local_rows(),), float(out), dtype=torch.float32, device=idf.device)
    return out.to(torch.float32)


# Advanced imputers / latent features live in transformers_advanced but are
# part of this module's API surface in the reference (transformers.py:1677-3168).
from anovos_amd.data_transformer.transformers_advanced import (  # noqa: E402,F401
    PCA_latentFeatures,
    auto_imputation,
    autoencoder_latentFeatures,
    imputation_matrixFactorization,
    imputation_sklearn,
)
