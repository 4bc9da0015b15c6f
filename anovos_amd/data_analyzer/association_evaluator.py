"""Attribute associations — parity with reference
data_analyzer/association_evaluator.py (586 LoC).

- correlation_matrix (:38): bf16 MFMA Gram kernel / rocBLAS path (K8);
  method="spearman" (beyond the reference) ranks on a grid first (K24),
  null_policy="pairwise" (beyond the reference) takes every entry over
  the rows where both columns are present (masked Gram kernel, K25),
- variable_clustering (:142): one fused covariance pass + driver-side
  VarClusHi (association_eval_varclus.py),
- IV_calculation (:253): per-bin label histograms (K9) + WOE/IV sums,
- IG_calculation (:427): entropy before/after split.

Beyond the reference: categorical_association_matrix (pair-count kernel,
K22) and numerical_categorical_association (grouped-moments kernel, K23).
"""

from __future__ import annotations

import math
import warnings

import numpy as np
import pandas as pd
import torch

from anovos_amd.core import dist
from anovos_amd.core.dtypes import NULL_CODE
from anovos_amd.data_analyzer.association_eval_varclus import VarClusHi
from anovos_amd.data_analyzer.stats_generator import uniqueCount_computation
from anovos_amd.data_transformer.transformers import (
    attribute_binning,
    cat_to_num_unsupervised,
    imputation_MMM,
    monotonic_binning,
    _event_indicator,
)
from anovos_amd.ops import corr as corr_ops
from anovos_amd.ops import rank as rank_ops
from anovos_amd.shared.utils import attributeType_segregation, normalize_columns
from anovos_amd.shared.tracing import traced


@traced
def correlation_matrix(ctx, idf, list_of_cols="all", drop_cols=[], use_sampling=False, sample_size=1000000, print_impact=False, use_bf16=True, method="pearson", rank_cells=1024, null_policy="mean", min_periods=2):
    """[attribute, <cols...>] — reference association_evaluator.py:38-139.

    use_bf16=True (default) runs the hand-written bf16 MFMA Gram kernel:
    inputs are centered in f32 then quantized to bf16 (8-bit mantissa),
    giving up to ~1e-2 relative error on correlation entries vs the
    reference's exact fp64 MLlib corr. Pass use_bf16=False for the f32
    rocBLAS path (centered in f64, ~1e-6). Accumulation is fp32 either
    way; cross-rank merge is fp64.

    method="spearman" (the reference has no `method`) returns Spearman's
    rank correlation instead: Pearson's r of the columns' mid-ranks on a
    grid of `rank_cells` cells per column (2 .. 4096, see ops/rank.py),
    through the same Gram paths. Ranks are taken among a column's non-null
    rows and a null takes the mean rank, so it contributes zero — the
    Pearson path's convention. Rows that share a cell are tied; a column
    with at most `rank_cells` distinct values or rows is ranked exactly.

    null_policy="mean" (default) is the behaviour above: a null counts as
    the column mean and contributes zero to every sum — right on the
    imputed frame the workflow hands over. null_policy="pairwise" (the
    reference has neither keyword) is for a raw frame: every entry is
    Pearson's r over the rows where BOTH columns are present, as pandas
    `DataFrame.corr` and R `use="pairwise.complete.obs"` compute it, from
    one pass of the masked MFMA Gram kernel (K25; `use_bf16=False` takes
    f32 rocBLAS matmuls, the CPU backend fp64). An entry, diagonal
    included, is NaN where fewer than max(min_periods, 2) rows have both
    values or where either column is constant on those rows (see
    ops/corr.py for the thresholds); `pairwise_observation_counts` returns
    the row count behind each entry. Pearson only: Spearman ranks would
    have to be retaken per pair."""
    if method not in ("pearson", "spearman"):
        raise TypeError("Invalid input for method: 'pearson' or 'spearman'")
    if null_policy not in ("mean", "pairwise"):
        raise TypeError("Invalid input for null_policy: 'mean' or 'pairwise'")
    if isinstance(min_periods, bool) or not isinstance(min_periods, (int, np.integer)) or min_periods < 1:
        raise TypeError("Invalid input for min_periods: an integer >= 1")
    if null_policy == "pairwise" and method == "spearman":
        raise TypeError(
            "Invalid input for null_policy: 'pairwise' is not available with method='spearman' "
            "(ranks would have to be retaken per pair of columns)"
        )
    if (
        isinstance(rank_cells, bool) or not isinstance(rank_cells, (int, np.integer))
        or not 2 <= rank_cells <= rank_ops.GRADE_MAX_CELLS
    ):
        raise TypeError(f"Invalid input for rank_cells: an integer in [2, {rank_ops.GRADE_MAX_CELLS}]")
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if any(x not in num_cols for x in cols) or len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    if use_sampling and idf.count() > sample_size:
        warnings.warn("Using sampling. Only " + str(sample_size) + " random sampled rows are considered.")
        from anovos_amd.data_ingest.data_sampling import data_sample

        idf = data_sample(idf, fraction=float(sample_size) / idf.count(), method_type="random")
    if method == "spearman":
        corr = rank_ops.spearman_matrix(idf, cols, cells=int(rank_cells), use_bf16=use_bf16)
    elif null_policy == "pairwise":
        corr = corr_ops.pairwise_pearson_matrix(idf, cols, use_bf16=use_bf16, min_periods=int(min_periods))
    else:
        corr = corr_ops.pearson_matrix(idf, cols, use_bf16=use_bf16)
    odf = pd.DataFrame(corr, columns=cols, index=cols)
    odf["attribute"] = odf.index
    sorted_cols = sorted(cols)
    odf = odf[["attribute"] + sorted_cols].sort_values("attribute").reset_index(drop=True)
    if print_impact:
        print(odf.to_string(index=False))
    return odf


@traced
def pairwise_observation_counts(ctx, idf, list_of_cols="all", drop_cols=[]):
    """[attribute, <cols...>] of int64 counts: the rows where both columns
    are present — the denominator behind each entry of
    correlation_matrix(null_policy="pairwise"); the diagonal is a column's
    non-null count. Same shape and ordering as correlation_matrix."""
    num_cols = attributeType_segregation(idf)[0]
    if list_of_cols == "all":
        list_of_cols = num_cols
    cols = normalize_columns(idf, list_of_cols, drop_cols, restrict_to=num_cols)
    if any(x not in num_cols for x in cols) or len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    counts = np.rint(corr_ops.pairwise_sums(idf, cols)[0]).astype(np.int64)
    odf = pd.DataFrame(counts, columns=cols, index=cols)
    odf["attribute"] = odf.index
    odf = odf[["attribute"] + sorted(cols)].sort_values("attribute").reset_index(drop=True)
    return odf


@traced
def variable_clustering(ctx, idf, list_of_cols="all", drop_cols=[], stats_mode={}, persist=True, print_impact=False):
    """[Cluster, Attribute, RS_Ratio] — reference association_evaluator.py:142-250."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    cols = normalize_columns(idf, list_of_cols, drop_cols)
    if len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    uc = uniqueCount_computation(ctx, idf, cols)
    remove_cols = uc[uc["unique_values"] < 2]["attribute"].tolist()
    cols = [e for e in cols if e not in remove_cols]
    sub = idf.select(cols)
    cat_cols = attributeType_segregation(sub)[1]
    idf_encoded = cat_to_num_unsupervised(ctx, sub, list_of_cols=cat_cols, method_type="label_encoding")
    num_cols = attributeType_segregation(idf_encoded)[0]
    idf_encoded = idf_encoded.select(num_cols)
    idf_imputed = imputation_MMM(ctx, idf_encoded, stats_mode=stats_mode)
    # single fused pass: correlation matrix of standardized features
    corr = corr_ops.pearson_matrix(idf_imputed, num_cols)
    corr_df = pd.DataFrame(corr, columns=num_cols, index=num_cols)
    vc = VarClusHi(corr_df, maxeigval2=1, maxclus=None)
    vc.varclus()
    rs = vc.rsquare()
    odf = rs[["Cluster", "Variable", "RS_Ratio"]].rename(columns={"Variable": "Attribute"})
    odf["RS_Ratio"] = odf["RS_Ratio"].round(4)
    if print_impact:
        print(odf.to_string(index=False))
    return odf.reset_index(drop=True)


def _binned_label_counts(idf, col: str, label: torch.Tensor):
    """Per-group (label_0, label_1) counts for one column — thin wrapper
    over the batched path (kept for tests/back-compat)."""
    out = _binned_label_counts_multi(idf, [col], label)
    return out[col]



def _cached_event_indicator(idf, label_col, event_label):
    """(label tensor, global event count) memoized on the frame: IV and
    IG share one label reduction + host sync per step."""
    key = ("event_indicator", label_col, str(event_label))
    hit = idf.aux_cache.get(key)
    if hit is not None:
        return hit
    label = _event_indicator(idf, label_col, event_label)
    total = int(dist.all_reduce_scalar(int(label.sum())))
    idf.aux_cache[key] = (label, total)
    return label, total


def _encoded_label_counts(ctx, idf, cols, label_col, event_label, label, encoding_configs):
    """Shared IV/IG front end: bin numerics per encoding_configs, then one
    fused multi-column label-count pass. The result is memoized in the
    frame's aux_cache so IG reuses IV's binning AND counting when called
    with the same inputs (the reference recomputes both; the engine's
    stats-reuse contract makes the pair one pass)."""
    num_cols = attributeType_segregation(idf.select(cols))[0]
    key = (
        "ivig_counts",
        label_col,
        str(event_label),
        repr(sorted(encoding_configs.items())) if encoding_configs else "",
        tuple(cols),
    )
    hit = idf.aux_cache.get(key)
    if hit is not None:
        return hit
    from anovos_amd.ops import backend as _backend
    from anovos_amd.ops.groupby import align_dictionaries

    # dictionary-indexed slot layout below must be rank-identical (both
    # the fused-path eligibility check and the final all-reduce key off
    # dictionary sizes)
    align_dictionaries(idf, list(cols) + [label_col])

    use_fused = (
        bool(encoding_configs)
        and encoding_configs.get("monotonicity_check", 0) == 0
        and len(num_cols) > 0
        and idf.device.type == "cuda"
        and all(idf.col(c).data.is_cuda for c in cols)
        and _backend.use_hip(idf.col(num_cols[0]).data)
        and all(
            len(idf.col(c).dictionary or []) + 1 <= 8192
            for c in cols
            if idf.col(c).kind == "categorical"
        )
    )
    if use_fused:
        # fused K6+K9: place raw values against the cutoffs inside the
        # counting kernel — the binned frame is never materialized
        from anovos_amd.data_transformer.transformers import _device_bin_cutoffs, compute_bin_cutoffs

        bin_size = int(encoding_configs["bin_size"])
        bin_method = encoding_configs["bin_method"]
        numset = set(num_cols)
        ncols_order = [c for c in cols if c in numset]
        ccols_order = [c for c in cols if c not in numset]
        ext = _backend.hip_ext()
        lab_u8 = label.to(torch.uint8).contiguous()
        nsizes = [bin_size + 2] * len(ncols_order)
        tensors = [idf.col(c).data.contiguous() for c in ncols_order]
        # cutoffs from the cached device histograms feed the counting kernel
        # directly: query -> bucketize+count -> categorical counts, and the
        # first sync is the one that fetches the counts
        cut_matrix = _device_bin_cutoffs(idf, ncols_order, bin_method, bin_size)
        if cut_matrix is not None:
            parts = [ext.bucketize_label_counts_dev(tensors, cut_matrix, lab_u8, nsizes)]
        else:
            kept, cutlists = compute_bin_cutoffs(ctx, idf, num_cols, bin_method, bin_size)
            cutmap = dict(zip(kept, cutlists))
            cuts = [torch.tensor(cutmap.get(c, []), dtype=torch.float64) for c in ncols_order]
            parts = [ext.bucketize_label_counts(tensors, cuts, lab_u8, nsizes)]
        csizes = []
        if ccols_order:
            ctensors = []
            for c in ccols_order:
                t = idf.col(c).data
                ctensors.append(t.contiguous() if t.dtype == torch.int32 else t.to(torch.int32).contiguous())
            csizes = [len(idf.col(c).dictionary or []) + 1 for c in ccols_order]
            parts.append(ext.label_counts_multi(ctensors, lab_u8, csizes))
        flat = torch.cat(parts) if len(parts) > 1 else parts[0]
        flat = dist.all_reduce_(flat.to(torch.float64), "sum").cpu().numpy()
        out, off = {}, 0
        for c, s in zip(ncols_order + ccols_order, nsizes + csizes):
            tot = flat[off : off + s]
            n1 = flat[off + s : off + 2 * s]
            out[c] = (tot - n1, n1)
            off += 2 * s
        idf.aux_cache[key] = out
        return out
    nmax = None
    if len(num_cols) > 0 and bool(encoding_configs):
        bin_size = encoding_configs["bin_size"]
        bin_method = encoding_configs["bin_method"]
        if encoding_configs.get("monotonicity_check", 0) == 1:
            idf_encoded = monotonic_binning(ctx, idf, num_cols, [], label_col, event_label, bin_method, bin_size)
            cap = max(int(bin_size), 20)
        else:
            idf_encoded = attribute_binning(ctx, idf, num_cols, [], bin_method, bin_size)
            cap = int(bin_size)
        nmax = {c: cap for c in num_cols}
    else:
        idf_encoded = idf
    counts = _binned_label_counts_multi(idf_encoded, cols, label, numeric_max=nmax)
    idf.aux_cache[key] = counts
    return counts


def _binned_label_counts_multi(idf, cols, label: torch.Tensor, numeric_max=None):
    """Per-group (n0, n1) counts for MANY columns in one fused K9 launch
    (GPU: anovos_label_counts_multi — one frame read, LDS-staged
    2-counter histograms) and ONE batched cross-rank all-reduce.

    Slot layout matches the reference's groupBy semantics
    (association_evaluator.py:368-409): categorical null = last slot,
    numeric binned null = slot 0, bin b -> slot b+1.
    numeric_max: optional {col: known max int value} (e.g. bin_size for
    freshly binned columns) — skips the max-reduction for those columns.
    """
    from anovos_amd.ops import backend as _backend

    numeric_max = numeric_max or {}
    lab_sum_check = None  # noqa: F841 (clarity)
    dev = idf.device
    # --- per-column slot counts ---
    need_max, local_max = [], []
    for col in cols:
        c = idf.col(col)
        if c.kind != "categorical" and col not in numeric_max:
            need_max.append(col)
            codes = torch.nan_to_num(c.data, nan=-1.0)
            local_max.append(float(codes.max().item()) if codes.numel() else 0.0)
    if need_max:
        merged = dist.all_reduce_scalars(local_max, "max")
        for col, m in zip(need_max, merged):
            numeric_max[col] = max(int(m), 0)
    sizes = []
    for col in cols:
        c = idf.col(col)
        if c.kind == "categorical":
            sizes.append(len(c.dictionary or []) + 1)
        else:
            sizes.append(int(numeric_max[col]) + 2)  # null slot 0 + codes 1..max+1

    use_gpu = (
        dev.type == "cuda"
        and all(idf.col(c).data.is_cuda for c in cols)
        and all(1 <= s <= 8192 for s in sizes)
        and _backend.use_hip(idf.col(cols[0]).data)
    )
    if use_gpu:
        ext = _backend.hip_ext()
        lab_u8 = label.to(torch.uint8).contiguous()
        tensors = []
        for col in cols:
            c = idf.col(col)
            t = c.data
            if c.kind == "categorical":
                tensors.append(t.contiguous() if t.dtype == torch.int32 else t.to(torch.int32).contiguous())
            else:
                tensors.append(t.contiguous() if t.dtype == torch.float32 else t.to(torch.float32).contiguous())
        flat = ext.label_counts_multi(tensors, lab_u8, sizes)
        flat = dist.all_reduce_(flat.to(torch.float64), "sum").cpu().numpy()
        out, off = {}, 0
        for col, s in zip(cols, sizes):
            tot = flat[off : off + s]
            n1 = flat[off + s : off + 2 * s]
            out[col] = (tot - n1, n1)
            off += 2 * s
        return out

    # CPU / fallback: per-column scatter_add into ONE flat buffer, one
    # batched all-reduce at the end
    lab = label.to(torch.float64)
    offsets = np.cumsum([0] + sizes)
    n0 = torch.zeros(int(offsets[-1]), dtype=torch.float64, device=dev)
    n1 = torch.zeros_like(n0)
    for col, off in zip(cols, offsets[:-1]):
        c = idf.col(col)
        if c.kind == "categorical":
            size = len(c.dictionary or []) + 1
            codes = c.data.to(torch.long)
            codes = torch.where(codes == NULL_CODE, torch.full_like(codes, size - 1), codes)
        else:
            codes = (torch.nan_to_num(c.data, nan=-1.0).to(torch.long) + 1).clamp(min=0)
        codes = codes + int(off)
        n1.scatter_add_(0, codes, lab)
        n0.scatter_add_(0, codes, 1.0 - lab)
    both = torch.stack([n0, n1])
    dist.all_reduce_(both, "sum")
    both = both.cpu().numpy()
    return {
        col: (both[0, off : off + s], both[1, off : off + s])
        for col, off, s in zip(cols, offsets[:-1], sizes)
    }


@traced
def IV_calculation(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    label_col="label",
    event_label=1,
    encoding_configs={"bin_method": "equal_frequency", "bin_size": 10, "monotonicity_check": 0},
    print_impact=False,
):
    """[attribute, iv] — reference association_evaluator.py:253-424."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|")]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    cols = [e for e in dict.fromkeys(list_of_cols) if e not in (list(drop_cols) + [label_col])]
    if any(x not in idf.columns for x in cols) or len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    label, _n_events = _cached_event_indicator(idf, label_col, event_label)
    if _n_events == 0:
        raise TypeError("Invalid input for Event Label Value")
    counts = _encoded_label_counts(ctx, idf, cols, label_col, event_label, label, encoding_configs)
    rows = []
    for col in cols:
        n0, n1 = counts[col]
        keep = (n0 + n1) > 0
        n0, n1 = n0[keep], n1[keep]
        t0, t1 = n0.sum(), n1.sum()
        event_pcr = n1 / t1
        nonevent_pcr = n0 / t0
        diff = nonevent_pcr - event_pcr
        with np.errstate(divide="ignore", invalid="ignore"):
            woe = np.where(
                (nonevent_pcr != 0) & (event_pcr != 0),
                np.log(nonevent_pcr / event_pcr),
                np.log(((n0 + 0.5) / t0) / ((n1 + 0.5) / t1)),
            )
        iv = float(np.sum(woe * diff))
        rows.append([col, iv])
    odf = pd.DataFrame(rows, columns=["attribute", "iv"])
    if print_impact:
        print(odf.to_string(index=False))
    return odf


@traced
def IG_calculation(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    label_col="label",
    event_label=1,
    encoding_configs={"bin_method": "equal_frequency", "bin_size": 10, "monotonicity_check": 0},
    print_impact=False,
):
    """[attribute, ig] — reference association_evaluator.py:427-586."""
    if list_of_cols == "all":
        num_cols, cat_cols, _ = attributeType_segregation(idf)
        list_of_cols = num_cols + cat_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|")]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    cols = [e for e in dict.fromkeys(list_of_cols) if e not in (list(drop_cols) + [label_col])]
    if any(x not in idf.columns for x in cols) or len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")
    label, total_events = _cached_event_indicator(idf, label_col, event_label)
    total_rows = idf.count()
    if total_events == 0:
        raise TypeError("Invalid input for Event Label Value")
    total_event = total_events / total_rows
    total_entropy = -(total_event * math.log2(total_event) + (1 - total_event) * math.log2(1 - total_event))
    counts = _encoded_label_counts(ctx, idf, cols, label_col, event_label, label, encoding_configs)
    rows = []
    for col in cols:
        n0, n1 = counts[col]
        tot = n0 + n1
        keep = tot > 0
        n0, n1, tot = n0[keep], n1[keep], tot[keep]
        event_pct = n1 / tot
        segment_pct = tot / tot.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            ent = -segment_pct * (event_pct * np.log2(event_pct) + (1 - event_pct) * np.log2(1 - event_pct))
        # Spark's sum skips null (0*log0) entries — emulate by nan-skipping
        entropy_sum = float(np.nansum(np.where(np.isfinite(ent), ent, np.nan)))
        rows.append([col, float(total_entropy - entropy_sum)])
    odf = pd.DataFrame(rows, columns=["attribute", "ig"])
    if print_impact:
        print(odf.to_string(index=False))
    return odf


def _association_stats(tab: np.ndarray, bias_correction: bool = False):
    """(cramers_v, mutual_info, u_row_given_col, u_col_given_row) of one
    contingency table whose LAST row and column are the null slots — fp64
    numpy throughout. The null row/column go first (pairwise-complete
    rows), then categories without a row left; N, r, c are what remains.
    mutual_info is in nats; u_row_given_col = MI / H(row variable).
    Undefined entries are NaN."""
    nan = float("nan")
    t = np.asarray(tab, dtype=np.float64)[:-1, :-1]
    t = t[t.sum(axis=1) > 0][:, t.sum(axis=0) > 0] if t.size else t
    n = float(t.sum()) if t.size else 0.0
    if n <= 0:
        return nan, nan, nan, nan
    r, c = t.shape
    ri = t.sum(axis=1)
    cj = t.sum(axis=0)
    expected = np.outer(ri, cj) / n
    phi2 = float((((t - expected) ** 2) / expected).sum()) / n
    v = nan
    if min(r, c) >= 2:
        if not bias_correction:
            v = math.sqrt(phi2 / min(r - 1, c - 1))
        elif n >= 2:
            # Bergsma (2013)
            phi2c = max(0.0, phi2 - (r - 1) * (c - 1) / (n - 1))
            rt = r - (r - 1) ** 2 / (n - 1)
            ct = c - (c - 1) ** 2 / (n - 1)
            den = min(rt - 1, ct - 1)
            if den > 0:
                v = math.sqrt(phi2c / den)
    nz = t > 0
    mi = max(0.0, float((t[nz] / n * np.log(t[nz] * n / np.outer(ri, cj)[nz])).sum()))
    h_row = -float((ri / n * np.log(ri / n)).sum())
    h_col = -float((cj / n * np.log(cj / n)).sum())
    u_row = mi / h_row if h_row > 0 else nan
    u_col = mi / h_col if h_col > 0 else nan
    return v, mi, u_row, u_col


@traced
def categorical_association_matrix(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    method_type="cramers_v",
    bias_correction=False,
    encoding_configs={"bin_method": "equal_frequency", "bin_size": 10},
    max_categories=1000,
    print_impact=False,
):
    """[attribute, <cols...>] — association between categorical attributes
    (numerical ones are binned first), beyond the reference, which only
    offers Pearson over label-encoded codes for this.

    method_type: "cramers_v" (symmetric, [0, 1]; bias_correction=True
    applies Bergsma's correction), "mutual_info" (symmetric, nats) or
    "theils_u" (entry [row x, column y] = MI(x, y) / H(x), asymmetric).
    Every pair uses its pairwise-complete rows; undefined entries (no
    complete row, a constant column where the measure needs two
    categories) are NaN. Categorical columns with more than
    max_categories dictionary entries are left out with a warning. One
    pass of the pair-count kernel (K22) yields all contingency tables;
    the statistics are fp64 numpy on the host, not rounded."""
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.ops.contingency import pair_contingency_tables
    from anovos_amd.ops.groupby import align_dictionaries

    if method_type not in ("cramers_v", "mutual_info", "theils_u"):
        raise TypeError("Invalid input for method_type")
    num_cols, cat_cols, _ = attributeType_segregation(idf)
    if list_of_cols == "all":
        list_of_cols = num_cols + cat_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|")]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    cols = [e for e in dict.fromkeys(list_of_cols) if e not in list(drop_cols)]
    if any(x not in num_cols + cat_cols for x in cols) or len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")

    my_cat = [c for c in cols if c in cat_cols]
    my_num = [c for c in cols if c in num_cols]
    # dictionary sizes decide which columns stay: make them rank-identical first
    align_dictionaries(idf, my_cat)
    too_wide = [c for c in my_cat if len(idf.col(c).dictionary or []) > max_categories]
    if too_wide:
        warnings.warn(
            "categorical_association_matrix: more than " + str(max_categories)
            + " categories, column(s) left out: " + ", ".join(too_wide)
        )
        cols = [c for c in cols if c not in too_wide]
    if len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")

    work = {c: idf.col(c) for c in cols if c in cat_cols}
    if my_num:
        bin_size = int(encoding_configs["bin_size"])
        binned = attribute_binning(
            ctx, idf.select(my_num), my_num, [], encoding_configs["bin_method"], bin_size,
            "numerical", False, "NA", "append",
        )
        labels = [str(b) for b in range(1, bin_size + 1)]
        for c in my_num:
            if c + "_binned" in binned:
                b = binned.col(c + "_binned").data  # bin label 1..bin_size, NaN = null
                codes = torch.where(torch.isnan(b), torch.full_like(b, NULL_CODE), b - 1).to(torch.int32)
            else:  # all-null column: binning warned and left it out
                codes = torch.full((idf.local_rows(),), NULL_CODE, dtype=torch.int32, device=idf.device)
            work[c] = Column(c, "string", codes, labels)
            work[c].cache["dict_aligned"] = True  # same labels on every rank
    wf = AnovosFrame({c: work[c] for c in cols}, idf.device)

    k = len(cols)
    pairs = [(cols[a], cols[b]) for a in range(k) for b in range(a + 1, k)]
    if k == 1:
        pairs = [(cols[0], cols[0])]  # only the marginal is needed
    tables = pair_contingency_tables(wf, cols, pairs)

    pick = {"cramers_v": 0, "mutual_info": 1, "theils_u": 2}[method_type]
    mat = np.full((k, k), np.nan, dtype=np.float64)
    for a in range(k):
        # diagonal: the column against itself is the diagonal table of its
        # marginal (rows of any of its tables, null column included)
        if k == 1:
            marg = np.diag(tables[pairs[0]])
        elif a + 1 < k:
            marg = tables[(cols[a], cols[a + 1])].sum(axis=1)
        else:
            marg = tables[(cols[a - 1], cols[a])].sum(axis=0)
        m = marg[:-1]
        diag = np.zeros((m.size + 1, m.size + 1), dtype=np.int64)
        diag[np.arange(m.size), np.arange(m.size)] = m
        st = _association_stats(diag, bias_correction)
        # a constant (or empty) column has no association with itself
        mat[a, a] = st[pick] if np.count_nonzero(m) >= 2 else np.nan
        for b in range(a + 1, k):
            st = _association_stats(tables[(cols[a], cols[b])], bias_correction)
            mat[a, b] = st[pick]
            mat[b, a] = st[3] if method_type == "theils_u" else st[pick]
    odf = pd.DataFrame(mat, columns=cols, index=cols)
    odf["attribute"] = odf.index
    sorted_cols = sorted(cols)
    odf = odf[["attribute"] + sorted_cols].sort_values("attribute").reset_index(drop=True)
    if print_impact:
        print(odf.to_string(index=False))
    return odf


def _anova_stats(mom: np.ndarray):
    """(eta_squared, anova_f) of one pair from its per-group moments
    [(n, mean, M2)] whose LAST row is the null slot — fp64 numpy
    throughout. The null slot goes first (pairwise-complete rows), then
    groups without a row; k groups and N rows remain. SSW is the sum of the
    groups' M2, never SST - SSB, so eta near 1 does not cancel. Undefined
    entries are NaN."""
    nan = float("nan")
    m = np.asarray(mom, dtype=np.float64)[:-1]
    m = m[m[:, 0] > 0]
    k = m.shape[0]
    if k < 2:
        return nan, nan
    n, mean, m2 = m[:, 0], m[:, 1], m[:, 2]
    if not (np.isfinite(mean).all() and np.isfinite(m2).all()):
        return nan, nan  # a non-finite value among the rows used
    big_n = float(n.sum())
    # group means about the first one: equal means give SSB = 0 exactly,
    # whatever the rounding of the grand mean
    delta = mean - mean[0]
    mu = float((n * delta).sum()) / big_n
    ssw = float(m2.sum())
    ssb = float((n * (delta - mu) ** 2).sum())
    sst = ssb + ssw
    eta2 = min(max(ssb / sst, 0.0), 1.0) if sst > 0 else nan
    f = nan
    if big_n > k:
        if ssw > 0:
            f = (ssb / (k - 1)) / (ssw / (big_n - k))
        elif ssb > 0:
            f = float("inf")
    return eta2, f


@traced
def numerical_categorical_association(
    ctx,
    idf,
    list_of_cols="all",
    drop_cols=[],
    method_type="correlation_ratio",
    max_categories=1000,
    print_impact=False,
):
    """[attribute, <numerical cols...>], one row per categorical attribute —
    how much of a numerical attribute a categorical one explains, beyond
    the reference, which has no measure for this kind of pair.

    method_type: "eta_squared" (SSB / SST, [0, 1]), "correlation_ratio"
    (its square root) or "anova_f" (the one-way ANOVA F statistic,
    (SSB / (k - 1)) / (SSW / (N - k)); +inf where the groups differ and no
    group varies). Every pair uses its pairwise-complete rows (non-null
    category, non-NaN value) and drops empty groups; undefined entries
    (fewer than two groups, a constant numerical attribute for the eta
    methods, N <= k for anova_f, a non-finite value) are NaN. Categorical
    columns with more than max_categories dictionary entries are left out
    with a warning. One pass of the grouped-moments kernel (K23) yields
    (n, mean, M2) per group for all pairs; the statistics are fp64 numpy on
    the host, not rounded."""
    from anovos_amd.ops.grouped import grouped_moments
    from anovos_amd.ops.groupby import align_dictionaries

    if method_type not in ("correlation_ratio", "eta_squared", "anova_f"):
        raise TypeError("Invalid input for method_type")
    num_cols, cat_cols, _ = attributeType_segregation(idf)
    if list_of_cols == "all":
        list_of_cols = num_cols + cat_cols
    if isinstance(list_of_cols, str):
        list_of_cols = [x.strip() for x in list_of_cols.split("|")]
    if isinstance(drop_cols, str):
        drop_cols = [x.strip() for x in drop_cols.split("|")]
    cols = [e for e in dict.fromkeys(list_of_cols) if e not in list(drop_cols)]
    if any(x not in num_cols + cat_cols for x in cols) or len(cols) == 0:
        raise TypeError("Invalid input for Column(s)")

    my_cat = [c for c in cols if c in cat_cols]
    my_num = [c for c in cols if c in num_cols]
    # dictionary sizes decide which columns stay: make them rank-identical first
    align_dictionaries(idf, my_cat)
    too_wide = [c for c in my_cat if len(idf.col(c).dictionary or []) > max_categories]
    if too_wide:
        warnings.warn(
            "numerical_categorical_association: more than " + str(max_categories)
            + " categories, column(s) left out: " + ", ".join(too_wide)
        )
        my_cat = [c for c in my_cat if c not in too_wide]
    if len(my_cat) == 0 or len(my_num) == 0:
        raise TypeError("Invalid input for Column(s)")

    my_cat, my_num = sorted(my_cat), sorted(my_num)
    moments = grouped_moments(idf, my_cat, my_num)
    mat = np.full((len(my_cat), len(my_num)), np.nan, dtype=np.float64)
    for a, c in enumerate(my_cat):
        for b, v in enumerate(my_num):
            eta2, f = _anova_stats(moments[(c, v)])
            if method_type == "anova_f":
                mat[a, b] = f
            elif method_type == "eta_squared":
                mat[a, b] = eta2
            else:
                mat[a, b] = math.sqrt(eta2) if eta2 == eta2 else np.nan
    odf = pd.DataFrame(mat, columns=my_num)
    odf.insert(0, "attribute", my_cat)
    if print_impact:
        print(odf.to_string(index=False))
    return odf
